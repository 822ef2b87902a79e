"""Input cubes for the DTW alignment tests (tests/test_dtw_math.py on the host function, tests/test_dtw_kernels_gpu.py on the kernels) and
tools/dtw_probe.py: cross-attention-like probabilities [n_heads][n_tokens][n_ctx] F32, seeded, with the shapes and the degenerate
contents at which the alignment can go wrong.  A case is a dict: name, cube, M (audio tokens in use), sot_len, and N = n_tokens - sot_len - 1."""
import numpy as np


def softmax_cube(seed, n_heads, n_tokens, n_ctx, M, sharp=6.0):
    """Rows that sum to one over n_ctx, with a ridge that moves along the audio axis with the token index plus noise: what an alignment head looks like."""
    rng = np.random.default_rng(seed)
    j = np.arange(n_ctx, dtype=np.float64)[None, None, :]
    centre = (np.arange(n_tokens, dtype=np.float64)[None, :, None] + 0.5) * (M / n_tokens) + rng.normal(0.0, 1.5, (n_heads, n_tokens, 1))
    width = max(1.5, M / 24.0)
    logits = -((j - centre) / width) ** 2 + rng.normal(0.0, 1.0, (n_heads, n_tokens, n_ctx)) * (sharp / 6.0)
    e = np.exp(logits - logits.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def case(name, cube, M, sot_len):
    n_heads, n_tokens, n_ctx = cube.shape
    return dict(name=name, cube=np.ascontiguousarray(cube, dtype=np.float32), M=M, sot_len=sot_len, N=n_tokens - sot_len - 1)


def shaped(name, seed, n_heads, N, M, n_ctx, sot_len=2):
    return case(name, softmax_cube(seed, n_heads, N + sot_len + 1, n_ctx, M), M, sot_len)


def constant(n_heads=3, N=5, M=12, n_ctx=14, sot_len=2):
    """every cost ties: the path is the tie rule's alone"""
    return case("constant", np.full((n_heads, N + sot_len + 1, n_ctx), 0.125, dtype=np.float32), M, sot_len)


def zero_variance(seed=11, n_heads=3, N=10, M=20, n_ctx=24, sot_len=2):
    """every third column is constant over the tokens (variance 0: the scale is 1 / sqrt(eps))"""
    c = softmax_cube(seed, n_heads, N + sot_len + 1, n_ctx, M)
    c[:, :, ::3] = np.float32(0.03125)
    return case("zero_variance", c, M, sot_len)


def mean_rounds(seed, n_heads, N=60, M=33, n_ctx=40, sot_len=2):
    """2^23 + small integers: the F64 sum is exact and sum / n_tokens is not an F32 (the mean rounds); an F32 sum loses the integers' low bits"""
    rng = np.random.default_rng(seed)
    c = (8388608.0 + rng.integers(0, 16, (n_heads, N + sot_len + 1, n_ctx))).astype(np.float32)
    return case("mean_rounds_h%d" % n_heads, c, M, sot_len)


def signed_zeros(seed=13, n_heads=3, N=12, M=24, n_ctx=24, sot_len=2):
    """columns of +0 and -0 in a seeded pattern: the mean is +0 and the normalised values keep their signs, so the median network's
    exchanges meet +0 against -0 (the host function and the kernels must agree; sorted() need not)"""
    rng = np.random.default_rng(seed)
    c = softmax_cube(seed, n_heads, N + sot_len + 1, n_ctx, M)
    z = np.where(rng.integers(0, 2, c.shape) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    cols = rng.integers(0, 2, n_ctx) == 1
    c[:, :, cols] = z[:, :, cols]
    return case("signed_zeros", c, M, sot_len)


def small_cases():
    """M = 8, 9, 64, 65; N = 1, 2, 63, 64, 65; 1 and 3 heads; n_ctx > M and n_ctx == M"""
    return [
        shaped("h3_N65_M65", 1, 3, 65, 65, 70),
        shaped("h1_N64_M64", 2, 1, 64, 64, 64),
        shaped("h3_N63_M9", 3, 3, 63, 9, 12),
        shaped("h1_N1_M8", 4, 1, 1, 8, 8),
        shaped("h3_N2_M9_sot1", 5, 3, 2, 9, 16, sot_len=1),
        shaped("h1_N2_M65", 6, 1, 2, 65, 66),
        shaped("h3_N64_M8", 7, 3, 64, 8, 10),
        constant(),
        zero_variance(),
        mean_rounds(8, 1),
        mean_rounds(9, 3),
    ]

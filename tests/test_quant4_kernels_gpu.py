"""The Q4_0 / Q4_K launchers one by one (MI355X) against the host statement whisper-rust_amd/csrc/wa_quant4.h (itself held to the reference library by
tests/test_quant4_math.py), as equality of bytes.  Operands are seeded: raw blocks with every nibble / scale-byte pattern and F16 scales of both signs over four
decades; activation rows with block scales over four decades, an all-zero block, a block of rint ties that holds - m before + m in row 0 (a four-row-rule row
of Q4_K once M >= 4) and in the last row (a leftover row unless M % 4 == 0).  Harness: tests/native/quant4_kernels.hip, linked against the product's objects."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, ENC_QKV, GELU_F32, RESID, F32, CROSS_KV, DEC_QKV = 0, 1, 7, 3, 5, 6, 8        # wa_epi_mode
PF, PB, PI = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
BLOCK = {"q4_0": (32, 18), "q4_k": (256, 144)}        # values and bytes of a block
FORMATS = pytest.mark.parametrize("fmt", ["q4_0", "q4_k"])


class Epi(C.Structure):
    _fields_ = [("bias", PF), ("scale", PF), ("resid", PF), ("gelu", C.POINTER(C.c_uint16))] + \
               [(n, C.c_int) for n in ("split0", "split1", "row_off", "aux0", "aux1", "ldo", "ldo2", "ldo3", "ldr")] + \
               [("out", PB), ("out2", PB), ("out3", PB), ("out_bytes", C.c_size_t), ("out2_bytes", C.c_size_t), ("out3_bytes", C.c_size_t)]


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(os.path.join(ROOT, "tests", "native", "libquant4_kernels.so"))
    lib.q4k_gemm.argtypes = [C.c_int] * 6 + [PF, PB, C.POINTER(Epi), PB, PB, PF, PF]
    lib.q4k_plain.argtypes = [C.c_int] * 4 + [PF, PB, PF, C.c_int, PI, PI, PF, C.c_int, PF]
    lib.q4k_host_pack.argtypes = [C.c_int, PB, C.c_int, C.c_int, PB, PB, PF, PF]
    lib.q4k_host_dot.argtypes = [C.c_int] * 5 + [PF, PB, PF, PF]
    lib.q4k_quant.argtypes = lib.q4k_host_quant.argtypes = [C.c_int] * 3 + [PF, C.POINTER(C.c_int8), PF, C.POINTER(C.c_int16)]
    return lib


def p(a, t=PF):
    return a.ctypes.data_as(t) if a is not None else None


def operands(fmt, M, N, K, seed):
    rng = np.random.default_rng(seed)
    per, size = BLOCK[fmt]
    nb, nd = K // per, 1 if fmt == "q4_0" else 2
    blk = rng.integers(0, 256, (N * nb, size), dtype=np.uint8)
    d = (rng.uniform(-1, 1, (N * nb, nd)) * 10.0 ** rng.uniform(-4, 0, (N * nb, nd))).astype(np.float16)
    blk[:, :2 * nd] = d.view(np.uint8).reshape(-1, 2 * nd)
    x = (rng.standard_normal((M, nb, per)) * 10.0 ** rng.uniform(-2, 2, (M, nb, 1))).astype(np.float32)
    x[M - 1, nb - 1] = 0.0
    for m in (0, M - 1):
        x[m, 0] = np.arange(per) % 20 + 0.5
        x[m, 0, 5], x[m, 0, 21] = -127.0, 127.0
    return np.ascontiguousarray(blk.reshape(-1)), np.ascontiguousarray(x.reshape(M, K))


def host_acc(h, fmt, plain, M, N, K, x, blk):
    acc, deq = np.empty((M, N), np.float32), np.empty((N, K), np.float32)
    h.q4k_host_dot(fmt == "q4_k", plain, M, N, K, p(x), p(blk, PB), p(acc), p(deq))
    return acc, deq


def arena(fmt, N, K):
    nb = K // BLOCK[fmt][0]
    return [np.zeros(N * K // 2, np.uint8), np.zeros(N * nb * 16, np.uint8) if fmt == "q4_k" else None, np.zeros(N * nb, np.float32),
            np.zeros(N * nb, np.float32) if fmt == "q4_k" else None]


def run(h, fmt, mode, route, M, N, K, x, blk, outs, lds=(0, 0, 0), **kw):
    """outs: the pre-filled output arrays (out, out2, out3); returns the arena arrays the device load kernel wrote."""
    keep = {k: np.ascontiguousarray(v) for k, v in kw.items() if isinstance(v, np.ndarray)}
    e = Epi(**{k: (p(v, C.POINTER(C.c_uint16)) if k == "gelu" else p(v)) for k, v in keep.items()}, **{k: v for k, v in kw.items() if k not in keep})
    e.ldo, e.ldo2, e.ldo3 = lds
    for name, a in zip(("out", "out2", "out3"), outs):
        setattr(e, name, p(a, PB)); setattr(e, name + "_bytes", a.nbytes)
    ar = arena(fmt, N, K)
    assert h.q4k_gemm(fmt == "q4_k", mode, route, M, N, K, p(x), p(blk, PB), C.byref(e), p(ar[0], PB), p(ar[1], PB), p(ar[2]), p(ar[3])) == 0
    return ar


@pytest.mark.parametrize("fmt,K", [("q4_0", 32), ("q4_0", 96), ("q4_0", 768), ("q4_k", 256), ("q4_k", 768)])
@pytest.mark.parametrize("N", [8, 24])
@pytest.mark.parametrize("M", [1, 3, 4, 7, 8, 9, 20])
def test_interleaved_product_and_load_equal_host_statement(h, fmt, M, N, K):
    """F32 results of the launcher's own rule (the few-rows kernel up to 8 rows, the matrix cores above: M = 9 and 20 leave a partly filled tile, N = 24 is one
    16-column tile + 8) and of the OTHER kernel named (the few-rows kernel in slices for M > 8, the matrix cores for M <= 8) are the host statement's bits; the
    arena arrays are the host pack's."""
    blk, x = operands(fmt, M, N, K, 1000 * M + N + K)
    want, _ = host_acc(h, fmt, 0, M, N, K, x, blk)
    assert h.q4k_kernel(M, 0) == (3 if M >= 9 else 2)
    for route in (0, 3 if M <= 8 else 2):
        out = np.full((M, N), np.float32(-77.0))
        ar = run(h, fmt, F32, route, M, N, K, x, blk, [out], (N, 0, 0))
        assert out.tobytes() == want.tobytes(), (route, np.argwhere(out.view(np.uint32) != want.view(np.uint32))[:4])
    host = arena(fmt, N, K)
    h.q4k_host_pack(fmt == "q4_k", p(blk, PB), N, K, p(host[0], PB), p(host[1], PB), p(host[2]), p(host[3]))
    assert [a.tobytes() for a in ar if a is not None] == [a.tobytes() for a in host if a is not None]


@FORMATS
@pytest.mark.parametrize("M", [3, 20])
def test_longest_row(h, fmt, M):
    """K = 5120, the longest row of any model: five (Q4_0) and two (Q4_K) rounds of the few-rows kernels' LDS, 160 / 20 chain steps on the matrix cores."""
    blk, x = operands(fmt, M, 24, 5120, 77 + M)
    out = np.full((M, 24), np.float32(-77.0))
    run(h, fmt, F32, 0, M, 24, 5120, x, blk, [out], (24, 0, 0))
    assert out.tobytes() == host_acc(h, fmt, 0, M, 24, 5120, x, blk)[0].tobytes()


def _gelu(v, table):
    t = table[v.astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)
    return np.where(v <= -10.0, np.float32(0.0), np.where(v >= 10.0, v, t)).astype(np.float32)


@FORMATS
@pytest.mark.parametrize("M", [3, 9], ids=["few-rows", "mfma"])
def test_every_epilogue(h, fmt, M):
    """bias, scale, residual, GELU table, F16 and transposed / scattered stores: each epilogue of wa_launch_qgemm_exact from both kernels, at N = 128 (one
    cross K / V layer of d = 64) and one block of K; cells no epilogue writes keep their fill."""
    N, K = 128, BLOCK[fmt][0]
    blk, x = operands(fmt, M, N, K, 5 + M)
    x = x * np.float32(0.01 if fmt == "q4_0" else 1e-4)               # (results well inside the F16 range)
    acc, _ = host_acc(h, fmt, 0, M, N, K, x, blk)
    assert np.abs(acc).max() < 6e4
    rng = np.random.default_rng(9)
    bias, scale = rng.standard_normal(N).astype(np.float32), rng.uniform(0.2, 1, N).astype(np.float32)
    resid, table = rng.standard_normal((M, N)).astype(np.float32), rng.integers(0, 0x7c00, 65536).astype(np.uint16)
    v = acc + bias
    fill16 = lambda *s: np.full(s, 0x1234, np.uint16)
    f16 = lambda a: a.astype(np.float16).view(np.uint16)
    go = lambda mode, outs, lds=(0, 0, 0), **kw: run(h, fmt, mode, 0, M, N, K, x, blk, outs, lds, **kw)

    out = fill16(M, N); go(F16, [out], (N, 0, 0), bias=bias, scale=scale)
    assert np.array_equal(out, f16(v * scale))
    out = np.zeros((M, N), np.float32); go(RESID, [out], (N, 0, 0), bias=bias, resid=resid, ldr=N)
    assert out.tobytes() == (v + resid).tobytes()
    out = np.zeros((M, N), np.float32); go(GELU_F32, [out], (N, 0, 0), bias=bias, gelu=table)
    assert out.tobytes() == _gelu(v, table).tobytes()
    out, out2 = fill16(M, 64), fill16(64, M + 3); go(ENC_QKV, [out, out2], (64, M + 3, 0), bias=bias, split0=64)
    assert np.array_equal(out, f16(v[:, :64])) and np.array_equal(out2[:, :M], f16(v[:, 64:]).T) and (out2[:, M:] == 0x1234).all()
    tpad = 16; out, out2 = fill16(1, tpad, 64), fill16(1, tpad, 64)
    go(CROSS_KV, [out, out2], bias=bias, scale=scale, aux0=tpad, aux1=64)
    w = f16(v * scale)
    assert np.array_equal(out[0, :M], w[:, :64]) and np.array_equal(out2[0, :M], w[:, 64:]) and (out[0, M:] == 0x1234).all()
    out, out2, out3 = fill16(M, 64), fill16(M + 2, 32), fill16(M + 2, 32)
    go(DEC_QKV, [out, out2, out3], (64, 32, 32), bias=bias, scale=scale, split0=64, split1=96, row_off=2)
    assert np.array_equal(out, w[:, :64]) and np.array_equal(out2[2:], w[:, 64:96]) and np.array_equal(out3[2:], w[:, 96:]) and (out2[:2] == 0x1234).all()


@pytest.mark.parametrize("M", [3, 4, 7])
def test_q8_K_quantiser_rules(h, M):
    """k_q8k_quant4 (rows below M - M % 4 by the four-row rule, the rest by the row rule) and the row quantiser against the host statement: quants in the
    kernel layout, d and the 16-element sums; with M = 4 and 7 the two rules give the tie block of row 0 opposite signs, with M = 4 that of the last row too."""
    K, I8, I16 = 768, C.POINTER(C.c_int8), C.POINTER(C.c_int16)
    _, x = operands("q4_k", M, 8, K, 40 + M)
    d = {}
    for rule in (0, 1):
        dev = [np.zeros(M * K, np.int8), np.zeros(M * 3, np.float32), np.zeros(M * 48, np.int16)]
        host = [np.zeros_like(a) for a in dev]
        assert h.q4k_quant(rule, M, K, p(x), p(dev[0], I8), p(dev[1]), p(dev[2], I16)) == 0
        h.q4k_host_quant(rule, M, K, p(x), p(host[0], I8), p(host[1]), p(host[2], I16))
        assert [a.tobytes() for a in dev] == [a.tobytes() for a in host], rule
        d[rule] = dev[1].reshape(M, 3)[:, 0]
    assert (d[0][0] == -d[1][0]) == (M >= 4) and (d[0][M - 1] == -d[1][M - 1]) == (M == 4)


@pytest.mark.parametrize("fmt,K", [("q4_0", 96), ("q4_k", 512)])
def test_plain_product_and_embedding_fetch(h, fmt, K):
    """The token embedding's form: N = 9 rows (no multiple of 8) loaded as bytes, the logits product in ggml_vec_dot_q4_0_q8_0 / q4_K_q8_K order for 1 and 5
    rows, and rows fetched as dequantize_row + positional embedding."""
    N = 9
    for M in (1, 5):
        blk, x = operands(fmt, M, N, K, 31 + M)
        want, deq = host_acc(h, fmt, 1, M, N, K, x, blk)
        tok, pos = np.array([8, 0, 3], np.int32), np.array([1, 0, 1], np.int32)
        pe = np.random.default_rng(3).standard_normal((2, K)).astype(np.float32)
        out, emb = np.zeros((M, N), np.float32), np.zeros((3, K), np.float32)
        assert h.q4k_plain(fmt == "q4_k", M, N, K, p(x), p(blk, PB), p(out), 3, p(tok, PI), p(pos, PI), p(pe), 2, p(emb)) == 0
        assert out.tobytes() == want.tobytes()
        assert emb.tobytes() == (deq[tok] + pe[pos]).tobytes()

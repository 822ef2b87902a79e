"""The fallbacks of the certified F64 sums, run on purpose: rows built by tools/adversarial_rows.py (committed as
tests/golden/exact_sums_rows.npz) through the launchers of wa_exact.hip, every output compared BIT FOR BIT with a plain reference
(F64 sums in index order by a Python loop, float32 for the rest).

A reference-order kernel sums in whatever order is fast and accepts the result when its certificate (wa_device.h: wa_sum_bounds)
says the order cannot matter; otherwise it falls back - second-level certificate, then one lane sums in index order from an LDS
mirror of the row.  Random rows take those fallbacks once per 10^5 rows or rarer, so no parity test runs them.  Every row here fails
the certificate by construction, and the expected output differs from what a fallback that keeps a certificate bound would give
(tests/test_exact_sums_math.py re-verifies both on the CPU from the fixture).

The kernels are called through tests/native/libexact_kernels.so, which oracle/Makefile links against the product's own
whisper-rust_amd/build/wa_exact.o.  Every output buffer is filled with a sentinel first; padding must still hold it afterwards.

Not covered here: WA_MEGA_REDO of the one-launch kernels.  The q and k of a real step come out of products and cannot be dictated
from outside, so the host side of the redo stays with the existing tests of the one-launch step.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adversarial_rows as AR  # noqa: E402

LIB_PATH = os.environ.get("WA_XTEST_LIB") or os.path.join(ROOT, "tests", "native", "libexact_kernels.so")
SENT8 = np.int8(-128)         # sentinels: bit patterns no kernel result can have (a Q8 quant is -127 .. 127, the floats are NaNs)
SENT16 = np.uint16(0x7E5A)
SENT32 = np.uint32(0x7FC0DEAD)
f32 = np.float32

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        assert os.path.exists(LIB_PATH), "%s missing: build() makes it (oracle/Makefile, target harness)" % LIB_PATH
        L = C.CDLL(LIB_PATH)
        vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
        L.xtest_alloc.restype = vp; L.xtest_alloc.argtypes = [sz]
        L.xtest_free.argtypes = [vp]
        L.xtest_h2d.argtypes = [vp, vp, sz]; L.xtest_d2h.argtypes = [vp, vp, sz]
        L.xtest_layernorm_exact.argtypes = [vp, i, i, i, vp, vp, f, vp, i, vp, i, vp, vp, vp]
        L.xtest_ln_gemv_exact_f32.argtypes = [vp, i, vp, vp, f, vp, i, i, i, i, vp, i]
        L.xtest_ln_q8_row.argtypes = [vp, i, vp, vp, f, vp, vp, vp]
        L.xtest_attn_exact.argtypes = [vp, i, vp, sz, i, vp, sz, i, i, i, i, vp, f, vp, vp, vp, i, vp]
        L.xtest_attn_exact_mfma.argtypes = [vp, i, vp, i, i, i, i, f, vp, vp, i, vp, i]
        _LIB = L
    return _LIB


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().xtest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().xtest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().xtest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().xtest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().xtest_sync()
    assert err == 0, "HIP error %d after the launch" % err


# ----------------------------------------------------------------------------------------------------------------------------
# the rows and the case table
# ----------------------------------------------------------------------------------------------------------------------------
ROWS = {r["name"]: r for r in AR.load()}
WAVE_ROWS = sorted(n for n, r in ROWS.items() if r["d"] in AR.DIMS)            # d <= 1280: one wave per row where the launcher has that form
BLOCK_ROWS = sorted(n for n, r in ROWS.items() if r["d"] in AR.BLOCK_DIMS)


def path_class(path):
    """The fallback a row takes, as the meta-test counts them."""
    return "mean_inorder" if path.startswith("mean_inorder") else path


# (launcher, form) -> rows; the soft-max cases are added below
CASES = {
    ("layernorm_exact", "wave"): WAVE_ROWS,
    ("ln_gemv_exact", "block, M = 1"): WAVE_ROWS,
    ("ln_gemv_exact", "wave, M = 5"): WAVE_ROWS,
    ("ln_gemv_exact", "block, M = 2, K = 1536"): BLOCK_ROWS,
    ("ln_q8_row", "block"): WAVE_ROWS,
}
LN_PATHS = ("mean_second", "mean_inorder", "var_up", "var_down")

_FILLER = {}


def fillers(d, n):
    """n ordinary Gaussian rows of width d (shared by the cases of that width, never modified)."""
    if (d, n) not in _FILLER:
        g = np.random.default_rng(9000 + d).standard_normal((n, d)).astype(np.float32)
        g.setflags(write=False)
        _FILLER[(d, n)] = g
    return _FILLER[(d, n)]


def rows_with(row, n, at):
    """n rows of the row's width: the adversarial row at the indices `at`, ordinary rows elsewhere.  Where the row brings a large gamma
    (2^20 .. 2^41 at the element that equals a candidate mean), an ordinary row would overflow F16 there, so its element at that index
    is set to that row's own mean (t = 0 exactly, y = beta = 0)."""
    d = row["d"]
    X = fillers(d, n).copy()
    big = [i for i, (wi, _) in row["override"].items() if abs(wi) > 1024]
    for k in range(n if big else 0):
        for _ in range(8):
            m = f32(AR.seq_sum(X[k]) / d)
            if all(X[k][i] == m for i in big):
                break
            X[k][big] = m
        assert all(X[k][i] == f32(AR.seq_sum(X[k]) / d) for i in big)
    for k in at:
        X[k] = row["x"]
    return X


def expected_rows(X, w, b, row):
    """The reference LayerNorm of every row of X; the adversarial row's comes from the fixture (and is the same bits: asserted)."""
    Y = np.stack([AR.layernorm_ref(x, w, b) for x in X])
    assert np.all(np.isfinite(Y.astype(np.float16)))
    for k, x in enumerate(X):
        if np.array_equal(x, row["x"]):
            assert np.array_equal(AR.bits32(Y[k]), row["y32"])
    return Y


def q8_rows(Y):
    """quantize_row_q8_0 / q8_1 (arch/x86/quants.c, AVX2) of F32 rows, in the kernel layout of wa_q8_store:
    qs int8 [rows][8][K/32][4], qd / qsum f32 [rows][K/32] (both rounded through F16)."""
    rows, K = Y.shape
    nb = K // 32
    blk = Y.reshape(rows, nb, 32)
    amax = np.abs(blk).max(-1).astype(np.float32)
    d = (amax / f32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, f32(127.0) / amax, f32(0.0)).astype(np.float32)
    q = np.rint((blk * idv[..., None]).astype(np.float32)).astype(np.int32)
    qd = d.astype(np.float16).astype(np.float32)
    qsum = (d * q.sum(-1).astype(np.float32)).astype(np.float32).astype(np.float16).astype(np.float32)
    qs = q.reshape(rows, nb, 8, 4).transpose(0, 2, 1, 3).astype(np.int8)
    return np.ascontiguousarray(qs), qd, qsum


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, bad.size, want.size, bad[0], int(got.ravel()[bad[0]]),
                                                                                   int(want.ravel()[bad[0]]))


# ----------------------------------------------------------------------------------------------------------------------------
# wa_launch_layernorm_exact: one wave per row, four rows per block
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES[("layernorm_exact", "wave")])
def test_layernorm_exact(dev, name):
    """9 rows: the adversarial row at 0, 3 and 8 (wave 0, wave 3, the partial last block), Gaussian rows between them.  out16 and out32
    together; then once more with the Q8 outputs set, which must leave out32 (and out16) as they were."""
    row = ROWS[name]
    d, w, b = row["d"], row["w"], row["b"]
    rows, ldx, ld16, ld32 = 9, d + 8, d + 8, d + 4
    X = rows_with(row, rows, (0, 3, 8))
    Y = expected_rows(X, w, b, row)
    Xp = np.zeros((rows, ldx), np.float32)
    Xp[:, :d] = X
    want16 = np.full((rows, ld16), SENT16, np.uint16)
    want16[:, :d] = AR.bits16(Y)
    want32 = np.full((rows, ld32), SENT32, np.uint32)
    want32[:, :d] = AR.bits32(Y)
    dx, dw, db = dev.put(Xp), dev.put(w), dev.put(b)
    nb = d // 32
    qs_w, qd_w, qsum_w = q8_rows(Y)
    for with_q8 in (False, True):
        o16 = dev.put(np.full((rows, ld16), SENT16, np.uint16))
        o32 = dev.put(np.full((rows, ld32), SENT32, np.uint32))
        qs = dev.put(np.full((rows, 8, nb, 4), SENT8, np.int8)) if with_q8 else None
        qd = dev.put(np.full((rows, nb), SENT32, np.uint32)) if with_q8 else None
        qsum = dev.put(np.full((rows, nb), SENT32, np.uint32)) if with_q8 else None
        lib().xtest_layernorm_exact(dx, ldx, rows, d, dw, db, AR.EPS, o16, ld16, o32, ld32, qs, qd, qsum)
        sync()
        assert_bits(Dev.get(o32, want32), want32, "out32 (q8 %s)" % with_q8)
        assert_bits(Dev.get(o16, want16), want16, "out16 (q8 %s)" % with_q8)
        if with_q8:
            assert_bits(Dev.get(qs, qs_w).view(np.uint8), qs_w.view(np.uint8), "qs")
            assert_bits(Dev.get(qd, qd_w).view(np.uint32), qd_w.view(np.uint32), "qd")
            assert_bits(Dev.get(qsum, qsum_w).view(np.uint32), qsum_w.view(np.uint32), "qsum")


# ----------------------------------------------------------------------------------------------------------------------------
# wa_launch_ln_gemv_exact: W = the K x K identity in F16, mode WA_EPI_F32 - one non-zero per dot product is exact in the
# ggml_vec_dot_f16 order, so the output is float(f16(LayerNorm(x))) exactly (a -0 comes out as +0: it is added to +0)
# ----------------------------------------------------------------------------------------------------------------------------
_EYE = {}


def eye16(K):
    if K not in _EYE:
        _EYE[K] = np.eye(K, dtype=np.float16).view(np.uint16)
    return _EYE[K]


def run_ln_gemv(dev, row, X):
    d, w, b = row["d"], row["w"], row["b"]
    M = X.shape[0]
    Y = expected_rows(X, w, b, row)
    want = (Y.astype(np.float16).astype(np.float32) + f32(0.0)).astype(np.float32)
    ldo = d + 4
    want_bits = np.full((M, ldo), SENT32, np.uint32)
    want_bits[:, :d] = AR.bits32(want)
    out = dev.put(np.full((M, ldo), SENT32, np.uint32))
    lib().xtest_ln_gemv_exact_f32(dev.put(X), d, dev.put(w), dev.put(b), AR.EPS, dev.put(eye16(d)), d, M, d, d, out, ldo)
    sync()
    assert_bits(Dev.get(out, want_bits), want_bits, "f16(LayerNorm(x)) through the identity product")


@pytest.mark.parametrize("name", CASES[("ln_gemv_exact", "block, M = 1")])
def test_ln_gemv_exact_one_row(dev, name):
    """M = 1: the block-wide LayerNorm (wa_block_layernorm: 256 threads share the row, red[8] / red[9])."""
    row = ROWS[name]
    run_ln_gemv(dev, row, row["x"][None, :].copy())


@pytest.mark.parametrize("name", CASES[("ln_gemv_exact", "wave, M = 5")])
def test_ln_gemv_exact_five_rows(dev, name):
    """M = 5, K <= 1280: one wave per row (wa_ln_stats<20>); wave 0 takes rows 0 and 4, so the adversarial row at 4 finds the LDS
    mirror that row 0 left, and the one at 1 runs beside three ordinary rows."""
    row = ROWS[name]
    X = rows_with(row, 5, (1, 4))
    run_ln_gemv(dev, row, X)


@pytest.mark.parametrize("name", CASES[("ln_gemv_exact", "block, M = 2, K = 1536")])
def test_ln_gemv_exact_block_rows(dev, name):
    """K = 1536 is wider than the wave-per-row form takes, so the two rows go through wa_block_layernorm one after the other: the
    adversarial row comes second and finds red[] and the LDS mirror as the Gaussian row before it left them."""
    row = ROWS[name]
    X = rows_with(row, 2, (1,))
    run_ln_gemv(dev, row, X)


# ----------------------------------------------------------------------------------------------------------------------------
# wa_launch_ln_q8_row
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES[("ln_q8_row", "block")])
def test_ln_q8_row(dev, name):
    """One row -> LayerNorm -> Q8_0 / Q8_1 by one block, against a numpy quantize_row_q8_0 / q8_1 of the reference LayerNorm.
    An 8-bit quant cannot tell a 1-ulp slip of the mean or the variance apart (except at the elements the rows place on purpose, and
    not reliably there), so this case does NOT pin the rounding of the fallback; it still fails on a fallback that reads the wrong
    LDS, a stale row or a sum of something else."""
    row = ROWS[name]
    d, w, b = row["d"], row["w"], row["b"]
    nb = d // 32
    Y = expected_rows(row["x"][None, :], w, b, row)
    qs_w, qd_w, qsum_w = q8_rows(Y)
    for with_sum in (False, True):
        qs = dev.put(np.full((1, 8, nb, 4), SENT8, np.int8))
        qd = dev.put(np.full((1, nb), SENT32, np.uint32))
        qsum = dev.put(np.full((1, nb), SENT32, np.uint32)) if with_sum else None
        lib().xtest_ln_q8_row(dev.put(row["x"]), d, dev.put(w), dev.put(b), AR.EPS, qs, qd, qsum)
        sync()
        assert_bits(Dev.get(qs, qs_w).view(np.uint8), qs_w.view(np.uint8), "qs")
        assert_bits(Dev.get(qd, qd_w).view(np.uint32), qd_w.view(np.uint32), "qd")
        if with_sum:
            assert_bits(Dev.get(qsum, qsum_w).view(np.uint32), qsum_w.view(np.uint32), "qsum")


# ----------------------------------------------------------------------------------------------------------------------------
# soft-max: the in-order redo of the four attention kernels
# ----------------------------------------------------------------------------------------------------------------------------
# Every query is one-hot in element 0 of its head, so a score is float(k_c[0] * q[0]) * scale exactly, whatever else the key holds;
# the adversarial rows have q[0] = 1 against the fixture's keys.  V has ONE non-zero (a small integer) per head dimension, so every
# P V dot product is a single exact product in any order and an F64 P V is the expected output bit for bit; the cells the non-zeros
# sit in include the ones whose F16 probability tells the two candidate inverses apart.
SM_ROWS = {r["name"]: r for r in AR.load_softmax()}
Q0 = (1.0, 0.5, 0.75, 1.5, -1.0)
CASES.update({
    ("attn_exact", "k_attn_exact<1>"): ["sm_63_hi", "sm_63_lo"],
    ("attn_exact", "k_attn_exact<4> + k_attn_combine"): ["sm_519_hi", "sm_519_lo"],
    ("attn_exact", "k_attn_exact_mq<4>"): ["sm_63_hi", "sm_63_lo"],
    ("attn_exact_mfma", "k_attn_scores_mfma"): ["sm_135_hi", "sm_135_lo"],
})


def attention_case(row, n_head, n_tokens, ha, adversarial_tokens):
    """Operands and expected results of one launch: head `ha` holds the fixture's keys, the other heads Gaussian ones; the queries of
    `adversarial_tokens` in head ha have q[0] = 1.  Returns q, K, V ([n][n_head * 64] F16 bits / values), p32 / p16 bits
    [n_tokens][n_head][n_kv] and out F16 bits [n_tokens][n_head * 64]."""
    n_kv, d = row["n_kv"], n_head * 64
    rng = np.random.default_rng(77 + n_kv + n_head)
    K = (0.5 * rng.standard_normal((n_kv, d))).astype(np.float16)
    for h in range(n_head):
        K[:, h * 64] = row["k16"].view(np.float16) if h == ha else np.clip(2.0 * rng.standard_normal(n_kv), -7.5, 7.5).astype(np.float16)
    q = np.zeros((n_tokens, d), np.float16)
    q0 = np.array([[Q0[(7 * j + 3 * h) % len(Q0)] for h in range(n_head)] for j in range(n_tokens)], np.float32)
    q0[list(adversarial_tokens), ha] = 1.0
    q[:, 0::64] = q0
    cells16 = AR.check_softmax_row(row)["cells16"]             # (also re-asserts the row's preconditions before the GPU sees it)
    V = np.zeros((n_kv, d), np.float16)
    first = list(cells16) + list(range(n_kv & ~7, n_kv))
    sel = (first + [c for c in range(0, n_kv, max(1, n_kv // 64)) if c not in first])[:64]
    sel = sel + [c for c in range(n_kv) if c not in sel][:64 - len(sel)]
    for h in range(n_head):
        for dh in range(64):
            V[sel[(dh + 5 * h) % len(sel)], h * 64 + dh] = (1, -2, 3, -1, 2, -3)[(dh + h) % 6]
    p32 = np.zeros((n_tokens, n_head, n_kv), np.float32)
    cache = {}
    for j in range(n_tokens):
        for h in range(n_head):
            key = (h, float(q0[j, h]))
            if key not in cache:
                cache[key] = AR.softmax_oracle(AR.sm_scores(K[:, h * 64].view(np.uint16), q0[j, h]))[3]
            p32[j, h] = cache[key]
    for j in adversarial_tokens:
        assert np.array_equal(AR.bits32(p32[j, ha]), row["p32"])
    p16 = p32.astype(np.float16)
    out = np.zeros((n_tokens, d), np.float64)
    for h in range(n_head):                                     # F64 P V, exact: one non-zero V per column
        out[:, h * 64:(h + 1) * 64] = p16[:, h, :].astype(np.float64) @ V[:, h * 64:(h + 1) * 64].astype(np.float64)
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64))
    return q, K, V, p32, p16, out.astype(np.float32).astype(np.float16)


def run_attn_exact(dev, row, n_head, n_tokens, ha, adversarial_tokens, split):
    n_kv, d = row["n_kv"], n_head * 64
    q, K, V, p32, p16, out = attention_case(row, n_head, n_tokens, ha, adversarial_tokens)
    ldo = d + 8
    want_out = np.full((n_tokens, ldo), SENT16, np.uint16)
    want_out[:, :d] = out.view(np.uint16)
    o = dev.put(np.full((n_tokens, ldo), SENT16, np.uint16))
    qk = dev.put(np.full((n_tokens, n_head, n_kv), SENT32, np.uint32))
    partial = dev.put(np.full((n_tokens, n_head, 32, 64), SENT32, np.uint32))
    pl_host = np.full((n_tokens, n_head, 32), SENT16, np.uint16)
    pl = dev.put(pl_host)
    lib().xtest_attn_exact(dev.put(q), d, dev.put(K), 64, d, dev.put(V), 64, d, n_head, n_tokens, n_kv, None, AR.SM_SCALE, partial, pl, o, ldo, qk)
    sync()
    assert_bits(Dev.get(qk, p32).view(np.uint32), AR.bits32(p32), "probabilities (qk_out)")
    assert_bits(Dev.get(o, want_out), want_out, "attention output")
    got_pl = Dev.get(pl, pl_host)
    if split:
        n_p = n_kv & ~31
        want_pl = np.zeros((n_tokens, n_head, 32), np.uint16)
        want_pl[:, :, :n_kv - n_p] = p16[:, :, n_p:].view(np.uint16)
        assert_bits(got_pl, want_pl, "p_left")
    else:
        assert_bits(got_pl, pl_host, "p_left (unused by this form)")


@pytest.mark.parametrize("name", CASES[("attn_exact", "k_attn_exact<1>")])
def test_attn_exact_one_query(dev, name):
    """n_kv = 63, one query, two heads: k_attn_exact<1>, the adversarial row in head 1."""
    run_attn_exact(dev, SM_ROWS[name], n_head=2, n_tokens=1, ha=1, adversarial_tokens=(0,), split=False)


@pytest.mark.parametrize("name", CASES[("attn_exact", "k_attn_exact<4> + k_attn_combine")])
def test_attn_exact_split(dev, name):
    """n_kv = 519 with n_tokens * n_head < 512: four blocks per (query, head) redo the sum each for itself, k_attn_combine finishes
    (7 cells past n_kv & ~31 travel through p_left)."""
    run_attn_exact(dev, SM_ROWS[name], n_head=2, n_tokens=1, ha=1, adversarial_tokens=(0,), split=True)


@pytest.mark.parametrize("name", CASES[("attn_exact", "k_attn_exact_mq<4>")])
def test_attn_exact_four_queries(dev, name):
    """64 queries x 16 heads, n_kv = 63: k_attn_exact_mq<4>; the adversarial rows are queries 5 and 63 of head 3 (slots 1 and 3 of their
    blocks), every other row an ordinary one."""
    run_attn_exact(dev, SM_ROWS[name], n_head=16, n_tokens=64, ha=3, adversarial_tokens=(5, 63), split=False)


@pytest.mark.parametrize("name", CASES[("attn_exact_mfma", "k_attn_scores_mfma")])
def test_attn_exact_mfma(dev, name):
    """T = 135 encoder self-attention, two heads: k_attn_scores_mfma (one lane per half-wave redoes the sum), P and the 7 cells past
    T & ~31 (p_left) as the kernel hands them to the P V product, then that product's output."""
    row = SM_ROWS[name]
    T, n_head, ha, adv = row["n_kv"], 2, 1, (37, 134)
    d, kvp = n_head * 64, 256
    q, K, V, p32, p16, out = attention_case(row, n_head, T, ha, adv)
    qkm = np.concatenate([q, K], axis=1)                       # [T][2 d]: Q | K
    vt = np.zeros((d, kvp), np.float16)
    vt[:, :T] = V.T
    n_p = T & ~31
    want_p = np.zeros((n_head, T, kvp), np.uint16)
    want_p[:, :, :n_p] = p16.transpose(1, 0, 2)[:, :, :n_p].view(np.uint16)
    want_pl = np.full((n_head, T, 32), SENT16, np.uint16)
    want_pl[:, :, :T - n_p] = p16.transpose(1, 0, 2)[:, :, n_p:].view(np.uint16)
    ldo = d + 8
    want_out = np.full((T, ldo), SENT16, np.uint16)
    want_out[:, :d] = out.view(np.uint16)
    P = dev.put(np.full((n_head, T, kvp), SENT16, np.uint16))
    pl = dev.put(np.full((n_head, T, 32), SENT16, np.uint16))
    o = dev.put(np.full((T, ldo), SENT16, np.uint16))
    lib().xtest_attn_exact_mfma(dev.put(qkm), 2 * d, dev.put(vt), kvp, T, d, n_head, AR.SM_SCALE, P, pl, kvp, o, ldo)
    sync()
    assert_bits(Dev.get(P, want_p), want_p, "P")
    assert_bits(Dev.get(pl, want_pl), want_pl, "p_left")
    assert_bits(Dev.get(o, want_out), want_out, "attention output")


# ----------------------------------------------------------------------------------------------------------------------------
# the table is complete
# ----------------------------------------------------------------------------------------------------------------------------
def test_case_table_is_complete():
    """Every (launcher, form) holds every fallback: the mean's second level, the mean's in-order sum, a variance that rounds up and
    one that rounds down - at every width; and every soft-max kernel has a row whose reference takes ihi and one that takes ilo."""
    for (launcher, form), names in CASES.items():
        if launcher.startswith("attn"):
            assert {SM_ROWS[n]["ref_is_hi"] for n in names} == {True, False}, (launcher, form)
            continue
        if launcher == "one-launch step":                                                # (defined further down: the model variants)
            assert {path_class(n.split("model_")[1].rsplit("_d", 1)[0]) for n in names} == set(LN_PATHS), (launcher, form)
            continue
        dims = AR.BLOCK_DIMS if "1536" in form else AR.DIMS
        for d in dims:
            have = {path_class(ROWS[n]["path"]) for n in names if ROWS[n]["d"] == d}
            want = set(LN_PATHS)
            assert have >= want, (launcher, form, d, want - have)
    assert {k for k in CASES if k[0].startswith("attn")} == {("attn_exact", "k_attn_exact<1>"), ("attn_exact", "k_attn_exact<4> + k_attn_combine"),
                                                             ("attn_exact", "k_attn_exact_mq<4>"), ("attn_exact_mfma", "k_attn_scores_mfma")}
    assert {k[0] for k in CASES} == {"layernorm_exact", "ln_gemv_exact", "ln_q8_row", "attn_exact", "attn_exact_mfma", "one-launch step"}


# ----------------------------------------------------------------------------------------------------------------------------
# the one-launch kernels, end to end: mg_ln3 (wa_mega.hip) and the LayerNorm of wa_rows.hip can only be reached through a model
# ----------------------------------------------------------------------------------------------------------------------------
# Layer 0's first LayerNorm of the decoder reads te[token] + pe[position].  The model variants below have a zero token-embedding row
# for CRAFT_TOK, the generator's rows as positional embeddings 3, 4, ... (one fallback each, AR.MODEL_PATHS) and the gamma / beta those
# rows share as layer 0's attn_ln, so feeding CRAFT_TOK at those positions puts each row through that LayerNorm, bit for bit.
# That gamma is 2^20 at one index, where an ordinary row would leave the F16 range; so the prompt is CRAFT_TOK three times as well,
# at positions 0 .. 2, which hold copies of the second-level row (a batch of three: the launch sequence normalises it with
# wa_launch_layernorm_exact, a state with the one-launch forms serves it by the several-rows pass).
# What a shape can see: a kept MEAN bound changes the logits at every shape; a kept VARIANCE bound changes one LayerNorm output by one F16
# ulp, which at s128 the F16 rounding of the Q / K / V products absorbs (the logits stay bit-identical), while tiny, small and w1280 show it.
# So s128 pins the variance fallback only structurally (it runs, reads the LDS row, and gives the right bits); the larger shapes pin its rounding.
import hashlib  # noqa: E402

import wsynth  # noqa: E402
from conftest import ORACLE_LIB  # noqa: E402

CRAFT_TOK = 1000
CRAFT_POS0 = 3
MODEL_D = {"s128": 128, "tiny": 384, "small": 768, "w1280": 1280}
for _shape in MODEL_D:
    CASES[("one-launch step", _shape)] = ["model_%s_d%d" % (p, MODEL_D[_shape]) for p in AR.MODEL_PATHS]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def crafted_model(name):
    """Path of the variant of shape `name` ("small:q5_0": its quantised file), cached like the other synthetic models."""
    shape = name.split(":")[0]
    rows, w, b = AR.load_model_rows(MODEL_D[shape])
    for r in rows:
        AR.check_row(r)                                        # the preconditions hold under the shared gamma / beta

    def te(a):
        a[CRAFT_TOK] = 0
        return a

    def pe(a):
        a[:CRAFT_POS0] = rows[0]["x"]
        for k, r in enumerate(rows):
            a[CRAFT_POS0 + k] = r["x"]
        return a
    ov = {"decoder.token_embedding.weight": te, "decoder.positional_embedding": pe,
          "decoder.blocks.0.attn_ln.weight": lambda a: w.copy(), "decoder.blocks.0.attn_ln.bias": lambda a: b.copy()}
    if ":" in name:
        return wsynth.quant_model_path(shape, name.split(":")[1], overrides=ov, tag="exactsums")
    return wsynth.model_path(shape, overrides=ov, tag="exactsums")


def two_states(wrs, lib, name, monkeypatch, seed=1):
    """A context of the crafted model with a launch-sequence state and a one-launch state, both encoded and past the prompt."""
    ctx = wrs.WhisperContext.new_with_params(crafted_model(name), wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); ref = ctx.create_state()
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); one = ctx.create_state()
    pcm = wsynth.synth_audio(480000, seed)
    for st in (ref, one):
        st.pcm_to_mel(pcm); st.encode(0); st.decode([CRAFT_TOK] * CRAFT_POS0, 0)
    return ctx, ref, one


def crafted_steps(ref, one):
    for k, path in enumerate(AR.MODEL_PATHS):
        ref.decode([CRAFT_TOK], CRAFT_POS0 + k); one.decode([CRAFT_TOK], CRAFT_POS0 + k)
        a = ref.get_logits_last(1); b = one.get_logits_last(1)
        assert np.isfinite(a).all()
        assert digest(a) == digest(b), "position %d (%s): max|d| = %g" % (CRAFT_POS0 + k, path, float(np.abs(a - b).max()))


@pytest.mark.parametrize("name", ["s128", "small", "small:q5_0", "w1280"])
def test_one_launch_step_at_crafted_positions(wrs, amd_lib, name, monkeypatch):
    """The one-launch step (k_decode_mega; small: the own-query form k_decode_mega_cq; small:q5_0: k_decode_mega_q) against the launch
    sequence - which the kernel tests above pin - at positions whose layer-0 LayerNorm row takes each fallback: bit-identical logits,
    and the one-launch path is the one that ran."""
    amd_lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    ctx, ref, one = two_states(wrs, amd_lib, name, monkeypatch)
    assert amd_lib.whisper_amd_mega_enabled(ref.ptr) == 0 and amd_lib.whisper_amd_mega_enabled(one.ptr) == 1
    crafted_steps(ref, one)
    assert amd_lib.whisper_amd_mega_enabled(one.ptr) == 1, "the one-launch step gave up and fell back"
    ref.free(); one.free(); ctx.free()


@pytest.mark.parametrize("name", ["s128", "small"])
def test_one_launch_step_at_crafted_positions_under_stalls(wrs, name, monkeypatch):
    """The same on the build whose product waves stall at random (libwhisper_chaos.so): the in-order lane reads LDS that other waves wrote,
    so a dependence on timing would show here.  (small as well as s128: only there do the logits see the variance's rounding.)"""
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: build() makes it"
    chaos = wrs.load_library(path)
    wrs.set_log_callback(chaos, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    chaos.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    ctx, ref, one = two_states(wrs, chaos, name, monkeypatch)
    assert chaos.whisper_amd_mega_enabled(ref.ptr) == 0 and chaos.whisper_amd_mega_enabled(one.ptr) == 1
    crafted_steps(ref, one)
    assert chaos.whisper_amd_mega_enabled(one.ptr) == 1
    ref.free(); one.free(); ctx.free()


@pytest.mark.parametrize("name", ["s128", "tiny"])
def test_crafted_positions_against_live_oracle(wrs, amd_lib, name):
    """The independent reference: liboracle always sums in order.  Its logits at every crafted position equal the product's (default
    state: the one-launch step where the shape has one)."""
    assert os.path.exists(ORACLE_LIB), "oracle/liboracle.so missing"
    orc = C.CDLL(ORACLE_LIB)
    orc.wo_load.restype = C.c_void_p; orc.wo_load.argtypes = [C.c_char_p]; orc.wo_free.argtypes = [C.c_void_p]
    orc.wo_logits.restype = C.POINTER(C.c_float); orc.wo_logits.argtypes = [C.c_void_p]
    orc.wo_mel.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]; orc.wo_encode.argtypes = [C.c_void_p, C.c_int]
    orc.wo_decode.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
    mp = crafted_model(name)
    pcm = wsynth.synth_audio(480000, 3)
    m = orc.wo_load(mp.encode())
    orc.wo_mel(m, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm)); orc.wo_encode(m, 0)
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    st.pcm_to_mel(pcm); st.encode(0)
    nv = ctx.n_vocab()
    steps = [([CRAFT_TOK] * CRAFT_POS0, 0)] + [([CRAFT_TOK], CRAFT_POS0 + k) for k in range(len(AR.MODEL_PATHS))]
    for toks, n_past in steps:
        arr = (C.c_int32 * len(toks))(*toks)
        orc.wo_decode(m, arr, len(toks), n_past)
        st.decode(toks, n_past)
        assert digest(st.get_logits_last(len(toks))) == digest(np.ctypeslib.as_array(orc.wo_logits(m), shape=(nv,))), (toks, n_past)
    orc.wo_free(m); st.free(); ctx.free()


@pytest.mark.parametrize("name", ["s128", "small", "w1280"])
def test_several_rows_pass_at_crafted_positions(wrs, amd_lib, name, monkeypatch):
    """The several-rows one-launch pass (wa_rows.hip, its own LayerNorm with mb_seq_sum): 2 rows and then 5 rows, every one at a crafted
    position, against the launch sequence; every pass served by the one-launch form.  As in the reference's API, get_logits_last(n) hands
    out the LAST row's logits only: positions 4 and 7 are compared directly, the other rows of a pass through that row's self-attention over
    the K / V they wrote."""
    ctx, ref, row = two_states(wrs, amd_lib, name, monkeypatch)
    assert amd_lib.whisper_amd_rows_enabled(row.ptr) == 1, "several-rows step not available"
    for n in (2, 5):
        ref.decode([CRAFT_TOK] * n, CRAFT_POS0); row.decode([CRAFT_TOK] * n, CRAFT_POS0)
        a = ref.get_logits_last(n); b = row.get_logits_last(n)
        assert digest(a) == digest(b), "%d rows: max|d| = %g" % (n, float(np.abs(a - b).max()))
    served, back = row.rows_stats()
    assert served == 3 and back == 0, (served, back)          # the prompt's three rows, then the 2 and the 5
    ref.free(); row.free(); ctx.free()

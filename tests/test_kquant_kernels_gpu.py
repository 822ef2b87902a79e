"""The kernels of wa_quantk.hip one by one - the Q8_K quantiser, the one-row and the 8-row product of Q5_K and Q6_K with every
epilogue, the token embedding - against the host reference (tests/native/kquant_ref.cpp = whisper-rust_amd/csrc/wa_quantk.h, which
tests/test_kquant_math.py holds to the reference library on the CPU), BIT FOR BIT.

Weights are raw blocks of random bytes (every quant, high-bit and scale-byte pattern) with d / dmin drawn as F16 values of both signs;
activation rows carry the rounding points of the quantiser: equal maxima of opposite sign in both orders, an all-zero block, a negative
maximum, products on a tie of nearest_int.  Shapes: K = 256, 512, 768, 1024, 5120; N = 1, 7, 8, 9, 64 output rows and the 51865 rows of
the logits at K = 256; M = 1, 2, 7, 8, 9, 13 activation rows (the one-row kernel, partial and several 8-row tiles).

The kernels are called through tests/native/libkquant_kernels.so, which whisper-rust_amd/Makefile links against the product's own
build/wa_quantk.o.  Every output buffer is filled with a sentinel first; padding (ldx > K, ldo > N, a row beyond M) must still hold it.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quant_cases as QC  # noqa: E402  (the epilogues' index maps, the GELU table and the bit comparisons are format-independent)

LIB_PATH = os.path.join(ROOT, "tests", "native", "libkquant_kernels.so")
REF_PATH = os.path.join(ROOT, "tests", "native", "libkquant_ref.so")
SENT8 = np.int8(-128)         # bit patterns no kernel result can have (a Q8_K quant is -127 .. 127, the others are NaNs with a payload)
SENT16 = np.uint16(0x7E5A)
SENT32 = np.uint32(0x7FC0DEAD)
BLOCK_BYTES = {13: 176, 14: 210}
KS = (256, 512, 768, 1024, 5120)
MS = (1, 2, 7, 8, 9, 13)
NS = (1, 7, 8, 9, 64)
vp, ci = C.c_void_p, C.c_int


class KtEpi(C.Structure):      # tests/native/kquant_kernels.hip: ktest_epi
    _fields_ = [("bias", vp), ("scale", vp), ("out", vp), ("ldo", ci), ("out2", vp), ("ldo2", ci), ("out3", vp), ("ldo3", ci), ("resid", vp), ("ldr", ci),
                ("gelu", vp), ("split0", ci), ("split1", ci), ("row_off", ci), ("aux0", ci), ("aux1", ci)]


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target kquant_harness)" % LIB_PATH
    L = C.CDLL(LIB_PATH)
    L.ktest_alloc.restype = vp; L.ktest_alloc.argtypes = [C.c_size_t]
    L.ktest_free.argtypes = [vp]
    L.ktest_h2d.argtypes = [vp, vp, C.c_size_t]; L.ktest_d2h.argtypes = [vp, vp, C.c_size_t]
    L.ktest_quantize_q8_K.argtypes = [vp, ci, ci, ci, vp, vp, vp]
    L.ktest_kgemm_exact.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, C.POINTER(KtEpi)]
    L.ktest_dec_embed_k.argtypes = [ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    return L


@functools.lru_cache(maxsize=None)
def ref():
    assert os.path.exists(REF_PATH), "%s missing: build() makes it" % REF_PATH
    R = C.CDLL(REF_PATH)
    R.kq_unpack_rows.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, ci]
    R.kq_q8_K_rows.argtypes = [vp, ci, ci, ci, vp, vp, vp, ci]
    R.kq_gemm.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci]
    R.kq_embed.argtypes = [ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    return R


def ptr(a):
    return a.ctypes.data


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().ktest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().ktest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().ktest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().ktest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().ktest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def assert_bits(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, bad.size, want.size, bad[0], int(got[bad[0]]) & 0xffffffff,
                                                                                   int(want[bad[0]]) & 0xffffffff)


# ----------------------------------------------------------------------------------------------------------------------------
# operands (made once per shape, shared by the tests, never changed)
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weights(wtype, N, K):
    """N rows of raw blocks -> the loader's arrays in the kernel layout: (qs, sc, d, dmin)."""
    rng = QC.rng_for("kquant_w_%d_%d_%d" % (wtype, N, K))
    nb, bsz = K // 256, BLOCK_BYTES[wtype]
    blk = rng.integers(0, 256, (N * nb, bsz), dtype=np.uint8)
    d16 = (rng.uniform(-1, 1, N * nb) * np.where(np.arange(N * nb) % 7 == 0, 3e-6, 2e-3)).astype(np.float16).view(np.uint16)
    m16 = (rng.uniform(-1, 1, N * nb) * np.where(np.arange(N * nb) % 5 == 0, 0.0, 1e-2)).astype(np.float16).view(np.uint16)
    if wtype == 13:
        blk[:, 0:2] = d16.view(np.uint8).reshape(-1, 2); blk[:, 2:4] = m16.view(np.uint8).reshape(-1, 2)
    else:
        blk[:, 208:210] = d16.view(np.uint8).reshape(-1, 2)
    qs, sc = np.empty((N, 8, nb, 8, 4), np.int8), np.empty((N, nb, 16), np.int8)
    d, dm = np.empty((N, nb), np.float32), np.empty((N, nb), np.float32)
    ref().kq_unpack_rows(wtype, N, K, ptr(blk), ptr(qs), ptr(sc), ptr(d), ptr(dm), 0)
    for a in (qs, sc, d, dm):
        a.setflags(write=False)
    return qs, sc, d, dm


@functools.lru_cache(maxsize=None)
def rows_f32(M, K):
    """M activation rows; their blocks rotate through the quantiser's rounding points."""
    rng = QC.rng_for("kquant_x_%d_%d" % (M, K))
    X = (rng.standard_normal((M, K)) * rng.choice([1.0, 37.5, 1e-3], (M, 1))).astype(np.float32)
    for m in range(M):
        for b in range(K // 256):
            xb = X[m, 256 * b: 256 * b + 256]
            kind = (m + 2 * b + 1) % 9
            if kind == 0:
                xb[:] = 0.0                                                  # an all-zero block: d = 0, quants and sums 0
            elif kind == 1:
                xb[:] *= 0.1 / max(1e-30, np.abs(xb).max()); xb[3] = 5.0; xb[100] = -5.0      # equal maxima, + first
            elif kind == 2:
                xb[:] *= 0.1 / max(1e-30, np.abs(xb).max()); xb[6] = -5.0; xb[7] = 5.0; xb[255] = -5.0     # ... - first, in one lane's four values and in the last lane
            elif kind == 3:
                xb[:] = (np.arange(256) % 120).astype(np.float32) + 0.5; xb[17] = -127.0      # iscale = 1: every product on a tie
            elif kind == 4:
                xb[:] = (2 * (np.arange(256) % 127) - 125).astype(np.float32); xb[200] = 254.0      # iscale = -0.5: ties, positive maximum
            elif kind == 5:
                xb[:] = -np.abs(xb); xb[255] = -9.0 * max(1.0, float(np.abs(xb).max()))       # a negative maximum in the last element
            elif kind == 6:
                xb[:] = np.where(np.arange(256) & 1, 3.0, -3.0)                               # every element holds the maximum: element 0 (-3) decides
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def activations(M, K):
    """The host's Q8_K rows of rows_f32(M, K): (qs layout, d, bsums)."""
    X = rows_f32(M, K)
    nb = K // 256
    qs, d, bs = np.empty((M, 8, nb, 8, 4), np.int8), np.empty((M, nb), np.float32), np.empty((M, nb, 16), np.int16)
    ref().kq_q8_K_rows(ptr(X), K, M, K, ptr(qs), ptr(d), ptr(bs), 0)
    for a in (qs, d, bs):
        a.setflags(write=False)
    return qs, d, bs


def host_gemm(wtype, M, N, K):
    wq, wsc, wd, wdm = weights(wtype, N, K)
    xq, xd, xbs = activations(M, K)
    out = np.empty((M, N), np.float32)
    ref().kq_gemm(wtype, M, N, K, ptr(wq), ptr(wsc), ptr(wd), ptr(wdm), ptr(xq), ptr(xd), ptr(xbs), ptr(out), 0)
    return out


def put_operands(dev, wtype, M, N, K):
    wq, wsc, wd, wdm = weights(wtype, N, K)
    xq, xd, xbs = activations(M, K)
    return (dev.put(xq), dev.put(xd), dev.put(xbs)), (dev.put(wq), dev.put(wsc), dev.put(wd), dev.put(wdm) if wtype == 13 else None)


# ----------------------------------------------------------------------------------------------------------------------------
# k_quantize_q8_K
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_quantize_q8_K(dev, K):
    """Rows with a stride ldx = K + 8 whose padding holds values far larger than the rows' (reading it would change a block's maximum);
    1, 7 and 13 rows end in a workgroup with idle waves.  The first index wins the arg-max on ties, opposite signs included."""
    nb = K // 256
    assert any(np.abs(rows_f32(13, K)[m, 256 * b: 256 * b + 256]).max() == 0 for m in range(13) for b in range(nb))
    for M in MS:
        X = rows_f32(M, K)
        Xp = np.full((M, K + 8), 3e38, np.float32)
        Xp[:, :K] = X
        q, d, bs = activations(M, K)
        p_q, p_d = dev.put(np.full(q.shape, SENT8, np.int8)), dev.put(np.full(d.shape, SENT32, np.uint32))
        p_bs = dev.put(np.full(bs.shape, -32768, np.int16))
        lib().ktest_quantize_q8_K(dev.put(Xp), K + 8, M, K, p_q, p_d, p_bs)
        sync()
        assert_bits(Dev.get(p_q, q), q, "quants M %d" % M)
        assert_bits(Dev.get(p_d, QC.bits32(d)), QC.bits32(d), "d M %d" % M)
        assert_bits(Dev.get(p_bs, bs), bs, "bsums M %d" % M)


# ----------------------------------------------------------------------------------------------------------------------------
# the products, WA_EPI_F32 without bias
# ----------------------------------------------------------------------------------------------------------------------------
def run_product(dev, wtype, M, N, K):
    ldo = N + 3
    want = np.full((M + 1, ldo), SENT32, np.uint32)            # one row beyond M
    want[:M, :N] = QC.bits32(host_gemm(wtype, M, N, K))
    p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
    x, w = put_operands(dev, wtype, M, N, K)
    e = KtEpi(out=p_out, ldo=ldo)
    lib().ktest_kgemm_exact(QC.F32, wtype, x[0], x[1], x[2], M, w[0], w[1], w[2], w[3], N, K, C.byref(e))
    sync()
    assert_bits(Dev.get(p_out, want), want, "type %d M %d N %d K %d" % (wtype, M, N, K))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("wtype", (13, 14), ids=("q5_K", "q6_K"))
def test_products(dev, wtype, K):
    """k_kgemv_exact (M = 1: N = 1, 7 fewer rows than a workgroup's 8, N = 9 a partial last workgroup) and k_kgemm_exact (M = 2, 7: one
    partial tile; 8; 9, 13: grid.y = 2 with a partial last tile; N = 1 .. 64: partial and two 32-row tiles).  K = 5120 with Q5_K is the
    largest activation tile: 46 720 B of LDS."""
    assert 8 * 5120 + 8 * 20 * 4 + 8 * 20 * 8 * 4 <= 48 * 1024
    for M in MS:
        for N in NS:
            run_product(dev, wtype, M, N, K)


@pytest.mark.parametrize("wtype", (13, 14), ids=("q5_K", "q6_K"))
def test_logits_product(dev, wtype):
    """The logits: the 51865 rows of the token embedding at K = 256, one row (the decode step) and five (a beam pass)."""
    for M in (1, 5):
        run_product(dev, wtype, M, 51865, 256)


# ----------------------------------------------------------------------------------------------------------------------------
# the epilogues
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (9, 1))
@pytest.mark.parametrize("wtype", (13, 14), ids=("q5_K", "q6_K"))
@pytest.mark.parametrize("epi", list(QC.EPI_MODES))
def test_epilogue(dev, epi, wtype, M):
    """M = 9 (k_kgemm_exact) and M = 1 (k_kgemv_exact), N = 70, K = 256: every value at the place the epilogue's index map gives it
    (wa_device.h: epi_apply), everything else still the sentinel."""
    N, K = 70, 256
    c = {"M": M, "N": N, "epi": epi}
    rng = QC.rng_for("kquant_epi_%s_%d_%d" % (epi, wtype, M))
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    scale = rng.uniform(0.25, 1.5, N).astype(np.float32) if epi in ("F16_scale", "DEC_QKV", "CROSS_KV") else None
    resid = (rng.standard_normal((M, N + 5)) * 2).astype(np.float32) if epi == "RESID" else None
    with np.errstate(over="ignore", invalid="ignore"):
        v = host_gemm(wtype, M, N, K) + bias[None, :]            # float32 throughout: one rounding per operation, as the kernel with contraction off
        if scale is not None:
            v = v * scale[None, :]
        if resid is not None:
            v = v + resid[:, :N]
        if epi == "GELU_F32":
            v = QC.gelu32(v)
        val = v.astype(np.float32).astype(np.float16).view(np.uint16) if epi in ("F16_scale", "ENC_QKV", "DEC_QKV", "CROSS_KV") else v.astype(np.float32)
    bufs, fields = QC.epi_layout(c)
    want = {name: np.full(n, SENT16 if t == "f16" else SENT32, np.uint16 if t == "f16" else np.uint32) for name, (n, t) in bufs.items()}
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    which, idx, names = QC.epi_out_index(c, fields, m, n)
    bits = val if val.dtype == np.uint16 else QC.bits32(val)
    for k, name in enumerate(names):
        sel = which == k
        assert np.unique(idx[sel]).size == np.count_nonzero(sel) and idx[sel].max() < want[name].size
        want[name][idx[sel]] = bits[sel]
    ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
    e = KtEpi(bias=dev.put(bias), scale=dev.put(scale) if scale is not None else None, resid=dev.put(resid) if resid is not None else None,
              gelu=dev.put(QC.GELU) if epi == "GELU_F32" else None, out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
    x, w = put_operands(dev, wtype, M, N, K)
    lib().ktest_kgemm_exact(QC.EPI_MODES[epi], wtype, x[0], x[1], x[2], M, w[0], w[1], w[2], w[3], N, K, C.byref(e))
    sync()
    for name, a in want.items():
        assert_bits(Dev.get(ptrs[name], a), a, "%s %s" % (epi, name))


# ----------------------------------------------------------------------------------------------------------------------------
# k_dec_embed_k
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (256, 768))
@pytest.mark.parametrize("wtype", (13, 14), ids=("q5_K", "q6_K"))
def test_token_embedding(dev, wtype, d):
    """Rows 0, 49 (the last) and repeats of a 50-row table at positions out of order: (d sc) q (- dmin m) + pe."""
    wq, wsc, wd, wdm = weights(wtype, 50, d)
    rng = QC.rng_for("kquant_embed_%d_%d" % (wtype, d))
    pe = rng.standard_normal((12, d)).astype(np.float32) * np.float32(1e-2)
    tok = np.array([0, 49, 7, 7, 23, 49, 1], np.int32)
    pos = np.array([5, 0, 11, 3, 3, 1, 2], np.int32)
    want = np.full((tok.size + 1, d), SENT32, np.uint32)
    out = np.empty((tok.size, d), np.float32)
    ref().kq_embed(wtype, tok.size, ptr(tok), ptr(pos), d, ptr(wq), ptr(wsc), ptr(wd), ptr(wdm), ptr(pe), ptr(out))
    want[:tok.size] = QC.bits32(out)
    p_x = dev.put(np.full_like(want, SENT32))
    lib().ktest_dec_embed_k(wtype, dev.put(tok), dev.put(pos), tok.size, d, dev.put(wq), dev.put(wsc), dev.put(wd), dev.put(wdm) if wtype == 13 else None,
                            dev.put(pe), p_x)
    sync()
    assert_bits(Dev.get(p_x, want), want, "embedding")

"""The kernels of wa_quantk.hip for Q2_K and Q3_K weights one by one - the one-row product, the 8-row product with each of the seven
epilogues, the token embedding - against the host statement (tests/native/kquant_ref.cpp = whisper-rust_amd/csrc/wa_quantk.h, which
tests/test_kquant23_math.py holds to the reference library on the CPU), BIT FOR BIT, through the K-format harness
(tests/native/libkquant_kernels.so, linked against the product's own wa_quantk.o and wa_quantk_q2.o).

Q2_K has instantiations of its own (the minimum term enters the lane accumulators before the product term); Q3_K, unpacked, runs the
Q6_K instantiations - one case holds the two weight types to identical output bits on the same arrays.

Weights are raw blocks of random bytes (every quant, high-bit, scale and minimum pattern) with d / dmin drawn as F16 values of both signs,
some tiny and some zero; activation rows carry the rounding points of the Q8_K quantiser (the rows of tests/test_kquant_kernels_gpu.py:
equal maxima of opposite sign in both orders, an all-zero block, a negative maximum, products on a tie of nearest_int).  Shapes: K = 256,
512, 768, 1024, 5120; N = 1, 7, 8, 9, 64 output rows and the 51865 rows of the logits at K = 256; M = 1, 2, 7, 8, 9, 13 activation rows.
Every output buffer is filled with a sentinel first; padding (ldo > N, a row beyond M) must still hold it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_kquant_kernels_gpu as KK      # the harness bindings, the device buffers and the activation rows: shared, computed once
from test_kquant_kernels_gpu import QC, Dev, KtEpi, assert_bits, dev, lib, ptr, ref, sync  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu

SENT16, SENT32 = KK.SENT16, KK.SENT32
BLOCK_BYTES = {10: 84, 11: 110}
D_AT = {10: 80, 11: 108}            # byte offset of the block's F16 d (Q2_K: dmin follows it)
KS, MS, NS = KK.KS, KK.MS, KK.NS
TYPES = pytest.mark.parametrize("wtype", (10, 11), ids=("q2_K", "q3_K"))


@functools.lru_cache(maxsize=None)
def weights(wtype, N, K):
    """N rows of raw blocks -> the loader's arrays in the kernel layout: (qs, sc, d, dmin)."""
    rng = QC.rng_for("kquant23_w_%d_%d_%d" % (wtype, N, K))
    nb, bsz = K // 256, BLOCK_BYTES[wtype]
    i = np.arange(N * nb)
    blk = rng.integers(0, 256, (N * nb, bsz), dtype=np.uint8)
    d16 = (rng.uniform(-1, 1, N * nb) * np.where(i % 7 == 0, 3e-6, np.where(i % 11 == 3, 0.0, 2e-3))).astype(np.float16).view(np.uint16)
    m16 = (rng.uniform(-1, 1, N * nb) * np.where(i % 5 == 0, 0.0, np.where(i % 13 == 4, 2e-6, 1e-2))).astype(np.float16).view(np.uint16)
    blk[:, D_AT[wtype]:D_AT[wtype] + 2] = d16.view(np.uint8).reshape(-1, 2)
    if wtype == 10:
        blk[:, 82:84] = m16.view(np.uint8).reshape(-1, 2)
    qs, sc = np.empty((N, 8, nb, 8, 4), np.int8), np.empty((N, nb, 16), np.int8)
    d, dm = np.empty((N, nb), np.float32), np.empty((N, nb), np.float32)
    ref().kq_unpack_rows(wtype, N, K, ptr(blk), ptr(qs), ptr(sc), ptr(d), ptr(dm), 0)
    if wtype == 10:
        assert qs.min() == 0 and qs.max() == 3
    else:
        assert qs.min() == -4 and qs.max() == 3 and sc.min() >= -32 and sc.max() <= 31
    for a in (qs, sc, d, dm):
        a.setflags(write=False)
    return qs, sc, d, dm


def host_gemm(wtype, M, N, K):
    wq, wsc, wd, wdm = weights(wtype, N, K)
    xq, xd, xbs = KK.activations(M, K)
    out = np.empty((M, N), np.float32)
    ref().kq_gemm(wtype, M, N, K, ptr(wq), ptr(wsc), ptr(wd), ptr(wdm), ptr(xq), ptr(xd), ptr(xbs), ptr(out), 0)
    return out


def put_operands(dev, wtype, M, N, K):
    wq, wsc, wd, wdm = weights(wtype, N, K)
    xq, xd, xbs = KK.activations(M, K)
    return (dev.put(xq), dev.put(xd), dev.put(xbs)), (dev.put(wq), dev.put(wsc), dev.put(wd), dev.put(wdm) if wtype == 10 else None)


def launch_f32(dev, wtype, x, w, M, N, K):
    """WA_EPI_F32 without bias into a sentinel-filled [M + 1][N + 3] buffer; returns its bits."""
    ldo = N + 3
    p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
    e = KtEpi(out=p_out, ldo=ldo)
    lib().ktest_kgemm_exact(QC.F32, wtype, x[0], x[1], x[2], M, w[0], w[1], w[2], w[3], N, K, C.byref(e))
    sync()
    return Dev.get(p_out, np.empty((M + 1, ldo), np.uint32))


def run_product(dev, wtype, M, N, K):
    want = np.full((M + 1, N + 3), SENT32, np.uint32)            # one row beyond M, three columns beyond N
    want[:M, :N] = QC.bits32(host_gemm(wtype, M, N, K))
    x, w = put_operands(dev, wtype, M, N, K)
    assert_bits(launch_f32(dev, wtype, x, w, M, N, K), want, "type %d M %d N %d K %d" % (wtype, M, N, K))


@pytest.mark.parametrize("K", KS)
@TYPES
def test_products(dev, wtype, K):
    """k_kgemv_exact (M = 1: N = 1, 7 fewer rows than a workgroup's 8, N = 9 a partial last workgroup) and k_kgemm_exact (M = 2, 7: one
    partial tile; 8; 9, 13: grid.y = 2 with a partial last tile; N = 1 .. 64: partial and two 32-row tiles).  K = 5120 with Q2_K is the
    largest activation tile (the rows and their sums): 46 720 B of LDS."""
    assert 8 * 5120 + 8 * 20 * 4 + 8 * 20 * 8 * 4 <= 48 * 1024
    for M in MS:
        for N in NS:
            run_product(dev, wtype, M, N, K)


@TYPES
def test_logits_product(dev, wtype):
    """The logits: the 51865 rows of the token embedding at K = 256, one row (the decode step) and five (a beam pass)."""
    for M in (1, 5):
        run_product(dev, wtype, M, 51865, 256)


def test_q3_K_runs_as_q6_K(dev):
    """A Q3_K weight and the Q6_K weight with the same unpacked arrays: identical output bits through the launchers, one-row and 8-row."""
    for M, N, K in ((1, 9, 768), (9, 64, 768), (13, 7, 5120)):
        x, w = put_operands(dev, 11, M, N, K)
        a, b = launch_f32(dev, 11, x, w, M, N, K), launch_f32(dev, 14, x, w, M, N, K)
        assert (a[:M, :N] != SENT32).all()
        assert_bits(a, b, "Q3_K against Q6_K M %d N %d K %d" % (M, N, K))


@pytest.mark.parametrize("M", (9, 1))
@TYPES
@pytest.mark.parametrize("epi", list(QC.EPI_MODES))
def test_epilogue(dev, epi, wtype, M):
    """M = 9 (k_kgemm_exact) and M = 1 (k_kgemv_exact), N = 70, K = 256: every value at the place the epilogue's index map gives it
    (wa_device.h: epi_apply), everything else still the sentinel."""
    N, K = 70, 256
    c = {"M": M, "N": N, "epi": epi}
    rng = QC.rng_for("kquant23_epi_%s_%d_%d" % (epi, wtype, M))
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


@pytest.mark.parametrize("d", (256, 768))
@TYPES
def test_token_embedding(dev, wtype, d):
    """Rows 0, 49 (the last) and repeats of a 50-row table at positions out of order: (d sc) q (- dmin m) + pe."""
    wq, wsc, wd, wdm = weights(wtype, 50, d)
    rng = QC.rng_for("kquant23_embed_%d_%d" % (wtype, d))
    pe = rng.standard_normal((12, d)).astype(np.float32) * np.float32(1e-2)
    tok = np.array([0, 49, 7, 7, 23, 49, 1], np.int32)
    pos = np.array([5, 0, 11, 3, 3, 1, 2], np.int32)
    want = np.full((tok.size + 1, d), SENT32, np.uint32)
    out = np.empty((tok.size, d), np.float32)
    ref().kq_embed(wtype, tok.size, ptr(tok), ptr(pos), d, ptr(wq), ptr(wsc), ptr(wd), ptr(wdm), ptr(pe), ptr(out))
    want[:tok.size] = QC.bits32(out)
    p_x = dev.put(np.full_like(want, SENT32))
    lib().ktest_dec_embed_k(wtype, dev.put(tok), dev.put(pos), tok.size, d, dev.put(wq), dev.put(wsc), dev.put(wd), dev.put(wdm) if wtype == 10 else None,
                            dev.put(pe), p_x)
    sync()
    assert_bits(Dev.get(p_x, want), want, "embedding")

"""The int8 matrix-core kernel of the K formats (whisper-rust_amd/csrc/wa_quantk_mfma.hip: k_kgemm_mfma, M > 8 activation rows,
v_mfma_i32_16x16x4_4b_i8 with slot = lane-sum index within a half and one sub-block scale per lane and instruction) on its own, BIT FOR BIT.
No tolerance anywhere in this file.

Every product runs through tests/native/libkquant_mfma.so (linked against the product's own wa_quantk_mfma.o, wa_quantk.o and wa_quantk_q2.o),
whose kmtest_kgemm hands its route to wa_launch_kgemm_route unchanged: route 3, k_kgemm_mfma, and route 1, the general kernel k_kgemm_exact.
Both are compared with the host reference tests/native/libkquant_ref.so (kq_gemm, variant 0, which tests/test_kquant_math.py and
tests/test_kquant23_math.py hold to the reference library on the CPU).

Operands are those of tests/test_kquant_kernels_gpu.py / test_kquant23_kernels_gpu.py: raw blocks of random bytes with F16 d / dmin of both
signs, activation rows with the quantiser's rounding points.  Shapes, the smallest that can go wrong: M = 9 (the smallest routed: one partial
16-row tile), 16 (exactly one tile), 17 (a tile and a one-row tile), 40 (two tiles and half of one); N = 16 (one column tile), 40 (a partial
column tile), 264 (several, a partial last one); nb = K / 256 = 1 .. 5 and 20 (K = 5120 is fc2 at d = 1280) - the kernel has ONE loop over the
blocks, with the next block's loads clamped to the last, so no block count changes its form; nb = 1 is the loop whose prefetch is all clamped.
Grids this small take the one-row-per-lane form (four waves share a tile); test_four_rows_per_lane holds the other form at 513 x 1000 and
test_both_forms_at_the_threshold the two forms on either side of the 128 workgroups from which the launcher takes it.
Output buffers are filled with a sentinel first; the row beyond M, the columns beyond N and the padding must still hold it.

The operand-role case is the in-product twin of tools/micro/mfma_i8_blocks.hip: small integer quants, distinct sub-block scales per group and
half and power-of-two d (dmin) built so that the exact result - stated in closed form, independent of any summation order - names a swapped
row, column, block, group, half or scale byte.

Which kernel a route takes is asked of kmtest_kernel (the kernels give the same bits, so results cannot tell)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import test_kquant_kernels_gpu as KK      # the reference bindings, the activation rows and the Q5_K / Q6_K weights: shared, computed once
import test_kquant23_kernels_gpu as K23   # the Q2_K / Q3_K weights
from test_kquant_kernels_gpu import QC, assert_bits, ptr, ref

pytestmark = pytest.mark.gpu

LIB_PATH = os.path.join(KK.ROOT, "tests", "native", "libkquant_mfma.so")
SENT16, SENT32 = KK.SENT16, KK.SENT32
ROUTES = {"k_kgemm_mfma": 3, "k_kgemm_exact": 1}
WTYPES = {10: "q2_K", 11: "q3_K", 13: "q5_K", 14: "q6_K"}
TYPES = pytest.mark.parametrize("wtype", list(WTYPES), ids=list(WTYPES.values()))
TYPES3 = pytest.mark.parametrize("wtype", (14, 13, 10), ids=("q6_K", "q5_K", "q2_K"))       # the three instantiated formats (Q3_K runs as Q6_K)
MS, NS, NBS = (9, 16, 17, 40), (16, 40, 264), (1, 2, 3, 4, 5, 20)
vp, ci = C.c_void_p, C.c_int


class KmEpi(C.Structure):      # tests/native/kquant_mfma.hip: kmtest_epi
    _fields_ = [("bias", vp), ("scale", vp), ("out", vp), ("ldo", ci), ("out2", vp), ("ldo2", ci), ("out3", vp), ("ldo3", ci), ("resid", vp), ("ldr", ci),
                ("gelu", vp), ("split0", ci), ("split1", ci), ("row_off", ci), ("aux0", ci), ("aux1", ci)]


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target kquant_harness)" % LIB_PATH
    L = C.CDLL(LIB_PATH)
    L.kmtest_alloc.restype = vp; L.kmtest_alloc.argtypes = [C.c_size_t]
    L.kmtest_free.argtypes = [vp]
    L.kmtest_h2d.argtypes = [vp, vp, C.c_size_t]; L.kmtest_d2h.argtypes = [vp, vp, C.c_size_t]
    L.kmtest_kgemm.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, C.POINTER(KmEpi)]
    L.kmtest_kernel.argtypes = [ci] * 7
    return L


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().kmtest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().kmtest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().kmtest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().kmtest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().kmtest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def has_min(wtype):
    return wtype in (13, 10)


def weights(wtype, N, K):
    return (KK if wtype in (13, 14) else K23).weights(wtype, N, K)


@functools.lru_cache(maxsize=None)
def host_gemm(wtype, M, N, K):
    out = (KK if wtype in (13, 14) else K23).host_gemm(wtype, M, N, K)
    out.setflags(write=False)
    return out


def put_arrays(dev, wtype, w, x):
    """(xq, xd, xbs), (wq, wsc, wd, wdm or null) on the device."""
    return [dev.put(a) for a in x], [dev.put(w[0]), dev.put(w[1]), dev.put(w[2]), dev.put(w[3]) if has_min(wtype) else None]


def launch(route, mode, wtype, x, w, M, N, K, e):
    lib().kmtest_kgemm(route, mode, wtype, x[0], x[1], x[2], M, w[0], w[1], w[2], w[3], N, K, C.byref(e))
    sync()


def both_routes_f32(dev, wtype, w, x, M, N, K, expected, what):
    """WA_EPI_F32 without bias through route 3 and route 1 into sentinel-filled [M + 1][N + 3] buffers: both hold `expected` and the sentinel elsewhere."""
    ldo = N + 3
    want = np.full((M + 1, ldo), SENT32, np.uint32)            # one row beyond M, three columns beyond N
    want[:M, :N] = QC.bits32(expected)
    xp, wp = put_arrays(dev, wtype, w, x)
    for kernel, route in ROUTES.items():
        assert lib().kmtest_kernel(route, QC.F32, wtype, M, N, K, 0) == route, "%s is not what route %d takes for %s" % (kernel, route, what)
        p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
        launch(route, QC.F32, wtype, xp, wp, M, N, K, KmEpi(out=p_out, ldo=ldo))
        assert_bits(Dev.get(p_out, want), want, "%s %s" % (kernel, what))


# ----------------------------------------------------------------------------------------------------------------------------
# the products, WA_EPI_F32 without bias: both kernels against the host reference
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", NBS, ids=["K%d" % (256 * nb) for nb in NBS])
@TYPES
def test_matrix_core_product(wtype, nb):
    """M = 9, 16, 17, 40 x N = 16, 40, 264 at one K and format: k_kgemm_mfma and k_kgemm_exact both give the host reference's bits."""
    K = 256 * nb
    for M in MS:
        for N in NS:
            shape_dev = Dev()            # this shape's buffers, freed before the next shape
            try:
                both_routes_f32(shape_dev, wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K, host_gemm(wtype, M, N, K),
                                "%s M %d N %d K %d" % (WTYPES[wtype], M, N, K))
            finally:
                shape_dev.close()


@pytest.mark.parametrize("nb", (1, 3), ids=("K256", "K768"))
@TYPES3
def test_four_rows_per_lane(dev, wtype, nb):
    """The form with four rows per lane and one column tile per wave (the encoder's shapes): M = 513 (32 row tiles and a one-row tile) x N = 1000
    (15 workgroups and one with 40 columns: a partial wave and an idle one), 33 x 16 = 528 workgroups of 64 columns x 16 rows."""
    M, N, K = 513, 1000, 256 * nb
    assert ((N + 63) // 64) * ((M + 15) // 16) == 528
    both_routes_f32(dev, wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K, host_gemm(wtype, M, N, K), "%s 513 x 1000 K %d" % (WTYPES[wtype], K))


@TYPES3
def test_both_forms_at_the_threshold(dev, wtype):
    """The launcher takes the four-rows form from 128 workgroups of 64 columns x 16 rows on (wa_quantk_mfma.hip: kmfma_wide): M = 127 x N = 1000 is
    8 x 16 = 128 of them, the smallest grid that does; M = 112 x N = 1000 is 7 x 16 = 112, the one-row form with 7 x 63 tiles - many more than
    the shapes of test_matrix_core_product give it."""
    for M in (127, 112):
        N, K = 1000, 512
        both_routes_f32(dev, wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K, host_gemm(wtype, M, N, K), "%s %d x 1000 K 512" % (WTYPES[wtype], M))


# ----------------------------------------------------------------------------------------------------------------------------
# operand roles: integers and powers of two, the exact result in closed form
# ----------------------------------------------------------------------------------------------------------------------------
ROLE_M, ROLE_N = 17, 48


@functools.lru_cache(maxsize=None)
def role_case(wtype, nb):
    """Arrays in element order - x [m][b][g][l][4], w [n][b][g][l][4] (element 32 g + 4 l + i of block b), scales s [n][b][h][g] (sub-block
    2 g + h), minimums mn [n][b][h][g] (Q5_K: [n][b][0][g]) - and the power-of-two d:
      x: one byte (byte m % 4 of the quad) of 1 + (m + l + 2 g + b) % 19, w: four bytes of 1 + (n + 2 l + g + 2 b) % 3;
      scales: Q6_K the 16 values -8 .. -1, 1 .. 8, Q2_K the 16 nibbles 0 .. 15, both rotated by n + b over the 16 (half, group) places - every
      place of a block a different one; Q5_K 1 .. 8 rotated over the 8 groups; minimums likewise, with another stride;
      dx[m][b] = 2^(m - 16), dw[n][b] = 2^(-n - b % 4), dmin = dw / 4.
    Every term of an output is then an integer multiple of 2^(m - n - 21) and their magnitudes sum to far less than 2^24 of that (asserted
    by role_expected): every partial sum is exact in F32, in any order."""
    M, N = ROLE_M, ROLE_N
    m, n = np.arange(M), np.arange(N)
    b, g, l, h = np.arange(nb), np.arange(8), np.arange(8), np.arange(2)
    x = np.zeros((M, nb, 8, 8, 4), np.int64)
    xv = 1 + (m[:, None, None, None] + l[None, None, None, :] + 2 * g[None, None, :, None] + b[None, :, None, None]) % 19
    for mm in range(M):
        x[mm, :, :, :, mm % 4] = xv[mm]
    w = np.empty((N, nb, 8, 8, 4), np.int64)
    w[:] = (1 + (n[:, None, None, None] + 2 * l[None, None, None, :] + g[None, None, :, None] + 2 * b[None, :, None, None]) % 3)[..., None]
    place = 8 * h[None, None, :, None] + g[None, None, None, :]                       # [1][1][h][g]
    rot = (n[:, None, None, None] + b[None, :, None, None])
    if wtype == 14:
        s = np.array([-8, -7, -6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6, 7, 8])[(3 * place + rot) % 16]
        mn = np.zeros_like(s)
    elif wtype == 10:
        s = (3 * place + rot) % 16
        mn = (5 * place + rot + b[None, :, None, None] + 1) % 16
    else:
        s = np.broadcast_to(1 + (3 * g[None, None, None, :] + rot) % 8, (N, nb, 2, 8)).copy()         # one scale per group: both halves
        mn = np.broadcast_to(1 + (5 * g[None, None, None, :] + rot + b[None, :, None, None]) % 8, (N, nb, 2, 8)).copy()
    dx = np.broadcast_to(2.0 ** (m[:, None] - 16.0), (M, nb)).astype(np.float32)
    dw = (2.0 ** (-n[:, None] - (b[None, :] % 4).astype(np.float64))).astype(np.float32)
    dm = (dw / 4).astype(np.float32) if has_min(wtype) else np.zeros_like(dw)
    return x, w, s, mn, dx, dw, dm


def role_expected(wtype, nb, mutate=None):
    """The closed form, in exact float64 arithmetic over integers and powers of two:
        out[m][n] = sum_b dx dw sum_{g, l} s[n][b][l / 4][g] sum_i w x  -  sum_b dx dmin (the minimums against the 16-element sums of x)
    Q2_K: sum_{h, g} mn[h][g] bsum[2 g + h]; Q5_K: sum_g mn[g] (bsum[2 g] + bsum[2 g + 1]).  `mutate` names a wrong role taken on the weight
    side (test_role_operands_name_every_role shows that each one changes outputs)."""
    x, w, s, mn, dx, dw, dm = role_case(wtype, nb)
    if mutate == "halves":
        s = s[:, :, ::-1, :]
    elif mutate == "groups":
        s = np.roll(s, 1, axis=3)
    elif mutate == "scale blocks":
        s = np.roll(s, 1, axis=1)
    elif mutate == "quant blocks":
        w = np.roll(w, 1, axis=1)
    elif mutate == "quant groups":
        w = np.roll(w, 1, axis=2)
    elif mutate == "lane sums":
        w = np.roll(w, 1, axis=3)
    elif mutate == "columns":
        w, s, mn = np.roll(w, 1, axis=0), np.roll(s, 1, axis=0), np.roll(mn, 1, axis=0)
    elif mutate == "rows":
        x = np.roll(x, 1, axis=0)
    elif mutate == "minimum halves":
        mn = mn[:, :, ::-1, :]
    elif mutate == "minimum groups":
        mn = np.roll(mn, 1, axis=3)
    elif mutate == "minimum for scale":
        s, mn = mn, s
    else:
        assert mutate is None
    dot = np.einsum("mbgli,nbgli->mnbgl", x, w)                                       # the 4-element dot products
    sl = np.stack([s[:, :, ll // 4, :] for ll in range(8)], axis=-1)                  # [n][b][g][l]: the scale of lane sum l's group g
    t = np.einsum("mnbgl,nbgl->mnb", dot, sl)
    bsum = x.reshape(ROLE_M, nb, 8, 2, 16).sum(-1)                                    # [m][b][g][h]: elements 32 g + 16 h ..
    if wtype == 10:
        mins = np.einsum("mbgh,nbhg->mnb", bsum, mn)
    else:
        mins = np.einsum("mbg,nbg->mnb", bsum.sum(-1), mn[:, :, 0, :])
    dd = dx.astype(np.float64)[:, None, :] * dw.astype(np.float64)[None, :, :]
    dn = dx.astype(np.float64)[:, None, :] * dm.astype(np.float64)[None, :, :]
    out = (dd * t).sum(-1) - (dn * mins).sum(-1)
    if mutate is None:
        unit = 2.0 ** (np.arange(ROLE_M)[:, None] - np.arange(ROLE_N)[None, :] - 21.0)
        terms = np.abs(dd[:, :, :, None, None] * dot * np.abs(sl)[None]).sum((2, 3, 4)) + (dn * np.abs(mins)).sum(-1)
        assert np.all(terms / unit < 2.0 ** 24), (terms / unit).max()
        assert np.array_equal(out, out.astype(np.float32).astype(np.float64)) and np.unique(out).size == out.size
    return out.astype(np.float32)


def role_arrays(wtype, nb):
    """role_case in the kernel layout: (xq, xd, xbs), (wq, wsc, wd, wdm)."""
    x, w, s, mn, dx, dw, dm = role_case(wtype, nb)
    xq = np.ascontiguousarray(x.transpose(0, 3, 1, 2, 4)).astype(np.int8)             # [row][l][b][g][4]
    wq = np.ascontiguousarray(w.transpose(0, 3, 1, 2, 4)).astype(np.int8)
    xbs = np.ascontiguousarray(x.reshape(ROLE_M, nb, 8, 2, 16).sum(-1).reshape(ROLE_M, nb, 16)).astype(np.int16)      # sub-block 2 g + h
    if wtype == 13:
        sc = np.concatenate([s[:, :, 0, :], mn[:, :, 0, :]], axis=-1)                 # the 8 scales, then the 8 minimums
    elif wtype == 10:
        sc = (s | (mn << 4)).reshape(ROLE_N, nb, 16)                                   # byte 8 h + g: sub-block 2 g + h
    else:
        sc = s.reshape(ROLE_N, nb, 16)
    wsc = sc.astype(np.uint8).view(np.int8) if wtype != 14 else sc.astype(np.int8)
    return (xq, dx.copy(), xbs), (wq, np.ascontiguousarray(wsc), dw.copy(), dm.copy())


MUTATIONS = ("halves", "groups", "scale blocks", "quant blocks", "quant groups", "lane sums", "columns", "rows")
MIN_MUTATIONS = ("minimum halves", "minimum groups", "minimum for scale")


@pytest.mark.parametrize("nb", (8, 9))
@TYPES3
def test_operand_roles(dev, wtype, nb):
    """The exact result of an integer / power-of-two product in which every (row, column, lane-sum index, group) has a term of its own: the
    closed form equals the host reference, every wrong role changes it, and both kernels give it."""
    want = role_expected(wtype, nb)
    x, w = role_arrays(wtype, nb)
    host = np.empty((ROLE_M, ROLE_N), np.float32)
    ref().kq_gemm(wtype, ROLE_M, ROLE_N, 256 * nb, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(x[0]), ptr(x[1]), ptr(x[2]), ptr(host), 0)
    assert_bits(QC.bits32(host), QC.bits32(want), "the host reference on the role operands")
    for mutation in MUTATIONS + (MIN_MUTATIONS if has_min(wtype) else ()):
        if wtype == 13 and mutation in ("halves", "minimum halves"):
            continue                                             # Q5_K has one scale and one minimum per group, none per half
        moved = role_expected(wtype, nb, mutation) != want
        assert moved.mean() > 0.9, "taking the wrong %s changes only %d of %d outputs" % (mutation, moved.sum(), moved.size)
    both_routes_f32(dev, wtype, w, x, ROLE_M, ROLE_N, 256 * nb, want, "operand roles %s nb %d" % (WTYPES[wtype], nb))


# ----------------------------------------------------------------------------------------------------------------------------
# every epilogue mode of the launcher at M 17, N 48, K 256 and 768: route 3 = route 1 in every output buffer
# ----------------------------------------------------------------------------------------------------------------------------
EPI_M, EPI_N, EPI_TPAD = 17, 48, 24


def epi_fields(epi):
    """Output buffers name -> (element count, 'f16' | 'f32') and the launch's scalar fields for M = 17, N = 48."""
    M, N = EPI_M, EPI_N
    if epi in ("F32_bias", "RESID", "GELU_F32"):
        return {"out": (M * (N + 6), "f32")}, {"ldo": N + 6, "ldr": N + 5 if epi == "RESID" else 0}
    if epi == "F16_scale":
        return {"out": (M * (N + 6), "f16")}, {"ldo": N + 6}
    if epi == "ENC_QKV":
        return {"out": (M * 24, "f16"), "out2": ((N - 20) * (M + 7), "f16")}, {"ldo": 24, "split0": 20, "ldo2": M + 7}
    if epi == "DEC_QKV":
        return ({"out": (M * 18, "f16"), "out2": ((3 + M + 1) * 18, "f16"), "out3": ((3 + M + 1) * 20, "f16")},
                {"ldo": 18, "split0": 16, "split1": 32, "row_off": 3, "ldo2": 18, "ldo3": 20})
    if epi == "CROSS_KV":       # d = 64, N = 48: the K of layer 0, head 0
        return {"out": (EPI_TPAD * 64, "f16"), "out2": (EPI_TPAD * 64, "f16")}, {"aux0": EPI_TPAD, "aux1": 64}
    raise ValueError(epi)


@pytest.mark.parametrize("K", (256, 768))
@TYPES
@pytest.mark.parametrize("epi", list(QC.EPI_MODES))
def test_epilogue_modes(dev, epi, wtype, K):
    """Every mode wa_launch_kgemm_route has a case for: route 3 equals route 1 bit for bit in every output buffer - and both hold every value
    at the place the epilogue's index map gives it (wa_device.h: epi_apply), everything else still the sentinel."""
    M, N = EPI_M, EPI_N
    rng = QC.rng_for("kquant_mfma_epi_%s_%d_%d" % (epi, wtype, K))
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    scale = rng.uniform(0.25, 1.5, N).astype(np.float32) if epi in ("F16_scale", "DEC_QKV", "CROSS_KV") else None
    resid = (rng.standard_normal((M, N + 5)) * 2).astype(np.float32) if epi == "RESID" else None
    with np.errstate(over="ignore", invalid="ignore"):
        v = host_gemm(wtype, M, N, K) + bias[None, :]            # float32 throughout: one rounding per operation, as the kernels with contraction off
        if scale is not None:
            v = v * scale[None, :]
        if resid is not None:
            v = v + resid[:, :N]
        if epi == "GELU_F32":
            v = QC.gelu32(v)
        val = v.astype(np.float32).astype(np.float16).view(np.uint16) if epi in ("F16_scale", "ENC_QKV", "DEC_QKV", "CROSS_KV") else QC.bits32(v.astype(np.float32))
    bufs, fields = epi_fields(epi)
    want = {name: np.full(n, SENT16 if t == "f16" else SENT32, np.uint16 if t == "f16" else np.uint32) for name, (n, t) in bufs.items()}
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    which, idx, names = QC.epi_out_index({"epi": epi}, fields, m, n)
    for k, name in enumerate(names):
        sel = which == k
        if not np.any(sel):
            continue
        assert np.unique(idx[sel]).size == np.count_nonzero(sel) and idx[sel].max() < want[name].size
        want[name][idx[sel]] = val[sel]
    xp, wp = put_arrays(dev, wtype, weights(wtype, N, K), KK.activations(M, K))
    p_bias, p_scale = dev.put(bias), dev.put(scale) if scale is not None else None
    p_resid, p_gelu = dev.put(resid) if resid is not None else None, dev.put(QC.GELU) if epi == "GELU_F32" else None
    got = {}
    for kernel, route in ROUTES.items():
        assert lib().kmtest_kernel(route, QC.EPI_MODES[epi], wtype, M, N, K, 0) == route
        ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
        e = KmEpi(bias=p_bias, scale=p_scale, resid=p_resid, gelu=p_gelu, out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
        launch(route, QC.EPI_MODES[epi], wtype, xp, wp, M, N, K, e)
        got[kernel] = {name: Dev.get(ptrs[name], a) for name, a in want.items()}
    for name, a in want.items():
        assert np.array_equal(got["k_kgemm_mfma"][name], got["k_kgemm_exact"][name]), "%s %s K %d: %s of the two kernels differs" % (epi, WTYPES[wtype], K, name)
        assert_bits(got["k_kgemm_mfma"][name], a, "k_kgemm_mfma %s %s K %d %s" % (epi, WTYPES[wtype], K, name))


# ----------------------------------------------------------------------------------------------------------------------------
# route selection
# ----------------------------------------------------------------------------------------------------------------------------
@TYPES
def test_route_selection(dev, wtype):
    """Route 3 and route 0 never take the matrix-core kernel at M = 1, 2, 5, 8; route 3 does at M = 9 and route 1 never; with rows of different
    states (wa_epi::rowp) neither route 0 nor route 3 does.  Route 0 at 9 rows and more is the measured default rule: the
    matrix-core kernel for every class of products - the suite runs without WHISPER_AMD_NO_QMFMA.  A 5-row product through route 3 gives the
    reference's bits."""
    assert os.environ.get("WHISPER_AMD_NO_QMFMA") is None, "the suite runs with the default routing"
    k = lib().kmtest_kernel
    for mode in (QC.F32, QC.DEC_QKV, QC.ENC_QKV):
        for M in (1, 2, 5, 8):
            assert k(3, mode, wtype, M, 264, 768, 0) == 1 and k(0, mode, wtype, M, 264, 768, 0) == 1, (M, mode)
        for M, N, K in ((9, 264, 768), (40, 768, 768), (1500, 768, 768), (1500, 3072, 768), (1500, 5120, 1280), (200, 51865, 768)):
            assert k(3, mode, wtype, M, N, K, 0) == 3 and k(1, mode, wtype, M, N, K, 0) == 1, (M, N, K, mode)
            assert k(0, mode, wtype, M, N, K, 0) == 3, (M, N, K, mode)
            assert k(3, mode, wtype, M, N, K, 1) == 1 and k(0, mode, wtype, M, N, K, 1) == 1, (M, N, K, mode)
    M, N, K = 5, 40, 768
    want = np.full((M + 1, N + 3), SENT32, np.uint32)
    want[:M, :N] = QC.bits32(host_gemm(wtype, M, N, K))
    xp, wp = put_arrays(dev, wtype, weights(wtype, N, K), KK.activations(M, K))
    p_out = dev.put(np.full_like(want, SENT32))
    launch(3, QC.F32, wtype, xp, wp, M, N, K, KmEpi(out=p_out, ldo=N + 3))
    assert_bits(Dev.get(p_out, want), want, "route 3 at M = 5 (%s)" % WTYPES[wtype])

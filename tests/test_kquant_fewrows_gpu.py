"""The few-rows kernel of the K formats (whisper-rust_amd/csrc/wa_quantk_rows.hip: k_kgemv_rows, M = 2..8 activation rows, one wave per 8 output
rows, the weight loads of four blocks in flight) on its own, BIT FOR BIT.  No tolerance anywhere in this file.

Every product runs through tests/native/libkquant_rows.so (linked against the product's own wa_quantk_rows.o, wa_quantk_mfma.o, wa_quantk.o and
wa_quantk_q2.o), whose krtest_kgemm hands its route to wa_launch_kgemm_few_route unchanged: route 2, k_kgemv_rows, and route 1, the general kernel
k_kgemm_exact.  Both are compared with the host reference tests/native/libkquant_ref.so (kq_gemm, variant 0, which tests/test_kquant_math.py and
tests/test_kquant23_math.py hold to the reference library on the CPU).

Operands are those of tests/test_kquant_kernels_gpu.py / test_kquant23_kernels_gpu.py: raw blocks of random bytes with F16 d / dmin of both signs,
activation rows with the quantiser's rounding points.  Shapes, the smallest that can go wrong: every M = 2..8 (one instantiation each) at K = 256,
N = 9; M = 2, 5, 8 at N = 1, 7 (fewer rows than a wave's eight), 8, 9 (a partial last wave), 264 (many waves) and nb = K / 256 = 1, 3 (shorter
than the prefetch depth of four, odd), 5 (one full round and one block) and 20 (the longest row, five full rounds).
Output buffers are filled with a sentinel first; the row beyond M and the columns beyond N (ldo > N) must still hold it.

Which kernel a route takes is asked of krtest_kernel (the kernels give the same bits, so results cannot tell)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_kquant_kernels_gpu as KK      # the reference bindings, the activation rows and the Q5_K / Q6_K weights: shared, computed once
import test_kquant23_kernels_gpu as K23   # the Q2_K / Q3_K weights
from test_kquant_kernels_gpu import QC, assert_bits, ptr, ref

pytestmark = pytest.mark.gpu

LIB_PATH = os.path.join(KK.ROOT, "tests", "native", "libkquant_rows.so")
SENT16, SENT32 = KK.SENT16, KK.SENT32
ROUTES = {"k_kgemv_rows": 2, "k_kgemm_exact": 1}
WTYPES = {14: "q6_K", 13: "q5_K", 10: "q2_K", 11: "q3_K"}
TYPES = pytest.mark.parametrize("wtype", list(WTYPES), ids=list(WTYPES.values()))
TYPES3 = pytest.mark.parametrize("wtype", (14, 13, 10), ids=("q6_K", "q5_K", "q2_K"))       # the three instantiated formats (Q3_K runs as Q6_K)
FEW_EPILOGUES = {"F16_scale": QC.F16, "GELU_F32": QC.GELU_F32, "RESID": QC.RESID, "F32_bias": QC.F32, "DEC_QKV": QC.DEC_QKV}      # the decoder's five
# The default rule (wa_quantk_rows.hip: kfew_rule), mirrored: the (weight type, row count, model width d) classes route 0 gives to k_kgemv_rows in the five
# epilogues.  DESIGN.md 4.3 ("K formats: a product kernel for 2..8 rows") has the measured table behind it: 2..7 rows at every width, 8 rows at d = 768 only.
WIDTHS = (256, 512, 768, 1024, 1280)          # the widths a K format can hold (d % 256 == 0)
FEW_CLASSES = [(wtype, M, d) for wtype in (10, 11, 13, 14) for d in WIDTHS for M in range(2, 9) if M <= 7 or d == 768]
vp, ci = C.c_void_p, C.c_int


class KrEpi(C.Structure):      # tests/native/kquant_rows.hip: krtest_epi
    _fields_ = [("bias", vp), ("scale", vp), ("out", vp), ("ldo", ci), ("out2", vp), ("ldo2", ci), ("out3", vp), ("ldo3", ci), ("resid", vp), ("ldr", ci),
                ("gelu", vp), ("split0", ci), ("split1", ci), ("row_off", ci), ("aux0", ci), ("aux1", ci), ("rowp", vp), ("rowp_off", C.c_longlong)]


ROWPTR = np.dtype([("kv_k", "<u8"), ("kv_v", "<u8"), ("cross_k", "<u8"), ("cross_v", "<u8"), ("n_kv", "<i4"), ("kv_head", "<i4")])      # wa_kernels.h: wa_rowptr


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target kquant_harness)" % LIB_PATH
    L = C.CDLL(LIB_PATH)
    L.krtest_alloc.restype = vp; L.krtest_alloc.argtypes = [C.c_size_t]
    L.krtest_free.argtypes = [vp]
    L.krtest_h2d.argtypes = [vp, vp, C.c_size_t]; L.krtest_d2h.argtypes = [vp, vp, C.c_size_t]
    L.krtest_kgemm.argtypes = [ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, C.POINTER(KrEpi)]
    L.krtest_kernel.argtypes = [ci] * 7
    L.krtest_q2_host.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci]
    assert L.krtest_rowptr_bytes() == ROWPTR.itemsize
    return L


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().krtest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().krtest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().krtest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().krtest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().krtest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def has_min(wtype):
    return wtype in (13, 10)


def weights(wtype, N, K):
    return (KK if wtype in (13, 14) else K23).weights(wtype, N, K)


def gemm_of(wtype, w, x, M, N, K):
    """The host reference's product of the arrays w = (qs, sc, d, dmin) and x = (qs, d, bsums)."""
    out = np.empty((M, N), np.float32)
    ref().kq_gemm(wtype, M, N, K, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(x[0]), ptr(x[1]), ptr(x[2]), ptr(out), 0)
    return out


@functools.lru_cache(maxsize=None)
def host_gemm(wtype, M, N, K):
    out = gemm_of(wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K)
    out.setflags(write=False)
    return out


def put_arrays(dev, wtype, w, x):
    """(xq, xd, xbs), (wq, wsc, wd, wdm or null) on the device."""
    return [dev.put(a) for a in x], [dev.put(w[0]), dev.put(w[1]), dev.put(w[2]), dev.put(w[3]) if has_min(wtype) else None]


def launch(route, mode, wtype, x, w, M, N, K, e):
    lib().krtest_kgemm(route, mode, wtype, x[0], x[1], x[2], M, w[0], w[1], w[2], w[3], N, K, C.byref(e))
    sync()


def both_routes_f32(dev, wtype, w, x, M, N, K, expected, what, routes=ROUTES):
    """WA_EPI_F32 without bias through route 2 and route 1 into sentinel-filled [M + 1][N + 3] buffers: both hold `expected` and the sentinel elsewhere."""
    ldo = N + 3
    want = np.full((M + 1, ldo), SENT32, np.uint32)            # one row beyond M, three columns beyond N
    want[:M, :N] = QC.bits32(expected)
    xp, wp = put_arrays(dev, wtype, w, x)
    for kernel, route in routes.items():
        assert lib().krtest_kernel(route, QC.F32, wtype, M, N, K, 0) == route, "%s is not what route %d takes for %s" % (kernel, route, what)
        p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
        launch(route, QC.F32, wtype, xp, wp, M, N, K, KrEpi(out=p_out, ldo=ldo))
        assert_bits(Dev.get(p_out, want), want, "%s %s" % (kernel, what))


# ----------------------------------------------------------------------------------------------------------------------------
# the products, WA_EPI_F32 without bias: both kernels against the host reference
# ----------------------------------------------------------------------------------------------------------------------------
@TYPES
def test_every_row_count(dev, wtype):
    """M = 2 .. 8 at K = 256, N = 9: every row-count instantiation of a format (one block: all of the prefetch is clamped; a partial second wave)."""
    N, K = 9, 256
    for M in range(2, 9):
        both_routes_f32(dev, wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K, host_gemm(wtype, M, N, K), "%s M %d N 9 K 256" % (WTYPES[wtype], M))


@pytest.mark.parametrize("K", (256, 768, 1280, 5120))
@TYPES
def test_few_rows_product(wtype, K):
    """M = 2, 5, 8 x N = 1, 7, 8, 9, 264 at one K and format: k_kgemv_rows and k_kgemm_exact both give the host reference's bits."""
    for M in (2, 5, 8):
        for N in (1, 7, 8, 9, 264):
            shape_dev = Dev()            # this shape's buffers, freed before the next shape
            try:
                both_routes_f32(shape_dev, wtype, weights(wtype, N, K), KK.activations(M, K), M, N, K, host_gemm(wtype, M, N, K),
                                "%s M %d N %d K %d" % (WTYPES[wtype], M, N, K))
            finally:
                shape_dev.close()


# ----------------------------------------------------------------------------------------------------------------------------
# Q5_K: which lane runs which row's minimum chain
# ----------------------------------------------------------------------------------------------------------------------------
def q5_chain_case(M, N=9, K=768):
    """Q5_K weights whose every dmin is nonzero, the activation rows of KK.activations, and the rows' chains in F32 on the host:
    summs[m][n] = summs + ((-dx * dmin) * (float) sum_g m[g] (bsums[2 g] + bsums[2 g + 1])), block after block."""
    wq, wsc, wd, wdm = weights(13, N, K)
    wdm = np.where(wdm == 0, np.float32(2.0 ** -8), wdm).astype(np.float32)
    xq, xd, xbs = KK.activations(M, K)
    nb = K // 256
    mins = wsc.view(np.uint8)[:, :, 8:].astype(np.int64)                                   # [n][b][g]
    gs = xbs.astype(np.int64).reshape(M, nb, 8, 2).sum(-1)                                 # [m][b][g]
    tot = np.einsum("nbg,mbg->mnb", mins, gs)
    summs = np.zeros((M, N), np.float32)
    for b in range(nb):
        dm = (-xd[:, b])[:, None] * wdm[:, b][None, :]
        p = dm * tot[:, :, b].astype(np.float32)
        summs = summs + p
    assert summs.dtype == np.float32
    return (wq, wsc, wd, wdm), (xq, xd, xbs), summs


@pytest.mark.parametrize("M", (2, 3, 5, 8))
def test_q5_K_chain_roles(dev, M):
    """Lane l of an output's group runs the chain of activation row min(l, M - 1) and lane 0 fetches row r's: with every row's chain nonzero and
    different from every other row's (asserted on the host), a lane running - or lane 0 fetching - the wrong row's chain changes the output."""
    N, K = 9, 768
    w, x, summs = q5_chain_case(M, N, K)
    assert np.all(summs != 0), "a row's minimum chain is zero"
    for n in range(N):
        assert np.unique(summs[:, n]).size == M, "two rows share a chain value at output %d" % n
    both_routes_f32(dev, 13, w, x, M, N, K, gemm_of(13, w, x, M, N, K), "q5_K chain roles M %d" % M)


# ----------------------------------------------------------------------------------------------------------------------------
# Q2_K: the minimum term before the product term
# ----------------------------------------------------------------------------------------------------------------------------
def q2_orders(M, N, K):
    """The host's Q2_K product with the minimum term of a block first (the reference's order) and with it after the product term."""
    w, x = weights(10, N, K), KK.activations(M, K)
    outs = []
    for after in (0, 1):
        out = np.empty((M, N), np.float32)
        lib().krtest_q2_host(M, N, K, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(x[0]), ptr(x[1]), ptr(x[2]), ptr(out), after)
        outs.append(out)
    return w, x, outs[0], outs[1]


def test_q2_K_minimum_order(dev):
    """M = 5, N = 40, K = 768: the two orders give different bits on the host (so the operands tell them apart), the reference's order is the host
    reference's, and the kernel gives it."""
    M, N, K = 5, 40, 768
    w, x, first, after = q2_orders(M, N, K)
    want = host_gemm(10, M, N, K)
    assert_bits(QC.bits32(first), QC.bits32(want), "the harness's host statement of the Q2_K product against the host reference")
    moved = QC.bits32(first) != QC.bits32(after)
    assert moved.any(axis=1).all(), "the order of the minimum term changes no output of some activation row: %r" % (moved.sum(axis=1),)
    both_routes_f32(dev, 10, w, x, M, N, K, want, "q2_K minimum order")


# ----------------------------------------------------------------------------------------------------------------------------
# the five epilogues at M 5, N 264, K 256 and 768: route 2 = route 1 in every output buffer, every value at its place
# ----------------------------------------------------------------------------------------------------------------------------
EPI_M, EPI_N = 5, 264


def epi_fields(epi):
    """Output buffers name -> (element count, 'f16' | 'f32') and the launch's scalar fields for M = 5, N = 264."""
    M, N = EPI_M, EPI_N
    if epi in ("F32_bias", "RESID", "GELU_F32"):
        return {"out": (M * (N + 6), "f32")}, {"ldo": N + 6, "ldr": N + 5 if epi == "RESID" else 0}
    if epi == "F16_scale":
        return {"out": (M * (N + 6), "f16")}, {"ldo": N + 6}
    if epi == "DEC_QKV":
        return ({"out": (M * 90, "f16"), "out2": ((3 + M + 1) * 92, "f16"), "out3": ((3 + M + 1) * 94, "f16")},
                {"ldo": 90, "split0": 88, "split1": 176, "row_off": 3, "ldo2": 92, "ldo3": 94})
    raise ValueError(epi)


@functools.lru_cache(maxsize=None)
def epi_case(epi, wtype, K):
    """bias, scale, resid and the expected output bits [M][N] of one epilogue over host_gemm."""
    M, N = EPI_M, EPI_N
    rng = QC.rng_for("kquant_fewrows_epi_%s_%d_%d" % (epi, wtype, K))
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    scale = rng.uniform(0.25, 1.5, N).astype(np.float32) if epi in ("F16_scale", "DEC_QKV") else None
    resid = (rng.standard_normal((M, N + 5)) * 2).astype(np.float32) if epi == "RESID" else None
    with np.errstate(over="ignore", invalid="ignore"):
        v = host_gemm(wtype, M, N, K) + bias[None, :]            # float32 throughout: one rounding per operation, as the kernels with contraction off
        if scale is not None:
            v = v * scale[None, :]
        if resid is not None:
            v = v + resid[:, :N]
        if epi == "GELU_F32":
            v = QC.gelu32(v)
        val = v.astype(np.float32).astype(np.float16).view(np.uint16) if epi in ("F16_scale", "DEC_QKV") else QC.bits32(v.astype(np.float32))
    return bias, scale, resid, val


@pytest.mark.parametrize("K", (256, 768))
@TYPES3
@pytest.mark.parametrize("epi", list(FEW_EPILOGUES))
def test_epilogue_modes(dev, epi, wtype, K):
    """Each of the decoder's five epilogues: route 2 equals route 1 bit for bit in every output buffer - and both hold every value at the place the
    epilogue's index map gives it (wa_device.h: epi_apply; DEC_QKV with row_off = 3), everything else still the sentinel."""
    M, N = EPI_M, EPI_N
    bias, scale, resid, val = epi_case(epi, wtype, K)
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
        assert lib().krtest_kernel(route, FEW_EPILOGUES[epi], wtype, M, N, K, 0) == route
        ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
        e = KrEpi(bias=p_bias, scale=p_scale, resid=p_resid, gelu=p_gelu, out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
        launch(route, FEW_EPILOGUES[epi], wtype, xp, wp, M, N, K, e)
        got[kernel] = {name: Dev.get(ptrs[name], a) for name, a in want.items()}
    for name, a in want.items():
        assert np.array_equal(got["k_kgemv_rows"][name], got["k_kgemm_exact"][name]), "%s %s K %d: %s of the two kernels differs" % (epi, WTYPES[wtype], K, name)
        assert_bits(got["k_kgemv_rows"][name], a, "k_kgemv_rows %s %s K %d %s" % (epi, WTYPES[wtype], K, name))


# ----------------------------------------------------------------------------------------------------------------------------
# WA_EPI_DEC_QKV with rows of different states
# ----------------------------------------------------------------------------------------------------------------------------
ROWP_HEADS = (3, 0, 6, 1, 4)        # the cell of each row's state that takes its key / value
ROWP_CELLS, ROWP_LAYER = 8, 1       # cells per layer of every state; the launch writes layer 1 (rowp_off = one layer of cells)


@pytest.mark.parametrize("wtype", (13, 10), ids=("q5_K", "q2_K"))
def test_rows_of_different_states(dev, wtype):
    """Five rows, five K and five V buffers, distinct cells, layer 1, through k_kgemv_rows: each row's key and value land in its own state's cell
    (as tests/test_quant_fewrows_gpu.py::test_rows_of_different_states_k_format holds for the general kernel), every other half-word keeps the
    sentinel, out2 / out3 are not touched."""
    M, N, K, d = EPI_M, EPI_N, 256, 88
    bias, scale, _, val = epi_case("DEC_QKV", wtype, K)
    val = val.reshape(M, N)
    assert np.unique(val).size > 200            # the rows differ: a value in the wrong row's cell would show
    ldo, ld2, ld3 = 90, 92, 94
    layer2 = ROWP_CELLS * ld2           # ONE element offset serves the key and the value pointer (the model's two strides are equal)
    sent_k, sent_v = np.full((2, ROWP_CELLS, ld2), SENT16, np.uint16), np.full((2, ROWP_CELLS, ld3), SENT16, np.uint16)       # two layers each
    p_k = [dev.put(sent_k) for _ in range(M)]
    p_v = [dev.put(sent_v) for _ in range(M)]
    rp = np.zeros(M, ROWPTR)
    for i in range(M):
        rp[i] = (p_k[i], p_v[i], 0, 0, ROWP_HEADS[i] + 1, ROWP_HEADS[i])
    want_q = np.full((M + 1, ldo), SENT16, np.uint16)
    want_q[:M, :d] = val[:, :d]
    p_q = dev.put(np.full_like(want_q, SENT16))
    p_o2, p_o3 = dev.put(np.full(8, SENT16, np.uint16)), dev.put(np.full(8, SENT16, np.uint16))      # NOT used with rowp set: their sentinel must survive
    e = KrEpi(bias=dev.put(bias), scale=dev.put(scale), out=p_q, ldo=ldo, out2=p_o2, ldo2=ld2, out3=p_o3, ldo3=ld3, split0=d, split1=2 * d, row_off=2,
              rowp=dev.put(rp), rowp_off=ROWP_LAYER * layer2)
    assert lib().krtest_kernel(2, QC.DEC_QKV, wtype, M, N, K, 1) == 2
    xp, wp = put_arrays(dev, wtype, weights(wtype, N, K), KK.activations(M, K))
    launch(2, QC.DEC_QKV, wtype, xp, wp, M, N, K, e)
    what = "k_kgemv_rows %s rowp" % WTYPES[wtype]
    assert_bits(Dev.get(p_q, want_q), want_q, what + " q")
    for p in (p_o2, p_o3):
        assert_bits(Dev.get(p, np.empty(8, np.uint16)), np.full(8, SENT16, np.uint16), what + " out2 / out3")
    for i in range(M):
        wk, wv = sent_k.copy().ravel(), sent_v.copy().ravel()
        wk[ROWP_LAYER * layer2 + ROWP_HEADS[i] * ld2:][:d] = val[i, d:2 * d]
        wv[ROWP_LAYER * layer2 + ROWP_HEADS[i] * ld3:][:d] = val[i, 2 * d:]
        assert_bits(Dev.get(p_k[i], wk), wk, "%s key buffer of row %d" % (what, i))
        assert_bits(Dev.get(p_v[i], wv), wv, "%s value buffer of row %d" % (what, i))


# ----------------------------------------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------------------------------------
def shapes_of(d):
    """(N, K) of a decoder's products at width d: q|k|v, out / cross, the two MLP products, the logits - and a narrow one."""
    return ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d), (51865, d), (264, d))


def test_rule():
    """Route 0 answers 2 for the classes of FEW_CLASSES in the five epilogues (and for no other class); routes 0 and 2 never at M = 1, M = 9 or for
    the encoder's two epilogues; route 1 never; from 9 rows on every route answers as wa_kgemm_kernel does (the matrix-core kernel unless route 1
    or rows of different states).  The suite runs without WHISPER_AMD_NO_FEW_ROWS."""
    assert os.environ.get("WHISPER_AMD_NO_FEW_ROWS") is None and os.environ.get("WHISPER_AMD_NO_QMFMA") is None, "the suite runs with the default routing"
    k = lib().krtest_kernel
    assert any(c[1] == 8 for c in FEW_CLASSES) and any((14, 8, d) not in FEW_CLASSES for d in WIDTHS)
    for wtype in WTYPES:
        for d in WIDTHS:
            for N, K in shapes_of(d):
                for mode in FEW_EPILOGUES.values():
                    for M in range(2, 9):
                        for rowp in (0, 1):
                            assert k(0, mode, wtype, M, N, K, rowp) == (2 if (wtype, M, d) in FEW_CLASSES else 1), (wtype, mode, M, N, K)
                            assert k(2, mode, wtype, M, N, K, rowp) == 2 and k(1, mode, wtype, M, N, K, rowp) == 1, (wtype, mode, M, N, K)
                    for route in (0, 1, 2):
                        assert k(route, mode, wtype, 1, N, K, 0) == 1, (wtype, mode, route)
                    for M in (9, 40, 200):
                        assert k(0, mode, wtype, M, N, K, 0) == 3 and k(2, mode, wtype, M, N, K, 0) == 3 and k(3, mode, wtype, M, N, K, 0) == 3, (wtype, mode, M, N, K)
                        assert k(1, mode, wtype, M, N, K, 0) == 1 and k(0, mode, wtype, M, N, K, 1) == 1 and k(2, mode, wtype, M, N, K, 1) == 1, (wtype, mode, M, N, K)
                for mode in (QC.ENC_QKV, QC.CROSS_KV):
                    for M in (1, 2, 5, 8):
                        for route in (0, 1, 2):
                            assert k(route, mode, wtype, M, N, K, 0) == 1, (wtype, mode, M, route)
                    assert k(0, mode, wtype, 9, N, K, 0) == 3 and k(2, mode, wtype, 9, N, K, 0) == 3


CHILD = """
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
L.krtest_kernel.argtypes = [C.c_int] * 7
bad = [(r, mode, w, M) for r in (0, 1) for mode in (0, 7, 3, 5, 8) for w in (10, 11, 13, 14) for M in range(1, 10) if L.krtest_kernel(r, mode, w, M, 768, 768, 0) == 2]
forced = all(L.krtest_kernel(2, 5, w, M, 768, 768, 0) == 2 for w in (10, 11, 13, 14) for M in range(2, 9))          # (d = 768: route 0 would answer 2 for every M without the switch)
print("few-rows answers", len(bad), "forced", int(forced))
"""


def test_switch_in_a_fresh_process():
    """WHISPER_AMD_NO_FEW_ROWS=1 is read once per process: in a fresh child route 0 never answers 2 (route 2, the tests' own, still does)."""
    assert sorted((QC.F16, QC.GELU_F32, QC.RESID, QC.F32, QC.DEC_QKV)) == [0, 3, 5, 7, 8]          # the modes the child names
    env = dict(os.environ, WHISPER_AMD_NO_FEW_ROWS="1")
    r = subprocess.run([sys.executable, "-c", CHILD, LIB_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-800:])
    assert "few-rows answers 0 forced 1" in r.stdout, r.stdout[-400:]

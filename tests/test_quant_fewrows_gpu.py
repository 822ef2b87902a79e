"""The few-rows product kernel of wa_quant.hip (k_qgemv_rows: M = 2..8 activation rows, one wave per 8 output rows) and the quantised products
with rows of DIFFERENT states (wa_epi::rowp, the lock-step group's q|k|v product), kernel by kernel, BIT FOR BIT.

Every product runs twice through tests/native/libfewrows_kernels.so - route 1, the general kernel k_qgemm_exact (what WHISPER_AMD_NO_FEW_ROWS=1
selects; here a harness argument), and route 2, k_qgemv_rows - and both are compared with the host reference tests/native/libquant_ref.so
(variant 0, pinned to the reference library by tests/test_quant_kernels_math.py).  Shapes, the smallest that can go wrong: M = 2, 3, 5, 8;
N = 8 (a single wave), 40 and 264 (no multiples of 32; 264 = several workgroups of either kernel); K = 32, 96 (block-by-block loop), 128, 384,
2048, 5120 (pipelined loop: one round, a partial last round, many rounds); without and with a minimum.  Operands from tools/quant_cases.py:
dictated scales binades apart, saturated rows, minimum chains far from the lane sums, block sums of +-inf, besides seeded random rows.
Output buffers are filled with a sentinel first; padding and the row beyond M must still hold it.

The rowp cases: five rows, five K and five V buffers of their own, distinct cells - each row's key and value in its own buffer's cell, every
other half-word still the sentinel - for k_qgemm_exact, k_qgemv_rows and one K format (k_kgemm_exact).  No caller sets rowp on a quantised product yet; the branch of the
shared epilogue is held here so that the one who does finds it tested.  The harness is linked against the
product's own build/wa_quant.o, wa_quantk.o and wa_quantk_q2.o (whisper-rust_amd/Makefile)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quant_cases as QC  # noqa: E402

LIB_PATH = os.path.join(ROOT, "tests", "native", "libfewrows_kernels.so")
SENT16 = np.uint16(0x7E5A)          # bit patterns no kernel result can have (NaNs with a payload)
SENT32 = np.uint32(0x7FC0DEAD)
ROUTES = {"k_qgemm_exact": 1, "k_qgemv_rows": 2}
MS, NS, NBS = (2, 3, 5, 8), (8, 40, 264), (1, 3, 4, 12, 64, 160)


class FrEpi(C.Structure):      # tests/native/fewrows_kernels.hip: frtest_epi
    _fields_ = [("bias", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int), ("out2", C.c_void_p), ("ldo2", C.c_int),
                ("out3", C.c_void_p), ("ldo3", C.c_int), ("resid", C.c_void_p), ("ldr", C.c_int), ("gelu", C.c_void_p),
                ("split0", C.c_int), ("split1", C.c_int), ("row_off", C.c_int), ("aux0", C.c_int), ("aux1", C.c_int),
                ("rowp", C.c_void_p), ("rowp_off", C.c_longlong)]


ROWPTR = np.dtype([("kv_k", "<u8"), ("kv_v", "<u8"), ("cross_k", "<u8"), ("cross_v", "<u8"), ("n_kv", "<i4"), ("kv_head", "<i4")])      # wa_kernels.h: wa_rowptr


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target kquant_harness)" % LIB_PATH
    L = C.CDLL(LIB_PATH)
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    L.frtest_alloc.restype = vp; L.frtest_alloc.argtypes = [sz]
    L.frtest_free.argtypes = [vp]
    L.frtest_h2d.argtypes = [vp, vp, sz]; L.frtest_d2h.argtypes = [vp, vp, sz]
    L.frtest_qgemm.argtypes = [i, i, vp, vp, i, vp, vp, i, i, C.POINTER(FrEpi), vp, vp]
    L.frtest_kgemm.argtypes = [i, i, vp, vp, vp, i, vp, vp, vp, vp, i, i, C.POINTER(FrEpi)]
    assert L.frtest_rowptr_bytes() == ROWPTR.itemsize
    return L


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().frtest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().frtest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().frtest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().frtest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().frtest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def assert_same(got, want, what):
    """Bits: equal, except that where a NaN is expected (block sums of +-inf) any NaN but the sentinel will do."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    ok = got == want
    if want.dtype == np.uint32:
        want_nan = np.isnan(want.view(np.float32)) & (want != SENT32)
        ok = np.where(want_nan, np.isnan(got.view(np.float32)) & (got != SENT32), ok)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, bad.size, want.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


def put_weights(dev, w):
    return dev.put(QC.pack_qs(w["q"])), dev.put(w["d"]), (dev.put(w["m"]) if w["m"] is not None else None)


def put_activations(dev, x, q1):
    return dev.put(QC.pack_qs(x["q"])), dev.put(x["d"]), (dev.put(x["s"]) if q1 else None)


# ----------------------------------------------------------------------------------------------------------------------------
# the products, WA_EPI_F32 without bias: both kernels against the host reference
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", NBS, ids=["K%d" % (32 * nb) for nb in NBS])
@pytest.mark.parametrize("fam", ("Q0", "Q1"))
def test_few_rows_product(fam, nb):
    """M = 2, 3, 5, 8 x N = 8, 40, 264 at one K and family: k_qgemv_rows and k_qgemm_exact both give the host reference's bits; the row beyond M
    and the columns beyond N keep the sentinel."""
    K = nb * 32
    for i, M in enumerate(MS):
        for j, N in enumerate(NS):
            fmt = (("q8_0", "q5_0") if fam == "Q0" else ("q5_1", "q4_1"))[(i + j) % 2]
            c = {"name": "fewrows_%s_nb%d_M%d_N%d" % (fam, nb, M, N), "fmt": fmt, "nb": nb, "N": N, "M": M, "kind": QC.ACT_KINDS[(i + j + nb) % 5]}
            w, x = QC.product_operands(c)
            ldo = N + 3
            want = np.full((M + 1, ldo), SENT32, np.uint32)
            want[:M, :N] = QC.bits32(QC.ref_gemm(w, x))
            shape_dev = Dev()            # this shape's buffers, freed before the next shape (K = 5120 x N = 264 twelve times over is not needed at once)
            try:
                wq, wd, wm = put_weights(shape_dev, w)
                xq, xd, xs = put_activations(shape_dev, x, fam == "Q1")
                for kernel, route in ROUTES.items():
                    p_out = shape_dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
                    e = FrEpi(out=p_out, ldo=ldo)
                    lib().frtest_qgemm(route, QC.F32, xq, xd, M, wq, wd, N, K, C.byref(e), xs, wm)
                    sync()
                    assert_same(Dev.get(p_out, want), want, "%s %s (%s, %s)" % (kernel, c["name"], fmt, c["kind"]))
            finally:
                shape_dev.close()


# ----------------------------------------------------------------------------------------------------------------------------
# every epilogue once at M 5, N 264, K 384
# ----------------------------------------------------------------------------------------------------------------------------
EPI_M, EPI_N, EPI_NB, EPI_TPAD = 5, 264, 12, 16


def epi_fields(epi):
    """Output buffers name -> (element count, 'f16' | 'f32') and the launch's scalar fields for N = 264 (tools/quant_cases.py: epi_layout is N = 70's)."""
    M, N = EPI_M, EPI_N
    if epi in ("F32_bias", "RESID", "GELU_F32"):
        return {"out": (M * (N + 6), "f32")}, {"ldo": N + 6, "ldr": N + 5 if epi == "RESID" else 0}
    if epi == "F16_scale":
        return {"out": (M * (N + 6), "f16")}, {"ldo": N + 6}
    if epi == "ENC_QKV":
        return {"out": (M * 104, "f16"), "out2": ((N - 96) * (M + 7), "f16")}, {"ldo": 104, "split0": 96, "ldo2": M + 7}
    if epi == "DEC_QKV":
        return ({"out": (M * 90, "f16"), "out2": ((3 + M + 1) * 92, "f16"), "out3": ((3 + M + 1) * 94, "f16")},
                {"ldo": 90, "split0": 88, "split1": 176, "row_off": 3, "ldo2": 92, "ldo3": 94})
    if epi == "CROSS_KV":       # d = 64: n = 256 .. 263 is the K of layer 2
        return {"out": (3 * EPI_TPAD * 64, "f16"), "out2": (3 * EPI_TPAD * 64, "f16")}, {"aux0": EPI_TPAD, "aux1": 64}
    raise ValueError(epi)


@functools.lru_cache(maxsize=None)
def epi_case(epi, fmt):
    """Operands with moderate scales (the F16 outputs stay finite and every bit of them depends on the product) and the expected values [M][N]."""
    rng = QC.rng_for("fewrows_epi_%s_%s" % (epi, fmt))
    M, N, nb = EPI_M, EPI_N, EPI_NB
    w = QC.weights(fmt, N, nb, rng, -9, -5)
    x = QC.activations("random", M, nb, rng)
    x["d"] = QC.f16_values(rng, (M, nb), -5, -2, signed=False)
    x["s"] = QC.f16r(x["d"] * x["q"].reshape(M, nb, 32).sum(-1).astype(np.float32))
    bias = (rng.standard_normal(N) * 0.5).astype(np.float32)
    scale = rng.uniform(0.25, 1.5, N).astype(np.float32) if epi in ("F16_scale", "DEC_QKV", "CROSS_KV") else None
    resid = (rng.standard_normal((M, N + 5)) * 2).astype(np.float32) if epi == "RESID" else None
    with np.errstate(over="ignore", invalid="ignore"):
        v = QC.ref_gemm(w, x) + bias[None, :]          # float32 throughout: one rounding per operation, as the kernels with contraction off
        if scale is not None:
            v = v * scale[None, :]
        if resid is not None:
            v = v + resid[:, :N]
        if epi == "GELU_F32":
            v = QC.gelu32(v)
        val = v.astype(np.float32).astype(np.float16).view(np.uint16) if epi in ("F16_scale", "ENC_QKV", "DEC_QKV", "CROSS_KV") else QC.bits32(v.astype(np.float32))
    return w, x, bias, scale, resid, val


@pytest.mark.parametrize("fmt", ("q5_0", "q5_1"))
@pytest.mark.parametrize("epi", list(QC.EPI_MODES))
def test_epilogue_of_either_kernel(dev, epi, fmt):
    """Every value at the place the epilogue's index map gives it (wa_device.h: epi_apply), everything else still the sentinel - through either
    route (the encoder's two epilogues have no few-rows form: route 2 falls to the general kernel and must still be right)."""
    M, N, K = EPI_M, EPI_N, EPI_NB * 32
    w, x, bias, scale, resid, val = epi_case(epi, fmt)
    bufs, fields = epi_fields(epi)
    want = {name: np.full(n, SENT16 if t == "f16" else SENT32, np.uint16 if t == "f16" else np.uint32) for name, (n, t) in bufs.items()}
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    which, idx, names = QC.epi_out_index({"epi": epi}, fields, m, n)
    for k, name in enumerate(names):
        sel = which == k
        assert np.unique(idx[sel]).size == np.count_nonzero(sel) and idx[sel].max() < want[name].size
        want[name][idx[sel]] = val[sel]
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    p_bias, p_scale = dev.put(bias), dev.put(scale) if scale is not None else None
    p_resid, p_gelu = dev.put(resid) if resid is not None else None, dev.put(QC.GELU) if epi == "GELU_F32" else None
    for kernel, route in ROUTES.items():
        ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
        e = FrEpi(bias=p_bias, scale=p_scale, resid=p_resid, gelu=p_gelu, out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
        lib().frtest_qgemm(route, QC.EPI_MODES[epi], xq, xd, M, wq, wd, N, K, C.byref(e), xs, wm)
        sync()
        for name, a in want.items():
            assert_same(Dev.get(ptrs[name], a), a, "%s %s %s %s" % (kernel, epi, fmt, name))


# ----------------------------------------------------------------------------------------------------------------------------
# WA_EPI_DEC_QKV with rows of different states
# ----------------------------------------------------------------------------------------------------------------------------
ROWP_HEADS = (3, 0, 6, 1, 4)        # the cell of each row's state that takes its key / value
ROWP_CELLS, ROWP_LAYER = 8, 1       # cells per layer of every state; the launch writes layer 1 (rowp_off = one layer of cells)


def check_rowp(dev, launch, val, what):
    """`launch(e)` runs a DEC_QKV product of M = 5 rows with e.rowp set; val: the expected F16 bits [5][264] (q | k | v, 88 each)."""
    M, d = 5, 88
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
    # out2 / out3 are NOT used with rowp set: they point at one-element buffers whose sentinel must survive
    p_o2, p_o3 = dev.put(np.full(8, SENT16, np.uint16)), dev.put(np.full(8, SENT16, np.uint16))
    e = FrEpi(out=p_q, ldo=ldo, out2=p_o2, ldo2=ld2, out3=p_o3, ldo3=ld3, split0=d, split1=2 * d, row_off=2, rowp=dev.put(rp), rowp_off=ROWP_LAYER * layer2)
    launch(e)
    sync()
    assert_same(Dev.get(p_q, want_q), want_q, what + " q")
    for p in (p_o2, p_o3):
        assert_same(Dev.get(p, np.empty(8, np.uint16)), np.full(8, SENT16, np.uint16), what + " out2 / out3")
    for i in range(M):
        wk, wv = sent_k.copy().ravel(), sent_v.copy().ravel()
        wk[ROWP_LAYER * layer2 + ROWP_HEADS[i] * ld2:][:d] = val[i, d:2 * d]
        wv[ROWP_LAYER * layer2 + ROWP_HEADS[i] * ld3:][:d] = val[i, 2 * d:]
        assert_same(Dev.get(p_k[i], wk), wk, "%s key buffer of row %d" % (what, i))
        assert_same(Dev.get(p_v[i], wv), wv, "%s value buffer of row %d" % (what, i))


@pytest.mark.parametrize("fmt", ("q5_0", "q5_1"))
@pytest.mark.parametrize("kernel", list(ROUTES))
def test_rows_of_different_states(dev, kernel, fmt):
    """Five rows, five K and five V buffers, distinct cells, layer 1: each row's key and value land in its own state's cell."""
    w, x, bias, scale, _, val = epi_case("DEC_QKV", fmt)
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    p_bias, p_scale = dev.put(bias), dev.put(scale)

    def launch(e):
        e.bias, e.scale = p_bias, p_scale
        lib().frtest_qgemm(ROUTES[kernel], QC.DEC_QKV, xq, xd, EPI_M, wq, wd, EPI_N, EPI_NB * 32, C.byref(e), xs, wm)
    check_rowp(dev, launch, val, "%s %s" % (kernel, fmt))


def dec_qkv_plain(dev, launch):
    """The same DEC_QKV product WITHOUT rowp (rows m -> cells row_off + m of ONE K / V buffer): the F16 bits [5][264] it stores."""
    M, d = 5, 88
    p_q, p_k, p_v = (dev.put(np.full((M, d), SENT16, np.uint16)) for _ in range(3))
    launch(FrEpi(out=p_q, ldo=d, out2=p_k, ldo2=d, out3=p_v, ldo3=d, split0=d, split1=2 * d, row_off=0))
    sync()
    val = np.concatenate([Dev.get(p, np.empty((M, d), np.uint16)) for p in (p_q, p_k, p_v)], axis=1)
    assert not np.any(val == SENT16)
    return val


def test_rows_of_different_states_k_format(dev):
    """The same through k_kgemm_exact (Q5_K, K = 256).  Expected: what the kernel stores for the same operands without rowp - that path is held to
    the host statement of the product by tests/test_kquant_kernels_gpu.py; here only WHERE each row's key and value go is in question, so the
    operands are seeded random arrays in the kernel layout (quants -16 .. 15 / -127 .. 127, scales, F32 d / dmin, block sums)."""
    M, N, K, wtype = 5, 264, 256, 13
    nb = K // 256
    rng = QC.rng_for("fewrows_rowp_q5_K")
    wo = (dev.put(rng.integers(0, 32, (N, 8, nb, 8, 4)).astype(np.int8)), dev.put(rng.integers(0, 64, (N, nb, 16)).astype(np.int8)),
          dev.put((rng.uniform(-1, 1, (N, nb)) * 2e-3).astype(np.float32)), dev.put((rng.uniform(-1, 1, (N, nb)) * 1e-2).astype(np.float32)))
    xo = (dev.put(rng.integers(-127, 128, (M, 8, nb, 8, 4)).astype(np.int8)), dev.put(rng.uniform(0.01, 0.05, (M, nb)).astype(np.float32)),
          dev.put(rng.integers(-2000, 2000, (M, nb, 16)).astype(np.int16)))
    p_bias, p_scale = dev.put((rng.standard_normal(N) * 0.5).astype(np.float32)), dev.put(rng.uniform(0.25, 1.5, N).astype(np.float32))

    def launch(e):
        e.bias, e.scale = p_bias, p_scale
        lib().frtest_kgemm(QC.DEC_QKV, wtype, xo[0], xo[1], xo[2], M, wo[0], wo[1], wo[2], wo[3], N, K, C.byref(e))
    val = dec_qkv_plain(dev, launch)
    assert np.unique(val).size > 200            # the rows differ: a value in the wrong row's cell would show
    check_rowp(dev, launch, val, "k_kgemm_exact q5_K")

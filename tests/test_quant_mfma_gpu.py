"""The int8 matrix-core product kernel of wa_quant.hip (k_qgemm_mfma: M > 8 activation rows, v_mfma_i32_16x16x4_4b_i8 with block = lane-sum
index) on its own, BIT FOR BIT.  No tolerance anywhere in this file.

Every product runs through tests/native/libfewrows_kernels.so, whose frtest_qgemm hands its route to wa_launch_qgemm_exact_route unchanged:
route 3, k_qgemm_mfma, and route 1, the general kernel k_qgemm_exact.  Both are compared with the host reference tests/native/libquant_ref.so
(variant 0, pinned to the reference library by tests/test_quant_kernels_math.py).  Shapes, the smallest that can go wrong: M = 9 (the smallest
routed: one partial 16-row tile), 16 (exactly one tile), 17 (a tile and a one-row tile), 40 (two tiles and half of one); N = 16 (one column tile),
40 (a partial column tile), 264 (several, a partial last one); nb = 1, 3, 6 (block-by-block loop), 4 (one round of the pipelined loop), 24, 160
(many rounds; K = 5120 is fc2 of a d = 1280 model); without and with a minimum.  Grids this small take the kernel's one-row-per-lane form (four
waves share a tile); test_four_wave_workgroups holds the four-rows-per-lane form of the encoder's grids at the smallest grid that takes it.  Operands from
tools/quant_cases.py: dictated scales binades apart, saturated rows, minimum chains far from the lane sums, block sums of +-inf (where a NaN of
any payload but the sentinel is accepted), seeded random rows.  Output buffers are filled with a sentinel first; rows beyond M, columns beyond N
and the padding must still hold it.

The operand-role case is the in-product twin of tools/micro/mfma_i8_blocks.hip: integer quants and power-of-two scales built so that every
(row, column, lane-sum index) contributes a different power-of-two term - the exact result names any swapped row, column, block or scale.

Which kernel a route takes is asked of tests/native/libqmfma_route.so (the kernels give the same bits, so results cannot tell): route 3 never
applies below 9 rows, and never to a product whose rows belong to different states (wa_epi::rowp)."""
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
ROUTE_LIB_PATH = os.path.join(ROOT, "tests", "native", "libqmfma_route.so")
SENT16 = np.uint16(0x7E5A)          # bit patterns no kernel result can have (NaNs with a payload)
SENT32 = np.uint32(0x7FC0DEAD)
ROUTES = {"k_qgemm_mfma": 3, "k_qgemm_exact": 1}
MS, NS, NBS = (9, 16, 17, 40), (16, 40, 264), (1, 3, 4, 6, 24, 160)


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
    assert L.frtest_rowptr_bytes() == ROWPTR.itemsize
    return L


@functools.lru_cache(maxsize=None)
def route_lib():
    assert os.path.exists(ROUTE_LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target kquant_harness)" % ROUTE_LIB_PATH
    L = C.CDLL(ROUTE_LIB_PATH)
    L.qmtest_kernel.argtypes = [C.c_int] * 6
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
def test_matrix_core_product(fam, nb):
    """M = 9, 16, 17, 40 x N = 16, 40, 264 at one K and family: k_qgemm_mfma and k_qgemm_exact both give the host reference's bits; the row
    beyond M and the columns beyond N keep the sentinel."""
    K = nb * 32
    for i, M in enumerate(MS):
        for j, N in enumerate(NS):
            fmt = (("q8_0", "q5_0") if fam == "Q0" else ("q5_1", "q4_1"))[(i + j) % 2]
            c = {"name": "qmfma_%s_nb%d_M%d_N%d" % (fam, nb, M, N), "fmt": fmt, "nb": nb, "N": N, "M": M, "kind": QC.ACT_KINDS[(i + j + nb) % 5]}
            w, x = QC.product_operands(c)
            ldo = N + 3
            want = np.full((M + 1, ldo), SENT32, np.uint32)
            want[:M, :N] = QC.bits32(QC.ref_gemm(w, x))
            shape_dev = Dev()            # this shape's buffers, freed before the next shape
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


@pytest.mark.parametrize("nb", (3, 8), ids=("K96", "K256"))
@pytest.mark.parametrize("fmt", ("q5_0", "q5_1"))
def test_four_wave_workgroups(dev, fmt, nb):
    """The shapes above are few enough tiles for the kernel's one-row-per-lane form; from 512 workgroups of 64 columns x 16 rows on the launcher
    takes the form with four rows per lane and one column tile per wave (the encoder's shapes).  M = 513 (32 row tiles and a one-row tile) x
    N = 1000 (15 workgroups and one with 40 columns: a partial wave and an idle one) is 33 x 16 = 528 of them: about the smallest grid that does."""
    M, N, K = 513, 1000, nb * 32
    c = {"name": "qmfma4_%s_nb%d" % (fmt, nb), "fmt": fmt, "nb": nb, "N": N, "M": M, "kind": "random"}
    w, x = QC.product_operands(c)
    ldo = N + 3
    want = np.full((M + 1, ldo), SENT32, np.uint32)
    want[:M, :N] = QC.bits32(QC.ref_gemm(w, x))
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    for kernel, route in ROUTES.items():
        p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
        lib().frtest_qgemm(route, QC.F32, xq, xd, M, wq, wd, N, K, C.byref(FrEpi(out=p_out, ldo=ldo)), xs, wm)
        sync()
        assert_same(Dev.get(p_out, want), want, "%s %s" % (kernel, c["name"]))


# ----------------------------------------------------------------------------------------------------------------------------
# operand roles: every (row, column, lane-sum index) a different power-of-two term
# ----------------------------------------------------------------------------------------------------------------------------
ROLE_M, ROLE_N = 17, 48


def role_codes():
    """One distinct byte per row and per column, chosen so that all 17 x 48 expected outputs differ (role_expected asserts it): an output in
    another output's place is seen, not only a wrong value."""
    return np.arange(ROLE_M) + 11, 3 * np.arange(ROLE_N) + 5


def role_operands(fmt, nb):
    """Block b < 8 holds quants in lane-sum index l = b only: the activation row m one byte (byte m % 4 of the quad) of value 2^bit_l(code(m)),
    the weight row n four bytes of value 2^bit_l(code(n)); scales dx[m][b] = 2^(m - b - 16), dw[n][b] = 2^(-n - 2 b).  Lane sum l of block l is then
    2^(bit_l(code m) + bit_l(code n)) and every other lane sum of every block is 0 - unless a row, a column, a block or a lane-sum index is
    taken from the wrong place.  Blocks from 8 on (nb = 9: the block-by-block loop) hold zero quants under scales of 1.  Minimums are 0."""
    cm, cn = role_codes()
    xq = np.zeros((ROLE_M, nb, 8, 4), np.int8)
    wq = np.zeros((ROLE_N, nb, 8, 4), np.int8)
    xd, wd = np.ones((ROLE_M, nb), np.float32), np.ones((ROLE_N, nb), np.float32)
    for b in range(8):
        for m in range(ROLE_M):
            xq[m, b, b, m % 4] = 1 << ((cm[m] >> b) & 1)
            xd[m, b] = 2.0 ** (m - b - 16)
        for n in range(ROLE_N):
            wq[n, b, b, :] = 1 << ((cn[n] >> b) & 1)
            wd[n, b] = 2.0 ** (-n - 2 * b)
    q1 = QC.FORMATS[fmt][2]
    w = {"fmt": fmt, "q": wq.reshape(ROLE_N, nb * 32), "d": wd, "m": np.zeros((ROLE_N, nb), np.float32) if q1 else None}
    xqf = xq.reshape(ROLE_M, nb * 32)
    x = {"q": xqf, "d": xd, "s": QC.f16r(xd * xqf.reshape(ROLE_M, nb, 32).sum(-1).astype(np.float32))}
    return w, x


def role_expected():
    """sum_l 2^(m - n - 16 - 3 l + bit_l(code m) + bit_l(code n)): eight digits of three bits, 24 bits in all - exact in F32 whatever the order."""
    cm, cn = role_codes()
    out = np.zeros((ROLE_M, ROLE_N), np.float64)
    for b in range(8):
        out += 2.0 ** ((np.arange(ROLE_M)[:, None] - np.arange(ROLE_N)[None, :] - 16 - 3 * b) + ((cm[:, None] >> b) & 1) + ((cn[None, :] >> b) & 1))
    assert np.array_equal(out, out.astype(np.float32).astype(np.float64)) and np.unique(out).size == out.size
    return out.astype(np.float32)


@pytest.mark.parametrize("nb", (8, 9))
@pytest.mark.parametrize("fmt", ("q8_0", "q5_1"))
def test_operand_roles(dev, fmt, nb):
    """The exact result of an integer / power-of-two product in which every (row, column, lane-sum index) has a term of its own."""
    w, x = role_operands(fmt, nb)
    want = np.full((ROLE_M + 1, ROLE_N + 3), SENT32, np.uint32)
    want[:ROLE_M, :ROLE_N] = QC.bits32(role_expected())
    assert_same(QC.bits32(QC.ref_gemm(w, x)), want[:ROLE_M, :ROLE_N], "the host reference on the role operands")
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    for kernel, route in ROUTES.items():
        p_out = dev.put(np.full_like(want, SENT32))
        e = FrEpi(out=p_out, ldo=ROLE_N + 3)
        lib().frtest_qgemm(route, QC.F32, xq, xd, ROLE_M, wq, wd, ROLE_N, nb * 32, C.byref(e), xs, wm)
        sync()
        assert_same(Dev.get(p_out, want), want, "%s operand roles %s nb %d" % (kernel, fmt, nb))


# ----------------------------------------------------------------------------------------------------------------------------
# every epilogue mode of the launcher at M 17, N 48, K 128 and 192: route 3 = route 1 in every output buffer
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


@functools.lru_cache(maxsize=None)
def epi_case(epi, fmt, nb):
    """Operands with moderate scales (the F16 outputs stay finite and every bit of them depends on the product) and the expected values [M][N]."""
    rng = QC.rng_for("qmfma_epi_%s_%s_%d" % (epi, fmt, nb))
    M, N = EPI_M, EPI_N
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


@pytest.mark.parametrize("nb", (4, 6), ids=("K128", "K192"))
@pytest.mark.parametrize("fmt", ("q5_0", "q5_1"))
@pytest.mark.parametrize("epi", list(QC.EPI_MODES))
def test_epilogue_modes(dev, epi, fmt, nb):
    """Every mode wa_launch_qgemm_exact_route has a case for: route 3 equals route 1 bit for bit in every output buffer - and both hold every value
    at the place the epilogue's index map gives it (wa_device.h: epi_apply), everything else still the sentinel."""
    M, N, K = EPI_M, EPI_N, nb * 32
    w, x, bias, scale, resid, val = epi_case(epi, fmt, nb)
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
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    p_bias, p_scale = dev.put(bias), dev.put(scale) if scale is not None else None
    p_resid, p_gelu = dev.put(resid) if resid is not None else None, dev.put(QC.GELU) if epi == "GELU_F32" else None
    got = {}
    for kernel, route in ROUTES.items():
        ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
        e = FrEpi(bias=p_bias, scale=p_scale, resid=p_resid, gelu=p_gelu, out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
        lib().frtest_qgemm(route, QC.EPI_MODES[epi], xq, xd, M, wq, wd, N, K, C.byref(e), xs, wm)
        sync()
        got[kernel] = {name: Dev.get(ptrs[name], a) for name, a in want.items()}
    for name, a in want.items():
        assert np.array_equal(got["k_qgemm_mfma"][name], got["k_qgemm_exact"][name]), "%s %s K %d: %s of the two kernels differs" % (epi, fmt, K, name)
        assert_same(got["k_qgemm_mfma"][name], a, "k_qgemm_mfma %s %s K %d %s" % (epi, fmt, K, name))


# ----------------------------------------------------------------------------------------------------------------------------
# route selection
# ----------------------------------------------------------------------------------------------------------------------------
def test_route_3_never_below_nine_rows(dev):
    """M = 5 (and 8, and 1) with route 3: not the matrix-core kernel, and the few-rows / general kernel's bits."""
    for M in (1, 2, 5, 8):
        for mode in (QC.F32, QC.DEC_QKV, QC.ENC_QKV):
            assert route_lib().qmtest_kernel(3, mode, M, 264, 384, 0) in (1, 2), (M, mode)
            assert route_lib().qmtest_kernel(0, mode, M, 264, 384, 0) == route_lib().qmtest_kernel(3, mode, M, 264, 384, 0), (M, mode)
    assert route_lib().qmtest_kernel(3, QC.F32, 9, 264, 384, 0) == 3 and route_lib().qmtest_kernel(1, QC.F32, 9, 264, 384, 0) == 1
    assert route_lib().qmtest_kernel(2, QC.F32, 9, 264, 384, 0) == 1
    M, N, nb = 5, 40, 12
    c = {"name": "qmfma_route_M5", "fmt": "q5_1", "nb": nb, "N": N, "M": M, "kind": "random"}
    w, x = QC.product_operands(c)
    want = np.full((M + 1, N + 3), SENT32, np.uint32)
    want[:M, :N] = QC.bits32(QC.ref_gemm(w, x))
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, True)
    for route in (3, 1, 2):
        p_out = dev.put(np.full_like(want, SENT32))
        lib().frtest_qgemm(route, QC.F32, xq, xd, M, wq, wd, N, nb * 32, C.byref(FrEpi(out=p_out, ldo=N + 3)), xs, wm)
        sync()
        assert_same(Dev.get(p_out, want), want, "M = 5 through route %d" % route)


@pytest.mark.parametrize("fmt", ("q5_0", "q5_1"))
def test_rows_of_different_states_stay_with_the_general_kernel(dev, fmt):
    """With wa_epi::rowp set a product of 17 rows does not take the matrix-core kernel, by its own rule or when route 3 asks for it - and each row's
    key and value land in its own state's cell, whichever route was named."""
    for route in (0, 3):
        assert route_lib().qmtest_kernel(route, QC.DEC_QKV, EPI_M, EPI_N, 128, 1) == 1, route
    assert route_lib().qmtest_kernel(3, QC.DEC_QKV, EPI_M, EPI_N, 128, 0) == 3
    M, N, d, cells, ld2, ld3 = EPI_M, EPI_N, 16, 4, 18, 20
    w, x, bias, scale, _, val = epi_case("DEC_QKV", fmt, 4)
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, wm is not None)
    p_bias, p_scale = dev.put(bias), dev.put(scale)
    heads = [(3 * i + 1) % cells for i in range(M)]
    for route in (3, 1):
        p_k = [dev.put(np.full(cells * ld2, SENT16, np.uint16)) for _ in range(M)]
        p_v = [dev.put(np.full(cells * ld3, SENT16, np.uint16)) for _ in range(M)]
        rp = np.zeros(M, ROWPTR)
        for i in range(M):
            rp[i] = (p_k[i], p_v[i], 0, 0, heads[i] + 1, heads[i])
        want_q = np.full((M + 1, 18), SENT16, np.uint16)
        want_q[:M, :d] = val[:, :d]
        p_q = dev.put(np.full_like(want_q, SENT16))
        p_o2, p_o3 = dev.put(np.full(8, SENT16, np.uint16)), dev.put(np.full(8, SENT16, np.uint16))      # not used with rowp set: their sentinel must survive
        e = FrEpi(bias=p_bias, scale=p_scale, out=p_q, ldo=18, out2=p_o2, ldo2=ld2, out3=p_o3, ldo3=ld3, split0=d, split1=2 * d, row_off=2,
                  rowp=dev.put(rp), rowp_off=0)
        lib().frtest_qgemm(route, QC.DEC_QKV, xq, xd, M, wq, wd, N, 128, C.byref(e), xs, wm)
        sync()
        assert_same(Dev.get(p_q, want_q), want_q, "route %d %s q" % (route, fmt))
        for p in (p_o2, p_o3):
            assert_same(Dev.get(p, np.empty(8, np.uint16)), np.full(8, SENT16, np.uint16), "route %d out2 / out3" % route)
        for i in range(M):
            wk, wv = np.full(cells * ld2, SENT16, np.uint16), np.full(cells * ld3, SENT16, np.uint16)
            wk[heads[i] * ld2:][:d] = val[i, d:2 * d]
            wv[heads[i] * ld3:][:d] = val[i, 2 * d:]
            assert_same(Dev.get(p_k[i], wk), wk, "route %d %s key buffer of row %d" % (route, fmt, i))
            assert_same(Dev.get(p_v[i], wv), wv, "route %d %s value buffer of row %d" % (route, fmt, i))

"""Inputs, layouts and expected values for the kernel-by-kernel tests of wa_quant.hip (tests/test_quant_kernels_gpu.py runs them on the
GPU, tests/test_quant_kernels_math.py shows on the CPU that they tell a wrong kernel from a right one).

Everything is generated from seeded numpy; no fixture file.  The operands of the products are DICTATED - quants, scales, minimums and
block sums are chosen directly, not produced by the quantiser under test - so that they reach what a model's weights and activations
never do: scales of both signs spread over several binades (where summation order and a fused multiply-add matter), subnormal halfs,
zeros, Q8_0 bytes of -128, saturated rows, block sums of +-inf.  The expected values come from tests/native/libquant_ref.so (variant 0:
wa_quant1.h and the Q5_0 / Q8_0 product beside it, pinned to the reference library by tests/native/quant_ref_pin.cpp); its variants
1.. are deliberately wrong and serve the CPU test only.

Layouts: host side everything is plain, quants [rows][K] with K = 32 nb; the kernels read quants as qs [row][8][K/32][4] (lane l of a
dot product owns elements 4l .. 4l+3 of every block) and qd / qm / qsum as [row][K/32].
"""
import ctypes as C
import functools
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB_PATH = os.path.join(ROOT, "tests", "native", "libquant_ref.so")
f32 = np.float32

# wa_kernels.h: wa_epi_mode
F16, ENC_QKV, GELU_F16, RESID, CONV2, F32, CROSS_KV, GELU_F32, DEC_QKV = range(9)

# variants of libquant_ref.so (tests/native/quant_ref.cpp)
DOT_VARIANTS = {"hsum in linear order": 1, "fmaf as a multiplication and an addition": 2, "minimum chain fused": 3, "minimum chain without block 0": 4}
DOT_VARIANTS_Q1_ONLY = ("minimum chain fused", "minimum chain without block 0")
Q_VARIANTS = {"ties away from zero": 1, "id = 1 / d": 2, "s from the rounded d": 3, "s summed in float": 4}
Q_VARIANTS_S_ONLY = ("s from the rounded d", "s summed in float")          # change qsum only: asked where qsum is an output

FORMATS = {"q8_0": (-128, 127, False), "q5_0": (-16, 15, False), "q5_1": (0, 31, True), "q4_1": (0, 15, True)}       # lowest, highest quant, has a minimum

_REF = None


def ref():
    global _REF
    if _REF is None:
        assert os.path.exists(REF_LIB_PATH), "%s missing: build() makes it (oracle/Makefile, target harness)" % REF_LIB_PATH
        L = C.CDLL(REF_LIB_PATH)
        vp, i = C.c_void_p, C.c_int
        L.qref_gemm.argtypes = [i, i, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.qref_quantize.argtypes = [i, vp, i, i, i, vp, vp, vp]
        L.qref_dequant.argtypes = [i, vp, vp, vp, vp]
        L.qref_dequant.restype = None
        _REF = L
    return _REF


def _ptr(a):
    return None if a is None else a.ctypes.data


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """Element-wise: the same F32 bits, or both NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits32(a) == bits32(b)) | (np.isnan(a) & np.isnan(b))


def f16r(x):
    """Round to the nearest F16 value, as F32 (overflow gives inf)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------------
def pack_qs(q):
    """int8 [rows][K] -> the kernel layout [rows][8][K/32][4]."""
    rows, K = q.shape
    return np.ascontiguousarray(q.reshape(rows, K // 32, 8, 4).transpose(0, 2, 1, 3))


def unpack_qs(qs):
    """The kernel layout [rows][8][nb][4] -> int8 [rows][32 nb]."""
    rows, _, nb, _ = qs.shape
    return np.ascontiguousarray(qs.transpose(0, 2, 1, 3)).reshape(rows, nb * 32)


# ----------------------------------------------------------------------------------------------------------------------------
# the host reference
# ----------------------------------------------------------------------------------------------------------------------------
def ref_gemm(w, x, variant=0):
    """out f32 [M][N] of weights w = {q [N][K], d [N][nb], m [N][nb] or None} and activations x = {q [M][K], d [M][nb], s [M][nb]}."""
    N, K = w["q"].shape
    M = x["q"].shape[0]
    out = np.empty((M, N), np.float32)
    q1 = w["m"] is not None
    arrs = [np.ascontiguousarray(a) for a in (w["q"], w["d"], w["m"] if q1 else np.zeros(1, f32), x["q"], x["d"], x["s"])]
    rc = ref().qref_gemm(variant, M, N, K // 32, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]) if q1 else None, _ptr(arrs[3]), _ptr(arrs[4]),
                         _ptr(arrs[5]) if q1 else None, _ptr(out))
    assert rc == 0, "qref_gemm refused variant %d" % variant
    return out


def ref_quantize(X, variant=0):
    """quantize_row_q8_1 of F32 rows X [rows][K]: q int8 [rows][K], d, s f32 [rows][K/32] (the F32 values of their F16 fields)."""
    X = np.ascontiguousarray(X, np.float32)
    rows, K = X.shape
    q = np.empty((rows, K), np.int8)
    d = np.empty((rows, K // 32), np.float32)
    s = np.empty((rows, K // 32), np.float32)
    rc = ref().qref_quantize(variant, _ptr(X), K, rows, K // 32, _ptr(q), _ptr(d), _ptr(s))
    assert rc == 0, "qref_quantize refused variant %d" % variant
    return q, d, s


def ref_dequant(q, d, m=None):
    q, d = np.ascontiguousarray(q, np.int8), np.ascontiguousarray(d, np.float32)
    m = None if m is None else np.ascontiguousarray(m, np.float32)
    out = np.empty(q.shape, np.float32)
    ref().qref_dequant(q.size, _ptr(q), _ptr(d), _ptr(m), _ptr(out))
    return out


def gelu_table():
    """The loader's table (wa_loader.cpp: gelu_f32 at every F16 value, rounded to F16).  The kernels only look it up."""
    x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        g = np.float32(0.5) * x * (np.float32(1) + np.tanh(np.float32(0.79788456080286535587989211986876) * x *
                                                             (np.float32(1) + np.float32(0.044715) * x * x)))
    return g.astype(np.float16).view(np.uint16)


GELU = gelu_table()


def gelu32(v):
    """wa_gelu on F32 values: the table at f16(v), identity at >= 10, zero at <= -10."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore"):
        t = GELU[v.astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)
    return np.where(v <= -10, np.float32(0), np.where(v >= 10, v, t)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# operands of the products
# ----------------------------------------------------------------------------------------------------------------------------
def f16_values(rng, shape, lo, hi, signed=True):
    """F16-representable values: a random 11-bit significand times 2^e, e drawn per value from [lo, hi) - neighbouring blocks lie
    binades apart -, of both signs; one in 16 a subnormal half (k 2^-24), one in 16 zero."""
    mag = rng.integers(1024, 2048, size=shape).astype(np.float64) * 2.0 ** (rng.integers(lo, hi, size=shape) - 10.0)
    pick = rng.integers(0, 16, size=shape)
    mag = np.where(pick == 0, rng.integers(1, 1024, size=shape) * 2.0 ** -24, np.where(pick == 1, 0.0, mag))
    sign = np.where(rng.integers(0, 2, size=shape) == 1, -1.0, 1.0) if signed else 1.0
    v = (sign * mag).astype(np.float32)
    assert np.array_equal(bits32(v), bits32(f16r(v)))
    return v


def off_f16(a, rng):
    """The values moved off the F16 grid by a relative 2^-13 .. 2^-12: all 24 bits of the significand in use."""
    return (a * (1 + rng.uniform(2.0 ** -13, 2.0 ** -12, size=a.shape))).astype(np.float32)


def weights(fmt, N, nb, rng, lo=-9, hi=3):
    """Weight rows of a format: quants over its whole range (both extremes forced into every row), scales and minimums as f16_values."""
    qlo, qhi, q1 = FORMATS[fmt]
    q = rng.integers(qlo, qhi + 1, size=(N, nb * 32)).astype(np.int8)
    q[:, 0] = qlo
    q[:, -1] = qhi
    return {"fmt": fmt, "q": q, "d": f16_values(rng, (N, nb), lo, hi), "m": f16_values(rng, (N, nb), lo + 2, hi + 2) if q1 else None}


def zero_rows(w, rows):
    """Weight rows whose scales (and minimums) are zero: the product is +0 exactly, so bias[n] IS the pre-activation."""
    w["d"][rows] = 0.0
    if w["m"] is not None:
        w["m"][rows] = 0.0


def activations(kind, M, nb, rng, w=None):
    """Activation rows: quants -127 .. 127, d and s F16-representable.
    random      s = f16(d * sum q) in most blocks, an arbitrary F16 value in one of eight
    random_inf  the same with s = +-inf in a few blocks (the outputs of a product with a minimum are inf or NaN there)
    saturated   every quant +-127, the sign alternating from lane to lane; weight row 0 (when w is given) is put at the format's lowest
                quant throughout, so sum4 reaches -+4 * 127 * 128 with Q8_0
    minchain    kind (d) of quant1_math.cpp, dictated: quants of one magnitude class with every third negative, so that s is large, and
                (when w is given) weights of a tiny negative scale under a minimum near 0.9 - the minimum chain is far from the lane
                sums and of the opposite sign
    minchain_f32  minchain with minimums that are NOT F16 values.  The product of two F16 values is exact in F32 (11 x 11 bits), so within
                the F16 set a fused minimum chain and the stated one - a multiplication, then an addition - are the same function;
                the kernels read the minimums as F32, and this kind uses that to hold them to the statement (wa_quant1.h)"""
    K = nb * 32
    if kind in ("random", "random_inf"):
        q = rng.integers(-127, 128, size=(M, K))
        d = f16_values(rng, (M, nb), -6, 4, signed=False)
    elif kind == "saturated":
        q = np.tile(np.repeat(np.array([127, -127]), 4), (M, K // 8)) * np.where(rng.integers(0, 2, size=(M, 1)) == 1, -1, 1)
        d = f16_values(rng, (M, nb), -6, 4, signed=False)
        if w is not None:
            w["q"][0, :] = FORMATS[w["fmt"]][0]
    elif kind in ("minchain", "minchain_f32"):
        q = rng.integers(60, 128, size=(M, K))
        q[:, ::3] *= -1
        d = f16r(rng.uniform(0.03, 0.09, size=(M, nb)))
        if w is not None:
            w["d"][:] = -f16r(rng.uniform(0.0005, 0.004, size=w["d"].shape))
            if w["m"] is not None:
                w["m"][:] = f16r(rng.uniform(0.85, 0.93, size=w["m"].shape))
                if kind == "minchain_f32":
                    w["m"][:] = off_f16(w["m"], rng)
    else:
        raise ValueError(kind)
    q = q.astype(np.int8)
    s = f16r(d * q.reshape(M, nb, 32).sum(-1).astype(np.float32))
    if kind in ("random", "random_inf"):
        other = f16_values(rng, (M, nb), -4, 12)
        s = np.where(rng.integers(0, 8, size=(M, nb)) == 0, other, s)
    if kind == "random_inf":
        for _ in range(max(1, M * nb // 8)):
            s[rng.integers(0, M), rng.integers(0, nb)] = np.float32(np.inf) * (1 if rng.integers(0, 2) else -1)
    return {"kind": kind, "q": q, "d": d.astype(np.float32), "s": s.astype(np.float32)}


ACT_KINDS = ("random", "saturated", "minchain", "minchain_f32", "random_inf")


def loop_class(nb):
    """The loop of wq_row_dot / k_qgemm_exact a block count takes."""
    return "pipelined" if nb % 4 == 0 else "block-by-block"


def family(fmt):
    return "Q1" if FORMATS[fmt][2] else "Q0"


# ---- the one-row product: WA_EPI_F32 without bias ---------------------------------------------------------------------------
GEMV_NB = (1, 2, 3, 5, 6, 4, 8, 12, 16, 20, 24, 36, 96)
GEMV_N = (1, 7, 8, 13, 40)
GEMV_CASES = [{"name": "gemv_%s_nb%d_N%d" % (fmt, nb, N), "fmt": fmt, "nb": nb, "N": N, "M": 1, "kind": ACT_KINDS[(i + j) % 5]}
              for fmt in FORMATS for i, nb in enumerate(GEMV_NB) for j, N in enumerate(GEMV_N)]

# ---- the 8-row product ------------------------------------------------------------------------------------------------------
GEMM_M = (2, 8, 9, 17)
GEMM_N = (5, 32, 33, 70)
GEMM_NB = (1, 3, 4, 6, 8, 24)
GEMM_CASES = [{"name": "gemm_%s_nb%d_M%d_N%d" % (fam, nb, M, N), "fmt": (("q8_0", "q5_0") if fam == "Q0" else ("q5_1", "q4_1"))[(i + j + k) % 2],
               "nb": nb, "N": N, "M": M, "kind": ACT_KINDS[(i + j + k) % 5]}
              for fam in ("Q0", "Q1") for i, nb in enumerate(GEMM_NB) for j, M in enumerate(GEMM_M) for k, N in enumerate(GEMM_N)]
# K = 5120 (the second MLP product of a d = 1280 model): with a minimum the activation tile needs 51 200 B of LDS, above the 48 KiB a
# kernel gets unasked, so the launcher raises the limit; without a minimum it needs 46 080 B and does not
GEMM_BIG_CASES = [{"name": "gemm_q5_1_K5120", "fmt": "q5_1", "nb": 160, "N": 40, "M": 9, "kind": "random"},
                  {"name": "gemm_q8_0_K5120", "fmt": "q8_0", "nb": 160, "N": 40, "M": 9, "kind": "random"}]


@functools.lru_cache(maxsize=None)
def _product_case(name, fmt, nb, N, M, kind, lo, hi):
    rng = rng_for(name)
    w = weights(fmt, N, nb, rng, lo, hi)
    x = activations(kind, M, nb, rng, w)
    for a in (w["q"], w["d"], w["m"], x["q"], x["d"], x["s"]):
        if a is not None:
            a.setflags(write=False)
    return w, x


def product_operands(c, lo=-9, hi=3):
    """(weights, activations) of a product case; built once, read-only."""
    return _product_case(c["name"], c["fmt"], c["nb"], c["N"], c["M"], c["kind"], lo, hi)


# ---- the quantiser ----------------------------------------------------------------------------------------------------------
QUANT_CASES = [{"name": "quantize_%dx%d" % (rows, K), "rows": rows, "K": K, "ldx": K + 8} for rows, K in ((1, 32), (3, 96), (9, 128), (5, 160), (2, 3072))]


def tie_block(rng, positive_from=None):
    """32 values whose quants sit exactly on ties of rint, chosen so that a wrong inverse scale shows as well: element 0 is the block's
    maximum a, picked so that 127 / a and 1 / (a / 127) are different floats; the others are y with y * (127 / a) == k + 0.5 exactly
    and y * (1 / (a / 127)) on the side of the tie that rounds the other way.  positive_from: only values >= it (the output of a GELU
    at >= 10 is its argument), else both signs."""
    one, c127 = np.float32(1), np.float32(127)
    for _ in range(1000):
        a = np.float32(rng.uniform(600.0, 4000.0))
        idg, idb = c127 / a, one / (a / c127)
        if idg == idb:
            continue
        k = np.arange(2, 126, dtype=np.float32) + np.float32(0.5)
        y0 = (k / idg).astype(np.float32)
        found, exact = [], []
        for step in range(-3, 4):
            y = y0
            for _ in range(abs(step)):
                y = np.nextafter(y, np.float32(np.inf if step > 0 else -np.inf))
            tg, tb = (y * idg).astype(np.float32), (y * idb).astype(np.float32)
            hit = tg == k
            if positive_from is not None:
                hit &= y >= positive_from
            exact += y[hit].tolist()
            found += y[hit & (np.rint(tb) != np.rint(tg)) & (np.floor(tg) % 2 == 0)].tolist()      # a tie towards an even quant below it: roundf goes up
        found, exact = sorted(set(found)), sorted(set(exact))
        if len(found) >= 6 and len(exact) >= 12:
            pick = np.array([found[i % len(found)] if i % 3 != 2 else exact[(5 * i) % len(exact)] for i in range(31)], np.float32)
            if positive_from is None:
                pick[1::2] *= -1
            blk = np.concatenate([[a], pick]).astype(np.float32)
            assert np.abs(blk).max() == a
            return blk
    raise AssertionError("no tie block found")


def s_edge_block(rng):
    """A Gaussian block whose d * sum q lies so close to the midpoint of two F16 values that a block sum accumulated in float from the
    products d * q lands on the other side (a seeded search over Gaussian blocks: about one in a few hundred is such a block)."""
    for _ in range(64):
        X = (rng.standard_normal((4096, 32)) * 2.0 ** rng.integers(-3, 6, size=(4096, 1))).astype(np.float32)
        s0, s4 = ref_quantize(X)[2], ref_quantize(X, Q_VARIANTS["s summed in float"])[2]
        hit = np.flatnonzero(~same_bits(s0, s4).ravel())
        if hit.size:
            return X[hit[0]]
    raise AssertionError("no block found")


def quant_block(kind, rng, rep=0):
    """One 32-value block of a quantiser row.  Kinds 0 .. 7 are the rounding points of quant1_math.cpp section (c)."""
    e = np.arange(32)
    if kind == "gauss1":
        return rng.standard_normal(32)
    if kind == "gauss37":
        return 37.5 * rng.standard_normal(32)
    if kind == "gauss1e-3":
        return 1e-3 * rng.standard_normal(32)
    if kind == 0:
        return np.zeros(32)                                                 # id = 0
    if kind == 1:
        return np.where(e == 0, 127.0, (e - 16) + 0.5)                      # id = 1: every quant at a tie of rint
    if kind == 2:
        return np.where(e == 0, -254.0, 2.0 * e - 31)                       # id = 0.5: ties again, negative maximum
    if kind == 3:
        return np.full(32, 2047.0)                                          # s = d * 4064 close to the F16 limit 65504
    if kind == 4:
        return np.full(32, 2047.5 + 0.25 * rep)                             # ... at the limit
    if kind == 5:
        return np.full(32, -3000.0)                                         # beyond it
    if kind == 6:
        return np.where(e & 1, 65000.0, 64999.0)                            # d itself stays finite, s does not
    if kind == 7:
        return 1e-7 * rng.uniform(-1, 1, 32)                                # d a subnormal half
    if kind == "negzero":
        x = rng.standard_normal(32)
        x[[3, 17]] = -0.0
        return x
    if kind == "allnegzero":
        return np.full(32, -0.0)                                            # a == 0 although no element is +0
    if kind == "negmax":
        x = rng.uniform(-1, 1, 32)
        x[11] = -2.5                                                        # the maximum is negative and unique: its quant is -127
        return x
    if kind == "1e7":
        return 1e7 * rng.uniform(0.5, 1, 32) * np.where(e & 1, -1, 1)       # d becomes an F16 infinity
    if kind == "tie":
        return tie_block(rng)
    if kind == "s_edge":
        return s_edge_block(rng)
    raise ValueError(kind)


QUANT_BLOCK_KINDS = ("tie", "gauss1", "s_edge", 1, "gauss37", 2, "gauss1e-3", 0, 3, "negzero", 4, 5, "negmax", 6, 7, "1e7", "allnegzero")
TIE_KINDS = ("tie", 1, 2)


@functools.lru_cache(maxsize=None)
def _quant_rows(name, rows, K):
    rng = rng_for(name)
    nb = K // 32
    kinds = [[QUANT_BLOCK_KINDS[(r * nb + b) % len(QUANT_BLOCK_KINDS)] for b in range(nb)] for r in range(rows)]
    X = np.stack([np.concatenate([quant_block(kinds[r][b], rng, b // 8) for b in range(nb)]) for r in range(rows)]).astype(np.float32)
    a = np.abs(X.reshape(rows, nb, 32)).max(-1)
    assert np.all((a == 0) | (a >= 2.0 ** -120))            # below that 127 / a overflows: outside the contract of wa_q8_store
    assert not np.isnan(X).any()
    X.setflags(write=False)
    return X, kinds


def quant_rows(c):
    """(X f32 [rows][K], the kind of every block) of a quantiser case."""
    return _quant_rows(c["name"], c["rows"], c["K"])


# ---- the fused GELU product -------------------------------------------------------------------------------------------------
GELU_CASES = [{"name": "gelu_q8_%s_nb%d_N%d" % (fmt, nb, N), "fmt": fmt, "nb": nb, "N": N, "M": 1, "kind": "random"}
              for fmt in ("q8_0", "q5_1") for nb in (3, 4, 20) for N in (32, 96)]
GELU_BLOCK_KINDS = ("zero", "big", "tie")


def gelu_block_kinds(c):
    """What each 32-output block of a case holds after the GELU (N = 32 has one block: its kind goes round with nb, so that both loop
    classes see a block that depends on the product)."""
    nblk = c["N"] // 32
    return [GELU_BLOCK_KINDS[(b + ({3: 1, 4: 2, 20: 0}[c["nb"]] if nblk == 1 else 0)) % 3] for b in range(nblk)]


@functools.lru_cache(maxsize=None)
def _gelu_case(name, fmt, nb, N):
    rng = rng_for(name)
    c = {"name": name, "nb": nb, "N": N}
    w = weights(fmt, N, nb, rng, -6, 2)
    x = activations("random", 1, nb, rng)
    x["s"] = f16r(x["d"] * x["q"].reshape(1, nb, 32).sum(-1).astype(np.float32))
    kinds = gelu_block_kinds(c)
    for b, kind in enumerate(kinds):
        if kind == "tie":
            zero_rows(w, np.arange(32 * b, 32 * b + 32))
        elif kind == "zero":
            zero_rows(w, np.arange(32 * b, 32 * b + 4))
        else:
            zero_rows(w, [32 * b + 5])                     # the block's maximum: a pre-activation >= 10 placed through the bias
    # scale the weights by a power of two until a typical product is about 2^21: one ulp of it is then 0.25, which the Q8 quantisation of
    # an output block whose largest value is about 12 resolves (a step is 0.1) - so a product that is one ulp off changes a quant
    dot = ref_gemm(w, x)[0]
    live = np.abs(dot[np.isfinite(dot) & (dot != 0)])
    k = int(np.round(21 - np.log2(np.median(live)))) if live.size else 0
    for a in (w["d"], w["m"]):
        if a is not None:
            a[:] = f16r(a * np.float32(2.0 ** k))
            assert np.all(np.isfinite(a))
    if w["m"] is not None:
        w["m"][1::2] = off_f16(w["m"][1::2], rng)          # odd rows: minimums off the F16 grid (activations(): minchain_f32)
    dot = ref_gemm(w, x)[0]
    assert np.all(np.isfinite(dot))
    bias = np.zeros(N, np.float32)
    for b, kind in enumerate(kinds):
        sl = slice(32 * b, 32 * b + 32)
        if kind == "tie":
            bias[sl] = tie_block(rng, positive_from=10.0)                         # zero rows: the pre-activation is the bias, and >= 10
        elif kind == "zero":
            bias[sl] = -(2 * np.abs(dot[sl]) + 20 + rng.uniform(0, 5, 32)).astype(np.float32)
            bias[32 * b:32 * b + 4] = [-10.0, -10.5, np.nextafter(f32(-10), f32(-np.inf)), -65536.0]
        else:
            # pre-activations of both signs below 10 and one above.  With a minimum the block sum is an output too: the draw is repeated
            # until the block is one whose sum tells the wrong ways of forming it from the right one (s_edge_block)
            T = 8192 if w["m"] is not None else 1
            for _ in range(64):
                target = rng.uniform(0.3, 6.0, (T, 32)) * np.where(rng.integers(0, 2, (T, 32)) == 1, -1, 1)
                target[:, 5] = rng.uniform(10.0, 14.0, T)                         # >= 10: the GELU is the identity there
                cand = (target - dot[sl].astype(np.float64)[None, :]).astype(np.float32)
                g = gelu32(dot[sl][None, :] + cand)
                ok = np.ones(T, bool)
                if w["m"] is not None:
                    s0 = ref_quantize(g)[2]
                    for v in Q_VARIANTS_S_ONLY:
                        ok &= ~same_bits(s0, ref_quantize(g, Q_VARIANTS[v])[2]).ravel()
                if ok.any():
                    bias[sl] = cand[np.flatnonzero(ok)[0]]
                    break
            else:
                raise AssertionError("no bias found")
    for a in (w["q"], w["d"], w["m"], x["q"], x["d"], x["s"], bias):
        if a is not None:
            a.setflags(write=False)
    return w, x, bias, kinds


def gelu_operands(c):
    return _gelu_case(c["name"], c["fmt"], c["nb"], c["N"])


def gelu_expected(c, dot_variant=0, q_variant=0):
    """The host quantiser applied to gelu32(dot + bias): (g f32 [N], q int8 [1][N], d, s f32 [1][N/32])."""
    w, x, bias, _ = gelu_operands(c)
    g = gelu32(ref_gemm(w, x, dot_variant)[0] + bias)
    return (g,) + ref_quantize(g[None, :], q_variant)


# ---- the epilogues: one shape, M = 9 and M = 1, both families -------------------------------------------------------------------
EPI_N, EPI_NB = 70, 4
EPI_MODES = {"F32_bias": F32, "RESID": RESID, "GELU_F32": GELU_F32, "F16_scale": F16, "ENC_QKV": ENC_QKV, "DEC_QKV": DEC_QKV, "CROSS_KV": CROSS_KV}
EPI_CASES = [{"name": "epi_%s_%s_M%d" % (mode, fmt, M), "epi": mode, "mode": EPI_MODES[mode], "fmt": fmt, "nb": EPI_NB, "N": EPI_N, "M": M, "kind": "random"}
             for mode in EPI_MODES for fmt in ("q5_0", "q4_1") for M in (9, 1)]
EPI_TPAD = 16             # aux0 of CROSS_KV: rows per head of the cross K / V buffers (>= M)
EPI_HEAD_D = 64           # aux1 of CROSS_KV: the model width d; N = 70 < 2 d, so every n is layer 0: K head 0 below 64, V head 0 from 64 on
# pre-activations of the GELU epilogue, placed through the bias of rows whose product is +0: the ends of the table's range exactly and
# just inside (f16(9.999999) is 10: the comparison must come before the rounding), a tiny negative value whose F16 is -0.0 (table index
# 0x8000; -0.0 itself cannot be reached, +0 + -0 is +0), and values beyond the F16 range (identity above, zero below)
GELU_EDGES = (10.0, -10.0, float(np.nextafter(f32(10), f32(0))), float(np.nextafter(f32(-10), f32(0))), -1e-30, -0.0, 0.0, 70000.0, -70000.0, 65520.0, 9.9975,
              -9.9975, 1e-8)


@functools.lru_cache(maxsize=None)
def _epi_case(name, epi, fmt, M):
    rng = rng_for(name)
    N, nb = EPI_N, EPI_NB
    # moderate scales: the F16 outputs stay finite and every bit of them depends on the product
    w = weights(fmt, N, nb, rng, -9, -5)
    x = activations("random", M, nb, rng)
    x["d"] = f16_values(rng, (M, nb), -5, -2, signed=False)
    x["s"] = f16r(x["d"] * x["q"].reshape(M, nb, 32).sum(-1).astype(np.float32))
    ops = {"bias": (rng.standard_normal(N) * 0.5).astype(np.float32), "scale": None, "resid": None}
    if epi in ("F16_scale", "DEC_QKV", "CROSS_KV"):
        ops["scale"] = rng.uniform(0.25, 1.5, N).astype(np.float32)
    if epi == "RESID":
        ops["resid"] = (rng.standard_normal((M, N + 5)) * 2).astype(np.float32)          # ldr = N + 5
    if epi == "GELU_F32":
        rows = np.arange(3, 3 + 5 * len(GELU_EDGES), 5)                                  # n = 3, 8, .. 63: in both 32-row tiles
        zero_rows(w, rows)
        ops["bias"] = (rng.standard_normal(N) * 3).astype(np.float32)
        ops["bias"][rows] = np.array(GELU_EDGES, np.float32)
    return w, x, ops


def epi_operands(c):
    return _epi_case(c["name"], c["epi"], c["fmt"], c["M"])


def epi_layout(c):
    """Output buffers of an epilogue case: name -> (element count, 'f16' or 'f32'), and the launch's scalar fields."""
    M, N, epi = c["M"], c["N"], c["epi"]
    if epi in ("F32_bias", "RESID", "GELU_F32"):
        return {"out": (M * (N + 6), "f32")}, {"ldo": N + 6, "ldr": N + 5 if epi == "RESID" else 0}
    if epi == "F16_scale":
        return {"out": (M * (N + 6), "f16")}, {"ldo": N + 6}
    if epi == "ENC_QKV":
        return {"out": (M * 40, "f16"), "out2": ((N - 32) * (M + 7), "f16")}, {"ldo": 40, "split0": 32, "ldo2": M + 7}
    if epi == "DEC_QKV":
        return ({"out": (M * 30, "f16"), "out2": ((3 + M + 1) * 28, "f16"), "out3": ((3 + M + 1) * 26, "f16")},
                {"ldo": 30, "split0": 24, "split1": 48, "row_off": 3, "ldo2": 28, "ldo3": 26})
    if epi == "CROSS_KV":
        return {"out": (EPI_TPAD * 64, "f16"), "out2": (EPI_TPAD * 64, "f16")}, {"aux0": EPI_TPAD, "aux1": EPI_HEAD_D}
    raise ValueError(epi)


def epi_out_index(c, f, m, n):
    """(buffer name index, flat element index, buffer names) of result (m, n) as the epilogue stores it (wa_device.h: epi_apply)."""
    epi = c["epi"]
    if epi == "ENC_QKV":
        s0 = f["split0"]
        return np.where(n < s0, 0, 1), np.where(n < s0, m * f["ldo"] + n, (n - s0) * f["ldo2"] + m), ("out", "out2")
    if epi == "CROSS_KV":
        d = f["aux1"]
        il, r = n // (2 * d), n % (2 * d)
        kv = (r >= d).astype(np.int64)
        rr = r - kv * d
        return kv, ((il * (d // 64) + rr // 64) * f["aux0"] + m) * 64 + rr % 64, ("out", "out2")
    if epi == "DEC_QKV":
        s0, s1, ro = f["split0"], f["split1"], f["row_off"]
        which = np.where(n < s0, 0, np.where(n < s1, 1, 2))
        idx = np.where(n < s0, m * f["ldo"] + n, np.where(n < s1, (ro + m) * f["ldo2"] + n - s0, (ro + m) * f["ldo3"] + n - s1))
        return which, idx, ("out", "out2", "out3")
    return np.zeros_like(n), m * f["ldo"] + n, ("out",)


def epi_expected(c, variant=0):
    """The epilogue on the host product, in float32 (one rounding per operation, as the kernel with contraction off): [M][N], F32, or
    F16 bits as uint16 where the mode stores F16."""
    w, x, ops = epi_operands(c)
    epi = c["epi"]
    with np.errstate(over="ignore", invalid="ignore"):
        v = ref_gemm(w, x, variant)
        if ops["bias"] is not None:
            v = v + ops["bias"][None, :]
        if ops["scale"] is not None:
            v = v * ops["scale"][None, :]
        if epi == "RESID":
            v = v + ops["resid"][:, :c["N"]]
        if epi == "GELU_F32":
            v = gelu32(v)
        if epi in ("F16_scale", "ENC_QKV", "DEC_QKV", "CROSS_KV"):
            return v.astype(np.float32).astype(np.float16).view(np.uint16)
    return v.astype(np.float32)


# ---- the quantised token embedding ------------------------------------------------------------------------------------------
EMBED_CASES = [{"name": "embed_%s_d%d" % (fmt, d), "fmt": fmt, "d": d, "n_vocab": 50, "n_pos": 12} for fmt in ("q8_0", "q5_1") for d in (96, 128)]


@functools.lru_cache(maxsize=None)
def _embed_case(name, fmt, d, n_vocab, n_pos):
    rng = rng_for(name)
    w = weights(fmt, n_vocab, d // 32, rng, -9, 1)
    pe = rng.standard_normal((n_pos, d)).astype(np.float32)
    pe[2, :8] = [0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 2.0 ** -140, 1.0]
    tok = np.array([0, n_vocab - 1, 7, n_vocab - 1, 23, 0, 31], np.int32)               # row 0, the last row, repeats
    pos = np.array([5, 0, 11, 2, 2, 9, 1], np.int32)                                    # out of order, one repeated
    return w, pe, tok, pos


def embed_operands(c):
    return _embed_case(c["name"], c["fmt"], c["d"], c["n_vocab"], c["n_pos"])


def embed_expected(c):
    """ggml_get_rows of the quantised matrix, then + pe: q * d, (+ m,) + pe - one float32 rounding each."""
    w, pe, tok, pos = embed_operands(c)
    d = np.repeat(w["d"][tok], 32, axis=1)
    v = (w["q"][tok].astype(np.float32) * d).astype(np.float32)
    if w["m"] is not None:
        v = (v + np.repeat(w["m"][tok], 32, axis=1)).astype(np.float32)
        assert np.array_equal(bits32(v), bits32(ref_dequant(w["q"][tok], d, np.repeat(w["m"][tok], 32, axis=1))))
    return (v + pe[pos]).astype(np.float32)

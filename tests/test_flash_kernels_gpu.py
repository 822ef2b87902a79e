"""Kernel-level tests of the tolerance path (flash_attn = true): the F16-MFMA launchers of wa_kernels.hip - wa_launch_gemm,
wa_launch_layernorm, wa_launch_enc_attn - each against a float64 numpy restatement of the same operation, at the products' real
widths (d = 384 .. 1280) and at the shapes where tiled kernels go wrong (tile edges, partial tiles, overlapping operand rows).

The kernels are called through tests/native/libflash_kernels.so, which oracle/Makefile links against the product's own
whisper-rust_amd/build/wa_kernels.o.  WA_KTEST_LIB points the tests at another build of that library.

Two kinds of operands per case:
  exact  - small dyadic operands ({-3..3}/4 for GEMMs; 0, +-1 codes and integers for attention).  Every F32 partial sum is then exact
           in any order, so the kernel must match the reference BIT FOR BIT, its epilogue modelled in float32 (one rounding per
           bias add / scale multiply, the F16 GELU table at f16(acc + bias), the F16 output conversion).  This catches any wrong
           index, a dropped or repeated k-stage and a mixed-up tile or layout, however small its numerical effect.
  random - Gaussian F16 operands against float64, within an error bound derived below from the arithmetic of each kernel.
Every output buffer is filled with a sentinel first: whatever lies outside the documented result must still hold it afterwards.
"""
import ctypes as C
import os
import subprocess
import sys
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("WA_KTEST_LIB") or os.path.join(ROOT, "tests", "native", "libflash_kernels.so")

# wa_kernels.h: wa_epi_mode
F16, ENC_QKV, GELU_F16, RESID, CONV2, F32, CROSS_KV, GELU_F32, DEC_QKV, ATTN_PV = range(10)
MODE_NAME = {F16: "F16", ENC_QKV: "ENC_QKV", GELU_F16: "GELU_F16", RESID: "RESID", CONV2: "CONV2", F32: "F32", CROSS_KV: "CROSS_KV",
             DEC_QKV: "DEC_QKV"}
# The modes wa_launch_gemm has a case for.  GELU_F32 and ATTN_PV launch nothing there (wa_kernels.h) and stay out of the tables.
GEMM_MODES = tuple(MODE_NAME)

U32 = 2.0 ** -24            # unit roundoff of F32
U16 = 2.0 ** -11            # unit roundoff of F16
SENT16 = np.uint16(0x7E5A)  # sentinels: NaN bit patterns no kernel result can have
SENT32 = np.uint32(0x7FC0DEAD)
TPAD = 1536                 # wa_pad(1500, WA_TPAD = 128): enc_tpad / cross_tpad of every model (wa_encode.cpp:72-74)


# ----------------------------------------------------------------------------------------------------------------------------
# the harness library
# ----------------------------------------------------------------------------------------------------------------------------
class KtEpi(C.Structure):      # tests/native/flash_kernels.hip: ktest_epi
    _fields_ = [("bias", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int), ("out2", C.c_void_p), ("ldo2", C.c_int),
                ("out3", C.c_void_p), ("ldo3", C.c_int), ("resid", C.c_void_p), ("ldr", C.c_int), ("dbg", C.c_void_p), ("gelu", C.c_void_p),
                ("split0", C.c_int), ("split1", C.c_int), ("row_off", C.c_int), ("aux0", C.c_int), ("aux1", C.c_int)]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        assert os.path.exists(LIB_PATH), "%s missing: build() makes it (oracle/Makefile, target harness)" % LIB_PATH
        L = C.CDLL(LIB_PATH)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.ktest_alloc.restype = vp; L.ktest_alloc.argtypes = [C.c_size_t]
        L.ktest_free.argtypes = [vp]
        L.ktest_h2d.argtypes = [vp, vp, C.c_size_t]; L.ktest_d2h.argtypes = [vp, vp, C.c_size_t]
        L.ktest_gemm.argtypes = [i, vp, i, vp, i, i, i, i, C.POINTER(KtEpi)]
        L.ktest_layernorm.argtypes = [vp, i, i, i, vp, vp, f, vp, i, vp, i]
        L.ktest_enc_attn.argtypes = [vp, i, vp, i, i, i, i, f, vp, i]
        _LIB = L
    return _LIB


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


def sync():
    err = lib().ktest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def gelu_table():
    """The loader's table (wa_loader.cpp: gelu_f32 at every F16 value, rounded to F16; ggml-cpu.c:3509-3517).  The kernels only look
    it up, so the reference reads this same array."""
    x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        g = np.float32(0.5) * x * (np.float32(1) + np.tanh(np.float32(0.79788456080286535587989211986876) * x *
                                                             (np.float32(1) + np.float32(0.044715) * x * x)))
    return g.astype(np.float16).view(np.uint16)


GELU = gelu_table()


def gelu32(v):
    """wa_gelu / wa_gelu_nb on F32 values: the table at f16(v), identity at >= 10, zero at <= -10."""
    with np.errstate(over="ignore"):
        t = GELU[v.astype(np.float32).astype(np.float16).view(np.uint16)].view(np.float16).astype(np.float32)
    return np.where(v <= -10, np.float32(0), np.where(v >= 10, v, t)).astype(np.float32)


def ulp16(x):
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(x).astype(np.float16)).astype(np.float64)


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def edge_sample(n, rng, tile=64, extra=48):
    """Every tile-boundary index (0, 63, 64, 127, 128, ..., n-1) plus a seeded random sample."""
    e = set(range(0, n, tile)) | set(range(tile - 1, n, tile)) | {n - 1}
    e |= set(rng.integers(0, n, size=min(extra, n)).tolist())
    return np.array(sorted(e), dtype=np.int64)


# ----------------------------------------------------------------------------------------------------------------------------
# GEMM: the launcher's choice of form, restated (wa_kernels.hip:303-323, wa_launch_gemm)
# ----------------------------------------------------------------------------------------------------------------------------
def gemm_form(c, env=""):
    """env: "" (the default), "128" (WHISPER_AMD_GEMM_128 set) or "reg" (WHISPER_AMD_NO_GEMM_DMA set).
    LDS-DMA form when K % 64 == 0, K / 64 >= 4 (a ring of 4 stages), lda % 8 == 0 and ldw % 8 == 0 (16-byte rows); there the 128-tile
    form only when WHISPER_AMD_GEMM_128 is set, the product has >= 200 tiles of 128 x 128 and no per-element epilogue operand
    (RESID, CONV2); everything else runs in the register-staged form k_gemm_f16<64, 64>."""
    M, N, K = c["M"], c["N"], c["K"]
    if env != "reg" and K % 64 == 0 and K // 64 >= 4 and c["lda"] % 8 == 0 and c["ldw"] % 8 == 0:
        big = ((M + 127) // 128) * ((N + 127) // 128)
        if env == "128" and c["mode"] not in (RESID, CONV2) and big >= 200:
            return "dma128"
        return "dma64"
    return "reg"


REACHABLE = {(f, m) for f in ("reg", "dma64") for m in GEMM_MODES} | {("dma128", m) for m in GEMM_MODES if m not in (RESID, CONV2)}


def G(name, mode, M, N, K, lda=None, ldw=None, **kw):
    return dict(name=name, mode=mode, M=M, N=N, K=K, lda=lda or K, ldw=ldw or K, **kw)


def n_mels_of(d):
    return 128 if d == 1280 else 80          # large-v3's width has 128 mel bands


def encoder_cases(d, T):
    """The encoder's products as wa_encode.cpp:272-381 calls them (flash path), at audio context T."""
    nm = n_mels_of(d)
    kpad = (3 * nm + 31) // 32 * 32          # conv1_kpad (wa_loader.cpp:243): 256 / 384
    layers = 4 if d <= 512 else 2
    t = "d%d T%d" % (d, T)
    return [
        # conv1: row t reads mel rows t..t+2 as one run of the time-major window (lda = n_mels, overlapping rows); weight columns
        # past 3 n_mels are zero
        G("conv1 " + t, GELU_F16, 2 * T, d, kpad, lda=nm, conv1=nm),
        # conv2: row t reads h1 rows 2t..2t+2 (lda = 2d), + positional embedding, GELU values also into dbg
        G("conv2 " + t, CONV2, T, d, 3 * d, lda=2 * d, conv2=True),
        G("qkv " + t, ENC_QKV, T, 3 * d, d, split0=2 * d),
        G("out " + t, RESID, T, d, d),
        G("fc1 " + t, GELU_F16, T, 4 * d, d),
        G("fc2 " + t, RESID, T, d, 4 * d),
        G("cross_kv %s L%d" % (t, layers), CROSS_KV, T, layers * 2 * d, d, layers=layers),
    ]


def prompt_cases(d, M):
    """A prompt pass of M > 8 rows (wa_decode.cpp:85-99, 124-165): q|k|v into the KV cells at row_off, out / cross_out / fc2 in
    place, cross_q (F16), fc1; plus F16 with a scale and F32, which the launcher serves too."""
    t = "d%d M%d" % (d, M)
    return [
        G("dec_qkv " + t, DEC_QKV, M, 3 * d, d, split0=d, split1=2 * d, row_off=7 + M % 5),
        G("dec_out " + t, RESID, M, d, d),
        G("cross_q " + t, F16, M, d, d),
        G("dec_fc1 " + t, GELU_F16, M, 4 * d, d),
        G("dec_fc2 " + t, RESID, M, d, 4 * d),
        G("f16_scale " + t, F16, M, d, d, scale=True),
        G("f32 " + t, F32, M, d, d),
    ]


WIDTHS = (384, 512, 768, 1024, 1280)
PROMPT_M = {384: (9, 224), 512: (40, 65), 768: (64, 9), 1024: (65, 40), 1280: (224, 64)}
SHORT_T = {384: 50, 768: 257, 1024: 1000}          # reduced audio_ctx (streaming windows)
# products of the launcher that no model call makes but the 128-tile form serves (>= 200 tiles): F16 / F32 / DEC_QKV that wide
WIDE = [G("wide f16_scale M1500", F16, 1500, 2304, 768, scale=True), G("wide f32 M1500", F32, 1500, 2304, 768),
        G("wide dec_qkv M1500", DEC_QKV, 1500, 3072, 1024, split0=1024, split1=2048, row_off=5)]
# register-staged form at K % 32 == 0 but K % 64 != 0 or K < 256 (the s128 / s192 widths and below)
REG_K = [G("reg qkv K128", ENC_QKV, 1500, 384, 128, split0=256), G("reg out K128", RESID, 1500, 128, 128),
         G("reg fc1 K192", GELU_F16, 1500, 768, 192), G("reg conv2 K192", CONV2, 1500, 64, 192, lda=128, conv2=True),
         G("reg cross_kv K192", CROSS_KV, 1500, 2 * 2 * 192, 192, layers=2), G("reg dec_qkv K192", DEC_QKV, 40, 576, 192, split0=192, split1=384, row_off=3),
         G("reg f16_scale K224", F16, 65, 320, 224, scale=True), G("reg f32 K224", F32, 224, 160, 224), G("reg resid K224", RESID, 9, 96, 224)]

GEMM_CASES = ([c for d in WIDTHS for c in encoder_cases(d, 1500)] + [c for d, T in SHORT_T.items() for c in encoder_cases(d, T)] +
              [c for d in WIDTHS for M in PROMPT_M[d] for c in prompt_cases(d, M)] + WIDE + REG_K)
# the forms that need an environment switch, each in a child process of its own: 128-tile cases, and the forced register form at the
# real widths
CHILD_CASES = {"128": [c for c in GEMM_CASES if gemm_form(c, "128") == "dma128"],
               "reg": encoder_cases(384, 1500) + prompt_cases(512, 40)}
CHILD_ENV = {"128": "WHISPER_AMD_GEMM_128", "reg": "WHISPER_AMD_NO_GEMM_DMA"}


def test_case_tables_cover_every_form_and_epilogue():
    assert all(c["mode"] in GEMM_MODES for c in GEMM_CASES)
    covered = {(gemm_form(c), c["mode"]) for c in GEMM_CASES}
    for env, cases in CHILD_CASES.items():
        covered |= {(gemm_form(c, env), c["mode"]) for c in cases}
    assert covered == REACHABLE, sorted(REACHABLE - covered)
    assert {1500, 3000} <= {c["M"] for c in GEMM_CASES} and {9, 40, 64, 65, 224} <= {c["M"] for c in GEMM_CASES if c["mode"] == DEC_QKV}
    assert {128, 192, 224} <= {c["K"] for c in GEMM_CASES if gemm_form(c) == "reg"}
    assert {ln_nv(d) for d in LN_WIDTHS} == {2, 3, 4, 5}
    assert set(ATT_T) <= {T for T, _ in ATT_CASES} and set(ATT_HEADS) <= {h for _, h in ATT_CASES}


def _operand(kind, n, rng, sigma):
    if kind == "exact":
        return (rng.integers(-3, 4, size=n) / 4.0).astype(np.float16)
    return (rng.standard_normal(n) * sigma).astype(np.float16)


def _strided(flat, rows, cols, ld):
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, cols), strides=(ld * flat.itemsize, flat.itemsize))


def _out_index(c, m, n):
    """(buffer name, flat element index) of result (m, n) as the epilogue stores it (wa_device.h: epi_apply)."""
    mode, ldo = c["mode"], c["ldo"]
    if mode == ENC_QKV:
        s0 = c["split0"]
        return np.where(n < s0, 0, 1), np.where(n < s0, m * ldo + n, (n - s0) * c["ldo2"] + m), ("out", "out2")
    if mode == CROSS_KV:
        d = c["N"] // (2 * c["layers"])
        il, r = n // (2 * d), n % (2 * d)
        kv = (r >= d).astype(np.int64)
        rr = r - kv * d
        return kv, ((il * (d // 64) + rr // 64) * TPAD + m) * 64 + rr % 64, ("out", "out2")
    if mode == DEC_QKV:
        s0, s1, ro = c["split0"], c["split1"], c["row_off"]
        which = np.where(n < s0, 0, np.where(n < s1, 1, 2))
        idx = np.where(n < s0, m * ldo + n, np.where(n < s1, (ro + m) * c["ldo2"] + n - s0, (ro + m) * c["ldo3"] + n - s1))
        return which, idx, ("out", "out2", "out3")
    return np.zeros_like(n), m * ldo + n, ("out",)


def _model_exact(c, acc, ops, R, Cn):
    """The epilogue on an exact F32 accumulator, in float32 (one rounding per operation, as the kernel with -ffp-contract=off)."""
    mode = c["mode"]
    v = acc + ops["bias"][Cn][None, :]
    if mode in (F16, CROSS_KV, DEC_QKV) and ops.get("scale") is not None:
        v = v * ops["scale"][Cn][None, :]
    if mode in (F16, ENC_QKV, CROSS_KV, DEC_QKV):
        return {"main": v.astype(np.float16)}
    if mode == GELU_F16:
        return {"main": gelu32(v).astype(np.float16)}
    if mode == RESID:
        return {"main": v + ops["resid"][np.ix_(R, Cn)]}
    if mode == CONV2:
        g = gelu32(v)
        return {"main": ops["resid"][np.ix_(R, Cn)] + g, "dbg": g}
    return {"main": v}          # F32


def _bound_random(c, c64, s64, ops, R, Cn):
    """float64 result and error bound of the epilogue applied to an MFMA accumulator.
    Accumulator: F16 x F16 products are exact in F32; v_mfma_f32_16x16x32_f16 adds 32 of them to the accumulator per step with at most
    about two F32 roundings, each <= 2^-24 of a partial sum <= sum_k |a_k w_k|, over K/32 steps:
        |acc - c64| <= (K/16) 2^-24 sum_k |a_k w_k|       (a dropped 64-deep k-stage is ~ sqrt(64) |a w| away: far outside)
    then one F32 rounding per epilogue operation (<= 2^-24 of its result) and the output's own rounding (F16: 2^-11 relative + 2^-25
    absolute below the normal range).  GELU: the kernel reads the table at f16(v) with v within E of v64; the index moves by at most
    E plus one F16 step, the table's slope is within [-0.17, 1.13], and either entry is rounded to F16."""
    mode, K = c["mode"], c["K"]
    E = (K / 16.0) * U32 * s64
    v = c64 + ops["bias"][Cn].astype(np.float64)[None, :]
    E = E + U32 * (np.abs(v) + E)
    if mode in (F16, CROSS_KV, DEC_QKV) and ops.get("scale") is not None:
        sc = ops["scale"][Cn].astype(np.float64)[None, :]
        v = v * sc
        E = np.abs(sc) * E
        E = E + U32 * (np.abs(v) + E)
    if mode in (F16, ENC_QKV, CROSS_KV, DEC_QKV):
        return {"main": (v, E + U16 * (np.abs(v) + E) + 2.0 ** -25)}
    if mode in (GELU_F16, CONV2):
        g = gelu32(v.astype(np.float32)).astype(np.float64)
        Eg = 1.13 * (E + ulp16(np.abs(v) + E)) + ulp16(np.abs(g) + 1.13 * E)
        if mode == GELU_F16:
            return {"main": (g, Eg + U16 * (np.abs(g) + Eg) + 2.0 ** -25)}
        r = ops["resid"][np.ix_(R, Cn)].astype(np.float64) + g
        return {"main": (r, Eg + U32 * (np.abs(r) + Eg)), "dbg": (g, Eg)}
    if mode == RESID:
        r = v + ops["resid"][np.ix_(R, Cn)].astype(np.float64)
        return {"main": (r, E + U32 * (np.abs(r) + E))}
    return {"main": (v, E + U32 * (np.abs(v) + E))}       # F32


def run_gemm_case(c, kind):
    """Runs one case with one kind of operands; raises AssertionError on a wrong value or a store outside the result.
    Returns the largest |error| / bound of the random kind (0 for exact)."""
    c = dict(c)
    mode, M, N, K, lda, ldw = c["mode"], c["M"], c["N"], c["K"], c["lda"], c["ldw"]
    rng = rng_for(c["name"] + kind)
    f16_out = mode in (F16, ENC_QKV, GELU_F16, CROSS_KV, DEC_QKV)
    c["ldo"] = N + 8 if mode in (F16, GELU_F16, RESID, CONV2, F32) else (2 * (N // 3) if mode == ENC_QKV else N // 3 if mode == DEC_QKV else 0)
    # operands: A as the flat buffer the kernel indexes (row m at m * lda), W likewise
    if c.get("conv1"):
        a_len = (M + 8) * c["conv1"]                    # the mel window: 2T + 8 rows of n_mels (wa_encode.cpp:270)
    elif c.get("conv2"):
        a_len = (2 * M + 2) * N                         # h1: one zero row in front, 2T rows, one behind
    else:
        a_len = (M - 1) * lda + K
    A = _operand(kind, a_len, rng, 1.0)
    W = _operand(kind, N * ldw, rng, 1.0 / np.sqrt(K)).reshape(N, ldw)
    if c.get("conv1"):
        W[:, 3 * c["conv1"]:] = 0                       # the padded weight columns
    ops = {"bias": (rng.standard_normal(N) * 0.5).astype(np.float32)}
    if mode in (CROSS_KV, DEC_QKV) or c.get("scale"):
        ops["scale"] = rng.uniform(0.25, 1.5, N).astype(np.float32)
    if mode in (RESID, CONV2):
        ops["resid"] = (rng.standard_normal((M, N)) * 2).astype(np.float32)

    # output buffers, sentinel-filled
    bufs = {}
    if mode == ENC_QKV:
        c["split0"] = 2 * N // 3; c["ldo2"] = TPAD
        bufs["out"] = np.full(M * c["ldo"], SENT16); bufs["out2"] = np.full((N - c["split0"]) * TPAD, SENT16)
    elif mode == CROSS_KV:
        n = c["layers"] * (N // (2 * c["layers"] * 64)) * TPAD * 64
        bufs["out"] = np.full(n, SENT16); bufs["out2"] = np.full(n, SENT16)
        c["ldo2"] = 0               # CROSS_KV: the layout is [layer][head][aux0 = tpad][64], no leading dimensions
    elif mode == DEC_QKV:
        d = N // 3
        c["ldo2"] = c["ldo3"] = d
        cells = c["row_off"] + M + 16
        bufs["out"] = np.full(M * d, SENT16); bufs["out2"] = np.full(cells * d, SENT16); bufs["out3"] = np.full(cells * d, SENT16)
    elif f16_out:
        bufs["out"] = np.full(M * c["ldo"], SENT16)
    else:
        bufs["out"] = np.full(M * c["ldo"], SENT32)
        if mode == RESID:            # in place: out == resid, as the product calls it
            _strided(bufs["out"].view(np.float32), M, N, c["ldo"])[:] = ops["resid"]
        if mode == CONV2:
            bufs["dbg"] = np.full(M * c["ldo"], SENT32)

    dev = Dev()
    try:
        pA, pW = dev.put(A), dev.put(W)
        ptr = {k: dev.put(v) for k, v in bufs.items()}
        e = KtEpi()
        e.bias = dev.put(ops["bias"])
        if "scale" in ops:
            e.scale = dev.put(ops["scale"])
        e.out, e.ldo = ptr["out"], c["ldo"]
        if "out2" in ptr:
            e.out2, e.ldo2 = ptr["out2"], c["ldo2"]
        if "out3" in ptr:
            e.out3, e.ldo3 = ptr["out3"], c["ldo3"]
        if mode == RESID:
            e.resid, e.ldr = ptr["out"], c["ldo"]
        if mode == CONV2:
            e.resid, e.ldr, e.dbg = dev.put(ops["resid"]), N, ptr["dbg"]
        if mode in (GELU_F16, CONV2):
            e.gelu = dev.put(GELU)
        if mode in (ENC_QKV, DEC_QKV):
            e.split0 = c["split0"]
        if mode == DEC_QKV:
            e.split1, e.row_off = c["split1"], c["row_off"]
        if mode == CROSS_KV:
            e.aux0, e.aux1 = TPAD, N // (2 * c["layers"])
        lib().ktest_gemm(mode, pA, lda, pW, ldw, M, N, K, C.byref(e))
        sync()
        got = {k: Dev.get(ptr[k], v) for k, v in bufs.items()}
    finally:
        dev.close()

    # nothing outside the result: every element the epilogue does not own still holds the sentinel
    mm, nn = np.meshgrid(np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64), indexing="ij")
    which, idx, names = _out_index(c, mm.ravel(), nn.ravel())
    for b, name in enumerate(names):
        keep = np.ones(got[name].size, bool)
        keep[idx[which == b]] = False
        sent = SENT16 if got[name].dtype == np.uint16 else SENT32
        bad = np.flatnonzero(keep & (got[name] != sent))
        assert bad.size == 0, "%s [%s]: %d stores outside the result in %s, first at %d" % (c["name"], kind, bad.size, name, bad[0])
    if mode == CONV2:
        keep = np.ones(got["dbg"].size, bool); keep[idx] = False
        assert (got["dbg"][keep] == SENT32).all(), "%s: dbg written outside the result" % c["name"]

    # the result: whole when small, else every tile-boundary row and column plus a seeded sample (full rows, full columns)
    A64 = _strided(A, M, K, lda).astype(np.float64)
    W64 = W[:, :K].astype(np.float64)
    if M * N * K <= 4e9:
        blocks = [(np.arange(M), np.arange(N))]
    else:
        blocks = [(edge_sample(M, rng), np.arange(N)), (np.arange(M), edge_sample(N, rng))]
    worst = 0.0
    for R, Cn in blocks:
        c64 = A64[R] @ W64[Cn].T
        w_, i_, names = _out_index(c, R[:, None], Cn[None, :])
        w_, i_ = np.broadcast_to(w_, c64.shape), np.broadcast_to(i_, c64.shape)
        kv = np.zeros(c64.shape, np.uint32 if not f16_out else np.uint16)
        for b, name in enumerate(names):
            sel = w_ == b
            kv[sel] = got[name][i_[sel]]
        kvals = {"main": kv}
        if mode == CONV2:
            kvals["dbg"] = got["dbg"][i_]
        where = lambda bad: "(m %d, n %d)" % (R[bad[0][0]], Cn[bad[1][0]])
        if kind == "exact":
            assert np.array_equal(c64, c64.astype(np.float32).astype(np.float64)), "operands not exact"
            want = _model_exact(c, c64.astype(np.float32), ops, R, Cn)
            for k, w in want.items():
                wb = w.view(np.uint16 if w.dtype == np.float16 else np.uint32)
                bad = np.nonzero(kvals[k] != wb)
                assert bad[0].size == 0, "%s [exact] %s: %d results differ in bits, first at %s: got %r want %r" % (
                    c["name"], k, bad[0].size, where(bad), kvals[k][bad][0], wb[bad][0])
        else:
            s64 = np.abs(A64[R]) @ np.abs(W64[Cn]).T
            for k, (r64, bnd) in _bound_random(c, c64, s64, ops, R, Cn).items():
                g = kvals[k].view(np.float16 if kvals[k].dtype == np.uint16 else np.float32).astype(np.float64)
                err = np.abs(g - r64)
                bad = np.nonzero(~(err <= bnd))
                assert bad[0].size == 0, "%s [random] %s: %d results outside the bound, first at %s: |err| %.3e > %.3e" % (
                    c["name"], k, bad[0].size, where(bad), err[bad][0], bnd[bad][0])
                worst = max(worst, float((err / bnd).max()))
    return worst


def _ids(cases):
    return [c["name"].replace(" ", "-") for c in cases]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_gemm(case, kind):
    run_gemm_case(case, kind)


@pytest.mark.parametrize("env", ["128", "reg"])
def test_gemm_forced_form_in_child(env):
    """WHISPER_AMD_GEMM_128 / WHISPER_AMD_NO_GEMM_DMA are read once per process: each form runs in a fresh child of its own."""
    assert CHILD_CASES[env]
    ev = dict(os.environ)
    ev[CHILD_ENV[env]] = "1"
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "child", env], env=ev,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=480)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, "child (%s=1) exited with %d after %.0f s:\n%s" % (CHILD_ENV[env], r.returncode, time.time() - t0, r.stdout[-3000:])


def _child(env):
    fails = 0
    for c in CHILD_CASES[env]:
        for kind in ("exact", "random"):
            try:
                w = run_gemm_case(c, kind)
                print("ok   %-8s %-32s %-6s %s" % (gemm_form(c, env), c["name"], kind, "" if kind == "exact" else "err/bound %.3f" % w))
            except AssertionError as ex:
                fails += 1
                print("FAIL %-8s %-32s %-6s %s" % (gemm_form(c, env), c["name"], kind, ex))
    print("%d failures in %d runs" % (fails, 2 * len(CHILD_CASES[env])))
    return 1 if fails else 0


# ----------------------------------------------------------------------------------------------------------------------------
# LayerNorm (k_layernorm<NV>: one wave per row, F32 sums)
# ----------------------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (128, 192, 384, 512, 768, 1024, 1280)
LN_ROWS = (1, 3, 4, 5, 1500)


def ln_nv(d):           # wa_launch_layernorm's instantiation
    return 2 if d <= 512 else 3 if d <= 768 else 4 if d <= 1024 else 5


LN_CASES = [(d, r, o) for d in LN_WIDTHS for r in LN_ROWS for o in (("both",) if r != 1500 else ("16", "32", "both"))]


@pytest.mark.parametrize("d,rows,outs", LN_CASES, ids=["d%d-r%d-%s" % c for c in LN_CASES])
def test_layernorm(d, rows, outs):
    """Against float64.  Bound (u = 2^-24, per row; k1 = NV + 8 is the depth of the kernel's F32 sums - (x+y)+(z+w) per float4, one
    add per float4 a lane holds, 6 butterfly levels):
        mean:      E_mu  = k1 u sum|x| / d + u |mu|                       (grows with the row's offset: sum|x| ~ d |offset|)
        x - mean:  E_t   = E_mu + u (|x - mu| + E_mu)
        variance:  E_var = [sum_i (2 |x_i - mu| E_t + E_t^2) + (k1 + 1) u sum (x - mu)^2] / d + u var
        1/sqrt:    rho   = (E_var + u (var + eps)) / (2 (var + eps - E_var)) + 3u       (relative)
        y:         one rounding each for * scale, * w, + b;  out16: + half an F16 ulp.
    Leaving one float4 out of the sums moves the mean by ~ 4 |x| / d and the variance by ~ 4 / d of itself: far outside this."""
    rng = rng_for("ln%d-%d-%s" % (d, rows, outs))
    ldx, ld16, ld32, eps = d + 12, d + 8, d + 4, 1e-5
    x = (rng.standard_normal((rows, ldx)) * rng.uniform(0.2, 4, (rows, 1)) + rng.uniform(-3, 3, (rows, 1))).astype(np.float32)
    kinds = np.arange(rows) % 4
    x[kinds == 1] = (1000 + rng.standard_normal((int((kinds == 1).sum()), ldx))).astype(np.float32)      # large common offset
    x[kinds == 2] = np.float32(0.1) * (1 + rng.integers(0, 20, (int((kinds == 2).sum()), 1)))               # constant rows
    x[:, d:] = np.float32(np.nan)           # beyond d: never read
    w = (rng.standard_normal(d) * 0.5 + 1).astype(np.float32)
    b = (rng.standard_normal(d) * 0.3).astype(np.float32)
    o16 = np.full(rows * ld16, SENT16) if outs in ("16", "both") else None
    o32 = np.full(rows * ld32, SENT32) if outs in ("32", "both") else None
    dev = Dev()
    try:
        p16 = dev.put(o16) if o16 is not None else None
        p32 = dev.put(o32) if o32 is not None else None
        lib().ktest_layernorm(dev.put(x), ldx, rows, d, dev.put(w), dev.put(b), eps, p16, ld16, p32, ld32)
        sync()
        g16 = Dev.get(p16, o16).reshape(rows, ld16) if o16 is not None else None
        g32 = Dev.get(p32, o32).reshape(rows, ld32) if o32 is not None else None
    finally:
        dev.close()

    X = x[:, :d].astype(np.float64)
    mu = X.mean(1, keepdims=True)
    t = X - mu
    var = (t * t).mean(1, keepdims=True)
    sig = 1.0 / np.sqrt(var + eps)
    y = t * sig * w + b
    k1 = ln_nv(d) + 8
    E_mu = k1 * U32 * np.abs(X).sum(1, keepdims=True) / d + U32 * np.abs(mu)
    E_t = E_mu + U32 * (np.abs(t) + E_mu)
    E_var = ((2 * np.abs(t) * E_t + E_t ** 2).sum(1, keepdims=True) + (k1 + 1) * U32 * (t * t).sum(1, keepdims=True)) / d + U32 * var
    rho = (E_var + U32 * (var + eps)) / (2 * (var + eps - E_var)) + 3 * U32
    P = np.abs(t) * sig
    E1 = E_t * sig * (1 + rho) + P * rho
    E1 = E1 + U32 * (P + E1)
    E2 = np.abs(w) * E1
    E2 = E2 + U32 * (np.abs(w) * P + E2)
    Ey = E2 + U32 * (np.abs(y) + E2)
    for name, g, ld, sent in (("out16", g16, ld16, SENT16), ("out32", g32, ld32, SENT32)):
        if g is None:
            continue
        assert (g[:, d:] == sent).all(), "%s: stores in columns [d, ld)" % name
        gv = g[:, :d].view(np.float16 if sent is SENT16 else np.float32).astype(np.float64)
        bnd = Ey + (U16 * (np.abs(y) + Ey) + 2.0 ** -25 if sent is SENT16 else 0)
        err = np.abs(gv - y)
        bad = np.nonzero(~(err <= bnd))
        assert bad[0].size == 0, "%s d %d: %d values outside the bound, first row %d col %d (row kind %d): |err| %.3e > %.3e" % (
            name, d, bad[0].size, bad[0][0], bad[1][0], kinds[bad[0][0]], err[bad][0], bnd[bad][0])


# ----------------------------------------------------------------------------------------------------------------------------
# encoder self-attention (k_enc_attn: one sweep with a running maximum, F16 probabilities)
# ----------------------------------------------------------------------------------------------------------------------------
ATT_T = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1000, 1499, 1500)
ATT_HEADS = (2, 6, 12, 16, 20)
ATT_CASES = [(T, ATT_HEADS[i % 5]) for i, T in enumerate(ATT_T)] + [(1500, h) for h in (2, 6, 12, 20)] + [(1499, 6), (65, 20), (1, 16)]
ATT_SCALE = np.float32(1.0 / np.sqrt(64.0))      # KQscale of the encoder (wa_encode.cpp:301)
VT_FAR = 30000.0                                  # vt columns in [T, ldvt): finite, as the contract requires, and large


def _run_attn(T, H, q, k, v):
    """q, k: f16 [T][d]; v: f16 [T][d] (stored transposed into vt [d][TPAD], columns >= T filled with +-VT_FAR).  Returns f16 [T][d] and
    checks that no row >= T and no column >= d of the output was written."""
    d = 64 * H
    ldo = d + 8
    rows_pad = (T + 63) // 64 * 64 + 1
    qk = np.concatenate([q, k], axis=1)
    vt = np.empty((d, TPAD), np.float16)
    vt[:, :T] = v.T
    vt[:, T:] = np.where(np.arange(TPAD - T) % 2 == 0, VT_FAR, -VT_FAR).astype(np.float16)
    out = np.full(rows_pad * ldo, SENT16)
    dev = Dev()
    try:
        po = dev.put(out)
        lib().ktest_enc_attn(dev.put(qk), 2 * d, dev.put(vt), TPAD, T, d, H, ATT_SCALE, po, ldo)
        sync()
        g = Dev.get(po, out).reshape(rows_pad, ldo)
    finally:
        dev.close()
    assert (g[T:] == SENT16).all(), "stores in rows >= T"
    assert (g[:T, d:] == SENT16).all(), "stores in columns >= d"
    return g[:T, :d]


@pytest.mark.parametrize("T,H", ATT_CASES, ids=["T%d-h%d" % c for c in ATT_CASES])
def test_enc_attn_uniform(T, H):
    """Q = 0: every visible key scores 0, P~ = 1 exactly, masked keys exactly 0; V integer, so O = sum_j v_j is exact in F32 and the
    result is f16(f32(O) * f32(1 / T)) bit for bit - the column mean, within one F16 ulp."""
    rng = rng_for("attu%d-%d" % (T, H))
    d = 64 * H
    v = rng.integers(-8, 9, (T, d)).astype(np.float16)
    g = _run_attn(T, H, np.zeros((T, d), np.float16), rng.standard_normal((T, d)).astype(np.float16), v)
    o = v.astype(np.float64).sum(0)
    want = (o.astype(np.float32) * np.float32(1.0 / T)).astype(np.float16)
    assert (np.abs(want.astype(np.float64) - o / T) <= ulp16(o / T)).all()
    bad = np.nonzero(g != want.view(np.uint16)[None, :])
    assert bad[0].size == 0, "%d outputs differ, first at (%d, %d): %r vs %r" % (
        bad[0].size, bad[0][0], bad[1][0], g[bad][0:1].view(np.float16), want[bad[1][0]])


@pytest.mark.parametrize("T,H", ATT_CASES, ids=["T%d-h%d" % c for c in ATT_CASES])
def test_enc_attn_one_hot_permutation(T, H):
    """Key j of head h carries a distinct +-1 code of length 64; query i is gamma * code(pi(i)).  The runner-up score is at least
    2 gamma (64 - max off-diagonal code product) / 2 below the top one; gamma makes that gap >= 32 in the kernel's base-2 exponent, so
    the runner-up's F16 probability underflows to 0 and row i must equal V row pi(i) bit for bit: every query-to-key and key-to-value
    index, ring stage and mask."""
    rng = rng_for("atto%d-%d" % (T, H))
    d = 64 * H
    q = np.empty((T, d), np.float16)
    k = np.empty((T, d), np.float16)
    v = rng.standard_normal((T, d))
    v = np.where(np.abs(v) < 0.0625, 0.5, v).astype(np.float16)      # no value small enough to feel the underflowed terms
    perm = np.empty((H, T), np.int64)
    for h in range(H):
        code = rng.choice(np.array([-1.0, 1.0]), size=(T, 64))
        gram = code @ code.T
        np.fill_diagonal(gram, -64)
        ipmax = gram.max() if T > 1 else 0
        assert ipmax < 64, "two equal codes"
        gamma = 1.0
        while gamma * (64 - ipmax) * float(ATT_SCALE) * np.log2(np.e) < 32:
            gamma *= 2
        perm[h] = rng.permutation(T)
        k[:, 64 * h:64 * h + 64] = code
        q[:, 64 * h:64 * h + 64] = gamma * code[perm[h]]
    g = _run_attn(T, H, q, k, v)
    want = np.concatenate([v[perm[h], 64 * h:64 * h + 64] for h in range(H)], axis=1)
    bad = np.nonzero(g != want.view(np.uint16))
    assert bad[0].size == 0, "%d outputs differ, first at (%d, %d)" % (bad[0].size, bad[0][0], bad[1][0])


@pytest.mark.parametrize("T,H", ATT_CASES, ids=["T%d-h%d" % c for c in ATT_CASES])
def test_enc_attn_random(T, H):
    """Gaussian Q, K, V against float64 soft-max attention.  Bound: the F16 rounding of the unnormalised probabilities P~ (relative
    2^-11 each) moves o = sum p_j v_j / sum p_j by at most 2^-11 max_j |v_j - o| <= 2^-10 max_j |v_j|; scores (two 32-deep MFMA
    steps on F16 products), exp2 and the F32 sums of P V and of the row (K/16 2^-24 relative) are orders of magnitude below it;
    the output's F16 rounding adds half an ulp.  Asserted:  |o - o64| <= 2^-9 max_j |v_j| + (T/16) 2^-24 max_j |v_j| + ulp16/2."""
    rng = rng_for("attr%d-%d" % (T, H))
    d = 64 * H
    q = rng.standard_normal((T, d)).astype(np.float16)
    k = rng.standard_normal((T, d)).astype(np.float16)
    v = rng.standard_normal((T, d)).astype(np.float16)
    g = _run_attn(T, H, q, k, v).view(np.float16).astype(np.float64)
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        s = (q[:, sl].astype(np.float64) @ k[:, sl].astype(np.float64).T) * float(ATT_SCALE)
        p = np.exp(s - s.max(1, keepdims=True))
        vh = v[:, sl].astype(np.float64)
        o = (p @ vh) / p.sum(1, keepdims=True)
        vmax = np.abs(vh).max(0)[None, :]
        bnd = (2.0 ** -9 + T / 16.0 * U32) * vmax + 0.5 * ulp16(np.abs(o) + 2.0 ** -9 * vmax)
        err = np.abs(g[:, sl] - o)
        bad = np.nonzero(~(err <= bnd))
        assert bad[0].size == 0, "head %d: %d outputs outside the bound, first (%d, %d): |err| %.3e > %.3e" % (
            h, bad[0].size, bad[0][0], bad[1][0], err[bad][0], bnd[bad][0])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "child":
    sys.exit(_child(sys.argv[2]))

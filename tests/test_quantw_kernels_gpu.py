"""The weight-quantising kernels (whisper-rust_amd/csrc/wa_quantw.hip) through whisper_amd_quantize_rows: the rows of test_quantw_math.py
at 1, 3 (edge rows) and 70 (all rows, repeated) super-blocks (one workgroup, a ragged one, many with a ragged last), from F32 and from F16 values, given on
the host and lying in device memory, must be the bytes of ggml_quantize_chunk of the reference library.  A row with an infinity or a NaN is refused
by the kernels and by the host statement alike."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_quantw_math import REF_LIB, TYPES, quantw_rows  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 70)      # super-blocks of 256 values


class _init_params(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


@functools.lru_cache(maxsize=None)
def _ref():
    ref = C.CDLL(REF_LIB)
    ref.ggml_init.restype, ref.ggml_init.argtypes = C.c_void_p, [_init_params]
    assert ref.ggml_init(_init_params(1 << 20, None, False))      # fills the reference's F16 -> F32 table
    ref.ggml_quantize_chunk.restype = C.c_size_t
    ref.ggml_quantize_chunk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
    return ref


@functools.lru_cache(maxsize=None)
def _values(f16: bool, nsb: int) -> np.ndarray:
    rows = quantw_rows()      # 1: the clamp row; 3: the zero block, the zero super-block, the tied extremes; 70: all 17, four times over and two more
    x = rows[12 * 256:13 * 256] if nsb == 1 else rows[9 * 256:12 * 256] if nsb == 3 else np.resize(rows, 256 * nsb)
    return x.astype(np.float16) if f16 else x


@functools.lru_cache(maxsize=None)
def _want(t: int, f16: bool, nsb: int) -> bytes:
    import whisper_rs as W
    x = np.ascontiguousarray(_values(f16, nsb).astype(np.float32))
    bv, bs = W.QUANTIZE_BLOCK[t]
    out = np.zeros(x.size // bv * bs, np.uint8)
    assert _ref().ggml_quantize_chunk(t, x.ctypes.data, out.ctypes.data, 0, 1, x.size, None) == out.size
    return out.tobytes()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    import whisper_rs as W
    return W.load_library()


@pytest.mark.parametrize("resident", ["host", "device"])
@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("name", list(TYPES))
def test_quantize_rows_kernels_equal_reference(lib, name, f16, resident):
    import whisper_rs as W
    t = TYPES[name]
    for nsb in SIZES:
        x = _values(f16, nsb)
        if resident == "device":
            hip, d = C.CDLL("libamdhip64.so"), C.c_void_p()
            assert hip.hipMalloc(C.byref(d), C.c_size_t(x.nbytes)) == 0
            assert hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
            got = W.quantize_rows(lib, t, None, 1, device_ptr=d.value, n=x.size, f16=f16)
            hip.hipFree(d)
        else:
            got = W.quantize_rows(lib, t, x, 1)
        assert not isinstance(got, int), got
        want = np.frombuffer(_want(t, f16, nsb), np.uint8)
        bs = W.QUANTIZE_BLOCK[t][1]
        bad = np.flatnonzero((got.reshape(-1, bs) != want.reshape(-1, bs)).any(axis=1))
        assert bad.size == 0, "%s, %d super-blocks: %d blocks differ, first %d" % (name, nsb, bad.size, bad[0])


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("name", list(TYPES))
def test_quantize_rows_refuses_values_that_are_not_finite(lib, name, bad):
    import whisper_rs as W
    x = _values(False, 3).copy()
    x[300] = bad
    assert W.quantize_rows(lib, TYPES[name], x, 1) == W.QUANTIZE_NOT_FINITE
    assert W.quantize_rows(lib, TYPES[name], x, 0) == W.QUANTIZE_NOT_FINITE
    assert W.quantize_rows(lib, 10, x, 1) == W.QUANTIZE_REFUSED      # Q2_K: out of scope, by name
    assert W.quantize_rows(lib, TYPES[name], x[:48], 1) == W.QUANTIZE_REFUSED

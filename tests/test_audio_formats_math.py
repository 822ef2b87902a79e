"""The host code of the audio front end's sample formats beyond int16 and F32, and of the WAV header parser (whisper-rust_amd/csrc/wa_audio.h,
wa_channels.h, wa_stream.h, wa_wav.h through tests/native/audio_formats_math.cpp, g++ alone: no HIP, no device).

1. Both G.711 expansions, all 256 codes, are the formulas restated in numpy (whisper_rs.ulaw_to_linear / alaw_to_linear), audioop's where that
   module imports, and the anchor values.
2. wa_audio_ref of every new format equals, bit for bit, wa_audio_ref of the equivalent input the existing code serves: G.711 -> I16 holding the
   expansion, U8 / S24 / S32 / F64 -> F32 holding the per-sample v / S (F64: v).  Both channel counts, 8000 / 16000 / 44100 / 48000 Hz,
   1, 2, 3, K/2 - 1, K and 1000 frames, the extremes of every format, NaN and Inf in a case of their own, the host pointer 0 .. 3 bytes into a
   heap block that ends with the last sample.  The same for the split's and the live feed's host forms.
3. At 16 kHz the conversions are numpy float32 arithmetic written out literally.
4. wa_wav_parse: files Python's wave module writes, hand-built headers, every refusal code, the record untouched after a refusal.
5. The driver built with -fsanitize=address,undefined runs the same commands clean as a stand-alone program and prints the same.
6. The code object wa_audio_fmt.o holds the 48 kernels and none has scratch or a spilled register.
CPU only."""
import io
import math
import os
import shutil
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import whisper_rs as W  # noqa: E402  (the numpy restatements only: no library is loaded here)

SRC = os.path.join(ROOT, "tests", "native", "audio_formats_math.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"

I16, F32, U8, S24, S32, F64, ULAW, ALAW = 0, 1, 3, 4, 5, 6, 7, 8
NEW = [U8, S24, S32, F64, ULAW, ALAW]
SCALE = {U8: 128.0, S24: 8388608.0, S32: 2147483648.0, ULAW: 32768.0, ALAW: 32768.0}
RATES = [8000, 16000, 44100, 48000]
PACKETS = [1, 159, 160, 161, 4000]


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def lengths_of(rate):
    K = plan_of(rate)[2] or 64                      # 16 kHz has no taps: the lengths of K = 64
    return [1, 2, 3, K // 2 - 1, K, 1000]


def make_input(rng, n, fmt):
    """n samples of a new format: (the array the entry reads, its values v as float32).  The extremes come first."""
    def lead(x, ext):
        x[:min(n, len(ext))] = ext[:min(n, len(ext))]
        return x
    if fmt == U8:
        x = lead(rng.integers(0, 256, n).astype(np.uint8), np.array([0, 255, 255, 0, 128, 127], np.uint8))
        return x, (x.astype(np.int32) - 128).astype(np.float32)
    if fmt == S24:
        s = lead(rng.integers(-2 ** 23, 2 ** 23, n).astype(np.int32), np.array([2 ** 23 - 1, -2 ** 23, -(2 ** 23 - 1), 2 ** 23 - 1, -2 ** 23, -2 ** 23, 0, -1], np.int32))
        return W.pack_s24(s), s.astype(np.float32)                  # 24 bits: exact
    if fmt == S32:
        # INT_MAX and 2^24 + 1 round in (float); so do most random values
        s = lead(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
                 np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 31 - 65, 2 ** 31 - 64], np.int32))
        return s, s.astype(np.float32)                              # numpy converts with round to nearest even
    if fmt == F64:
        x = lead(rng.uniform(-1.0, 1.0, n), np.array([1.0, -1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e-40, -1e-40, 0.1, 2.0 ** -126 * (1 - 2.0 ** -25)]))
        return x, x.astype(np.float32)
    x = lead(rng.integers(0, 256, n).astype(np.uint8), np.array([0x00, 0x80, 0x7F, 0xFF, 0x55, 0xD5, 0x2A, 0xAA, 0x01], np.uint8))
    return x, (W.ulaw_to_linear(x) if fmt == ULAW else W.alaw_to_linear(x)).astype(np.float32)


def equivalent(x, v, fmt):
    """(format, array) of the input the existing code serves with the same bits"""
    if fmt in (ULAW, ALAW):
        return I16, v.astype(np.int16)
    return F32, (v if fmt == F64 else v / np.float32(SCALE[fmt]))


class Driver:
    def __init__(self, exe, work):
        self.exe, self.work, self.n, self.lines, self.files = exe, work, 0, [], 0

    def put(self, x):
        self.files += 1
        p = str(self.work / ("f_%d.bin" % self.files))
        (x if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), np.uint8)).tofile(p)
        return p

    def out(self):
        self.files += 1
        return str(self.work / ("o_%d.bin" % self.files))

    def run(self, lines, exe=None):
        self.n += 1
        cmd = str(self.work / ("cmd_%d.txt" % self.n))
        with open(cmd, "w") as f:
            f.write("".join(l + "\n" for l in lines))
        r = subprocess.run([exe or self.exe, cmd], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        return r.stdout.splitlines()


def floats(path, n):
    return np.fromfile(path, np.float32) if n > 0 else np.zeros(0, np.float32)


# ---- WAV images ----
GUID_TAIL = bytes([0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def chunk(cid, body, size=None, pad=True):
    return cid + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if pad and len(body) % 2 else b"")


def fmt_body(tag, ch, rate, bits, block=None, ext=None, valid=None, guid_tail=GUID_TAIL, cb=None):
    block = ch * bits // 8 if block is None else block
    b = struct.pack("<HHIIHH", tag, ch, rate, rate * block, block, bits)
    if tag == 0xFFFE:
        b += struct.pack("<HHI", 22, bits if valid is None else valid, 3) + struct.pack("<H", ext) + guid_tail
    elif cb is not None:
        b += struct.pack("<H", cb)
    return b


def riff(chunks, form=b"RIFF", wave_id=b"WAVE"):
    body = wave_id + b"".join(chunks)
    return form + struct.pack("<I", len(body)) + body


def wave_module_image(width, ch, rate, n_frames, rng):
    frames = rng.integers(0, 256, n_frames * ch * width).astype(np.uint8).tobytes()
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(ch); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes(frames)
    return buf.getvalue(), frames


def wav_images(rng):
    """name -> (image, expected "rc data_offset n_frames channels rate format bits"; a refusal leaves the record at -7)"""
    im = {}

    def ok(name, image, off, n, ch, rate, fmt, bits):
        im[name] = (image, "wav 0 %d %d %d %d %d %d" % (off, n, ch, rate, fmt, bits))

    def bad(name, image, rc):
        im[name] = (image, "wav %d -7 -7 -7 -7 -7 -7" % rc)

    for width, fmt in ((1, U8), (2, I16), (3, S24), (4, S32)):
        for ch in (1, 2):
            image, frames = wave_module_image(width, ch, 8000 if ch == 1 else 44100, 37, rng)
            assert image[44:] == frames                                           # the module writes the canonical 44-byte header
            ok("wave_%d_%d" % (width, ch), image, 44, 37, ch, 8000 if ch == 1 else 44100, fmt, 8 * width)
    data = bytes(range(96))
    fact = chunk(b"fact", struct.pack("<I", 12))
    for name, tag, bits, fmt in (("f32", 3, 32, F32), ("f64", 3, 64, F64), ("alaw", 6, 8, ALAW), ("ulaw", 7, 8, ULAW)):
        image = riff([chunk(b"fmt ", fmt_body(tag, 2, 8000, bits, cb=0)), fact, chunk(b"data", data)])
        ok("tag_" + name, image, 12 + 8 + 18 + 12 + 8, 96 // (2 * bits // 8), 2, 8000, fmt, bits)
    for name, sub, bits, fmt in (("s24", 1, 24, S24), ("f32", 3, 32, F32), ("ulaw", 7, 8, ULAW), ("i16", 1, 16, I16)):
        image = riff([chunk(b"fmt ", fmt_body(0xFFFE, 1, 48000, bits, ext=sub)), chunk(b"data", data)])
        ok("ext_" + name, image, 12 + 8 + 40 + 8, 96 // (bits // 8), 1, 48000, fmt, bits)
    bad("ext_bad_guid", riff([chunk(b"fmt ", fmt_body(0xFFFE, 1, 48000, 16, ext=1, guid_tail=bytes(14))), chunk(b"data", data)]), -4)
    bad("ext_valid_bits", riff([chunk(b"fmt ", fmt_body(0xFFFE, 1, 48000, 24, ext=1, valid=20)), chunk(b"data", data)]), -4)
    bad("ext_short", riff([chunk(b"fmt ", fmt_body(0xFFFE, 1, 48000, 16, ext=1)[:24]), chunk(b"data", data)]), -4)
    fmt16 = chunk(b"fmt ", fmt_body(1, 2, 8000, 16))
    # an odd-sized LIST chunk: its pad byte is honoured, the data chunk starts on the even offset behind it
    ok("odd_list", riff([fmt16, chunk(b"LIST", b"INFOx"), chunk(b"data", data)]), 12 + 24 + 8 + 6 + 8, 24, 2, 8000, I16, 16)
    bad("odd_list_unpadded", riff([fmt16, chunk(b"LIST", b"INFOx", pad=False), chunk(b"data", data)]), -3)     # the walk lands one byte early: no chunk there
    # declared sizes a streaming writer leaves, and a declared size past the image: to the end of the image, whole frames only
    for name, size in (("size_0", 0), ("size_ffffffff", 0xFFFFFFFF), ("size_past", 4000)):
        ok(name, riff([fmt16, chunk(b"data", data[:94], size=size)]), 44, 23, 2, 8000, I16, 16)              # 94 bytes: 23 frames and half of one
    ok("size_smaller", riff([fmt16, chunk(b"data", data, size=40), chunk(b"LIST", b"abcd")]), 44, 10, 2, 8000, I16, 16)
    ok("no_samples", riff([fmt16, chunk(b"data", b"")]), 44, 0, 2, 8000, I16, 16)
    ok("three_channels_reported", riff([chunk(b"fmt ", fmt_body(1, 3, 4000, 16)), chunk(b"data", data)]), 44, 16, 3, 4000, I16, 16)
    # refusals
    good = riff([fmt16, chunk(b"data", data)])
    bad("rf64", b"RF64" + good[4:], -2)
    bad("rifx", b"RIFX" + good[4:], -2)
    bad("avi", riff([fmt16, chunk(b"data", data)], wave_id=b"AVI "), -2)
    bad("data_before_fmt", riff([chunk(b"data", data), fmt16]), -3)
    bad("chunk_past_image", riff([fmt16, chunk(b"LIST", b"abcd", size=4000), chunk(b"data", data)]), -3)
    bad("header_cut", riff([fmt16]) + b"dat", -3)
    bad("fmt_short", riff([chunk(b"fmt ", fmt_body(1, 2, 8000, 16)[:14]), chunk(b"data", data)]), -3)
    bad("adpcm", riff([chunk(b"fmt ", fmt_body(2, 1, 8000, 4, block=256, cb=0)), chunk(b"data", data)]), -4)
    bad("pcm_12_bits", riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 12, block=2)), chunk(b"data", data)]), -4)
    bad("pcm_64_bits", riff([chunk(b"fmt ", fmt_body(1, 1, 8000, 64)), chunk(b"data", data)]), -4)
    bad("float_16_bits", riff([chunk(b"fmt ", fmt_body(3, 1, 8000, 16)), chunk(b"data", data)]), -4)
    bad("ulaw_16_bits", riff([chunk(b"fmt ", fmt_body(7, 1, 8000, 16)), chunk(b"data", data)]), -4)
    bad("block_align", riff([chunk(b"fmt ", fmt_body(1, 2, 8000, 16, block=2)), chunk(b"data", data)]), -4)
    bad("no_channels", riff([chunk(b"fmt ", fmt_body(1, 0, 8000, 16)), chunk(b"data", data)]), -4)
    bad("no_data", riff([fmt16, fact]), -5)
    bad("riff_only", riff([]), -5)
    return im


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("audio_formats_math")
    exe = str(work / "audio_formats_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    drv = Driver(exe, work)
    rng = np.random.default_rng(20241021)
    lines, refs, splits, streams = ["g711"], [], [], []

    def ref(rate, fmt, ch, n, off, x):
        o = drv.out()
        lines.append("ref %d %d %d %d %d %s %s" % (rate, fmt, ch, n, off, drv.put(x), o))
        return o

    k = 0
    for fmt in NEW:
        for ch in (1, 2):
            for rate in RATES:
                for n in lengths_of(rate):
                    x, v = make_input(rng, n * ch, fmt)
                    efmt, ex = equivalent(x, v, fmt)
                    refs.append(dict(key=(fmt, ch, rate, n), x=x, v=v, got=ref(rate, fmt, ch, n, k % 4, x), want=ref(rate, efmt, ch, n, 0, ex)))
                    k += 1
    # NaN and Inf, a case of their own: F64 against F32 holding the same values
    special = np.array([0.25, np.nan, -0.5, np.inf, 0.125, -np.inf, 1e300, -1e300] * 50, np.float64)
    for ch in (1, 2):
        for rate in (16000, 48000):
            n = len(special) // ch
            with np.errstate(over="ignore"):
                e32 = special.astype(np.float32)
            refs.append(dict(key=(F64, ch, rate, n), x=special, v=e32, special=True, got=ref(rate, F64, ch, n, 1, special), want=ref(rate, F32, ch, n, 0, e32)))
    # the split's host form: each plane against the channel as a mono recording, and against the split of the equivalent input
    for fmt in NEW:
        for rate in (8000, 16000, 44100):
            n = 700
            x, v = make_input(rng, 2 * n, fmt)
            efmt, ex = equivalent(x, v, fmt)
            o, oe = drv.out(), drv.out()
            lines.append("split %d %d %d %d %s %s" % (rate, fmt, n, 1 + k % 3, drv.put(x), o))
            lines.append("split %d %d %d 0 %s %s" % (rate, efmt, n, drv.put(ex), oe))
            b = W.PCM_SAMPLE_BYTES[fmt]
            planes = [np.ascontiguousarray(x.view(np.uint8).reshape(n, 2, b)[:, c, :]).reshape(-1) for c in (0, 1)]
            splits.append(dict(key=(fmt, rate), got=o, want=oe, mono=[ref(rate, fmt, 1, n, 0, p) for p in planes]))
            k += 1
    # the live feed's host form: packets of 1, 159, 160, 161 and 4000 frames in turn, then the flush
    for fmt, ch, rate, n in ((ULAW, 1, 8000, 9000), (ALAW, 1, 8000, 9000), (U8, 2, 16000, 5000), (S24, 2, 48000, 9000), (S32, 1, 44100, 5000), (F64, 2, 8000, 5000)):
        x, v = make_input(rng, n * ch, fmt)
        efmt, ex = equivalent(x, v, fmt)
        o, oe = drv.out(), drv.out()
        pk = ",".join(str(p) for p in PACKETS)
        lines.append("stream %d %d %d %d %s %s %s" % (rate, fmt, ch, n, drv.put(x), o, pk))
        lines.append("stream %d %d %d %d %s %s %s" % (rate, efmt, ch, n, drv.put(ex), oe, pk))
        streams.append(dict(key=(fmt, ch, rate, n), got=o, want=oe, whole=ref(rate, fmt, ch, n, 0, x)))
    images = wav_images(rng)
    first_wav = len(lines)
    for name, (image, _) in images.items():
        lines.append("wav %s" % drv.put(image))
    lines.append("wavargs %s" % drv.put(images["wave_2_2"][0]))
    out = drv.run(lines)
    assert len(out) == len(lines) + 1                       # g711 prints two lines
    return dict(work=work, drv=drv, lines=lines, stdout=out, refs=refs, splits=splits, streams=streams, images=images, first_wav=first_wav + 1)


def test_g711_tables(env):
    codes = np.arange(256, dtype=np.uint8)
    for line, tag, restated, law in ((env["stdout"][0], "ulaw", W.ulaw_to_linear, "ulaw2lin"), (env["stdout"][1], "alaw", W.alaw_to_linear, "alaw2lin")):
        got = line.split()
        assert got[0] == tag and len(got) == 257
        table = np.array([int(v) for v in got[1:]])
        assert np.array_equal(table, restated(codes).astype(np.int64))
        assert np.abs(table).max() <= 32767
        try:
            import audioop
        except ImportError:
            continue
        assert np.array_equal(table, np.frombuffer(getattr(audioop, law)(codes.tobytes(), 2), np.int16).astype(np.int64))
    u = [int(v) for v in env["stdout"][0].split()[1:]]
    a = [int(v) for v in env["stdout"][1].split()[1:]]
    assert (u[0x00], u[0x80], u[0x7F], u[0xFF], u[0x01]) == (-32124, 32124, 0, 0, -31100)
    assert (a[0x55], a[0xD5], a[0x2A], a[0xAA], a[0x00]) == (-8, 8, -32256, 32256, -5504)
    # the compressor the GPU tests use brings every expansion back to a code that expands to the same value
    assert np.array_equal(W.ulaw_to_linear(W.linear_to_ulaw(np.array(u, np.int16))), np.array(u, np.int16))


def test_restatement_equals_the_equivalent_input(env):
    seen = set()
    for c in env["refs"]:
        fmt, ch, rate, n = c["key"]
        n_out = -(-n * 16000 // rate)
        got, want = floats(c["got"], n_out), floats(c["want"], n_out)
        assert len(got) == n_out and got.tobytes() == want.tobytes(), c["key"]
        if c.get("special"):
            assert np.isnan(got).any() and (rate != 16000 or np.isinf(got).any())
        else:
            assert np.all(np.isfinite(got))
            seen.add((fmt, ch, rate))
    assert len(seen) == len(NEW) * 2 * len(RATES)


def test_conversion_at_16_khz_is_literal_float32_arithmetic(env):
    seen = 0
    for c in env["refs"]:
        fmt, ch, rate, n = c["key"]
        if rate != 16000 or c.get("special"):
            continue
        x, two = c["x"], np.float32(2.0)
        if fmt == U8:
            v = (x.astype(np.int32) - 128).astype(np.float32)
        elif fmt == S24:
            b = x.reshape(-1, 3).astype(np.int32)
            v = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2].astype(np.int8).astype(np.int32) << 16)).astype(np.float32)
        elif fmt in (S32, F64):
            v = x.astype(np.float32)
        else:
            v = (W.ulaw_to_linear(x) if fmt == ULAW else W.alaw_to_linear(x)).astype(np.float32)
        mono = v if ch == 1 else (v[0::2] + v[1::2]) / two
        want = mono if fmt == F64 else mono / np.float32(SCALE[fmt])
        assert want.dtype == np.float32
        assert floats(c["got"], n).tobytes() == want.tobytes(), c["key"]
        seen += 1
    assert seen == len(NEW) * 2 * len(lengths_of(16000))
    # what the extremes give
    assert np.float32(-128.0) / np.float32(128.0) == -1.0 and np.float32(np.int32(2 ** 31 - 1)) == np.float32(2.0 ** 31)
    assert np.float64(1e-40).astype(np.float32) != 0.0                                  # a subnormal F32, not zero


def test_split_host_form(env):
    for c in env["splits"]:
        fmt, rate = c["key"]
        n_out = -(-700 * 16000 // rate)
        got, want = floats(c["got"], 2 * n_out), floats(c["want"], 2 * n_out)
        assert len(got) == 2 * n_out and got.tobytes() == want.tobytes(), c["key"]
        for ch in (0, 1):
            assert got[ch * n_out:(ch + 1) * n_out].tobytes() == floats(c["mono"][ch], n_out).tobytes(), (c["key"], ch)


def test_stream_host_form(env):
    for c in env["streams"]:
        fmt, ch, rate, n = c["key"]
        n_out = -(-n * 16000 // rate)
        got, want, whole = floats(c["got"], n_out), floats(c["want"], n_out), floats(c["whole"], n_out)
        assert got.tobytes() == want.tobytes(), c["key"]
        assert len(got) >= n_out and got[:n_out].tobytes() == whole.tobytes(), c["key"]           # packets and flush give the whole recording's samples


def test_wav_parser(env):
    out = env["stdout"][env["first_wav"]:]
    for (name, (image, want)), line in zip(env["images"].items(), out):
        assert line == want, name
    assert out[len(env["images"])] == "wavargs -1 -1 -1 -1"
    codes = {int(w.split()[1]) for _, w in env["images"].values()}
    assert codes == {0, -2, -3, -4, -5}                         # -1: wavargs


def test_sanitized_driver_runs_clean(env):
    exe = str(env["work"] / "audio_formats_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe])
    before = {c["got"]: open(c["got"], "rb").read() for c in env["refs"]}
    assert env["drv"].run(env["lines"], exe) == env["stdout"]
    for path, data in before.items():                           # the sanitised run rewrote the outputs: they are the same
        assert open(path, "rb").read() == data, path


def test_format_kernels_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_audio_math.py reads wa_audio_k.o."""
    if not os.path.exists(os.path.join(BUILD, "wa_quantk.o")):
        pytest.skip("no build tree here")
    obj = os.path.join(BUILD, "wa_audio_fmt.o")
    assert os.path.exists(obj), "the build made wa_quantk.o but not wa_audio_fmt.o"
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(TOOLS, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(TOOLS, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(TOOLS, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:") or line.startswith(".sgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    count = {k: len([n for n in seen if k in n]) for k in ("k_fmt_convert", "k_fmt_resample", "k_fmt_deinterleave", "k_fmt_split", "k_fmt_push")}
    assert count == {"k_fmt_convert": 12, "k_fmt_resample": 12, "k_fmt_deinterleave": 6, "k_fmt_split": 6, "k_fmt_push": 12} and len(seen) == 48, sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

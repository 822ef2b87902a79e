"""The kernels of the heuristic token timestamps (whisper-rust_amd/csrc/wa_tts.hip) against the host functions of wa_tts.h, byte for byte, through
whisper_amd_signal_energy and whisper_amd_token_snap (where = 1 against 0), the PCM as a host pointer and in HBM (whisper_amd_audio_to_pcm's buffer).
The integer finalisation on the records is checked on the CPU (tests/native/tts_math.cpp, no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

import wsynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SNAP = 3 * 16000
LENGTHS = [lambda T: 1, lambda T: 32, lambda T: 33, lambda T: 64, lambda T: 65, lambda T: 66, lambda T: T - 1, lambda T: T, lambda T: T + 1, lambda T: 2 * T + 31]


def test_finalisation_equals_the_pass_it_replaced(tmp_path):
    """10 000 seeded time lines: records + wa_tts_finalise give the ends the former sample-by-sample pass gave, and every branch was taken"""
    exe = str(tmp_path / "tts_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "tts_math.cpp"), "-o", exe])
    r = subprocess.run([exe, "10000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def st(wrs, amd_lib):
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    state = ctx.create_state()
    yield state
    state.free(); ctx.free()


def signal(kind, n):
    """seeded noise, or small values with -0.0, subnormals and one large value among them: a wrong order of the additions shows"""
    rng = np.random.default_rng(1000 + n)
    if kind == "noise":
        return rng.normal(0.0, 0.1, n).astype(np.float32)
    x = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    x[::7] = np.float32(-0.0)
    x[3::11] = np.float32(1e-40) * np.where(rng.random(len(x[3::11])) < 0.5, -1, 1).astype(np.float32)
    x[n // 2] = np.float32(-12345.678)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("where_pcm", ["host", "device"])
@pytest.mark.parametrize("kind", ["noise", "edge"])
@pytest.mark.parametrize("length", range(len(LENGTHS)))
def test_energy_device_equals_host(st, amd_lib, length, kind, where_pcm):
    """lengths on either side of the 65-sample window and of the kernel's tile; the last noise row also against float64: 64 additions and one division,
    each rounded to F32, of non-negative terms lie within (1 + 2^-24)^65 - 1 relative of the exact value (a guard against an error both paths share)"""
    x = signal(kind, LENGTHS[length](amd_lib.whisper_amd_tts_tile()))
    n, pcm = len(x), st.audio_to_pcm(x, 1, 16000) if where_pcm == "device" else x
    want, got = st.signal_energy(pcm, where=0), st.signal_energy(pcm, where=1)
    assert len(got) == n and got.tobytes() == want.tobytes(), np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8]
    if kind == "noise" and length == len(LENGTHS) - 1:
        c, i = np.concatenate([[0.0], np.cumsum(np.abs(x).astype(np.float64))]), np.arange(n)
        e64 = (c[np.minimum(i + 32, n - 1) + 1] - c[np.maximum(i - 32, 0)]) / 65.0
        bound = ((1.0 + 2.0 ** -24) ** 65 - 1.0) * e64 + 65 * 2.0 ** -53 * c[-1]       # (+ the float64 prefix sums' own roundings)
        assert (np.abs(got.astype(np.float64) - e64) <= bound).all()


def burst_signal():
    rng = np.random.default_rng(7)
    x = np.zeros(N_SNAP, np.float32)
    for a, b in ((0, 800), (5000, 9000), (20000, 26000), (40000, N_SNAP)):
        x[a:b] = (rng.uniform(0.5, 1.0, b - a) * rng.choice([-1.0, 1.0], b - a)).astype(np.float32)
    x[-200:] *= np.float32(4.0)           # the clipped windows at the end stay above the level
    return x


# (s_lo, s_hi, has_prev)
BURST_TOKENS = [(7000, 8000, 1), (7000, 8000, 0), (10000, 12000, 1), (44000, 45000, 1), (26500, 27900, 1), (500, 1500, 1), (46000, 47500, 1),
                (30000, 22000, 1), (26000, 22000, 0), (6000, 30000, 1), (N_SNAP - 1, N_SNAP - 1, 1), (0, 0, 0)]
BRANCHES = {
    "loud start, scans back past the previous token": lambda r, t: r["flags"] & 1 and t[2] and r["back_lo"] < t[0],
    "loud start of the first token": lambda r, t: r["flags"] & 1 and not t[2] and r["back_lo"] == t[0],
    "leading silence into s_hi": lambda r, t: not r["flags"] & 1 and t[0] < t[1] and r["fwd_lo"] == t[1],
    "loud end to n - 1": lambda r, t: r["flags"] & 2 and t[1] < N_SNAP - 1 and r["fwd_hi"] == N_SNAP - 1,
    "trailing silence back to s_lo": lambda r, t: not r["flags"] & 2 and t[0] < t[1] and r["back_hi"] <= t[0],
    "back scan to 0": lambda r, t: r["flags"] & 1 and t[2] and t[0] > 0 and r["back_lo"] == 0,
    "window clipped at 0": lambda r, t: 0 < t[0] < 2000 and r["level"] > 0,
    "window clipped at n": lambda r, t: N_SNAP - 2000 < t[1] < N_SNAP - 1 and r["level"] > 0,
    "inverted window": lambda r, t: t[0] - t[1] > 4000 and r["level"] == 0 and np.signbit(r["level"]),
    "empty window": lambda r, t: t[0] - t[1] == 4000 and np.isnan(r["level"]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("where_pcm", ["host", "device"])
@pytest.mark.parametrize("sig", ["bursts", "silence"])
def test_snap_records_device_equal_host(st, sig, where_pcm):
    """bursts in 3 s of silence and token ends that take every branch of the record, read from the host records: each must have been taken"""
    x = burst_signal() if sig == "bursts" else np.zeros(N_SNAP, np.float32)
    pcm = st.audio_to_pcm(x, 1, 16000) if where_pcm == "device" else x
    cols = [list(c) for c in zip(*BURST_TOKENS)]
    want, got = st.token_snap(pcm, *cols, where=0), st.token_snap(pcm, *cols, where=1)
    if sig == "bursts":
        for name, took in BRANCHES.items():
            assert any(took(r, t) for r, t in zip(want, BURST_TOKENS)), name
    else:       # level 0 (NaN for the empty window): nothing is loud, nothing is quiet, no scan moves
        assert all(r["flags"] == (4 if t[2] else 0) and (r["back_lo"], r["fwd_lo"], r["fwd_hi"], r["back_hi"]) == (t[0], t[0], t[1], t[1])
                   for r, t in zip(want, BURST_TOKENS))
    assert got.tobytes() == want.tobytes(), [(t, w, g) for t, w, g in zip(BURST_TOKENS, want, got) if w != g][:3]

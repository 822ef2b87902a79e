"""Stereo test recordings for the two-channel calls (whisper_amd_audio_split, whisper_amd_full_long_channels), built from tools/wsynth_vad.py.

Shared by tests/test_channels_full_gpu.py and tools/channels_probe.py.  Every recording is 14 s + 137 samples at 16 kHz, as the VAD audio.
The properties the tests rely on were checked on the CPU with the reference VAD (oracle/_ref/libwhisper_ref.so, default VAD parameters,
the synthetic VAD model of wsynth_vad):
  two_speakers()   channel 0 = synth_audio(0): segments (103, 224) (704, 953) (1203, 1264) cs;  channel 1 = synth_audio(1) delayed by DELAY samples
                   (1.3 s + 37 samples, no multiple of the VAD's 512-sample window): (234, 355) (835, 1085) (1331, 1402), so 704 .. 953 on
                   channel 0 overlaps 835 .. 1085 on channel 1; 3 + 3 chunks at a cap of 3000 ms.  at_8k_i16 of it gives the same lists.
  bleed(b)         channel 1 = b x channel 0 plus a burst of its own at 10.0 .. 11.2 s, where channel 0 is silent: at b = BLEED = 0.8 the reference VAD
                   finds (106, 224) (791, 953) (1207, 1264) - the bleed - and (1002, 1126) - the burst - on channel 1 (at b <= 0.6 it no longer
                   hears the bleed: the synthetic model's probability follows the energy).
  alternating()    the bursts of synth_audio alternate between the channels at twice the amplitude, so that the down-mix is synth_audio's signal: its
                   segments are (103, 224) (704, 953) (1203, 1264), the first and the last on channel 0, the middle one on channel 1.
"""
from __future__ import annotations

import numpy as np

import wsynth_vad as V

SR = 16000
DELAY = 20837            # 1.3 s + 37 samples; 20837 % 512 == 357
BLEED = 0.8
OWN_BURST = (10.0, 11.2)


def delayed(seed: int, delay: int) -> np.ndarray:
    rng = np.random.default_rng(4000 + seed)
    pad = (0.002 * rng.standard_normal(delay)).astype(np.float32)
    return np.concatenate([pad, V.synth_audio(seed)])[:V.N_AUDIO]


def interleave(ch0: np.ndarray, ch1: np.ndarray) -> np.ndarray:
    assert ch0.shape == ch1.shape
    return np.stack([ch0, ch1], axis=1).astype(np.float32).reshape(-1)


def two_speakers() -> np.ndarray:
    """interleaved F32 stereo at 16 kHz"""
    return interleave(V.synth_audio(0), delayed(1, DELAY))


def burst(t0: float, t1: float, seed: int) -> np.ndarray:
    """the tone + chirp of wsynth_vad inside [t0, t1), faint noise everywhere"""
    rng = np.random.default_rng(5000 + seed)
    t = np.arange(V.N_AUDIO, dtype=np.float64) / SR
    env = ((t >= t0) & (t < t1)).astype(np.float64)
    x = env * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 100.0 * t) * t))
    return (x + 0.002 * rng.standard_normal(V.N_AUDIO)).astype(np.float32)


def bleed(b: float = BLEED) -> np.ndarray:
    ch0 = V.synth_audio(0)
    return interleave(ch0, (np.float32(b) * ch0 + burst(*OWN_BURST, seed=1)).astype(np.float32))


def alternating() -> np.ndarray:
    t = np.arange(V.N_AUDIO, dtype=np.float64) / SR
    sig = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 100.0 * t) * t)
    ch = []
    for c in range(2):
        rng = np.random.default_rng(6000 + c)
        env = np.zeros(V.N_AUDIO)
        for a, b in V.BURSTS[c::2]:
            env[(t >= a) & (t < b)] = 2.0
        ch.append((env * sig + 0.002 * rng.standard_normal(V.N_AUDIO)).astype(np.float32))
    return interleave(ch[0], ch[1])


def to_i16(x: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def at_8k_i16(x: np.ndarray) -> np.ndarray:
    """every other frame of an interleaved 16 kHz stereo recording as int16: an 8 kHz recording (the signals stay below 4 kHz)"""
    return to_i16(x.reshape(-1, 2)[::2].reshape(-1))


def channel(x: np.ndarray, c: int) -> np.ndarray:
    """channel c of an interleaved stereo recording, extracted on the host, in the recording's own format"""
    return np.ascontiguousarray(x.reshape(-1, 2)[:, c])

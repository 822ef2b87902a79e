"""Synthetic Silero-shaped VAD model and test audio (the VAD counterpart of wsynth.py).

The model has the one shape the engine supports (whisper-rust_amd/csrc/wa_vad.h) with seeded weights: a real windowed-DFT basis, so
that the magnitudes behave like a spectrum, and random layers scaled so that activations neither die nor saturate.  The final layer
is biased towards "no speech" and has positive weights, which makes the probability follow the energy of the LSTM's output: the
test audio below then gives probabilities on both sides of the usual thresholds.  Nothing here is trained; the tests compare
engines, bit for bit, on identical inputs.
"""
from __future__ import annotations

import os
import struct

import numpy as np

GGML_MAGIC = 0x67676D6C
N_WINDOW = 512
ENC = [(129, 128), (128, 64), (64, 64), (64, 128)]       # (C_in, C_out), kernel 3


def tensors(seed: int = 0) -> list[tuple[str, np.ndarray]]:
    """(name, array) in file order; array shapes are slowest-varying first (the reverse of ggml's ne[])."""
    rng = np.random.default_rng(seed)
    n = np.arange(256, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * n / 256)
    k = np.arange(129, dtype=np.float64)[:, None]
    basis = np.concatenate([np.cos(2 * np.pi * k * n / 256) * hann, -np.sin(2 * np.pi * k * n / 256) * hann], axis=0)
    out = [("_model.stft.forward_basis_buffer", basis.reshape(258, 1, 256).astype(np.float16))]
    for i, (cin, cout) in enumerate(ENC):
        w = rng.normal(0.0, 1.0 / np.sqrt(cin * 3), size=(cout, cin, 3))
        b = rng.normal(0.0, 0.05, size=(cout,))
        out.append((f"_model.encoder.{i}.reparam_conv.weight", w.astype(np.float16)))
        out.append((f"_model.encoder.{i}.reparam_conv.bias", b.astype(np.float32)))
    w_ih = rng.normal(0.0, 1.0 / np.sqrt(128), size=(512, 128)).astype(np.float32)
    w_hh = rng.normal(0.0, 0.5 / np.sqrt(128), size=(512, 128)).astype(np.float32)
    b_ih = rng.normal(0.0, 0.1, size=(512,)).astype(np.float32)
    b_hh = rng.normal(0.0, 0.1, size=(512,)).astype(np.float32)
    out += [("_model.decoder.rnn.weight_ih", w_ih), ("_model.decoder.rnn.weight_hh", w_hh),
            ("_model.decoder.rnn.bias_ih", b_ih), ("_model.decoder.rnn.bias_hh", b_hh)]
    w_f = 2.0 * np.abs(rng.normal(0.0, 0.6, size=(1, 128)))
    out.append(("_model.decoder.decoder.2.weight", w_f.astype(np.float16)))
    out.append(("_model.decoder.decoder.2.bias", np.array([-5.2], dtype=np.float32)))
    return out


def model_bytes(seed: int = 0, *, magic: int = GGML_MAGIC, layers=None, drop: str | None = None, with_tensors: bool = True) -> bytes:
    """The model file.  `magic`, `layers` (another layer table) and `drop` (a tensor name to leave out) make the files the loader must refuse."""
    parts = [struct.pack("<I", magic)]
    mtype = b"silero-16k"
    parts.append(struct.pack("<i", len(mtype)) + mtype)
    parts.append(struct.pack("<3i", 5, 1, 2))
    parts.append(struct.pack("<2i", N_WINDOW, 64))                    # n_window, n_context
    layers = ENC if layers is None else layers
    parts.append(struct.pack("<i", len(layers)))
    for cin, cout in layers:
        parts.append(struct.pack("<3i", cin, cout, 3))
    parts.append(struct.pack("<4i", 128, 128, 128, 1))                # lstm_input_size, lstm_hidden_size, final_conv_in, final_conv_out
    if with_tensors:
        for name, arr in tensors(seed):
            if name == drop:
                continue
            nb = name.encode()
            parts.append(struct.pack("<3i", arr.ndim, len(nb), 1 if arr.dtype == np.float16 else 0))
            parts.append(struct.pack("<%di" % arr.ndim, *reversed(arr.shape)))
            parts.append(nb)
            parts.append(np.ascontiguousarray(arr).tobytes())
    return b"".join(parts)


def model_path(seed: int = 0, cache_dir: str | None = None) -> str:
    cache_dir = cache_dir or os.environ.get("WHISPER_AMD_CACHE", "/tmp/whisper_amd_cache")
    os.makedirs(cache_dir, exist_ok=True)
    p = os.path.join(cache_dir, f"synth-vad-seed{seed}.bin")
    if not os.path.exists(p):
        tmp = p + ".tmp%d" % os.getpid()
        with open(tmp, "wb") as f:
            f.write(model_bytes(seed))
        os.replace(tmp, p)
    return p


N_AUDIO = 16000 * 14 + 137                                           # 438 windows, the last one partial
BURSTS = [(1.0, 2.2), (2.35, 3.0), (5.0, 5.1), (7.0, 9.5), (12.0, 12.6)]    # seconds of "speech"


def synth_audio(seed: int = 0) -> np.ndarray:
    """Tone + chirp inside BURSTS, faint noise everywhere: long and short bursts, a short gap, a burst too short to count."""
    rng = np.random.default_rng(2000 + seed)
    t = np.arange(N_AUDIO, dtype=np.float64) / 16000.0
    env = np.zeros(N_AUDIO)
    for a, b in BURSTS:
        env[(t >= a) & (t < b)] = 1.0
    x = env * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 100.0 * t) * t))
    x += 0.002 * rng.standard_normal(N_AUDIO)
    return x.astype(np.float32)


# (threshold, min_speech_duration_ms, min_silence_duration_ms, max_speech_duration_s, speech_pad_ms, samples_overlap)
FLT_MAX = float(np.finfo(np.float32).max)
PARAM_SETS = {
    "default":   (0.5, 250, 100, FLT_MAX, 30, 0.1),
    "max1.5s":   (0.5, 250, 100, 1.5, 30, 0.1),
    "thr0.6":    (0.6, 100, 300, FLT_MAX, 100, 0.1),
}


if __name__ == "__main__":
    p = model_path()
    print(p, os.path.getsize(p))

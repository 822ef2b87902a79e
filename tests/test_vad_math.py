"""Voice activity detection, host part (whisper-rust_amd/csrc/wa_vad_host.cpp compiled alone by g++: no HIP, no device).

tests/native/vad_math.cpp links the product's model parser, LSTM recurrence, segment rules, speech-only audio and time mapping, and
adds a plain scalar restatement of the device's front end in the reference's order of operations.  Together they must give the
reference engine's probabilities BIT FOR BIT (tests/golden/vad.json, recorded from oracle/_ref/libwhisper_ref.so by
tools/gen_golden_vad.py; and the live reference library where it is built), its segments for three parameter sets, and the recorded
time mapping.  The restatement's front-end digests are the ones tests/test_vad_gpu.py holds the kernel to.  CPU only."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import wsynth_vad as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "vad.json"))) if os.path.exists(os.path.join(ROOT, "tests", "golden", "vad.json")) else None
SR = 16000


def fmt_params(ps):
    return " ".join(repr(float(np.float32(x))) if isinstance(x, float) else str(x) for x in ps)


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """The harness, the model file, the audio (checked against the hashes the golden file was recorded with)."""
    assert GOLDEN is not None, "tests/golden/vad.json is missing"
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("vad")
    exe = str(work / "vad_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-mavx2", "-mf16c", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "native", "vad_math.cpp"),
                           os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_vad_host.cpp"), "-o", exe])
    mp, pcm = V.model_path(), V.synth_audio()
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == GOLDEN["model_sha256"], "the synthetic VAD model is not the recorded one"
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == GOLDEN["audio_sha256"], "the synthetic audio is not the recorded one"
    pcm_path = str(work / "audio.f32")
    pcm.tofile(pcm_path)
    return dict(exe=exe, work=work, model=mp, pcm=pcm, pcm_path=pcm_path)


def run(env, lines, model=None):
    script = env["work"] / "script.txt"
    script.write_text("\n".join(["model " + (model or env["model"]), "audio " + env["pcm_path"]] + list(lines)) + "\n")
    out = subprocess.run([env["exe"], str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


def bits_of(line):
    f = line.split()
    assert f[0] == "probs" and int(f[1]) == len(f) - 2, line[:80]
    return [int(x, 16) for x in f[2:]]


@pytest.fixture(scope="module")
def probs(env):
    """One harness run for every recorded input; "full" a second time at the end (each call starts from a zero LSTM state)."""
    tags = list(GOLDEN["probs"])
    out = run(env, ["probs %d" % GOLDEN["probs"][t]["n_samples"] for t in tags] + ["probs %d" % GOLDEN["n_samples"]])
    assert out[0] == "model ok" and out[1] == "audio %d" % GOLDEN["n_samples"]
    got = {t: bits_of(line) for t, line in zip(tags, out[2:])}
    got["full_again"] = bits_of(out[2 + len(tags)])
    return got


@pytest.mark.parametrize("tag", ["full", "n1", "n511", "n512", "n513", "c1", "c7", "c8", "c9"])
def test_probabilities_bit_exact(probs, tag):
    want = GOLDEN["probs"][tag]["bits"]
    assert len(want) == -(-GOLDEN["probs"][tag]["n_samples"] // 512)
    assert probs[tag] == want


def test_probabilities_span_the_thresholds(probs):
    p = np.array(probs["full"], dtype=np.uint32).view(np.float32)
    assert len(p) == 438 and (p >= 0.5).sum() > 50 and (p < 0.35).sum() > 50 and ((p >= 0.35) & (p < 0.5)).sum() > 5


def test_state_is_reset_between_calls(probs):
    assert probs["full_again"] == GOLDEN["probs"]["full"]["bits"]


@pytest.mark.parametrize("tag", sorted(GOLDEN["front"]) if GOLDEN else [])
def test_front_end_digest(env, tag):
    g = GOLDEN["front"][tag]
    path = env["work"] / ("front_%s.f32" % tag)
    assert run(env, ["front %d %s" % (g["n_samples"], path)])[-1] == "front %d" % g["n_chunks"]
    a = np.fromfile(str(path), dtype=np.float32).reshape(-1, 512)
    assert a.shape[0] == g["n_chunks"]
    for r, want in g["rows"].items():
        assert [int(x) for x in a[int(r), ::64].view(np.uint32)] == want
    assert hashlib.sha256(a.tobytes()).hexdigest() == g["sha256"]


@pytest.mark.parametrize("tag", list(V.PARAM_SETS))
def test_segments(env, tag):
    g = GOLDEN["segments"][tag]
    out = run(env, ["segments %d %s" % (GOLDEN["n_samples"], fmt_params(V.PARAM_SETS[tag]))])[-1].split()
    assert out[0] == "segments"
    got = [[int(out[2 + 2 * i]), int(out[3 + 2 * i])] for i in range(int(out[1]))]
    assert got == g["segments"]
    if tag != "default":
        assert got != GOLDEN["segments"]["default"]["segments"]


def cs_to_samples(cs):
    return int((cs / 100.0) * SR + 0.5)


@pytest.mark.parametrize("tag", list(V.PARAM_SETS))
def test_time_mapping_and_filtered_audio(env, tag):
    g, segs = GOLDEN["map"][tag], GOLDEN["segments"][tag]["segments"]
    path = env["work"] / ("filtered_%s.f32" % tag)
    f = run(env, ["map %d %s %s" % (GOLDEN["n_samples"], fmt_params(V.PARAM_SETS[tag]), path)])[-1].split()
    assert f[0] == "map" and f[2] == "table"
    n_filtered, n_table = int(f[1]), int(f[3])
    table = [[int(f[4 + 2 * i]), int(f[5 + 2 * i])] for i in range(n_table)]
    at = 4 + 2 * n_table
    assert f[at] == "sweep"
    sweep = [int(x) for x in f[at + 2:at + 2 + int(f[at + 1])]]
    assert n_filtered == g["n_filtered"] == g["ref_n_copied"]          # the length the reference hands to the transcription
    assert table == g["table"]
    assert [p for p, _ in table] == sorted({p for p, _ in table})      # strictly increasing processed times
    for o0, o1, v0, v1 in g["ref_segment_info"]:                       # the points the reference logged
        assert [v0, o0] in table and (([v1, o1] in table) or any(p == v1 for p, _ in table))
    assert sweep == g["sweep"] and len(sweep) == n_filtered * 100 // SR + 2
    # the audio itself: each segment (+ 0.1 s overlap except the last), 0.1 s of zeros between them
    pcm, want = env["pcm"], []
    for i, (s, e) in enumerate(segs):
        last = i == len(segs) - 1
        want.append(pcm[min(cs_to_samples(s), len(pcm) - 1):min(cs_to_samples(e) + (0 if last else 1600), len(pcm))])
        if not last:
            want.append(np.zeros(1600, dtype=np.float32))
    want = np.concatenate(want)[:n_filtered]
    got = np.fromfile(str(path), dtype=np.float32)
    assert got.shape == (n_filtered,) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_loader_refusals(env):
    good = V.model_bytes()
    files = {
        "bad_magic": V.model_bytes(magic=0x12345678),
        "wrong_layers": V.model_bytes(layers=[(129, 128), (128, 64), (64, 96), (96, 128)]),
        "three_layers": V.model_bytes(layers=V.ENC[:3]),
        "missing_tensor": V.model_bytes(drop="_model.decoder.rnn.bias_hh"),
        "no_tensors": V.model_bytes(with_tensors=False),
        "truncated_tensor": good[:len(good) // 2],
        "truncated_header": good[:30],
    }
    for name, data in files.items():
        p = env["work"] / (name + ".bin")
        p.write_bytes(data)
        out = run(env, [], model=str(p))
        assert out[0].startswith("model fail "), (name, out[0])
        if name == "bad_magic":
            assert "magic" in out[0]
        else:
            assert "supported: n_window 512" in out[0], (name, out[0])       # the refusal names the one supported shape
        if name == "missing_tensor":
            assert "_model.decoder.rnn.bias_hh" in out[0]
    assert run(env, [])[0] == "model ok"


def test_live_reference(env, probs, ref_lib, wrs):
    """With the reference library built: the same probabilities and segments from it, now."""
    v = wrs.WhisperVadContext.new(env["model"], lib=ref_lib)
    try:
        for tag in ("full", "n1", "n511", "n512", "n513"):
            got = v.detect_speech(env["pcm"][:GOLDEN["probs"][tag]["n_samples"]])
            assert [int(x) for x in got.view(np.uint32)] == probs[tag], tag
        v.detect_speech(env["pcm"])
        for tag, ps in V.PARAM_SETS.items():
            assert [[int(a), int(b)] for a, b in v.segments_from_probs(wrs.vad_params(ref_lib, *ps))] == GOLDEN["segments"][tag]["segments"]
    finally:
        v.free()

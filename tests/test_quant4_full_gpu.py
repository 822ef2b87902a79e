"""Q4_0 and Q4_K model files (MI355X) through the C ABI: the formats the reference multiplies through its interleaved 8-row products - one float chain
per output (Q4_0), two with a step rule and an activation quantiser that depend on the row's place in the product (Q4_K)
(whisper-rust_amd/csrc/wa_quant4.h, held to the reference library on the CPU by tests/test_quant4_math.py; the kernels one by one:
tests/test_quant4_kernels_gpu.py).

  * goldens from the reference engine on s256 (tests/golden/s256_quant4.json, tools/gen_golden_quant4.py): model sha256, encoder digest, teacher-forced
    logits digests, token ids and a digest of the segments (times, text, ids, p, plog) of greedy, the default ladder and beam 3; greedy and beam 3 again on the stalled
    test build;
  * the reference engine itself run LIVE beside the product on base:q4_0 / base:q4_k (d = 512): encoder output, prompt / single-token / 5-token logits, a greedy full();
  * routes and switches: whisper_amd_qgemm_stats shows the matrix-core route taken, WHISPER_AMD_NO_QMFMA=1 and WHISPER_AMD_LOAD_HOST=1 in fresh
    processes give the default path's digest, both load paths give the same arena, a lock-step group of 3 gives its members' solo results, both
    one-launch forms decline the formats, a truncated file and a Q4_K header on d = 128 fail at load, and without WHISPER_AMD_REPACK_ORDER=1 (set for this module:
    the bits are those of the reference's AVX2 repack build) the files are refused as before.
Everything is equality of bytes or of token lists.  Before these formats loaded, every test here that opens such a file failed with "unsupported ftype 2" /
"unsupported ftype 12"."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import pytest

import wsynth
from conftest import GOLDEN
from test_kquant23_gpu import _get, _load_fails, _params, _segs, digest
from test_kquant23_gpu import test_base_live_beside_the_reference as _live
from test_load_device_gpu import load_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTYPE = {"q4_0": 2, "q4_k": 12}
QTYPES = pytest.mark.parametrize("qt", sorted(FTYPE))


@pytest.fixture(scope="module", autouse=True)
def repack_order():
    """These formats load only where the caller names the reference build whose bits they give (read at every load; child processes inherit it)."""
    old = os.environ.get("WHISPER_AMD_REPACK_ORDER")
    os.environ["WHISPER_AMD_REPACK_ORDER"] = "1"
    yield
    os.environ.pop("WHISPER_AMD_REPACK_ORDER")
    if old is not None:
        os.environ["WHISPER_AMD_REPACK_ORDER"] = old


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "s256_quant4.json")))


def _full(wrs, lib, ctx, tag, aseed):
    import gen_golden_quant as g
    st = ctx.create_state()
    st.full(_params(wrs, lib, g.FULL[tag]), wsynth.synth_audio(480000, aseed))
    sg = _segs(st)
    st.free()
    return dict(ids=[x["ids"] for x in sg], sha256=hashlib.sha256(json.dumps(sg, sort_keys=True).encode()).hexdigest())


@QTYPES
def test_models_bit_exact_against_goldens(wrs, amd_lib, gold, qt):
    """s256 quantised by the reference's own tool: the file the goldens were made from, ftype, encoder output and teacher-forced logits (a 3-token prompt, single
    steps, a 5-token batch, 40 tokens) bit-identical to the reference engine (digests), identical token ids and segment digest (times, text, ids, p, plog) for
    greedy, the temperature ladder and beam 3 (each >= 10 distinct ids), the encoder's 1500-row products on the matrix cores, neither one-launch form anywhere near."""
    gd = gold[qt]
    mp = wsynth.quant_model_path("s256", qt)
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == gd["model_sha256"], "the quantised model file differs from the goldens'"
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    assert ctx.model_ftype() == FTYPE[qt]
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0)); st.encode(0)
    assert digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * ctx.model_n_audio_state())) == gd["embd_enc"]["sha256"]
    n_mfma, n_general = st.qgemm_stats()
    assert n_mfma > 0 and n_general == 0, (n_mfma, n_general)
    for e in gd["logits"]:
        st.decode(e["tokens"], e["n_past"])
        assert digest(st.get_logits_last(len(e["tokens"]))) == e["sha256"], (e["tokens"][:3], e["n_past"])
    amd_lib.whisper_amd_mega_enabled.argtypes = amd_lib.whisper_amd_rows_enabled.argtypes = [C.c_void_p]
    assert amd_lib.whisper_amd_mega_enabled(st.ptr) == 0 and amd_lib.whisper_amd_rows_enabled(st.ptr) == 0 and st.rows_stats() == (0, 0)
    st.free()
    for key, want in gd["full"].items():
        assert len({i for ids in want["ids"] for i in ids}) >= 10, (qt, key)
        assert _full(wrs, amd_lib, ctx, key.split("_seed")[0], int(key[-1])) == want, (qt, key)
    ctx.free()


@QTYPES
def test_greedy_and_beam_on_the_stalled_build(wrs, gold, qt):
    chaos = wrs.load_library(os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so"))
    wrs.set_log_callback(chaos, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", qt), wrs.WhisperContextParameters(chaos), lib=chaos)
    for tag in ("greedy", "beam3"):
        assert _full(wrs, chaos, ctx, tag, 0) == gold[qt]["full"][tag + "_seed0"], (qt, tag)
    ctx.free()


@QTYPES
def test_base_live_beside_the_reference(wrs, amd_lib, ref_lib, qt):
    """base (d = 512; Q4_0: 16 blocks per row, 64 in the second MLP product; Q4_K: 2 and 8): encoder output, the logits of a 3-token prompt (gemv rows only), of a
    single token and of a 5-token batch (four gemm rows and a leftover row), and a greedy full() equal to the reference engine's on the same file and inputs."""
    _live(wrs, amd_lib, ref_lib, "base:" + qt)


def _switch_digest(qt, env_extra):
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_check.py"), "s256:" + qt], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_extra, r.stdout[-400:], r.stderr[-800:])
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")]
    assert line and int(line[-1].split()[-1]) > 0, (env_extra, r.stdout[-400:])
    return line[-1]


@QTYPES
def test_switches_do_not_change_a_bit(qt):
    """WHISPER_AMD_NO_QMFMA=1 (more than 8 rows through the few-rows kernel in slices) and WHISPER_AMD_LOAD_HOST=1 (the host load path), one fresh
    process each (tools/switch_check.py: four chunks in a lock-step group, greedy, beam 5, best_of 3 with the ladder): the default path's digest."""
    want = _switch_digest(qt, {})
    for env_extra in ({"WHISPER_AMD_NO_QMFMA": "1"}, {"WHISPER_AMD_LOAD_HOST": "1"}):
        assert _switch_digest(qt, env_extra) == want, env_extra


@QTYPES
def test_load_paths_lockstep_group_and_truncated_file(wrs, amd_lib, tmp_path, qt):
    """Both load paths leave the same arena, byte for byte; a lock-step group of 3 chunks gives each chunk's solo segments; a truncated file fails at load."""
    mp = wsynth.quant_model_path("s256", qt)
    arenas = []
    for host in (True, False):
        with load_env(host=host):
            ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
        assert ctx.load_stats()["path"] == (0 if host else 1)
        arenas.append(digest(ctx.arena()))
        if host:
            ctx.free()
    assert arenas[0] == arenas[1]
    pcms = [wsynth.synth_audio(480000, 50 + i) for i in range(3)]
    fp = wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0)
    solo = []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    assert any(solo)
    states = [ctx.create_state() for _ in pcms]
    wrs.full_batch(ctx, states, fp, pcms)
    for i, st in enumerate(states):
        assert _segs(st) == solo[i], i
        st.free()
    ctx.free()
    full = open(mp, "rb").read()
    cut = str(tmp_path / "cut.bin")
    open(cut, "wb").write(full[:len(full) - 100000])
    text = _load_fails(wrs, amd_lib, cut)
    assert "truncated tensor" in text or "not all tensors loaded" in text, text[-600:]


def test_q4_K_header_on_a_width_without_a_block_and_refusal_without_the_switch(wrs, amd_lib, tmp_path, monkeypatch):
    """An ftype-12 header on a d = 128 model (its rows hold no 256-value block) fails at load with a message that says why; so does a good file where the
    environment does not ask for the repack build's order."""
    src = wsynth.model_path("s128")
    raw = bytearray(open(src, "rb").read(4 + 11 * 4))
    assert struct.unpack_from("<i", raw, 4 + 2 * 4)[0] == 128
    struct.pack_into("<i", raw, 4 + 10 * 4, 12)
    bad = str(tmp_path / "s128-ftype12.bin")
    with open(src, "rb") as f, open(bad, "wb") as o:
        f.seek(len(raw)); o.write(raw); o.write(f.read())
    text = _load_fails(wrs, amd_lib, bad)
    assert "multiple of 256" in text and "128" in text and "Q4_K" in text, text[-600:]
    monkeypatch.delenv("WHISPER_AMD_REPACK_ORDER")
    text = _load_fails(wrs, amd_lib, wsynth.quant_model_path("s256", "q4_0"))
    assert "unsupported ftype 2" in text and "WHISPER_AMD_REPACK_ORDER" in text, text[-600:]

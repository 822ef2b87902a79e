"""The one-exchange cross-attention role of k_decode_mega_cq (wa_mega.hip, mg_role_cross X1: scores exchanged once, the soft-max whole in
every quarter, P V split by output) on the only shape that runs it - F16, d = 768 -, over the degenerate audio contexts: no full 32-cell
chain step (T < 32), quarters without a cell (T < 8), T % 8 and T % 32 tails, and the full 1500.  The launch sequence is the yardstick."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

N_TOK = 12
CHAOS_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust_amd", "libwhisper_chaos.so")


def _full_both_ways(wrs, lib, ctx, pcm, actx, monkeypatch):
    """whisper_full greedy, single_segment, at audio_ctx = actx: {"1": launch sequence, "0": one-launch step}; the latter must still be on
    afterwards.  Also compares, bit for bit, the logits of single-token steps against that audio context."""
    lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    lib.whisper_amd_mega_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    res, logits = {}, {}
    for nomega in ("1", "0"):
        monkeypatch.setenv("WHISPER_AMD_NO_MEGA", nomega)
        st = ctx.create_state()
        assert lib.whisper_amd_mega_enabled(st.ptr) == (0 if nomega == "1" else 1)
        st.full(wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0, audio_ctx=actx, single_segment=True), pcm)
        res[nomega] = [(s["t0"], s["t1"], s["ids"], s["p"], s["plog"]) for s in st.segments()]
        # A synthetic model may end such a window at once, and then no single-token step ran above.  So, against the audio context the
        # state has just encoded: N_TOK single-token steps from a fixed prompt, every logit kept.
        sot = ctx.token_sot()
        prompt = [sot, sot + 1, sot + 102]
        st.decode(prompt, 0)
        toks, rows = [1000 + 37 * i for i in range(N_TOK)], []
        for i, tok in enumerate(toks):
            st.decode([tok], len(prompt) + i)
            rows.append(st.get_logits_last(1).copy())
        logits[nomega] = np.stack(rows)
        if nomega == "0":
            assert lib.whisper_amd_mega_enabled(st.ptr) == 1, "audio_ctx %d: the one-launch step gave up and fell back" % actx
            # A step whose soft-max total cannot be certified ends with status WA_MEGA_REDO, and whisper_decode then redoes the token by the
            # launch sequence without switching the form off: a role that always asked for that would pass everything above.  So the same
            # steps once more as bare launches of the kernel (it rewrites KV cell n_past with the same values): status 0 and these logits.
            kernel = np.zeros((N_TOK, rows[0].size), dtype=np.float32)
            for i, tok in enumerate(toks):
                rc = lib.whisper_amd_mega_debug(ctx.ptr, st.ptr, tok, len(prompt) + i, None, kernel[i].ctypes.data)
                assert rc == 0, "audio_ctx %d, step %d: the one-launch kernel ended with status %d (9000 = redone by the launch sequence)" % (actx, i, rc)
            off = np.nonzero((kernel.view(np.uint32) != logits["1"].view(np.uint32)).any(axis=1))[0]
            assert off.size == 0, "audio_ctx %d: the kernel's own logits differ from the launch sequence's at steps %s" % (actx, off.tolist())
        st.free()
    assert np.isfinite(logits["1"]).all()
    differ = np.nonzero((logits["0"].view(np.uint32) != logits["1"].view(np.uint32)).any(axis=1))[0]
    assert differ.size == 0, "audio_ctx %d: logits differ from the launch sequence's at single-token steps %s" % (actx, differ.tolist())
    return res


@pytest.mark.parametrize("actx", [1, 7, 33, 50, 257, 1500])
def test_one_exchange_cross_attention_equals_launch_sequence(wrs, amd_lib, actx, monkeypatch):
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("small"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    res = _full_both_ways(wrs, amd_lib, ctx, wsynth.synth_audio(16000 * 3, 5), actx, monkeypatch)
    assert res["0"] == res["1"], actx
    ctx.free()


@pytest.mark.parametrize("actx", [50, 1500])
def test_one_exchange_cross_attention_under_stalls(wrs, actx, monkeypatch):
    """The same on the build whose waves stall at random in front of the gather, the soft-max and the P V product (-DWA_CHAOS)."""
    assert os.path.exists(CHAOS_LIB), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(CHAOS_LIB)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("small"), wrs.WhisperContextParameters(lib), lib=lib)
    res = _full_both_ways(wrs, lib, ctx, wsynth.synth_audio(16000 * 3, 5), actx, monkeypatch)
    assert res["0"] == res["1"], actx
    ctx.free()

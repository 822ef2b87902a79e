"""The self-attention role of the one-launch decode step (wa_mega.hip, mg_role_self) against the launch sequence, bit for bit on
single-token logits, over the context lengths at which the role changes its path: every n_kv from 4 to 70 (n % 8, n % 32, and 64 | 65,
the edge of the one-wave path of k_decode_mega_cq), the edges of the score passes and of the P V blocks (128, 192, 256) and the last cell
of WA_MEGA_KV_ROOM.  One pair of states per model: `small` runs k_decode_mega_cq (the role's serial path without LDS round trips),
`s128` k_decode_mega and `s128:q8_0` k_decode_mega_q (the role's first form, in the same function template)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

CHAOS_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust_amd", "libwhisper_chaos.so")
KV_ROOM = 448           # WA_MEGA_KV_ROOM (wa_mega.h): longer contexts go through the launch sequence
N_PROMPT = 3
ALL_NKV = list(range(4, 71)) + list(range(126, 132)) + list(range(190, 195)) + list(range(254, 259)) + list(range(445, 449))
STALL_NKV = list(range(60, 71)) + list(range(126, 132))


def _tok(pos):
    return 1000 + 37 * pos


def _walk(st, n_kvs):
    """Single-token steps at every context length of n_kvs (ascending); the cells in between are filled by batch decodes.  Returns
    [(token, n_past)] and the logits of every single step."""
    sot = st.ctx.token_sot()
    st.decode([sot, sot + 1, sot + 102], 0)
    n_past, steps, rows = N_PROMPT, [], []
    for n_kv in n_kvs:
        while n_past < n_kv - 1:        # move ahead: the same batches on both states
            n = min(n_kv - 1 - n_past, 48)
            st.decode([_tok(p) for p in range(n_past, n_past + n)], n_past)
            n_past += n
        st.decode([_tok(n_past)], n_past)
        rows.append(st.get_logits_last(1).copy())
        steps.append((_tok(n_past), n_past))
        n_past += 1
    return steps, np.stack(rows)


def _compare(wrs, lib, name, n_kvs, monkeypatch, limit):
    lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    lib.whisper_amd_mega_debug.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); ref = ctx.create_state()
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); meg = ctx.create_state()
    assert lib.whisper_amd_mega_enabled(ref.ptr) == 0 and lib.whisper_amd_mega_enabled(meg.ptr) == 1
    pcm = wsynth.synth_audio(16000 * 3, 5)
    for st in (ref, meg):
        st.pcm_to_mel(pcm); st.encode(0)
    steps, want = _walk(ref, n_kvs)
    steps_m, got = _walk(meg, n_kvs)
    assert steps == steps_m and [p + 1 for _, p in steps] == list(n_kvs)
    assert np.isfinite(want).all()
    assert lib.whisper_amd_mega_enabled(meg.ptr) == 1, "%s: the one-launch step gave up and fell back" % name
    off = [steps[i][1] + 1 for i in np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]]
    assert not off, "%s: logits differ from the launch sequence's at n_kv %s" % (name, off)
    # A step that ends with status WA_MEGA_REDO is redone by the launch sequence inside whisper_decode and would pass the comparison above.
    # So every step once more as a bare launch of the kernel (it rewrites cell n_past with the same values): status 0 and the same logits.
    kernel = np.zeros(want.shape[1], dtype=np.float32)
    for i, (tok, n_past) in enumerate(steps):
        rc = lib.whisper_amd_mega_debug(ctx.ptr, meg.ptr, tok, n_past, None, kernel.ctypes.data)
        assert rc == 0, "%s, n_kv %d: the one-launch kernel ended with status %d (9000 = redone by the launch sequence)" % (name, n_past + 1, rc)
        assert (kernel.view(np.uint32) == want[i].view(np.uint32)).all(), "%s, n_kv %d: the kernel's own logits differ from the launch sequence's" % (name, n_past + 1)
    if limit:       # n_kv = WA_MEGA_KV_ROOM + 1: the host does not build a one-launch step at all (whisper_decode routes it to the launch sequence)
        assert steps[-1][1] + 1 == KV_ROOM
        assert lib.whisper_amd_mega_debug(ctx.ptr, meg.ptr, _tok(KV_ROOM), KV_ROOM, None, kernel.ctypes.data) == -2
    ref.free(); meg.free(); ctx.free()


@pytest.mark.parametrize("name", ["small", "s128", "s128:q8_0"])
def test_self_role_equals_launch_sequence_at_every_path_edge(wrs, amd_lib, name, monkeypatch):
    _compare(wrs, amd_lib, name, ALL_NKV, monkeypatch, limit=True)


def test_self_role_under_stalls(wrs, monkeypatch):
    """The same on the build whose waves stall at random (-DWA_CHAOS) - in the role: after the gather, between scores and soft-max, and in
    front of P V -, on both sides of the one-wave edge and of the second wave pair."""
    assert os.path.exists(CHAOS_LIB), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(CHAOS_LIB)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    _compare(wrs, lib, "small", STALL_NKV, monkeypatch, limit=False)

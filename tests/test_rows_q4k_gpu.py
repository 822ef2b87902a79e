"""The several-rows one-launch decode step for Q4_K models (wa_rows.hip: k_decode_rows_q4k_np*; opt-in, WHISPER_AMD_ROWS_Q4K=1 when a state is made) against
a state made with the switch unset: the launch sequence, which test_quant4_full_gpu.py pins to the reference engine.  Equality of logits rows as uint32
words or of segment lists, and counts of served passes: a pass the kernel sends back would pass any comparison.  What a Q4_K row computes depends on its
place in the pass (wa_quant4.h): (a) runs passes whose rows are all gemv rows (B <= 3), all gemm rows (4, 8) and both (5, 6, 7); (b) rows that are
passes of their own whatever their number."""
import hashlib
import json
import os

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN
from test_quant1_gpu import CHAOS_LIB, _params, _segs
from test_quant4_full_gpu import repack_order  # noqa: F401  (a fixture: WHISPER_AMD_REPACK_ORDER=1 for this module, the format loads only under it)
from test_rows_kernel_gpu import EDGES_REDUCED, _Served, _advance, _bits_equal, _chunks, _fits, _tok, ctxs  # noqa: F401  (ctxs: a fixture)

pytestmark = pytest.mark.gpu
# model -> (the row counts wa_rows_lds_bytes(quant = 6) admits on 256 workgroups, the row counts a whisper_decode pass is served with).  DESIGN.md 4.3.1: the
# nibble rows are half of Q5_K's bytes, so eight rows fit even at d = 1280; but beyond d = 1024 only lock-step passes gained when measured, so there a
# whisper_decode pass keeps the launch sequence (wa_rows_lockstep_only) and the kernel is reached through (b)
MODELS = {"s256:q4_k": (8, 8), "base:q4_k": (8, 8), "w1280:q4_k": (8, 0)}
SWITCH = "WHISPER_AMD_ROWS_Q4K"


def _states(ctx, lib, monkeypatch, n=1, seeds=None):
    """n launch-sequence states and n states made under the switch; state i of either list has heard the same 3 s of audio"""
    monkeypatch.delenv(SWITCH, raising=False); refs = [ctx.create_state() for _ in range(n)]
    monkeypatch.setenv(SWITCH, "1"); rows = [ctx.create_state() for _ in range(n)]; monkeypatch.delenv(SWITCH)
    assert all(lib.whisper_amd_rows_enabled(s.ptr) == 1 for s in rows), "the several-rows form is off under %s=1" % SWITCH
    assert all(lib.whisper_amd_rows_enabled(s.ptr) == 0 for s in refs)
    for i, st in [(i, st) for i in range(n) for st in (refs[i], rows[i])]:
        st.pcm_to_mel(wsynth.synth_audio(16000 * 3, seeds[i] if seeds else 5)); st.encode(0)
    return refs, rows


@pytest.mark.parametrize("name", list(MODELS))
def test_causal_batches_at_path_edges(wrs, amd_lib, ctxs, name, monkeypatch):
    """(a) 1..8 rows through whisper_decode on both sides of the self-attention edges.  Blocks of a row, d-long / 4d-long: s256 1 / 4, base 2 / 8; w1280: no
    pass is served, and none comes back"""
    ctx = ctxs(name)
    assert _fits(ctx) == list(range(1, MODELS[name][0] + 1)), name
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch)
    count, cur = _Served(ctx, row), 0
    for n_kv in ([129, 160] if name.startswith("w1280") else EDGES_REDUCED):
        for B in range(1, 9):
            n_past = n_kv - B
            _advance((ref, row), cur, n_past)           # (fewer cells wanted than there are: whisper_decode drops the cells from n_past on)
            toks = [_tok(p) for p in range(n_past, n_kv)]
            ref.decode(toks, n_past); row.decode(toks, n_past)
            assert row.kv_op(4) == n_kv and ref.kv_op(4) == n_kv and (B > MODELS[name][1] or count.step(B))
            _bits_equal(ref.get_logits_last(B), row.get_logits_last(B), "%s, B %d, n_kv %d" % (name, B, n_kv))
            cur = n_kv
    count.check(name); ref.free(); row.free()


@pytest.mark.parametrize("name", ["s256:q4_k", "w1280:q4_k"])
def test_lockstep_rows_with_a_context_length_each(wrs, amd_lib, ctxs, name, monkeypatch):
    """(b) the lock-step shape: every row on its own state, with its own context length - and a pass of its own in the reference: gemv rows at every B.
    w1280 (5 / 20 blocks a row, k_decode_rows_q4k_np20): the passes that width is served with"""
    n_pasts = [3, 31, 64, 127, 160, 255, 300, 447]
    ctx, n = ctxs(name), len(n_pasts)
    refs, rows = _states(ctx, amd_lib, monkeypatch, n=n, seeds=[5 + i for i in range(n)])
    toks, want, stats0 = [_tok(n_pasts[i]) + i for i in range(n)], [], [st.rows_stats() for st in rows]
    for i in range(n):          # the same cells in both states of a pair; the twin's single-token step by the launch sequence is the reference, made once
        s = 0
        for c in _chunks(max(n_pasts[i], 9)):
            refs[i].decode([_tok(p) + i for p in range(s, s + c)], s); rows[i].decode([_tok(p) + i for p in range(s, s + c)], s)
            s += c
        refs[i].decode([toks[i]], n_pasts[i])
        want.append(refs[i].get_logits_last(1).copy())
    want = np.stack(want)
    for B in range(1, 9):
        for rot in range(n):    # every state meets every row index
            idx = [(rot + k) % n for k in range(B)]
            rc, got, status = wrs.rows_debug_rows(ctx, [rows[i] for i in idx], [toks[i] for i in idx], [n_pasts[i] for i in idx])
            what = "%s, B %d, rows of n_kv %s" % (name, B, [n_pasts[i] + 1 for i in idx])
            assert rc == 0 and (status == 0).all(), "%s: the kernel ended with status %d, row status %s" % (what, rc, status.tolist())
            _bits_equal(want[idx], got, what)
    assert [st.rows_stats() for st in rows] == stats0 and all(amd_lib.whisper_amd_rows_enabled(st.ptr) == 1 for st in rows)
    [st.free() for st in refs + rows]


@pytest.mark.parametrize("build,tags", [("product", ("greedy", "ladder", "beam3")), ("stalled", ("greedy",))])
def test_full_against_goldens(wrs, amd_lib, build, tags, monkeypatch):
    """(c) whisper_full under the switch against the reference engine's goldens (ids and segment digest, as test_quant4_full_gpu.py forms them); greedy once
    more on the build whose product waves stall at random"""
    import gen_golden_quant as g
    gold = json.load(open(os.path.join(GOLDEN, "s256_quant4.json")))["q4_k"]
    lib = wrs.load_library(CHAOS_LIB) if build == "stalled" else amd_lib
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", "q4_k"), wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv(SWITCH, "1")
    for tag in tags:
        for aseed in (0, 1):
            st = ctx.create_state()
            assert lib.whisper_amd_rows_enabled(st.ptr) == 1
            st.full(_params(wrs, lib, g.FULL[tag]), wsynth.synth_audio(480000, aseed))
            sg = _segs(st)
            got = dict(ids=[x["ids"] for x in sg], sha256=hashlib.sha256(json.dumps(sg, sort_keys=True).encode()).hexdigest())
            assert got == gold["full"]["%s_seed%d" % (tag, aseed)], (tag, aseed)
            assert st.rows_stats()[0] > 0 and st.rows_stats()[1] == 0 and lib.whisper_amd_rows_enabled(st.ptr) == 1, (tag, aseed, st.rows_stats())
            st.free()
    ctx.free()


def test_lockstep_group_equals_solo_and_is_served(wrs, amd_lib, monkeypatch):
    """(d) four s256:q4_k chunks through whisper_amd_full_batch (a context of its own: the group's private state is made under the switch too)"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", "q4_k"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcms, fp, solo = [wsynth.synth_audio(480000, 50 + i) for i in range(4)], wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0), []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    monkeypatch.setenv(SWITCH, "1"); states = [ctx.create_state() for _ in pcms]
    assert all(amd_lib.whisper_amd_rows_enabled(st.ptr) == 1 for st in states)
    wrs.full_batch(ctx, states, fp, pcms)
    assert int(amd_lib.whisper_amd_batch_served(ctx.ptr)) > 0, "no pass of the group was delivered by the group"
    assert [_segs(st) for st in states] == solo
    [st.free() for st in states]; ctx.free()


@pytest.mark.parametrize("name", ["s256:q4_0", "s256:q5_k", "s256:q5_0", "s256:q4_k"])
def test_switch_is_q4_k_s_alone(wrs, amd_lib, ctxs, name, monkeypatch):
    """(e) a Q4_0, a Q5_K or a Q5_0 state made under the switch is what it is without it; a Q4_K state made without it keeps the launch sequence"""
    ctx = ctxs(name)
    monkeypatch.delenv(SWITCH, raising=False); st = ctx.create_state(); without = amd_lib.whisper_amd_rows_enabled(st.ptr); st.free()
    assert name == "s256:q5_0" or without == 0, name
    monkeypatch.setenv(SWITCH, "1"); st = ctx.create_state()
    assert amd_lib.whisper_amd_rows_enabled(st.ptr) == (1 if name == "s256:q4_k" else without), name
    st.free()

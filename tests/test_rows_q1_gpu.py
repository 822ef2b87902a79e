"""The several-rows one-launch decode step for Q5_1 / Q4_1 models (wa_rows.hip: k_decode_rows_q1_np12 / 16 / 20; opt-in, WHISPER_AMD_ROWS_Q1=1 when a
state is made) against a state made with the switch unset: the launch sequence, which test_quant1_gpu.py pins to the reference engine.  Equality of
logits rows as uint32 words or of segment lists.  A pass the kernel sends back would pass any comparison, so where the test drives the passes (a - c)
`served` grows by exactly the passes expected and `back` by none; whisper_full decides its own passes (d): `served` has grown, `back` has not."""
import json
import os

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN
from test_quant1_gpu import CHAOS_LIB, _params, _segs
from test_rows_kernel_gpu import ALL_NKV, EDGES_REDUCED, _Served, _advance, _bits_equal, _chunks, _fits, _tok, ctxs  # noqa: F401  (ctxs: a fixture)

pytestmark = pytest.mark.gpu
MODELS = {"s128:q5_1": 8, "s128:q4_1": 8, "tiny:q5_1": 8, "small:q5_1": 8, "w1280:q5_1": 4}     # the row counts wa_rows_lds_bytes(quant = 2) admits on 256 workgroups
SWITCH = "WHISPER_AMD_ROWS_Q1"


def _states(ctx, lib, monkeypatch, n=1, seeds=None):
    """n launch-sequence states and n states made under the switch; state i of either list has heard the same 3 s of audio"""
    monkeypatch.delenv(SWITCH, raising=False); refs = [ctx.create_state() for _ in range(n)]
    monkeypatch.setenv(SWITCH, "1"); rows = [ctx.create_state() for _ in range(n)]; monkeypatch.delenv(SWITCH)
    assert all(lib.whisper_amd_rows_enabled(s.ptr) == 1 for s in rows), "the several-rows form is off under %s=1" % SWITCH
    assert all(lib.whisper_amd_rows_enabled(s.ptr) == 0 for s in refs)
    for i in range(n):
        for st in (refs[i], rows[i]):
            st.pcm_to_mel(wsynth.synth_audio(16000 * 3, seeds[i] if seeds else 5)); st.encode(0)
    return refs, rows


def _walk(ctx, ref, row, name, steps):
    """(n_kv, B) steps of B consecutive tokens at n_past = n_kv - B on both states: equal logits, and served exactly where rows_fits admits B"""
    count, cur = _Served(ctx, row), 0
    for n_kv, B in steps:
        n_past = n_kv - B
        _advance((ref, row), cur, n_past)           # (fewer cells wanted than there are: whisper_decode drops the cells from n_past on)
        toks = [_tok(p) for p in range(n_past, n_kv)]
        ref.decode(toks, n_past); row.decode(toks, n_past)
        assert row.kv_op(4) == n_kv and ref.kv_op(4) == n_kv and count.step(B) == (B <= MODELS[name])
        _bits_equal(ref.get_logits_last(B), row.get_logits_last(B), "%s, B %d, n_kv %d" % (name, B, n_kv))
        cur = n_kv
    count.check(name)
    ref.free(); row.free()


@pytest.mark.parametrize("name", list(MODELS))
def test_causal_batches_at_path_edges(wrs, amd_lib, ctxs, name, monkeypatch):
    """(a) 1..8 rows through whisper_decode on both sides of the self-attention edges; a row count not admitted is equal too and not counted"""
    ctx = ctxs(name)
    assert _fits(ctx) == list(range(1, MODELS[name] + 1)), name
    n_kvs = [129, 160] if name.startswith("w1280") else ([31, 32, 33] if name.startswith("s128") else []) + EDGES_REDUCED
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch)
    _walk(ctx, ref, row, name, [(n_kv, B) for n_kv in n_kvs for B in range(1, 9)])


@pytest.mark.parametrize("name", ["s128:q5_1", "small:q5_1"])
def test_single_tokens_walk(wrs, amd_lib, ctxs, name, monkeypatch):
    """(b) single tokens: the kernel with one row, at every width"""
    (ref,), (row,) = _states(ctxs(name), amd_lib, monkeypatch)
    _walk(ctxs(name), ref, row, name, [(n_kv, 1) for n_kv in ALL_NKV if n_kv <= 131])


def test_lockstep_rows_with_a_context_length_each(wrs, amd_lib, ctxs, monkeypatch):
    """(c) the lock-step shape: every row on its own state, with its own context length"""
    name, n_pasts = "s128:q5_1", [3, 31, 64, 127, 160, 255, 300, 447]
    ctx, n = ctxs(name), len(n_pasts)
    refs, rows = _states(ctx, amd_lib, monkeypatch, n=n, seeds=[5 + i for i in range(n)])
    toks, want, stats0 = [_tok(n_pasts[i]) + i for i in range(n)], [], [st.rows_stats() for st in rows]
    for i in range(n):          # the same cells in both states of a pair; the twin's single-token step by the launch sequence is the reference, made once
        s = 0
        for c in _chunks(max(n_pasts[i], 9)):
            for st in (refs[i], rows[i]):
                st.decode([_tok(p) + i for p in range(s, s + c)], s)
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
    for st in refs + rows:
        st.free()


@pytest.mark.parametrize("qt,build,tags", [("q5_1", "product", ("greedy", "ladder", "beam3")), ("q4_1", "product", ("greedy", "ladder", "beam3")), ("q5_1", "stalled", ("greedy",))])
def test_full_against_goldens(wrs, amd_lib, qt, build, tags, monkeypatch):
    """(d) whisper_full under the switch against the reference engine's goldens: greedy (the host overlap's window), the temperature ladder and beam 3;
    greedy once more on the build whose product waves stall at random"""
    import gen_golden_quant as g
    gold = json.load(open(os.path.join(GOLDEN, "s128_quant1.json")))[qt]
    lib = wrs.load_library(CHAOS_LIB) if build == "stalled" else amd_lib
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", qt), wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv(SWITCH, "1")
    for tag in tags:
        for aseed in (0, 1):
            st = ctx.create_state()
            assert lib.whisper_amd_rows_enabled(st.ptr) == 1
            st.full(_params(wrs, lib, g.FULL[tag]), wsynth.synth_audio(480000, aseed))
            assert _segs(st) == gold["full"]["%s_seed%d" % (tag, aseed)], (qt, tag, aseed)
            assert st.rows_stats()[0] > 0 and st.rows_stats()[1] == 0 and lib.whisper_amd_rows_enabled(st.ptr) == 1, (qt, tag, aseed, st.rows_stats())
            st.free()
    ctx.free()


def test_lockstep_group_equals_solo_and_is_served(wrs, amd_lib, monkeypatch):
    """(e) four s128:q5_1 chunks through whisper_amd_full_batch (a context of its own: the group's private state is made under the switch too)"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", "q5_1"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcms, fp, solo = [wsynth.synth_audio(480000, 50 + i) for i in range(4)], wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0), []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    monkeypatch.setenv(SWITCH, "1")
    states = [ctx.create_state() for _ in pcms]
    wrs.full_batch(ctx, states, fp, pcms)
    assert int(amd_lib.whisper_amd_batch_served(ctx.ptr)) > 0, "no pass of the group was delivered by the group"
    for i, st in enumerate(states):
        assert _segs(st) == solo[i], i
        st.free()
    ctx.free()

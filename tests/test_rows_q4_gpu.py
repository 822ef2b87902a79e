"""The several-rows one-launch decode step for Q4_0 models (wa_rows.hip: k_decode_rows_q4_np*; opt-in, WHISPER_AMD_ROWS_Q4=1 when a state is made) against
a state made with the switch unset: the launch sequence, which test_quant4_full_gpu.py pins to the reference engine.  Equality of logits rows as uint32
words or of segment lists, and counts of served passes: a pass the kernel sends back would pass any comparison."""
import hashlib
import json
import os

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN
from test_quant1_gpu import CHAOS_LIB, _params, _segs
from test_quant4_full_gpu import repack_order  # noqa: F401  (a fixture: WHISPER_AMD_REPACK_ORDER=1 for this module, the formats load only under it)
from test_rows_kernel_gpu import EDGES_REDUCED, _Served, _advance, _bits_equal, _chunks, _fits, _tok, ctxs  # noqa: F401  (ctxs: a fixture)

pytestmark = pytest.mark.gpu
# the row counts wa_rows_lds_bytes(quant = 5) admits on 256 workgroups (the nibble rows are half of Q5_0's bytes, so even at d = 1280
# eight operand rows, the exchange area and two slots that hold the eight rows of the second MLP product fit 160 KiB)
MODELS = {"s256:q4_0": 8, "tiny:q4_0": 8, "base:q4_0": 8, "w1280:q4_0": 8}
SWITCH = "WHISPER_AMD_ROWS_Q4"


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
    """(a) 1..8 rows through whisper_decode on both sides of the self-attention edges.  Blocks of a row, d-long / 4d-long: s256 8 / 32 (two active lanes; one
    full round), tiny 12 / 48 (a partial round that ends inside the lanes; a full round and a partial one), base 16 / 64 (two full rounds), w1280 40 / 160"""
    ctx = ctxs(name)
    assert _fits(ctx) == list(range(1, MODELS[name] + 1)), name
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch)
    count, cur = _Served(ctx, row), 0
    for n_kv in ([129, 160] if name.startswith("w1280") else EDGES_REDUCED):
        for B in range(1, 9):
            n_past = n_kv - B
            _advance((ref, row), cur, n_past)           # (fewer cells wanted than there are: whisper_decode drops the cells from n_past on)
            toks = [_tok(p) for p in range(n_past, n_kv)]
            ref.decode(toks, n_past); row.decode(toks, n_past)
            assert row.kv_op(4) == n_kv and ref.kv_op(4) == n_kv and count.step(B) == (B <= MODELS[name])
            _bits_equal(ref.get_logits_last(B), row.get_logits_last(B), "%s, B %d, n_kv %d" % (name, B, n_kv))
            cur = n_kv
    count.check(name); ref.free(); row.free()


def test_lockstep_rows_with_a_context_length_each(wrs, amd_lib, ctxs, monkeypatch):
    """(b) the lock-step shape: every row on its own state, with its own context length"""
    name, n_pasts = "s256:q4_0", [3, 31, 64, 127, 160, 255, 300, 447]
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
    gold = json.load(open(os.path.join(GOLDEN, "s256_quant4.json")))["q4_0"]
    lib = wrs.load_library(CHAOS_LIB) if build == "stalled" else amd_lib
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", "q4_0"), wrs.WhisperContextParameters(lib), lib=lib)
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
    """(d) four s256:q4_0 chunks through whisper_amd_full_batch (a context of its own: the group's private state is made under the switch too)"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", "q4_0"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcms, fp, solo = [wsynth.synth_audio(480000, 50 + i) for i in range(4)], wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0), []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    monkeypatch.setenv(SWITCH, "1"); states = [ctx.create_state() for _ in pcms]
    assert all(amd_lib.whisper_amd_rows_enabled(st.ptr) == 1 for st in states)
    wrs.full_batch(ctx, states, fp, pcms)
    assert int(amd_lib.whisper_amd_batch_served(ctx.ptr)) > 0, "no pass of the group was delivered by the group"
    assert [_segs(st) for st in states] == solo
    [st.free() for st in states]; ctx.free()


@pytest.mark.parametrize("name", ["s256:q4_k", "s256:q5_0", "s256:q4_0"])
def test_switch_leaves_other_formats_alone(wrs, amd_lib, ctxs, name, monkeypatch):
    """(e) the switch is Q4_0's alone: a Q4_K or a Q5_0 state made under it is what it is without it (Q4_K: the launch sequence); a Q4_0 state made without it
    keeps the launch sequence"""
    ctx = ctxs(name)
    monkeypatch.delenv(SWITCH, raising=False); st = ctx.create_state(); without = amd_lib.whisper_amd_rows_enabled(st.ptr); st.free()
    assert name == "s256:q5_0" or without == 0, name
    if name != "s256:q4_0":
        monkeypatch.setenv(SWITCH, "1"); st = ctx.create_state()
        assert amd_lib.whisper_amd_rows_enabled(st.ptr) == without, name
        st.free()

"""The several-rows one-launch decode step (wa_rows.hip: k_decode_rows_np12 / 16 / 20 and their quantised twins) against the launch sequence, bit
for bit on the logits of EVERY flagged row, at the context lengths, masks, row counts and logits selections at which the kernel changes its path.

The yardstick is a state created under WHISPER_AMD_NO_MEGA=1: it has neither one-launch form and runs the launch sequence, which the kernel tests and
the live-oracle tests pin.  Every step runs on such a state (`ref`) and on a state with the several-rows form (`row`).  A pass that the kernel sends
back is redone by the launch sequence and would pass any comparison, so every scenario also checks whisper_amd_rows_stats: `served` has grown by
exactly the passes the kernel is expected to take and `back` is 0.  (A legitimate WA_MEGA_REDO has probability ~1e-9 per soft-max; should a seed ever
hit one, change the audio seed and say so here - the assertion stays.)

Scenarios: (a) causal batches of 2..8 rows through whisper_decode with n_kv on both sides of every edge of mb_unit_self below n_text_ctx (P V steps of
32 cells, score blocks of 128, the four pre-loaded steps); (b) single tokens of a wide quantised model, which take this kernel with one row; (c) the
batches whisper_full builds - causal, beam search with a beam swap, rows that land in freed cells inside a P V chain - through
whisper_amd_decode_batch in a cache of 2560 cells, n_kv around 512 / 1024 / 2048 (second and third score trip, second soft-max trip, WA_ROWS_MAXKV)
with every logits selection (all rows, the last, two in the middle); (d) the lock-step shape - every row on its own state with its own context
length - through whisper_amd_rows_debug_rows; (e) reduced audio contexts in the cross-attention units.

In (c) the hidden cells stand under sequence id 17 and the cells that are freed again under 16: beams of 7 and 8 rows use the ids 6 and 7 themselves, and
the beam swap removes those ids from every cell, which would free the hidden block in the middle of the scenario."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

# model -> the row counts the kernel takes on 256 workgroups (wa_rows_lds_bytes: the weight slot of F16 d = 1280 shrinks with B and ends at 5 rows,
# Q5_0 d = 1280 at 6); whisper_amd_rows_fits must say the same, so that a changed rule shows itself
MODELS = {"small": 8, "s128": 8, "m1024": 8, "w1280": 5, "small:q5_0": 8, "s128:q8_0": 8, "w1280:q5_0": 6}
FULL = ("small", "s128:q8_0")       # these run the full edge lists, the others a reduced one
ROWS_MAXKV = 2048                   # WA_ROWS_MAXKV (wa_rows.h): longer contexts go to the launch sequence (wa_decode.cpp)
N_TEXT_CTX = 448
EDGES_FULL = [31, 32, 33, 127, 128, 129, 159, 160, 161, 255, 256, 257, 287, 288, 289, 383, 384, 385, 447, 448]
EDGES_REDUCED = [128, 129, 159, 160, 161]
NS_FULL = [511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049]
NS_REDUCED = [513, 514, 515, 2048]
# the context lengths of test_self_role_gpu.py (ALL_NKV)
ALL_NKV = list(range(4, 71)) + list(range(126, 132)) + list(range(190, 195)) + list(range(254, 259)) + list(range(445, 449))
KV_CELLS = 2560
V1, V2, HOLE_AT, HOLE_N = 64, 302, 80, 8
SEQ_HIDDEN, SEQ_HOLE = 17, 16


def _tok(pos):
    return 1000 + 37 * pos


def _chunks(n):
    """n >= 9 tokens in batches of 9..48: more than 8 rows is the launch sequence on both states"""
    assert n >= 9
    out = []
    while n > 0:
        t = min(48, n)
        if 0 < n - t < 9:
            t = n - 9
        out.append(t); n -= t
    return out


@pytest.fixture(scope="module")
def ctxs(wrs, amd_lib):
    """one context per model, made on first use"""
    made = {}

    def get(name):
        if name not in made:
            mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
            made[name] = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
        return made[name]
    yield get
    for c in made.values():
        c.free()


def _states(ctx, lib, monkeypatch, n=1, encode=True, seeds=None):
    """n launch-sequence states and n states with the several-rows form; state i of either list has heard the same 3 s of audio"""
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); refs = [ctx.create_state() for _ in range(n)]
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); rows = [ctx.create_state() for _ in range(n)]
    assert all(lib.whisper_amd_rows_enabled(s.ptr) == 0 for s in refs) and all(lib.whisper_amd_rows_enabled(s.ptr) == 1 for s in rows)
    if encode:
        for i in range(n):
            pcm = wsynth.synth_audio(16000 * 3, seeds[i] if seeds else 5)
            for st in (refs[i], rows[i]):
                st.pcm_to_mel(pcm); st.encode(0)
    return refs, rows


def _fits(ctx):
    return [B for B in range(1, 9) if ctx.amd_rows_fits(B) == 1]


def _bits_equal(want, got, what):
    """every row of `got` equals the row of `want` as uint32 words; the reference is finite"""
    want, got = np.atleast_2d(want), np.atleast_2d(got)
    assert want.shape == got.shape, what
    assert np.isfinite(want).all(), "%s: the launch sequence's logits are not finite" % what
    bad = np.nonzero((want.view(np.uint32) != got.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: logits row(s) %s differ from the launch sequence's (max |d| %g)" % (what, bad.tolist(), float(np.abs(want - got).max()))


def _advance(sts, cur, target):
    """cells [0, target) of the states hold the rule's tokens, given that cells [0, cur) do: whisper_decode batches of 9..48 tokens (a batch may
    start below `cur` or run past `target`; whisper_decode drops the cells from its n_past on, so the next step removes what it does not want)"""
    if target <= cur:
        return
    s = min(cur, max(0, target - 9))
    end = max(target, s + 9)
    assert end <= N_TEXT_CTX
    for n in _chunks(end - s):
        for st in sts:
            st.decode([_tok(p) for p in range(s, s + n)], s)
        s += n


class _Served:
    """the passes the kernel must have taken on `row` since this object was made: served grows by exactly that, nothing comes back"""

    def __init__(self, ctx, row):
        self.row, self.fits, self.expect = row, _fits(ctx), 0
        self.served0, self.back0 = row.rows_stats()

    def step(self, B, n_kv=None):
        """one pass of B rows has run on `row` (n_kv: the cells it attended over; default: what the cache says)"""
        n_kv = self.row.kv_op(4) if n_kv is None else n_kv
        taken = B in self.fits and n_kv <= ROWS_MAXKV
        self.expect += 1 if taken else 0
        return taken

    def check(self, what):
        served, back = self.row.rows_stats()
        assert back - self.back0 == 0, "%s: %d passes came back from the kernel and were redone by the launch sequence" % (what, back - self.back0)
        assert served - self.served0 == self.expect, "%s: the kernel served %d passes, expected %d" % (what, served - self.served0, self.expect)
        assert self.row.lib.whisper_amd_rows_enabled(self.row.ptr) == 1, "%s: the several-rows form gave up" % what


@pytest.mark.parametrize("name", list(MODELS))
def test_rows_fits_matches_the_table(ctxs, name):
    """the row counts the kernel takes, per model: the rule of wa_rows_lds_bytes on this device's workgroup count"""
    assert _fits(ctxs(name)) == list(range(1, MODELS[name] + 1)), name


# ---- a. causal batches through whisper_decode ----
@pytest.mark.parametrize("B", range(2, 9))
@pytest.mark.parametrize("name", list(MODELS))
def test_causal_batches_at_path_edges(wrs, amd_lib, ctxs, name, B, monkeypatch):
    """B consecutive tokens at n_past = n_kv - B for every n_kv of the edge list (and every n_kv from B + 3 to 40 for 2 and 8 rows on the models
    with the full list): the last row's logits.  A row count the kernel does not take gives the same logits and leaves both counters alone."""
    ctx = ctxs(name)
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch)
    n_kvs = EDGES_FULL if name in FULL else EDGES_REDUCED
    if name in FULL and B in (2, 8):
        n_kvs = sorted(set(n_kvs) | set(range(B + 3, 41)))
    count, cur = _Served(ctx, row), 0
    for n_kv in n_kvs:
        n_past = n_kv - B
        _advance((ref, row), cur, n_past)
        toks = [_tok(p) for p in range(n_past, n_kv)]
        ref.decode(toks, n_past); row.decode(toks, n_past)
        assert row.kv_op(4) == n_kv and ref.kv_op(4) == n_kv and row.kv_op(5) == n_past
        count.step(B)
        _bits_equal(ref.get_logits_last(B), row.get_logits_last(B), "%s, B %d, n_kv %d, row %d" % (name, B, n_kv, B - 1))
        cur = n_kv
    assert count.expect == (len(n_kvs) if B <= MODELS[name] else 0)
    count.check("%s, B %d" % (name, B))
    ref.free(); row.free()


# ---- b. single tokens of a wide quantised model: this kernel with one row ----
def test_single_tokens_of_wide_quantised_model_walk(wrs, amd_lib, ctxs, monkeypatch):
    name = "w1280:q5_0"
    ctx = ctxs(name)
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch)
    count, cur = _Served(ctx, row), 0
    for n_kv in ALL_NKV:
        n_past = n_kv - 1
        _advance((ref, row), cur, n_past)
        ref.decode([_tok(n_past)], n_past); row.decode([_tok(n_past)], n_past)
        assert row.kv_op(4) == n_kv
        assert count.step(1)
        _bits_equal(ref.get_logits_last(1), row.get_logits_last(1), "%s, B 1, n_kv %d, row 0" % (name, n_kv))
        served, back = row.rows_stats()
        assert (served - count.served0, back - count.back0) == (count.expect, 0), "%s, n_kv %d: the single token was not served by the several-rows kernel" % (name, n_kv)
        cur = n_kv
    count.check(name)
    ref.free(); row.free()


# ---- c. the batches whisper_full builds, in a cache for several decoders ----
def _batch(sts, toks, pos, seq, flags):
    return [st.decode_batch(toks, pos, seq, flags) for st in sts]


def _build_cache(sts, N):
    """Cells [0, N) of a cache of KV_CELLS cells, in this order: V1 visible cells of sequence 0 (positions 0..V1-1) | hidden cells (sequence
    SEQ_HIDDEN, positions that repeat: only the id hides them), among them HOLE_N cells of sequence SEQ_HOLE at HOLE_AT, inside the 32-cell P V chain
    step [64, 96) | V2 visible cells of sequence 0 that continue the positions.  With N > 512 + V2 every visible cell of the second block lies beyond
    cell 512."""
    hidden = N - V1 - V2
    assert hidden >= (HOLE_AT - V1) + HOLE_N + 9 and V1 + V2 + 3 + 9 <= N_TEXT_CTX
    for st in sts:
        st.kv_op(3, KV_CELLS)
        assert st.kv_op(6) == KV_CELLS and st.kv_op(5) == 0
    plan = [(list(range(p, p + n)), 0) for p, n in ((0, 48), (48, V1 - 48))]
    plan.append((list(range(HOLE_AT - V1)), SEQ_HIDDEN))
    plan.append((list(range(HOLE_N)), SEQ_HOLE))
    plan += [(list(range(n)), SEQ_HIDDEN) for n in _chunks(hidden - (HOLE_AT - V1) - HOLE_N)]
    p = V1
    for n in _chunks(V2):
        plan.append((list(range(p, p + n)), 0)); p += n
    for pos, seq in plan:
        n = len(pos)
        _batch(sts, [_tok(q) + seq for q in pos], pos, [seq] * n, [0] * (n - 1) + [1])
    for st in sts:
        assert st.kv_op(4) == N


def _flag_sets(B):
    sets = [("all", [1] * B)] if B <= 8 else []
    sets.append(("last", [0] * (B - 1) + [1]))
    if B >= 4:
        sets.append(("rows 1 and B-2", [1 if i in (1, B - 2) else 0 for i in range(B)]))
    return sets


@pytest.mark.parametrize("name,N", [(name, N) for name in MODELS for N in (NS_FULL if name in FULL else NS_REDUCED)])
def test_general_batches_in_a_cache_for_several_decoders(wrs, amd_lib, ctxs, name, N, monkeypatch):
    """n_kv = N for batches of 2..8 rows in three layouts: rows that land in freed cells inside a P V chain step (n_kv stays N), causal rows at the end
    of the cache, and three beam-search steps with a beam swap whose last one attends over N cells.  n_kv = 2049 and a batch of 9 rows go to the launch
    sequence by the host's own checks: equal logits, counters unchanged.  At N = 1025 two causal batches are also decoded one token at a time on a
    third launch-sequence state, over the same N cells."""
    ctx = ctxs(name)
    witness = N == 1025
    refs, (row,) = _states(ctx, amd_lib, monkeypatch, n=1)
    ref = refs[0]
    sts = [ref, row]
    if witness:
        monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); third = ctx.create_state()
        monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0")
        third.pcm_to_mel(wsynth.synth_audio(16000 * 3, 5)); third.encode(0)
        assert amd_lib.whisper_amd_rows_enabled(third.ptr) == 0
        sts.append(third)
    _build_cache(sts, N)
    count = _Served(ctx, row)
    tag = "%s, N %d" % (name, N)

    # rows that land in freed cells in the middle of the cache, inside a full 32-cell chain step; n_kv stays N
    for st in sts:
        st.kv_op(1, SEQ_HOLE)
        assert st.kv_op(5) == HOLE_AT, "the freed cells are not where the next batch is tried"
    P0 = V1 + V2
    for B in range(2, 9):
        toks, pos = [_tok(P0 + i) + 5 for i in range(B)], [P0 + i for i in range(B)]
        want, got = _batch((ref, row), toks, pos, [0] * B, [1] * B)
        assert row.kv_op(4) == N and row.kv_op(5) == HOLE_AT and ref.kv_op(5) == HOLE_AT
        count.step(B)
        _bits_equal(want, got, "%s, freed cells, B %d, n_kv %d" % (name, B, N))
        for st in sts:
            st.kv_op(1, 0, 0, P0, -1)
            assert st.kv_op(5) == HOLE_AT
    fill = list(range(HOLE_N))          # the freed cells are taken again, so that later batches go to the end of the cache
    _batch(sts, [_tok(q) + SEQ_HOLE for q in fill], fill, [SEQ_HOLE] * HOLE_N, [0] * (HOLE_N - 1) + [1])
    count.step(HOLE_N)
    assert row.kv_op(5) == HOLE_AT and row.kv_op(4) == N

    # causal batches and beam steps, in the order of shrinking second visible block (the cells above it are removed, never added)
    jobs = [("causal", B, V2 - B) for B in range(2, 9)] + [("beam", B, V2 - 3 * B) for B in range(2, 9)]
    if N == 2048:
        jobs.append(("causal", 9, V2 - 9))
    for layout, B, v2 in sorted(jobs, key=lambda j: -j[2]):
        P0 = V1 + v2
        for st in sts:
            st.kv_op(1, 0, 0, P0, -1)
            st.kv_op(2, 0, 0)           # (changes no cell: the search for free cells starts at cell 0 again, as after whisper_full's own copies)
        if layout == "causal":
            toks, pos = [_tok(P0 + i) + B for i in range(B)], [P0 + i for i in range(B)]
            rows_all = None
            for what, flags in _flag_sets(B):
                want, got = _batch((ref, row), toks, pos, [0] * B, flags)
                assert row.kv_op(4) == N and ref.kv_op(4) == N
                count.step(B)
                _bits_equal(want, got, "%s, causal, B %d, n_kv %d, logits of %s" % (name, B, N, what))
                if what == "all":
                    rows_all = got
                for st in (ref, row):
                    st.kv_op(1, 0, 0, P0, -1)
            if witness and B in (3, 8):
                # The third witness: the same tokens one at a time through the launch sequence.  The soft-max and the P V product take the cells in an
                # order that depends on n_kv (the n % 8 tail, the n % 32 leftover), in the reference too, so a token alone over fewer cells is a
                # different sum: a hidden cell at N - 1 keeps n_kv = N for every token but the last, which takes that cell itself.
                hide = [400 + i for i in range(B)]
                third.decode_batch([_tok(q) for q in hide], hide, [SEQ_HOLE] * B, [0] * (B - 1) + [1])
                assert third.kv_op(5) == N - B and third.kv_op(4) == N
                third.kv_op(1, SEQ_HOLE, 0, hide[0], hide[-1])
                one = []
                for i in range(B):
                    if i == B - 1:
                        third.kv_op(1, SEQ_HOLE, 0, hide[-1], -1)
                    one.append(third.decode_batch([toks[i]], [pos[i]], [0], [1])[0])
                    assert third.kv_op(4) == N and third.kv_op(5) == N - B + i
                _bits_equal(np.stack(one), rows_all, "%s, causal, B %d, n_kv %d, against one token at a time" % (name, B, N))
        else:
            for st in sts:
                for s in range(1, B):
                    st.kv_op(2, 0, s)
            for step in range(3):
                if step == 2:       # the beam swap of whisper_full: beam j goes on from beam src[j] - beam 1 is taken twice and beam 0 dropped, whose two
                    src = [max(j, 1) for j in range(B)]         # cells become free: single ones below the top, too short for the next batch
                    for st in sts:
                        for j in range(B):
                            st.kv_op(2, src[j], 8 + j)
                        for j in range(B):
                            st.kv_op(1, j); st.kv_op(2, 8 + j, j); st.kv_op(1, 8 + j)
                flags = [1] * B if step != 1 else _flag_sets(B)[-1][1]
                toks, pos, seq = [_tok(P0 + step) + j for j in range(B)], [P0 + step] * B, list(range(B))
                want, got = _batch((ref, row), toks, pos, seq, flags)
                n_kv = row.kv_op(4)
                assert n_kv == N - (2 - step) * B and ref.kv_op(4) == n_kv
                count.step(B)
                _bits_equal(want, got, "%s, beam step %d, B %d, n_kv %d, logits flags %s" % (name, step, B, n_kv, flags))
            for st in sts:
                for s in range(1, 16):
                    st.kv_op(1, s)
    if N > ROWS_MAXKV:      # only the first two beam steps, N - 2 B and N - B cells, are within the kernel's reach
        assert count.expect == 2 * len([B for B in range(2, 9) if B in count.fits]), tag
    count.check(tag)
    for st in sts:
        st.free()


# ---- d. the lock-step shape: every row on its own state, with its own context length ----
@pytest.mark.parametrize("name", list(MODELS))
def test_lockstep_rows_with_a_context_length_each(wrs, amd_lib, ctxs, name, monkeypatch):
    ctx = ctxs(name)
    n_pasts = [3, 64, 160, 300, 447] if name == "w1280" else [3, 31, 64, 127, 160, 255, 300, 447]
    n = len(n_pasts)
    refs, rows = _states(ctx, amd_lib, monkeypatch, n=n, seeds=[5 + i for i in range(n)])
    toks = [_tok(n_pasts[i]) + i for i in range(n)]
    want = []
    for i in range(n):          # the same cells in both states of a pair; the twin's single-token step by the launch sequence is the reference, made once
        s = 0
        for c in _chunks(max(n_pasts[i], 9)):
            for st in (refs[i], rows[i]):
                st.decode([_tok(p) + i for p in range(s, s + c)], s)
            s += c
        refs[i].decode([toks[i]], n_pasts[i])
        assert refs[i].kv_op(4) == n_pasts[i] + 1
        want.append(refs[i].get_logits_last(1).copy())
    want = np.stack(want)
    assert np.isfinite(want).all()
    stats0 = [st.rows_stats() for st in rows]
    for B in range(2, MODELS[name] + 1):
        for rot in range(n):    # every state meets every row index
            idx = [(rot + k) % n for k in range(B)]
            rc, got, status = wrs.rows_debug_rows(ctx, [rows[i] for i in idx], [toks[i] for i in idx], [n_pasts[i] for i in idx])
            what = "%s, B %d, rows of n_kv %s" % (name, B, [n_pasts[i] + 1 for i in idx])
            assert rc == 0, "%s: the kernel ended with status %d" % (what, rc)
            assert (status == 0).all(), "%s: row status %s (9000 = to be redone by the launch sequence)" % (what, status.tolist())
            _bits_equal(want[idx], got, what)
    if n > MODELS[name]:
        over = MODELS[name] + 1
        assert wrs.rows_debug_rows(ctx, rows[:over], toks[:over], n_pasts[:over])[0] == -2, "a row count the kernel does not take must be refused"
    assert wrs.rows_debug_rows(ctx, [rows[0], rows[0]], toks[:2], n_pasts[:2])[0] == -2, "the same state twice must be refused"
    assert [st.rows_stats() for st in rows] == stats0
    assert all(amd_lib.whisper_amd_rows_enabled(st.ptr) == 1 for st in rows)
    for st in refs + rows:
        st.free()


# ---- e. reduced audio contexts in the cross-attention units ----
@pytest.mark.parametrize("actx", [1, 7, 33, 50, 257])
@pytest.mark.parametrize("name", list(FULL))
def test_reduced_audio_contexts(wrs, amd_lib, ctxs, name, actx, monkeypatch):
    """T < 8, T < 32, T % 8 and T % 32 tails in mb_unit_cross: whisper_full encodes the reduced context, then batches of 3 and 8 rows"""
    ctx = ctxs(name)
    (ref,), (row,) = _states(ctx, amd_lib, monkeypatch, encode=False)
    pcm = wsynth.synth_audio(16000 * 3, 5)
    for st in (ref, row):
        st.full(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0, audio_ctx=actx, single_segment=True), pcm)
    count, n_past = _Served(ctx, row), 12
    for st in (ref, row):
        st.decode([_tok(p) for p in range(n_past)], 0)
    for B in (3, 8, 3, 8):
        toks = [_tok(p) for p in range(n_past, n_past + B)]
        ref.decode(toks, n_past); row.decode(toks, n_past)
        assert count.step(B)
        _bits_equal(ref.get_logits_last(B), row.get_logits_last(B), "%s, audio_ctx %d, B %d, n_kv %d, row %d" % (name, actx, B, n_past + B, B - 1))
        n_past += B
    count.check("%s, audio_ctx %d" % (name, actx))
    ref.free(); row.free()

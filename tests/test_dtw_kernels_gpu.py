"""The DTW alignment kernels (whisper-rust_amd/csrc/wa_dtw.hip: statistics over tokens, median + mean, the cost / trace table) against the host
function (wa_dtw_host.cpp, which tests/test_dtw_math.py holds to an independent restatement and the full() goldens hold to the reference
engine), through whisper_amd_dtw_path: where = 1 must give where = 0's path PAIR FOR PAIR.

Shapes: the small cases of the host test (M = 8, 9, 64, 65; N = 1, 2, 63, 64, 65; ties, zero variance, a rounding mean), a cube with +0 and
-0 after normalisation (fminf / fmaxf would order them, std::min / std::max do not), M = 750 and 1500, N = 200 and the largest N the capture
buffer takes (decoder rows - 3: the table kernel's upper threads), 1, 3 and 32 heads (32 only at a small n_tokens x M)."""
import numpy as np
import pytest

import dtw_cases
import wsynth

pytestmark = pytest.mark.gpu

SENTINEL = -77


@pytest.fixture(scope="module")
def state(wrs, amd_lib):
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    yield st
    st.free()
    ctx.free()


def dec_rows(state):
    return (state.ctx.n_text_ctx() + 63) // 64 * 64       # the state's decoder rows (dec_mpad): most tokens of a DTW pass


def both(state, c, width=7):
    h = state.dtw_path(c["cube"], c["M"], c["sot_len"], width, 0, fill=SENTINEL)
    d = state.dtw_path(c["cube"], c["M"], c["sot_len"], width, 1, fill=SENTINEL)
    return h, d


def assert_same_path(c, h, d):
    (hn, ht, hj), (dn, dt, dj) = h, d
    assert hn > 0 and hn <= c["N"] + c["M"], (c["name"], hn)
    assert dn == hn, (c["name"], dn, hn)
    assert np.array_equal(dt, ht) and np.array_equal(dj, hj), c["name"]
    assert (ht[0], hj[0]) == (0, 0) and (ht[hn - 1], hj[hn - 1]) == (c["N"] - 1, c["M"] - 1)
    assert (ht[hn:] == SENTINEL).all() and (dt[hn:] == SENTINEL).all()          # nothing behind the path


SMALL = dtw_cases.small_cases() + [dtw_cases.signed_zeros()]


@pytest.mark.parametrize("name", [c["name"] for c in SMALL])
def test_small_cases(state, name):
    c = next(c for c in SMALL if c["name"] == name)
    assert_same_path(c, *both(state, c))


def test_signed_zero_case_has_both_zeros():
    c = dtw_cases.signed_zeros()
    z = c["cube"][c["cube"] == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()


@pytest.mark.parametrize("n_heads,N,M,n_ctx", [(3, 200, 750, 1500), (1, 200, 1500, 1500), (32, 20, 40, 48), (32, 65, 130, 130)])
def test_real_widths(state, n_heads, N, M, n_ctx):
    c = dtw_cases.shaped("h%d_N%d_M%d" % (n_heads, N, M), 100 + n_heads + N + M, n_heads, N, M, n_ctx)
    assert_same_path(c, *both(state, c))


@pytest.mark.parametrize("n_heads,M", [(1, 1500), (3, 750)])
def test_largest_n_the_capture_buffer_takes(state, wrs, n_heads, M):
    """n_tokens == the state's decoder rows: N = rows - 3 with a two-token sot sequence (445 at the Whisper text context)"""
    rows = dec_rows(state)
    N = rows - 3
    c = dtw_cases.shaped("h%d_Nmax_M%d" % (n_heads, M), 7 + M, n_heads, N, M, M)
    assert c["cube"].shape[1] == rows
    assert_same_path(c, *both(state, c))
    # one token more does not fit the capture buffer: the device path does not take it, the host function does
    c1 = dtw_cases.shaped("over", 8, 1, N + 1, 64, 64)
    (hn, _, _), (dn, dt, dj) = both(state, c1)
    assert hn > 0 and dn == wrs.DTW_NOT_TAKEN
    assert (dt == SENTINEL).all() and (dj == SENTINEL).all()


def test_refused_arguments_same_code_nothing_written(state, wrs):
    cube = dtw_cases.shaped("r", 3, 1, 1, 8, 8)["cube"]          # 1 head, 4 tokens, 8 frames
    bad = [dict(M=8, sot_len=2, width=6), dict(M=8, sot_len=2, width=0), dict(M=7, sot_len=2, width=7), dict(M=8, sot_len=3, width=7),
           dict(M=9, sot_len=2, width=7), dict(M=8, sot_len=2, width=9), dict(M=8, sot_len=-1, width=7)]
    for b in bad:
        for where in (0, 1):
            n, t, j = state.dtw_path(cube, b["M"], b["sot_len"], b["width"], where, cap=16, fill=SENTINEL)
            assert n == wrs.DTW_REFUSED, (b, where, n)
            assert (t == SENTINEL).all() and (j == SENTINEL).all(), (b, where)
    n, t, j = state.dtw_path(cube, 8, 2, 7, 2, cap=16, fill=SENTINEL)           # no such `where`
    assert n == wrs.DTW_REFUSED and (t == SENTINEL).all()


def test_width_5_is_not_taken_by_the_device_path(state, wrs):
    c = dtw_cases.shaped("w5", 21, 3, 9, 17, 20)
    (hn, ht, _), (dn, dt, dj) = both(state, c, width=5)
    assert hn > 0 and (ht[:hn] >= 0).all()
    assert dn == wrs.DTW_NOT_TAKEN and (dt == SENTINEL).all() and (dj == SENTINEL).all()


def test_cap_limits_the_copy(state):
    c = SMALL[0]
    n, t, j = state.dtw_path(c["cube"], c["M"], c["sot_len"], 7, 1, cap=5, fill=SENTINEL)
    nf, tf, jf = state.dtw_path(c["cube"], c["M"], c["sot_len"], 7, 0, fill=SENTINEL)
    assert n == nf and n > 5 and np.array_equal(t, tf[:5]) and np.array_equal(j, jf[:5])


def test_stats_count_the_calls(state):
    c = SMALL[3]
    d0, h0, f0 = state.dtw_stats()
    both(state, c)
    both(state, c)
    d1, h1, f1 = state.dtw_stats()
    assert (d1 - d0, h1 - h0, f1 - f0) == (2, 2, 0)

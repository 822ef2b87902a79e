"""The Q8_K quantiser of the several-rows decode step's Q4_K form (wa_rows_q8k_dev.h: mk_quant_block<true, true>, launched in isolation by
tests/native/rows_q4k_quant.hip) against the host functions it restates, byte for byte on quants, d and bsums: wa_q8_K_row - the row rule, the sign of the
FIRST element of largest magnitude - and wa_q8_K_row4 - the four-row rule, negative scale when ANY element equals + max|x|.  The two differ only on a block
that holds - m and + m of equal largest magnitude; no audio produces one, so the decode tests cannot see it."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CASES = ["random", "minus_before_plus", "plus_before_minus", "zero_block", "tie_in_second_block_only"]


@pytest.fixture(scope="module")
def harness():
    return C.CDLL(os.path.join(ROOT, "tests", "native", "librows_q4k_quant.so"))


def _rows(case, nbk, rng):
    """four rows of nbk blocks; the case shapes the LAST block of each (the first, if there are two, stays random), at lanes and registers that differ by row"""
    x = rng.standard_normal((4, nbk, 256)).astype(np.float32)
    for r in range(4):
        b, m = x[r, nbk - 1], np.float32(8.0 + r)      # (beyond every standard normal value of the block)
        lo, hi = 5 + 67 * r, 40 + 70 * r            # lo < hi < 256: different registers (index // 64) and lanes (index % 64)
        if case == "minus_before_plus":
            b[lo], b[hi] = -m, m
        elif case == "plus_before_minus":
            b[lo], b[hi] = m, -m
        elif case == "zero_block":
            b[:] = 0.0
        elif case == "tie_in_second_block_only":
            b[lo], b[hi] = -m, m
            assert nbk == 2
    return x


@pytest.mark.parametrize("rule", [0, 1], ids=["row", "four_row"])
@pytest.mark.parametrize("case,nbk", [(c, 1) for c in CASES[:4]] + [(c, 2) for c in CASES])
def test_quantiser_equals_the_host_rule(harness, rule, case, nbk):
    x = _rows(case, nbk, np.random.default_rng(100 * nbk + CASES.index(case)))
    row4 = np.full(4, rule, np.int32)
    out = {}
    for who in ("dev", "host"):
        out[who] = (np.zeros((4, nbk * 256), np.int8), np.zeros((4, nbk), np.float32), np.zeros((4, nbk * 16), np.int16))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert harness.rows_q4k_quant(4, nbk, p(x), p(row4), *[p(a) for a in out["dev"]]) == 0
    harness.rows_q4k_quant_host(4, nbk, p(x), p(row4), *[p(a) for a in out["host"]])
    for what, dev, host in zip(("quants", "d", "bsums"), out["dev"], out["host"]):
        assert dev.tobytes() == host.tobytes(), "%s differ (%s rule, %s, %d blocks): rows %s" % (
            what, "four-row" if rule else "row", case, nbk, np.nonzero((dev != host).any(axis=1))[0].tolist())
    if case in ("minus_before_plus", "tie_in_second_block_only"):      # the case is what it claims: here the two rules give opposite signs
        assert (out["host"][1][:, nbk - 1] < 0).all() if rule else (out["host"][1][:, nbk - 1] > 0).all()

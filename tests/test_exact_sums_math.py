"""CPU side of the certified-sum tests: the rows of tests/golden/exact_sums_rows.npz really do what tests/test_exact_sums_gpu.py
relies on.  Nothing here searches: every precondition (tools/adversarial_rows.py: check_row / check_softmax_row) is re-verified from
the committed fixture, the stored expected bits are recomputed, and the numpy LayerNorm the expectations come from is held against
liboracle's on ordinary rows and on the fixture's.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import adversarial_rows as AR  # noqa: E402

ROWS = AR.load()
SM_ROWS = AR.load_softmax()


def test_fixture_holds_every_family_at_every_width():
    have = {(r["kind"], r["path"], r["d"]) for r in ROWS}
    for d in AR.DIMS:
        for kind, path in (("exact", "mean_inorder_zero"), ("exact", "var_up"), ("exact", "var_down"), ("searched", "mean_second"),
                           ("searched", "mean_inorder_up"), ("searched", "mean_inorder_down"), ("searched", "var_up"), ("searched", "var_down")):
            assert (kind, path, d) in have
    for d in AR.BLOCK_DIMS:
        for path in ("mean_inorder_zero", "var_up", "var_down"):
            assert ("exact", path, d) in have
        for path in ("mean_second", "mean_inorder_up", "mean_inorder_down", "var_up", "var_down"):
            assert ("searched", path, d) in have
    assert {(r["n_kv"], r["ref_is_hi"]) for r in SM_ROWS} == {(n, hi) for _, n in AR.SM_CASES for hi in (True, False)}


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_layernorm_row_preconditions(row):
    """The certificate fails at four orders, the row takes the intended level, and the expected output differs in F32 and in F16 from
    what every wrong candidate would give; the stored expected bits are the plain reference's and liboracle's."""
    info = AR.check_row(row)
    assert info["lo"] < info["hi"]
    y = AR.layernorm_ref(row["x"], row["w"], row["b"])
    assert np.array_equal(AR.bits32(y), row["y32"]) and np.array_equal(AR.bits16(y), row["y16"])
    assert np.array_equal(AR.bits32(AR.layernorm_oracle(row["x"], row["w"], row["b"])), row["y32"])


@pytest.mark.parametrize("row", SM_ROWS, ids=[r["name"] for r in SM_ROWS])
def test_softmax_row_preconditions(row):
    info = AR.check_softmax_row(row)
    assert info["ref_is_hi"] == row["ref_is_hi"]
    p, p16 = AR.softmax_expected(row)
    assert np.array_equal(AR.bits32(p), row["p32"]) and np.array_equal(p16, row["p16"])


@pytest.mark.parametrize("d", AR.DIMS + AR.BLOCK_DIMS + (8, 100))
def test_numpy_layernorm_equals_liboracle(d):
    """Ordinary rows (Gaussian, offset, tiny, large) through the numpy reference and through liboracle's layernorm_row: same bits."""
    rng = np.random.default_rng(d)
    w = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    for scale, shift in ((1.0, 0.0), (1.0, 3.0), (1e-4, 0.0), (300.0, -1000.0), (0.02, 1e-3)):
        x = (scale * rng.standard_normal(d) + shift).astype(np.float32)
        assert np.array_equal(AR.bits32(AR.layernorm_ref(x, w, b)), AR.bits32(AR.layernorm_oracle(x, w, b)))


def test_certificate_holds_on_ordinary_rows():
    """The restated certificate is not vacuous: on Gaussian rows with a mean away from zero it holds, and its value is the reference's."""
    rng = np.random.default_rng(5)
    held = 0
    for _ in range(50):
        x = (rng.standard_normal(384) + 0.5).astype(np.float32)
        lo, hi, _ = AR.sum_bounds(AR.seq_sum(x[::-1]), AR.seq_sum(np.abs(x)), x.size)
        if lo == hi:
            held += 1
            assert lo == np.float32(AR.seq_sum(x) / x.size)
    assert held >= 45


@pytest.mark.parametrize("d", AR.MODEL_DIMS)
def test_model_rows_preconditions(d):
    """The rows a model variant feeds to layer 0's LayerNorm hold their preconditions under the ONE gamma / beta they share, and the
    large gamma leaves every row's output finite in F16."""
    rows, w, b = AR.load_model_rows(d)
    assert [r["path"] for r in rows] == list(AR.MODEL_PATHS)
    for r in rows:
        AR.check_row(r)
        assert np.array_equal(AR.bits32(AR.layernorm_ref(r["x"], w, b)), AR.bits32(AR.layernorm_oracle(r["x"], w, b)))

"""CPU side of the kernel-by-kernel tests of wa_quant.hip: the cases of tools/quant_cases.py really tell a wrong kernel from a right
one.  tests/native/libquant_ref.so states the arithmetic (variant 0, pinned to the reference library by test_host_reference_equals_
reference_library) and, beside it, deliberately wrong restatements: hsum_float_8 in linear order, the fmaf of the lane chains as a
multiplication and an addition, the minimum chain fused or without its first block; a quantiser that rounds ties away from zero, takes
id = 1 / d, or forms s from the rounded d or in float.  For every group of cases - kernel family x loop class x format family - each
wrong variant must change at least one expected output bit: a kernel that computed that instead would fail tests/test_quant_kernels_gpu.py.
Also: the pack / unpack of the kernel layout, and the numpy quantiser of tests/test_exact_sums_gpu.py against this one.  No GPU."""
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quant_cases as QC  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")


def test_host_reference_equals_reference_library(tmp_path):
    """Variant 0 of quant_ref.cpp - the Q5_0 / Q8_0 product and the quantiser - against ggml_vec_dot_q5_0_q8_0, ggml_vec_dot_q8_0_q8_0 and
    quantize_row_q8_0 of the reference library, bit for bit (tests/native/quant_ref_pin.cpp; the Q4_1 / Q5_1 side is test_quant1_math.py's)."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "quant_ref_pin")
    # no -mfma and contraction off: a * b + c is two roundings, fmaf one, as in the library's build
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "quant_ref_pin.cpp"),
                           "-I", os.path.join(ROOT, "whisper-rust_amd", "csrc"), "-o", exe, "-ldl"])
    out = subprocess.run([exe, REF_LIB], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "quant_ref: 0 mismatches" in out.stdout, out.stdout[-4000:]


# ----------------------------------------------------------------------------------------------------------------------------
# the groups
# ----------------------------------------------------------------------------------------------------------------------------
def _product_groups(kernel, cases):
    groups = {}
    for c in cases:
        groups.setdefault((kernel, QC.loop_class(c["nb"]), QC.family(c["fmt"])), []).append(c)
    return groups


PRODUCT_GROUPS = {**_product_groups("one-row product", QC.GEMV_CASES), **_product_groups("8-row product", QC.GEMM_CASES + QC.GEMM_BIG_CASES)}
GELU_GROUPS = _product_groups("fused GELU product", QC.GELU_CASES)


def test_every_group_exists():
    for kernel in ("one-row product", "8-row product"):
        for loop in ("pipelined", "block-by-block"):
            for fam in ("Q0", "Q1"):
                assert PRODUCT_GROUPS[(kernel, loop, fam)]
    assert set(GELU_GROUPS) == {("fused GELU product", loop, fam) for loop in ("pipelined", "block-by-block") for fam in ("Q0", "Q1")}
    # every kind of activation row in every group of the plain products
    for g, cases in PRODUCT_GROUPS.items():
        assert {c["kind"] for c in cases} == set(QC.ACT_KINDS), g
    assert {b for c in QC.GELU_CASES for b in QC.gelu_block_kinds(c)} == set(QC.GELU_BLOCK_KINDS)
    for g, cases in GELU_GROUPS.items():
        assert {b for c in cases for b in QC.gelu_block_kinds(c)} == set(QC.GELU_BLOCK_KINDS), g


def _changed(a, b):
    return int(np.count_nonzero(~QC.same_bits(a, b)))


PRODUCT_ASKS = [(g, v) for g in PRODUCT_GROUPS for v in QC.DOT_VARIANTS if g[2] == "Q1" or v not in QC.DOT_VARIANTS_Q1_ONLY]


@pytest.mark.parametrize("group,variant", PRODUCT_ASKS, ids=["%s, %s, %s: %s" % (g + (v,)) for g, v in PRODUCT_ASKS])
def test_product_cases_discriminate(group, variant):
    changed = total = 0
    for c in PRODUCT_GROUPS[group]:
        w, x = QC.product_operands(c)
        want = QC.ref_gemm(w, x)
        changed += _changed(want, QC.ref_gemm(w, x, QC.DOT_VARIANTS[variant]))
        total += want.size
    print("%s: %d of %d outputs change" % (variant, changed, total))
    assert changed > 0, "%s changes %d of %d expected outputs of %s" % (variant, changed, total, group)


@pytest.mark.parametrize("fmt", sorted(QC.FORMATS))
def test_hsum_order_shows_with_one_block(fmt):
    """nb = 1: every lane holds one rounded product, so only the order of hsum_float_8 can go wrong.  The operands of one block share one
    scale (there is nothing else to spread); the eight lane sums still differ enough for the order to show."""
    changed = total = 0
    for c in QC.GEMV_CASES + QC.GEMM_CASES:
        if c["nb"] == 1 and c["fmt"] == fmt:
            w, x = QC.product_operands(c)
            want = QC.ref_gemm(w, x)
            changed += _changed(want, QC.ref_gemm(w, x, QC.DOT_VARIANTS["hsum in linear order"]))
            total += want.size
    print("%d of %d outputs change" % (changed, total))
    assert total > 0 and changed > 0, "hsum in linear order changes %d of %d outputs at nb = 1" % (changed, total)


def _has_tie(kinds):
    return any(k in QC.TIE_KINDS for row in kinds for k in row)


@pytest.mark.parametrize("variant", list(QC.Q_VARIANTS))
def test_quantiser_cases_discriminate(variant):
    changed = total = 0
    for c in QC.QUANT_CASES:
        X, kinds = QC.quant_rows(c)
        if variant == "ties away from zero" and not _has_tie(kinds):
            continue
        want, got = QC.ref_quantize(X), QC.ref_quantize(X, QC.Q_VARIANTS[variant])
        changed += int(np.count_nonzero(want[0] != got[0])) + _changed(want[1], got[1]) + _changed(want[2], got[2])
        total += want[0].size + want[1].size + want[2].size
    print("%s: %d of %d outputs change" % (variant, changed, total))
    assert total > 0 and changed > 0, "%s changes %d of %d expected outputs of the quantiser" % (variant, changed, total)


def test_every_quantiser_case_holds_a_tie_block():
    for c in QC.QUANT_CASES:
        assert _has_tie(QC.quant_rows(c)[1]), c["name"]
    assert {k for c in QC.QUANT_CASES for row in QC.quant_rows(c)[1] for k in row} == set(QC.QUANT_BLOCK_KINDS)


def test_tie_blocks_sit_on_ties():
    """The built tie block: with the right inverse scale every value but the maximum lands on k + 0.5 exactly."""
    blk = QC.tie_block(QC.rng_for("tie"))
    t = (blk * (np.float32(127) / np.abs(blk).max())).astype(np.float32)
    assert np.all(np.abs(t[1:]) % 1 == 0.5) and np.rint(abs(t[0])) == 127


GELU_ASKS = ([(g, "dot", v) for g in GELU_GROUPS for v in QC.DOT_VARIANTS if g[2] == "Q1" or v not in QC.DOT_VARIANTS_Q1_ONLY] +
             [(g, "q", v) for g in GELU_GROUPS for v in QC.Q_VARIANTS if g[2] == "Q1" or v not in QC.Q_VARIANTS_S_ONLY])


@pytest.mark.parametrize("group,what,variant", GELU_ASKS, ids=["%s, %s, %s: %s" % (g + (v,)) for g, _, v in GELU_ASKS])
def test_fused_gelu_cases_discriminate(group, what, variant):
    """The outputs are quants and block scales (and block sums with a minimum): a product one ulp off must still move one of them."""
    changed = total = 0
    for c in GELU_GROUPS[group]:
        if variant == "ties away from zero" and "tie" not in QC.gelu_block_kinds(c):
            continue
        _, q0, d0, s0 = QC.gelu_expected(c)
        _, q1, d1, s1 = QC.gelu_expected(c, QC.DOT_VARIANTS[variant], 0) if what == "dot" else QC.gelu_expected(c, 0, QC.Q_VARIANTS[variant])
        changed += int(np.count_nonzero(q0 != q1)) + _changed(d0, d1)
        total += q0.size + d0.size
        if group[2] == "Q1":
            changed += _changed(s0, s1)
            total += s0.size
    print("%s: %d of %d outputs change" % (variant, changed, total))
    assert total > 0 and changed > 0, "%s changes %d of %d expected outputs of %s" % (variant, changed, total, group)


@pytest.mark.parametrize("c", QC.GELU_CASES, ids=[c["name"] for c in QC.GELU_CASES])
def test_fused_gelu_blocks_are_what_they_claim(c):
    w, x, bias, kinds = QC.gelu_operands(c)
    v = QC.ref_gemm(w, x)[0] + bias
    g, q, d, s = QC.gelu_expected(c)
    for b, kind in enumerate(kinds):
        sl = slice(32 * b, 32 * b + 32)
        if kind == "zero":
            assert np.all(v[sl] <= -10) and np.any(v[sl] == -10) and np.all(g[sl] == 0) and d[0, b] == 0 and np.all(q[0, sl] == 0)
        elif kind == "big":
            assert np.any(v[sl] >= 10) and np.any(np.abs(v[sl]) < 10)
        else:
            t = (g[sl] * (np.float32(127) / g[sl].max())).astype(np.float32)
            assert np.all(v[sl] >= 10) and np.count_nonzero(t % 1 == 0.5) == 31


# ----------------------------------------------------------------------------------------------------------------------------
# layouts and the other numpy quantiser
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(1, 32), (3, 96), (5, 160), (2, 3072)])
def test_pack_unpack_round_trip(rows, K):
    q = np.random.default_rng(K).integers(-128, 128, size=(rows, K)).astype(np.int8)
    p = QC.pack_qs(q)
    assert p.shape == (rows, 8, K // 32, 4) and np.array_equal(QC.unpack_qs(p), q)
    # element e of block b of row r lies at qs[r][e / 4][b][e % 4] (wa_device.h: wa_q8_store)
    for r, b, e in ((0, 0, 0), (rows - 1, K // 32 - 1, 31), (0, K // 64, 13)):
        assert p[r, e // 4, b, e % 4] == q[r, 32 * b + e]
    assert np.array_equal(QC.pack_qs(QC.unpack_qs(p)), p)


def test_numpy_quantiser_of_the_exact_sums_test_agrees():
    """q8_rows of tests/test_exact_sums_gpu.py (the expectation of the LayerNorm -> Q8 kernels there) against libquant_ref.so on the
    quantiser rows, rounding points included."""
    spec = importlib.util.spec_from_file_location("_exact_sums_gpu", os.path.join(ROOT, "tests", "test_exact_sums_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for c in QC.QUANT_CASES:
        X, _ = QC.quant_rows(c)
        with np.errstate(over="ignore", invalid="ignore"):
            qs, qd, qsum = mod.q8_rows(np.array(X))
        q, d, s = QC.ref_quantize(X)
        assert np.array_equal(qs, QC.pack_qs(q)), c["name"]
        assert QC.same_bits(qd, d).all() and QC.same_bits(qsum, s).all(), c["name"]

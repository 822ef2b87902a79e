#!/usr/bin/env python3
"""Rows built to take the fallbacks of the certified F64 sums (wa_device.h: wa_sum_bounds / wa_mean_indifferent / wa_seq_sum_lds).

A reference-order kernel sums a LayerNorm row in whatever order is fast and accepts the result when (S -+ delta)/n rounds to
one float; otherwise it falls back (second-level certificate for a mean, then one lane sums in index order).  Random rows take
the variance fallback about once per 10^5 rows, so this generator BUILDS rows that take it, and states on the CPU why they do.

The reference evaluated here is a plain one: F64 sums in index order by a Python loop, float32 for every other step of
ops.cpp:3225-3242 and for the tail y = ((x - mean) * scale) * w + b, one rounding per operation.

Two families, for d in DIMS (the elements-per-lane dispatch edges of k_layernorm_exact plus the smallest model width):

  exact     every value lies on a dyadic grid, so every F64 partial sum is exact in ANY order: the expected result does not
            depend on the order at all, and the certificate must fail because the quotient itself is undecidable:
              mean      +-pairs and two zeros: S = 0 exactly, lo < 0 < hi, and the zeros defeat the second level (0 - lo != 0 - hi)
              variance  integer t with sum t^2 = d q, q a 25-bit odd integer: S/d is an exact tie between two floats.  One row
                        whose tie rounds (to even) to the upper neighbour, one to the lower.
  searched  a Gaussian row in which a handful of elements at graded magnitudes are bisected over their float bit patterns
            until the in-order quotient lies within delta/8 of a float rounding boundary, on a chosen side of it.
            These rows rest on the ACTUAL order-to-order deviation of an F64 sum being far below the worst-case delta (it is
            checked at four orders here, not proven for the kernel's own order).  The exact rows rest on nothing.

Every row carries preconditions that check_row() asserts on the CPU (conditions, not measurements):
  * the certificate fails: the kernel's formula (wa_device.h:247-254, restated in sum_bounds) gives lo != hi at the in-order sum
    and at three other orders (reversed, pairwise tree, stride 64); searched rows also have |q - boundary| <= delta/8;
  * the path is the intended one: the second level fails for the in-order mean rows and passes for the second-level ones;
  * the case discriminates: the expected output differs, in F32 and in F16, from the output computed with every candidate
    (lo, hi) that is not the reference's value - what a fallback that keeps a certificate bound would leave behind.  Gamma and
    beta are free inputs: a variance row has one w[i] placed so that y[i] straddles an F16 rounding boundary between the two
    candidate scales; an in-order mean row has a large w at the element that equals a candidate.  A second-level row cannot
    discriminate by construction (every mean in [lo, hi] gives the same output); it is there to run that level on its own.

`python tools/adversarial_rows.py` searches (seconds) and prints what it found; `--write` stores it as tests/golden/exact_sums_rows.npz.
The tests load that fixture and re-verify the preconditions; they never search.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "exact_sums_rows.npz")
DIMS = (128, 384, 768, 1024, 1280)
BLOCK_DIMS = (1536,)        # wider than one wave per row takes (64 x 20), so a several-row product normalises them block-wide, one after the other
EPS = np.float32(1e-5)
PATHS = ("mean_second", "mean_inorder_zero", "mean_inorder_up", "mean_inorder_down", "var_up", "var_down")
f32 = np.float32


# ---------------------------------------------------------------------------------------------------
# the reference, and the kernel's certificate restated
# ---------------------------------------------------------------------------------------------------
def seq_sum(values):
    """F64 sum in index order (ops.cpp:3225-3228)."""
    s = 0.0
    for v in np.asarray(values, dtype=np.float64).tolist():
        s += v
    return s


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def order_sums(values):
    """The F64 sum in four orders: index order, reversed, a pairwise tree, 64 strided partial sums."""
    v = np.asarray(values, dtype=np.float64).tolist()
    return [seq_sum(v), seq_sum(v[::-1]), _pairwise(v), seq_sum([seq_sum(v[l::64]) for l in range(64)])]


def sum_bounds(S, A, n):
    """wa_sum_bounds: (lo, hi, delta) of the quotient S / n; the certificate holds when lo == hi."""
    rn = 1.0 / float(n)
    delta = (2.0 * float(n) * 2.0 ** -53 * A + abs(S) * 2.0 ** -48) * rn * 1.000001
    q = S * rn
    return f32(q - delta), f32(q + delta), delta


def mean_indifferent(x, lo, hi):
    """wa_mean_indifferent over the row: every x - lo == x - hi in float32."""
    return bool(np.all((x - f32(lo)) == (x - f32(hi))))


def squares(x, mean):
    t = x - f32(mean)
    return (t * t).astype(np.float32)


def layernorm_ref(x, w, b, eps=EPS, mean=None, var=None):
    """The reference LayerNorm of one row in float32 with in-order F64 sums; `mean` / `var` replace the statistic when given."""
    x = np.asarray(x, dtype=np.float32)
    d = x.size
    if mean is None:
        mean = f32(seq_sum(x) / d)
    mean = f32(mean)
    t = x - mean
    if var is None:
        var = f32(seq_sum(squares(x, mean)) / d)
    var = f32(var)
    scale = f32(1.0) / np.sqrt(f32(var + f32(eps)))
    y = (t * scale).astype(np.float32)
    y = (y * np.asarray(w, dtype=np.float32)).astype(np.float32)
    return (y + np.asarray(b, dtype=np.float32)).astype(np.float32)


def scale_of(var, eps=EPS):
    return f32(1.0) / np.sqrt(f32(f32(var) + f32(eps)))


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits16(a):
    return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


def base_affine(d):
    """Ordinary gamma / beta of width d (the rows override single elements)."""
    rng = np.random.default_rng(7000 + d)
    w = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    return w, b


def _up(v):
    return np.nextafter(f32(v), f32(np.inf))


def _boundary_above(q):
    """The float rounding boundary (midpoint of two neighbouring floats, exact in F64) just above q > 0, and the two floats."""
    lo = f32(q)
    if float(lo) > q:
        lo = np.nextafter(lo, f32(-np.inf))
    while True:
        hi = _up(lo)
        B = (float(lo) + float(hi)) / 2.0
        if B > q:
            return B, lo, hi
        lo = hi


# ---------------------------------------------------------------------------------------------------
# exact rows
# ---------------------------------------------------------------------------------------------------
def exact_mean_row(d, seed=0):
    rng = np.random.default_rng(1000 * d + seed)
    m = rng.integers(1, 2048, size=d // 2 - 1).astype(np.float32) / f32(256.0)       # grid 2^-8, |x| < 8: sums and squares exact
    x = np.concatenate([m, -m, np.zeros(2, np.float32)])
    x = x[rng.permutation(d)]
    w, b = base_affine(d)
    lo, hi, delta = sum_bounds(0.0, float(np.sum(np.abs(x), dtype=np.float64)), d)
    sc = scale_of(f32(seq_sum(squares(x, 0.0)) / d))
    ov = {}
    for i in np.flatnonzero(x == 0):          # y = (0 - candidate) * scale * w: make it a normal F16 number for either candidate
        ov[int(i)] = (f32(2.0 ** np.round(np.log2(2.0 ** -4 / (delta * float(sc))))), f32(0.0))
    return dict(kind="exact", path="mean_inorder_zero", d=d, x=x, override=ov)


def exact_var_row(d, up, seed=0):
    """x = +-2m pairs, sum of m^2 over pairs = (d / 8) q, q odd with 25 bits: mean(x^2) = q exactly.  q % 4 == 3 rounds up."""
    for attempt in range(200):
        rng = np.random.default_rng(2000 * d + 10 * seed + attempt)
        m = np.clip(np.abs(rng.normal(0.0, 2500.0, size=d // 2 - 2)).astype(np.int64), 1, 4095)
        r0 = int(np.sum(m * m))
        u = d // 8
        a = np.arange(1, 4096, dtype=np.int64)
        q = -(-(r0 + 2) // u)
        while q % 4 != (3 if up else 1):
            q += 1
        found = None
        for _ in range(4000):
            rem = u * q - r0
            if rem > 2 * 4095 * 4095 or q >= 2 ** 25:
                break
            b2 = rem - a * a
            bb = np.sqrt(np.maximum(b2, 0).astype(np.float64)).astype(np.int64)
            ok = (b2 >= 1) & (bb * bb == b2) & (bb <= 4095)
            if q >= 2 ** 24 and ok.any() and scale_of(f32(q - 1)) != scale_of(f32(q + 1)):
                i = int(np.flatnonzero(ok)[0])
                found = (int(a[i]), int(bb[i]))
                break
            q += 4
        if found is None:
            continue
        m = np.concatenate([m, np.array(found, dtype=np.int64)])
        x = np.concatenate([2 * m, -2 * m]).astype(np.float32)
        x = x[rng.permutation(d)]
        row = dict(kind="exact", path="var_up" if up else "var_down", d=d, x=x, override={})
        if _place_var_override(row, f32(q - 1), f32(q + 1)):
            return row
    raise RuntimeError("no exact variance row for d = %d" % d)


def _place_var_override(row, var_lo, var_hi, avoid=()):
    """One w[i] (b[i] = 0) such that y[i] rounds to different F16 values for the two candidate scales."""
    x = row["x"]
    mean = f32(seq_sum(x) / x.size)
    t = x - mean
    s_lo, s_hi = scale_of(var_lo), scale_of(var_hi)
    if s_lo == s_hi:
        return False
    u_lo, u_hi = (t * s_lo).astype(np.float32), (t * s_hi).astype(np.float32)
    cand = [int(i) for i in np.argsort(-np.abs(t)) if u_lo[i] != u_hi[i] and int(i) not in avoid][:16]
    step = np.arange(-64, 65)
    for i in cand:
        for k in range(1, 40):
            B = 1.0 + (2 * k + 1) * 2.0 ** -11          # an F16 rounding boundary in (1, 2)
            w0 = f32(B / float(u_lo[i]))
            ws = (w0.view(np.int32) + step).astype(np.int32).view(np.float32)
            y_lo = (u_lo[i] * ws).astype(np.float32).astype(np.float16)
            y_hi = (u_hi[i] * ws).astype(np.float32).astype(np.float16)
            hit = np.flatnonzero(y_lo != y_hi)
            if hit.size:
                row["override"] = {i: (f32(ws[hit[0]]), f32(0.0))}
                return True
    return False


# ---------------------------------------------------------------------------------------------------
# searched rows
# ---------------------------------------------------------------------------------------------------
LEVELS = (1.0, 2.0 ** -5, 2.0 ** -10, 2.0 ** -14, 2.0 ** -18, 2.0 ** -22, 2.0 ** -26)


def _steer(x, idx, f, up, tol):
    """Bisect the controls idx[0], idx[1], ... over their bit patterns until f(x) lies within tol of zero on the wanted side (up: f > 0,
    else f < 0; never on it, where the quotient would be a tie).  A control is an element i (a positive float; f grows with it) or a
    pair (p, m): x[p] moves up by patterns and x[m] down by the same amount, which keeps the row's sum - and so its mean - where it is.
    Between levels the control stays on the last pattern before the crossing."""
    def crossed(v):
        return v > 0 if up else v >= 0
    xi = x.view(np.int32)
    for c in idx:
        p, m = c if isinstance(c, tuple) else (c, None)
        pair_sum = None if m is None else float(x[p]) + float(x[m])

        def put(bits):
            xi[p] = bits
            if m is not None:
                x[m] = f32(pair_sum - float(x[p]))
            return f(x)
        if crossed(f(x)):
            return False
        b0, step = int(xi[p]), 1
        while not crossed(put(b0 + step)):
            step *= 2
            if step > 1 << 22:
                return False
        lo_b, hi_b = b0 + step // 2, b0 + step
        while hi_b - lo_b > 1:
            mid = (lo_b + hi_b) // 2
            if crossed(put(mid)):
                hi_b = mid
            else:
                lo_b = mid
        f_hi = put(hi_b)
        f_lo = put(lo_b)
        if up and 0 < f_hi <= tol:
            put(hi_b)
            return True
        if not up and -tol <= f_lo < 0:
            return True
    return False


def searched_var_row(d, up, seed0=0, pin=None, avoid=()):
    """pin: an element kept 2^-10 above the mean (the model variants put a large gamma there); avoid: indices the override may not take."""
    for seed in range(seed0, seed0 + 40):
        rng = np.random.default_rng(3000 * d + seed)
        x = rng.standard_normal(d).astype(np.float32)
        pick = [int(i) for i in rng.choice(d, size=2 * len(LEVELS), replace=False)]
        if pin in pick:
            continue
        idx = list(zip(pick[0::2], pick[1::2]))
        for _ in range(4):                             # (placing them moves the mean: settle)
            mean0 = f32(seq_sum(x) / d)
            for (p, m), lv in zip(idx, LEVELS):         # t = +-lv around the mean: the sum of squares grows as the pair moves apart
                x[p], x[m] = mean0 + f32(lv), mean0 - f32(lv)
            if pin is not None:
                x[pin] = mean0 + f32(2.0 ** -10)
        mean0 = f32(seq_sum(x) / d)
        if np.any(x[[p for p, _ in idx]] <= 0):
            continue
        q0 = seq_sum(squares(x, f32(seq_sum(x) / d))) / d
        B, v_lo, v_hi = _boundary_above(q0)
        if scale_of(v_lo) == scale_of(v_hi):
            continue

        def f(xx):
            return seq_sum(squares(xx, f32(seq_sum(xx) / d))) / d - B
        s2 = seq_sum(squares(x, mean0))
        tol = sum_bounds(s2, s2, d)[2] / 8.0
        if not _steer(x, idx, f, up, tol):
            continue
        row = dict(kind="searched", path="var_up" if up else "var_down", d=d, x=x, override={}, boundary=B)
        if not _place_var_override(row, v_lo, v_hi, avoid=tuple(avoid) + ((pin,) if pin is not None else ())):
            continue
        try:
            check_row(row)
        except AssertionError:
            continue
        return row
    raise RuntimeError("no searched variance row for d = %d" % d)


def _nearest_boundary(q):
    f = f32(q)
    n = np.nextafter(f, f32(np.inf) if q >= float(f) else f32(-np.inf))
    return (float(f) + float(n)) / 2.0


def second_level_row(d, seed0=0, pin=None):
    """A Gaussian row whose sum one element cancels down to its own rounding error: the mean is so small that floats lie closer together
    there than delta (the spacing is asserted <= delta/4, so a boundary lies within delta/8 of ANY sum: the first level fails at every
    order), and no element is anywhere near it, so the second level passes."""
    for seed in range(seed0, seed0 + 60):
        rng = np.random.default_rng(4000 * d + seed)
        x = rng.standard_normal(d).astype(np.float32)
        x[np.abs(x) < 2.0 ** -6] = f32(0.75)
        if pin is not None:
            x[pin] = f32(2.0 ** -12)                    # (small enough for a gamma of 2^20 there, far enough from the mean for the second level)
        k = int(np.argmax(np.abs(x)))
        x[k] = f32(0.0)
        x[k] = f32(-seq_sum(x))
        q = seq_sum(x) / d
        lo, hi, delta = sum_bounds(seq_sum(x), seq_sum(np.abs(x)), d)
        if q == 0.0 or float(_up(abs(q))) - float(f32(abs(q))) > delta / 4.0:
            continue
        row = dict(kind="searched", path="mean_second", d=d, x=x, override={}, boundary=_nearest_boundary(q))
        try:
            check_row(row)
        except AssertionError:
            continue
        return row
    raise RuntimeError("no second-level row for d = %d" % d)


def searched_mean_row(d, path, seed0=0, pin=None):
    """path: mean_inorder_up / mean_inorder_down: the quotient just beyond a boundary, and one element (pin, when given) equal to the lo
    candidate, so the second level fails."""
    up = not path.endswith("down")
    for seed in range(seed0, seed0 + 60):
        rng = np.random.default_rng(4000 * d + seed + (500 if up else 900))
        x = rng.standard_normal(d).astype(np.float32)
        x += f32(0.25)                                  # a mean well away from zero: the boundary is one of a float of ordinary size
        idx = [int(i) for i in rng.choice(d, size=len(LEVELS) + 1, replace=False)]
        j, idx = idx[0], idx[1:]
        if pin is not None:
            if pin in idx:
                continue
            j = pin
        for i, m in zip(idx, LEVELS):
            x[i] = f32(1.5 * m)
        x[j] = _boundary_above(seq_sum(x) / d)[1]
        B, v_lo, v_hi = _boundary_above(seq_sum(x) / d)
        x[j] = v_lo
        if B <= seq_sum(x) / d:
            continue
        override = {j: (f32(2.0 ** 20), f32(0.0))}          # (lo - mean) * scale * w: 0 for one candidate, about 2^-7 for the other

        def f(xx):
            return seq_sum(xx) / d - B
        tol = sum_bounds(seq_sum(x), seq_sum(np.abs(x)), d)[2] / 8.0
        if not _steer(x, idx, f, up, tol):
            continue
        row = dict(kind="searched", path=path, d=d, x=x, override=override, boundary=B)
        try:
            check_row(row)
        except AssertionError:
            continue
        return row
    raise RuntimeError("no searched %s row for d = %d" % (path, d))


# ---------------------------------------------------------------------------------------------------
# rows for a whole model: one gamma / beta for all of them
# ---------------------------------------------------------------------------------------------------
# Layer 0's first LayerNorm of the decoder reads te[token] + pe[position], so with a zero token-embedding row the positional embedding IS
# the row, and attn_ln's gamma / beta are the free inputs - but one pair for every position.  So these rows share their overrides: the
# large gamma sits at one index (MODEL_PIN) for all of them, where the in-order mean rows hold their lo candidate and the other rows an
# element close to their mean; each variance row has its own tuned gamma at an index of its own.  Searched rows only (an exact mean row
# would need 2^38 there).
MODEL_DIMS = (128, 384, 768, 1280)                  # s128, tiny, small, w1280
MODEL_PATHS = ("mean_second", "mean_inorder_up", "mean_inorder_down", "var_up", "var_down")
MODEL_PIN = 7


def model_rows(d):
    """(rows in MODEL_PATHS order, w, b): every row passes check_row under the shared gamma / beta."""
    for seed0 in range(0, 1000, 100):
        try:
            rows = [second_level_row(d, seed0, pin=MODEL_PIN), searched_mean_row(d, "mean_inorder_up", seed0, pin=MODEL_PIN),
                    searched_mean_row(d, "mean_inorder_down", seed0, pin=MODEL_PIN)]
            rows.append(searched_var_row(d, True, seed0, pin=MODEL_PIN))
            rows.append(searched_var_row(d, False, seed0 + 50, pin=MODEL_PIN, avoid=tuple(rows[-1]["override"])))
            w, b = base_affine(d)
            w[MODEL_PIN], b[MODEL_PIN] = f32(2.0 ** 20), f32(0.0)
            for r in rows[3:]:
                for i, (wi, bi) in r["override"].items():
                    w[i], b[i] = wi, bi
            for r in rows:
                r["w"], r["b"] = w, b
                check_row(r)
            return rows, w, b
        except (AssertionError, RuntimeError):
            continue
    raise RuntimeError("no model rows for d = %d" % d)


# ---------------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------------
def affine_of(row):
    if "w" in row:                                  # a row of the fixture brings its gamma / beta along
        return row["w"].copy(), row["b"].copy()
    w, b = base_affine(row["d"])
    for i, (wi, bi) in row["override"].items():
        w[i], b[i] = wi, bi
    return w, b


def _differs(y_ref, y_c):
    return bool(np.any(bits32(y_ref) != bits32(y_c))) and bool(np.any(bits16(y_ref) != bits16(y_c)))


def check_row(row):
    """Assert the row's preconditions (module docstring); returns a summary dict of what it established."""
    x, d, path = row["x"], row["d"], row["path"]
    assert x.dtype == np.float32 and x.size == d and np.all(np.isfinite(x))
    w, b = affine_of(row)
    y_ref = layernorm_ref(x, w, b)
    assert np.all(np.isfinite(y_ref.astype(np.float16))), "the expected output overflows F16"
    A = seq_sum(np.abs(x))
    mean_ref = f32(seq_sum(x) / d)
    out = dict(path=path, kind=row["kind"], d=d)
    if path.startswith("mean"):
        cands = set()
        for S in order_sums(x):
            lo, hi, delta = sum_bounds(S, A, d)
            assert lo != hi, "the mean certificate holds at one order"
            if row["kind"] == "searched":
                assert abs(S / d - row["boundary"]) <= delta                      # every order inside the undecided band of the same boundary
            second = mean_indifferent(x, lo, hi)
            assert second == (path == "mean_second"), "second level: %s" % second
            cands.add((float(lo), float(hi)))
        assert len(cands) == 1, "the orders disagree on the candidates"
        lo, hi = cands.pop()
        assert f32(lo) <= mean_ref <= f32(hi)
        if row["kind"] == "searched":
            assert abs(seq_sum(x) / d - row["boundary"]) <= sum_bounds(seq_sum(x), A, d)[2] / 8.0
            if path != "mean_second":
                assert mean_ref == f32(hi if path.endswith("up") else lo)
        out.update(lo=lo, hi=hi, ref=float(mean_ref))
        wrong = [c for c in (lo, hi) if f32(c) != mean_ref]
        if path == "mean_second":
            for c in (lo, hi):
                assert np.array_equal(bits32(layernorm_ref(x, w, b, mean=c)), bits32(y_ref))
        else:
            assert wrong
            for c in wrong:
                assert _differs(y_ref, layernorm_ref(x, w, b, mean=c)), "a wrong mean would go unnoticed"
        # the variance of these rows is decided by whatever mean was taken; nothing is required of its certificate
    else:
        # the mean first: any path to it must give the reference's t = x - mean
        for S in order_sums(x):
            lo, hi, _ = sum_bounds(S, A, d)
            assert (lo == hi == mean_ref) or mean_indifferent(x, lo, hi), "the mean of a variance row needs the in-order sum"
            assert np.array_equal(x - lo, x - mean_ref)
        sq = squares(x, mean_ref)
        var_ref = f32(seq_sum(sq) / d)
        cands = set()
        for S in order_sums(sq):
            lo, hi, delta = sum_bounds(S, S, d)
            assert lo != hi, "the variance certificate holds at one order"
            if row["kind"] == "searched":
                assert abs(S / d - row["boundary"]) <= delta          # every order inside the undecided band, around the same boundary
            cands.add((float(lo), float(hi)))
        assert len(cands) == 1
        lo, hi = cands.pop()
        if row["kind"] == "searched":
            assert abs(seq_sum(sq) / d - row["boundary"]) <= sum_bounds(seq_sum(sq), seq_sum(sq), d)[2] / 8.0
        else:
            assert seq_sum(sq) / d == (lo + hi) / 2.0 and len(set(order_sums(sq))) == 1, "not an exact tie"
        assert var_ref == f32(hi if path == "var_up" else lo), "rounds the other way"
        assert scale_of(lo) != scale_of(hi)
        out.update(lo=lo, hi=hi, ref=float(var_ref))
        wrong = hi if path == "var_down" else lo
        assert _differs(y_ref, layernorm_ref(x, w, b, var=wrong)), "a wrong variance would go unnoticed"
    if row["kind"] == "exact" and path.startswith("mean"):
        assert len(set(order_sums(x))) == 1 and seq_sum(x) == 0.0 and lo < 0 < hi
        for c in (lo, hi):
            assert _differs(y_ref, layernorm_ref(x, w, b, mean=c))
    return out


# ---------------------------------------------------------------------------------------------------
# soft-max rows
# ---------------------------------------------------------------------------------------------------
# The query is one-hot in one head dimension (q[0] = 1), so the score of key c is float(float(k_c) * 1) * scale: one free F16 value per
# key.  n_kv % 8 == 7: the seven tail cells enter the F64 sum one by one (vec.cpp:301-305) and are the fine controls, placed about
# 12, 17, 21.5, 26, ... below the maximum and chosen, coarse to fine, among the F16 values around those places until the sum lies
# within delta/8 of the S whose inverse is a float rounding boundary (delta as the kernels compute it: 2 (n_kv/8 + 8) 2^-53 S).
# The exponentials come from liboracle (wo_softmax_row: the oracle's own soft-max row); nothing restates expf here.
SM_SCALE = f32(0.35355338)
SM_OFFSETS = (12.0, 17.0, 21.5, 26.0, 30.5, 35.0, 39.5)
SM_CASES = (("attn1", 63), ("attn4_combine", 519), ("attn_mq", 63), ("attn_mfma", 135))     # the kernel a row is run through, its n_kv
_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        import ctypes as C
        L = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
        L.wo_softmax_row.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wo_softmax_row.restype = None
        L.wo_layernorm_row.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.wo_layernorm_row.restype = None
        _ORACLE = L
    return _ORACLE


def softmax_oracle(x):
    """liboracle's soft-max row of the (already scaled) scores x: exponentials, F64 sum, inverse, probabilities."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    e, y = np.empty_like(x), np.empty_like(x)
    S, inv = np.zeros(1, np.float64), np.zeros(1, np.float32)
    oracle().wo_softmax_row(x.size, x.ctypes.data, e.ctypes.data, S.ctypes.data, inv.ctypes.data, y.ctypes.data)
    return e, float(S[0]), f32(inv[0]), y


def layernorm_oracle(x, w, b, eps=EPS):
    x, w, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, w, b))
    y = np.empty_like(x)
    oracle().wo_layernorm_row(x.size, x.ctypes.data, w.ctypes.data, b.ctypes.data, float(eps), y.ctypes.data)
    return y


def sm_scores(k16, q0=1.0):
    """Scores of a one-hot query with q[0] = q0 against keys whose element 0 is k16 (F16 bit patterns)."""
    k = np.asarray(k16, dtype=np.uint16).view(np.float16).astype(np.float32)
    return ((k * f32(q0)).astype(np.float32) * SM_SCALE).astype(np.float32)


def sm_terms(e):
    """The addends of the reference's F64 sum: one F32 group sum per 8 exponentials (vec.cpp:278-299), then the tail cells."""
    n8 = e.size & ~7
    v = e[:n8].reshape(-1, 8)
    g = ((v[:, 0] + v[:, 4]) + (v[:, 2] + v[:, 6])) + ((v[:, 1] + v[:, 5]) + (v[:, 3] + v[:, 7]))
    return np.concatenate([g.astype(np.float64), e[n8:].astype(np.float64)])


def sm_bounds(S, n_kv):
    """The kernels' certificate of a soft-max denominator: (ilo, ihi, delta)."""
    delta = 2.0 * float((n_kv >> 3) + 8) * 2.0 ** -53 * S * 1.000001
    return f32(1.0 / (S + delta)), f32(1.0 / (S - delta)), delta


def softmax_row(n_kv, want_hi, seed0=0, tries=4000):
    """Key values (F16 bits, element 0 of every key) whose soft-max row fails the certificate, with the reference's inverse equal to
    ihi (want_hi) or ilo, and with at least one probability whose F16 rounding tells the two candidates apart."""
    from fractions import Fraction
    assert n_kv % 8 == 7
    n8 = n_kv & ~7
    for seed in range(seed0, seed0 + tries):
        rng = np.random.default_rng(50000 * n_kv + seed)
        kf = np.clip(2.0 * rng.standard_normal(n_kv), -7.5, 7.5).astype(np.float16)
        kf[int(rng.integers(0, n8))] = np.float16(8.0)                           # the maximum, unique
        mx = float(sm_scores(np.array([np.float16(8.0)]).view(np.uint16))[0])
        for t, off in enumerate(SM_OFFSETS):
            kf[n8 + t] = np.float16((mx - off) / float(SM_SCALE))
        k16 = kf.view(np.uint16).copy()
        _, S0, _, _ = softmax_oracle(sm_scores(k16))
        lo = f32(1.0 / S0)
        nb = np.nextafter(lo, f32(np.inf) if 1.0 / S0 >= float(lo) else f32(-np.inf))
        B = (Fraction(float(lo)) + Fraction(float(nb))) / 2                          # the boundary of 1/S nearest to where the row starts
        SB = 1 / B
        ok = False
        for t in range(len(SM_OFFSETS)):                                             # coarse to fine: the F16 values within +-1.2 of the place
            c = n8 + t
            base = int(k16[c])
            best = None
            for pat in range(base - 160, base + 161):
                kv = float(np.array([pat], dtype=np.uint16).view(np.float16)[0])
                if not (kv < 0) or abs(kv * float(SM_SCALE) - (mx - SM_OFFSETS[t])) > 1.2:
                    continue
                k16[c] = pat
                _, S, _, _ = softmax_oracle(sm_scores(k16))
                miss = abs(Fraction(S) - SB)
                if best is None or miss < best[0]:
                    best = (miss, pat, S)
            k16[c] = best[1]
            if best[0] <= Fraction(sm_bounds(best[2], n_kv)[2]) / 8 and Fraction(best[2]) != SB:
                ok = True
                break
        if not ok:
            continue
        row = dict(n_kv=n_kv, k16=k16.copy(), boundary=float(B))
        try:
            info = check_softmax_row(row)
        except AssertionError:
            continue
        if info["ref_is_hi"] == want_hi:
            return row
    raise RuntimeError("no soft-max row for n_kv = %d (want_hi = %s)" % (n_kv, want_hi))


def softmax_expected(row, inv=None):
    """(p F32, p F16 bits) of the row; `inv` replaces the reference's inverse when given."""
    e, S, inv_ref, y = softmax_oracle(sm_scores(row["k16"]))
    if inv is None:
        return y, y.astype(np.float16).view(np.uint16)
    p = (e * f32(inv)).astype(np.float32)
    return p, p.astype(np.float16).view(np.uint16)


def check_softmax_row(row):
    """Assert the preconditions of a soft-max row: the certificate fails at the in-order sum and at three other orders, the sum lies
    within delta/8 of the S whose inverse is the float rounding boundary, and the expected probabilities differ from those of the
    other candidate in F32 and in F16."""
    from fractions import Fraction
    n_kv, k16 = row["n_kv"], row["k16"]
    e, S, inv, y = softmax_oracle(sm_scores(k16))
    terms = sm_terms(e)
    assert seq_sum(terms) == S, "the addends restated here are not the oracle's"
    assert inv == f32(1.0 / S) and np.array_equal(y, (e * inv).astype(np.float32))
    cands = set()
    for So in order_sums(terms):
        ilo, ihi, delta = sm_bounds(So, n_kv)
        assert ilo != ihi, "the soft-max certificate holds at one order"
        cands.add((float(ilo), float(ihi)))
    assert len(cands) == 1
    ilo, ihi = cands.pop()
    assert float(np.nextafter(f32(ilo), f32(np.inf))) == ihi and (ilo + ihi) / 2.0 == row["boundary"]
    assert abs(Fraction(S) - 1 / Fraction(row["boundary"])) <= Fraction(sm_bounds(S, n_kv)[2]) / 8
    assert float(inv) in (ilo, ihi)
    wrong = ilo if float(inv) == ihi else ihi
    p_w, p16_w = softmax_expected(row, inv=wrong)
    p16 = y.astype(np.float16).view(np.uint16)
    assert np.any(bits32(y) != bits32(p_w)), "a wrong inverse would go unnoticed in F32"
    cells = np.flatnonzero(p16 != p16_w)
    assert cells.size, "a wrong inverse would go unnoticed in F16"
    return dict(ilo=ilo, ihi=ihi, ref_is_hi=float(inv) == ihi, cells16=cells)


# ---------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------
def row_name(row):
    return "%s_%s_d%d" % (row["kind"], row["path"], row["d"])


def generate(dims=DIMS, log=None):
    rows = []
    for d in dims:
        made = [exact_mean_row(d), exact_var_row(d, True), exact_var_row(d, False),
                second_level_row(d), searched_mean_row(d, "mean_inorder_up"), searched_mean_row(d, "mean_inorder_down"),
                searched_var_row(d, True), searched_var_row(d, False)]
        for r in made:
            info = check_row(r)
            if log:
                log("%-34s lo %.9g hi %.9g ref %.9g override %s" % (row_name(r), info["lo"], info["hi"], info["ref"],
                                                                     {k: float(v[0]) for k, v in r["override"].items()}))
        rows += made
    for d in BLOCK_DIMS:
        made = [exact_mean_row(d), exact_var_row(d, True), exact_var_row(d, False), second_level_row(d), searched_mean_row(d, "mean_inorder_up"),
                searched_mean_row(d, "mean_inorder_down"), searched_var_row(d, True), searched_var_row(d, False)]
        for r in made:
            info = check_row(r)
            if log:
                log("%-34s lo %.9g hi %.9g ref %.9g" % (row_name(r), info["lo"], info["hi"], info["ref"]))
        rows += made
    return rows


def generate_softmax(log=None):
    rows = []
    for n_kv in sorted({n for _, n in SM_CASES}):
        for want_hi in (True, False):
            r = softmax_row(n_kv, want_hi)
            r["name"] = "sm_%d_%s" % (n_kv, "hi" if want_hi else "lo")
            info = check_softmax_row(r)
            if log:
                log("%-34s ilo %.9g ihi %.9g reference takes %s; F16 differs at cells %s" % (r["name"], info["ilo"], info["ihi"],
                                                                                          "ihi" if info["ref_is_hi"] else "ilo", info["cells16"].tolist()))
            rows.append(r)
    return rows


def save(rows, path=FIXTURE, sm_rows=(), models=()):
    z = {}
    for d, (mrows, w, b) in models:
        z["mdl_d%d/x" % d] = np.stack([r["x"] for r in mrows])
        z["mdl_d%d/boundary" % d] = np.array([r["boundary"] for r in mrows], dtype=np.float64)
        z["mdl_d%d/w" % d], z["mdl_d%d/b" % d] = w, b
    for r in sm_rows:
        p, p16 = softmax_expected(r)
        z[r["name"] + "/k16"] = r["k16"]
        z[r["name"] + "/boundary"] = np.array([r["boundary"]], dtype=np.float64)
        z[r["name"] + "/p32"] = bits32(p)
        z[r["name"] + "/p16"] = p16
    for r in rows:
        n = row_name(r)
        w, b = affine_of(r)
        y = layernorm_ref(r["x"], w, b)
        z[n + "/x"] = r["x"]
        z[n + "/ov_i"] = np.array(sorted(r["override"]), dtype=np.int32)
        z[n + "/ov_w"] = np.array([r["override"][i][0] for i in sorted(r["override"])], dtype=np.float32)
        z[n + "/ov_b"] = np.array([r["override"][i][1] for i in sorted(r["override"])], dtype=np.float32)
        z[n + "/boundary"] = np.array([r.get("boundary", 0.0)], dtype=np.float64)
        z[n + "/y32"] = bits32(y)
        z[n + "/y16"] = bits16(y)
    for d in sorted({r["d"] for r in rows}):
        z["affine_d%d/w" % d], z["affine_d%d/b" % d] = base_affine(d)
    np.savez_compressed(path, **z)


def load(path=FIXTURE):
    """The committed rows: a list of dicts as the generator makes them, plus the stored expected bits (y32, y16) and affine (w, b)."""
    z = np.load(path)
    rows = []
    for n in sorted({k.split("/")[0] for k in z.files if not k.startswith(("affine", "sm_", "mdl_"))}):
        kind, rest = n.split("_", 1)
        path_, d = rest.rsplit("_d", 1)
        d = int(d)
        ov = {int(i): (f32(wi), f32(bi)) for i, wi, bi in zip(z[n + "/ov_i"], z[n + "/ov_w"], z[n + "/ov_b"])}
        w, b = z["affine_d%d/w" % d].copy(), z["affine_d%d/b" % d].copy()
        for i, (wi, bi) in ov.items():
            w[i], b[i] = wi, bi
        rows.append(dict(name=n, kind=kind, path=path_, d=d, x=z[n + "/x"], override=ov, boundary=float(z[n + "/boundary"][0]),
                         y32=z[n + "/y32"], y16=z[n + "/y16"], w=w, b=b))
    return rows


def load_softmax(path=FIXTURE):
    """The committed soft-max rows: name, n_kv, k16 (F16 bits of element 0 of every key), boundary, expected p32 / p16 bits."""
    z = np.load(path)
    rows = []
    for n in sorted({k.split("/")[0] for k in z.files if k.startswith("sm_")}):
        rows.append(dict(name=n, n_kv=int(n.split("_")[1]), ref_is_hi=n.endswith("_hi"), k16=z[n + "/k16"], boundary=float(z[n + "/boundary"][0]),
                         p32=z[n + "/p32"], p16=z[n + "/p16"]))
    return rows


def load_model_rows(d, path=FIXTURE):
    """The rows of the model variant of width d, in MODEL_PATHS order, with the gamma / beta they share."""
    z = np.load(path)
    w, b = z["mdl_d%d/w" % d], z["mdl_d%d/b" % d]
    return [dict(name="model_%s_d%d" % (p, d), kind="searched", path=p, d=d, x=x, override={}, boundary=float(B), w=w, b=b)
            for p, x, B in zip(MODEL_PATHS, z["mdl_d%d/x" % d], z["mdl_d%d/boundary" % d])], w, b


def main(argv):
    rows = generate(log=print)
    sm_rows = generate_softmax(log=print)
    models = [(d, model_rows(d)) for d in MODEL_DIMS]
    print("%d LayerNorm rows, %d soft-max rows, model rows at d = %s" % (len(rows), len(sm_rows), list(MODEL_DIMS)))
    if "--write" in argv:
        save(rows, sm_rows=sm_rows, models=models)
        print("wrote %s (%d bytes)" % (FIXTURE, os.path.getsize(FIXTURE)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

"""Logits rows for the tests of the alignment scores (tests/test_align_math.py on the host restatement, tests/test_align_kernels_gpu.py on
k_align_score) and their yardstick: numpy float64 with math.fsum for the sum.  No device, no library.

A case is (name, logits [n_rows][n_vocab] F32, target [n_rows] int32)."""
import math

import numpy as np

N_VOCABS = [1, 3, 4, 5, 255, 256, 257, 1023, 51865, 51866]
N_ROWS = [1, 2, 3]
KINDS = ["random", "equal", "tie", "target_best", "target_last", "spike", "with_ninf", "ninf_target"]


def make_row(kind, n, rng):
    """one row and its target"""
    x = rng.normal(0.0, 3.0, n).astype(np.float32)
    t = int(rng.integers(0, n))
    if kind == "equal":
        x[:] = np.float32(1.25)
    elif kind == "tie":                         # the maximum at two indices: the lowest wins
        hi = np.float32(x.max() + np.float32(2.0))
        a, b = (0, 0) if n == 1 else sorted(int(v) for v in rng.choice(n, 2, replace=False))
        x[a] = x[b] = hi
        t = b                                   # the target is the LATER of the two: rank 1 (0 for n == 1)
    elif kind == "target_best":
        t = int(np.argmax(x))
    elif kind == "target_last":
        t = n - 1
    elif kind == "spike":                       # one logit 1e4 above the rest: the others' plog is x_t - mx exactly
        k = int(rng.integers(0, n))
        x[k] = np.float32(x.max() + np.float32(1.0e4))
        t = (k + 1) % n
    elif kind == "with_ninf":
        x[rng.random(n) < 0.3] = -np.inf
        if n > 1:
            x[(t + 1) % n] = -np.inf
        x[t] = np.float32(0.5)
    elif kind == "ninf_target":
        x[t] = -np.inf
        if n == 1:
            pass                                # the only logit: an all -inf row
    return x, t


def cases(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in N_VOCABS:
        for r in N_ROWS:
            # the big vocabularies take every kind once, spread over the row counts; the small ones take every kind at every row count
            kinds = KINDS if n < 50000 else KINDS[(r - 1) * 3:(r - 1) * 3 + 3] + (["random"] if r == 3 else [])
            for k0 in range(0, len(kinds)):
                rows = [make_row(kinds[(k0 + i) % len(kinds)], n, rng) for i in range(r)]
                out.append(("v%d_r%d_%s" % (n, r, kinds[k0]), np.stack([x for x, _ in rows]), np.array([t for _, t in rows], np.int32)))
    return out


def expected(logits, target):
    """float64 yardstick: per row (plog, p, best_id, best_plog, best_p, rank), the three scores as float64 values"""
    out = []
    for x, t in zip(np.asarray(logits, np.float32), target):
        xd = x.astype(np.float64)
        mx = xd.max()
        best = int(np.argmax(xd))               # numpy: the first index of the maximum
        # lse - mx = log1p(the sum over every index but `best`): the cancellation-free form of the definition, so that the yardstick keeps
        # its float64 relative precision where p -> 1 and plog -> -0
        l1p = math.log1p(math.fsum(math.exp(v - mx) for i, v in enumerate(xd) if i != best and v != -math.inf)) if mx != -math.inf else 0.0

        def lp(v):
            return (-math.inf, 0.0) if v == -math.inf else ((v - mx) - l1p, math.exp((v - mx) - l1p))
        idx = np.arange(len(xd))
        rank = int(np.sum((xd > xd[t]) | ((xd == xd[t]) & (idx < t))))
        out.append(lp(xd[t]) + (best,) + lp(mx) + (rank,))
    return out


def ulps32(got, want64):
    """distance in F32 units in the last place between a float32 result and the float64 value rounded to F32 (0 for equal infinities)"""
    g, w = np.float32(got), np.float32(want64)
    if np.isinf(g) or np.isinf(w) or np.isnan(g) or np.isnan(w):
        return 0 if (g == w) else 1 << 30

    def key(v):
        i = int(np.array(v, np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(g) - key(w))

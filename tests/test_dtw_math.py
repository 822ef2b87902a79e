"""DTW token timestamps, host part (whisper-rust_amd/csrc/wa_dtw_host.cpp compiled alone by g++: no HIP, no device).

tests/native/dtw_math.cpp runs the product's host function - normalise over tokens, 7-wide median over audio with reflect padding, mean
over heads times -1, the DTW table with its tie rule, the backtrace - on a strided view of each cube of tools/dtw_cases.py.  The yardstick
is an independent restatement below: numpy float32 / float64 scalars, explicit loops, sorted() for the median.  cost_in and the path must
match it BIT FOR BIT.  Three deliberately wrong variants of the restatement (F32 sums, a tie rule that prefers the diagonal, edge replication
instead of reflection) must each change a path on these inputs: otherwise the cases would prove nothing.  The same driver built with
-fsanitize=address,undefined runs clean as a stand-alone program.  CPU only."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dtw_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "native", "dtw_math.cpp"), os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_dtw_host.cpp")]
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
f32, f64 = np.float32, np.float64
CASES = dtw_cases.small_cases()
REFUSED = -1


def restate(cube, M, sot_len, width=7, sums=f64, tie="reference", pad="reflect"):
    """cost_in [n_tokens][M] and the path [(token index, time index)], every step a rounded scalar operation in the reference's order"""
    K, T, _ = cube.shape
    hw = width // 2
    norm = np.empty((K, T, M), dtype=f32)
    for k in range(K):
        for j in range(M):
            s = sums(0)
            for t in range(T):
                s = sums(s + sums(cube[k, t, j]))
            mean = f32(s / sums(T))
            s2, v = sums(0), []
            for t in range(T):
                d = f32(cube[k, t, j] - mean)
                v.append(d)
                s2 = sums(s2 + sums(f32(d * d)))
            variance = f32(s2 / sums(T))
            scale = f32(f32(1.0) / np.sqrt(f32(variance + f32(1e-9))))
            for t in range(T):
                norm[k, t, j] = f32(v[t] * scale)

    def at(j):
        if pad == "reflect":
            return -j if j < 0 else (2 * (M - 1) - j if j > M - 1 else j)
        return min(max(j, 0), M - 1)

    cost_in = np.empty((T, M), dtype=f32)
    for t in range(T):
        for j in range(M):
            s = sums(0)
            for k in range(K):
                med = sorted(norm[k, t, at(j + o)] for o in range(-hw, hw + 1))[hw]
                s = sums(s + sums(med))
            v = f32(s)
            v = f32(v / f32(K))
            cost_in[t, j] = f32(v * f32(-1.0))

    N = T - sot_len - 1
    inf = f32(np.inf)
    C = [[inf] * (M + 1) for _ in range(N + 1)]
    TR = [[-1] * (M + 1) for _ in range(N + 1)]
    C[0][0] = f32(0.0)
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = C[i - 1][j - 1], C[i - 1][j], C[i][j - 1]
            if tie == "reference":
                c, tr = (c0, 0) if (c0 < c1 and c0 < c2) else ((c1, 1) if (c1 < c0 and c1 < c2) else (c2, 2))
            else:       # wrong on purpose: the diagonal wins its ties
                c, tr = (c0, 0) if (c0 <= c1 and c0 <= c2) else ((c1, 1) if (c1 <= c2) else (c2, 2))
            C[i][j] = f32(cost_in[i - 1 + sot_len, j - 1] + c)
            TR[i][j] = tr
    for j in range(M + 1):
        TR[0][j] = 2
    for i in range(N + 1):
        TR[i][0] = 1
    path, i, j = [], N, M
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        tr = TR[i][j]
        if tr == 0:
            i, j = i - 1, j - 1
        elif tr == 1:
            i -= 1
        else:
            j -= 1
    return cost_in, path[::-1]


def write_cases(path, cases, width=7):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            K, T, n_ctx = c["cube"].shape
            f.write(struct.pack("<6i", K, T, n_ctx, c["M"], c["sot_len"], c.get("width", width)))
            f.write(c["cube"].tobytes())


def read_results(path, cases):
    data, at, out = open(path, "rb").read(), 0, []
    for c in cases:
        (rc,) = struct.unpack_from("<i", data, at); at += 4
        if rc < 0:
            out.append((rc, None, None))
            continue
        (n_cost,) = struct.unpack_from("<i", data, at); at += 4
        cost = np.frombuffer(data, dtype=np.float32, count=n_cost, offset=at).reshape(-1, c["M"]); at += 4 * n_cost
        pairs = np.frombuffer(data, dtype=np.int32, count=2 * rc, offset=at).reshape(rc, 2); at += 8 * rc
        out.append((rc, cost, [(int(a), int(b)) for a, b in pairs]))
    assert at == len(data)
    return out


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("dtw")
    exe = str(work / "dtw_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-mavx2", "-mf16c", "-ffp-contract=off", "-pthread", INC] + SRCS + ["-o", exe])
    inp, outp = str(work / "cases.bin"), str(work / "out.bin")
    write_cases(inp, CASES)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(work=work, exe=exe, inp=inp, outp=outp, got=dict(zip([c["name"] for c in CASES], read_results(outp, CASES))))


@pytest.fixture(scope="module")
def yardstick():
    """the restatement of every case, computed once"""
    return {c["name"]: restate(c["cube"], c["M"], c["sot_len"]) for c in CASES}


def test_cases_cover_the_shapes():
    assert {c["M"] for c in CASES} >= {8, 9, 64, 65}
    assert {c["N"] for c in CASES} >= {1, 2, 63, 64, 65}
    assert {c["cube"].shape[0] for c in CASES} >= {1, 3}
    assert any(c["cube"].shape[2] > c["M"] for c in CASES) and any(c["cube"].shape[2] == c["M"] for c in CASES)


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_host_function_matches_the_restatement(env, yardstick, name):
    c = next(c for c in CASES if c["name"] == name)
    rc, cost, path = env["got"][name]
    want_cost, want_path = yardstick[name]
    assert rc == len(want_path) and rc <= c["N"] + c["M"]
    assert cost.shape == want_cost.shape and np.array_equal(cost.view(np.uint32), want_cost.view(np.uint32))
    assert path == want_path
    assert path[0] == (0, 0) and path[-1] == (c["N"] - 1, c["M"] - 1)


def test_constant_cube_is_decided_by_the_tie_rule(yardstick):
    c = next(c for c in CASES if c["name"] == "constant")
    cost, path = yardstick["constant"]
    assert len(set(cost.view(np.uint32).ravel().tolist())) == 1            # every cost the same
    # all three neighbours tie wherever they are finite: neither strict comparison holds, the rule takes 2 (left) until column 0 ends it
    assert path == [(0, 0)] + [(i, 0) for i in range(1, c["N"])] + [(c["N"] - 1, j) for j in range(1, c["M"])]


def test_mean_rounds_in_the_rounding_case():
    c = next(c for c in CASES if c["name"] == "mean_rounds_h1")
    col = c["cube"][0, :, 0].astype(np.float64)
    assert float(np.float32(col.sum() / len(col))) != col.sum() / len(col)


@pytest.mark.parametrize("variant", ["f32_sums", "tie_prefers_0", "edge_replication"])
def test_wrong_variants_change_a_path(yardstick, variant):
    kw = dict(f32_sums=dict(sums=f32), tie_prefers_0=dict(tie="prefers 0"), edge_replication=dict(pad="edge"))[variant]
    changed = [c["name"] for c in CASES if restate(c["cube"], c["M"], c["sot_len"], **kw)[1] != yardstick[c["name"]][1]]
    assert changed, "the variant %s gives every path of the reference order: the cases do not tell them apart" % variant


def test_refusals(env):
    cube = CASES[3]["cube"]         # 1 head, 4 tokens, 8 frames
    bad = [dict(cube=cube, M=8, sot_len=2, width=6, name="even width"), dict(cube=cube, M=7, sot_len=2, name="M <= width"),
           dict(cube=cube, M=8, sot_len=3, name="N == 0"), dict(cube=cube, M=9, sot_len=2, name="M > n_ctx"),
           dict(cube=cube, M=8, sot_len=2, width=9, name="width > M")]
    inp, outp = str(env["work"] / "bad.bin"), str(env["work"] / "bad_out.bin")
    write_cases(inp, bad)
    r = subprocess.run([env["exe"], inp, outp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [x[0] for x in read_results(outp, bad)] == [REFUSED] * len(bad)


def test_other_widths_sort(env):
    """width 5 and 9 take the sorting median: same restatement"""
    cs = [dict(dtw_cases.shaped("w5", 21, 3, 9, 17, 20), width=5), dict(dtw_cases.shaped("w9", 22, 1, 6, 12, 12), width=9)]
    inp, outp = str(env["work"] / "w.bin"), str(env["work"] / "w_out.bin")
    write_cases(inp, cs)
    r = subprocess.run([env["exe"], inp, outp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    for c, (rc, cost, path) in zip(cs, read_results(outp, cs)):
        want_cost, want_path = restate(c["cube"], c["M"], c["sot_len"], width=c["width"])
        assert np.array_equal(cost.view(np.uint32), want_cost.view(np.uint32)) and path == want_path


def test_sanitized_driver_runs_clean(env):
    exe = str(env["work"] / "dtw_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           INC] + SRCS + ["-o", exe])
    outp = str(env["work"] / "out_san.bin")
    r = subprocess.run([exe, env["inp"], outp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert open(outp, "rb").read() == open(env["outp"], "rb").read()

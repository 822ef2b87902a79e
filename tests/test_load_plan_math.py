"""The model loader's chunk planner (whisper-rust_amd/csrc/wa_load_plan.h through tests/native/load_plan.cpp, g++ alone: no HIP, no device).

The device load path cuts every tensor into chunks that go through a staging buffer of `cap` bytes of which `used` are taken.  Whatever the
sizes, the chunks must tile the tensor exactly, none may be empty, none may exceed the buffer, and every boundary must be a row boundary: a
quantised block (22 .. 210 bytes) cut in two would be unpacked from bytes of two different buffers.  The last check is shown to bite: a
planner that cuts at byte boundaries (fill the buffer to the brim) fails it on these very cases.  The same driver built with
-fsanitize=address,undefined runs clean as a stand-alone program.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "load_plan.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")

Q5_0_K192, Q5_0_K256, Q3_K_K256, Q6_K_K1024 = 6 * 22, 8 * 22, 110, 4 * 210        # row bytes

# name -> (nbytes, row_bytes, cap, used)
CASES = {
    "smaller_than_a_chunk":         (3 * Q5_0_K192, Q5_0_K192, 4096, 0),
    "smaller_behind_other_tensors": (3 * Q5_0_K192, Q5_0_K192, 4096, 1024),
    "exactly_one_chunk":            (8 * Q5_0_K192, Q5_0_K192, 8 * Q5_0_K192, 0),
    "one_byte_short_of_a_chunk":    (8 * Q5_0_K192, Q5_0_K192, 8 * Q5_0_K192 - 1, 0),
    "rows_do_not_divide_cap":       (100 * Q5_0_K192, Q5_0_K192, 1000, 0),
    "one_row":                      (Q5_0_K256, Q5_0_K256, 4096, 0),
    "one_row_is_the_buffer":        (Q5_0_K256, Q5_0_K256, Q5_0_K256, 0),
    "one_row_no_room_left":         (Q5_0_K256, Q5_0_K256, 4096, 4000),
    "q3_k_rows_of_110":             (1000 * Q3_K_K256, Q3_K_K256, 4096, 0),
    "q3_k_behind_other_tensors":    (1000 * Q3_K_K256, Q3_K_K256, 4096, 3008),
    "q5_0_rows_of_176":             (515 * Q5_0_K256, Q5_0_K256, 4096, 16),
    "q5_0_rows_of_132":             (515 * Q5_0_K192, Q5_0_K192, 4096, 4096),
    "q6_k_one_row_per_chunk":       (7 * Q6_K_K1024, Q6_K_K1024, Q6_K_K1024 + 100, 0),
    "buffer_of_one_row_many_rows":  (51865 * Q3_K_K256, Q3_K_K256, 112, 0),
}
REFUSED = {
    "no_bytes":              (0, 110, 4096, 0),
    "no_row":                (110, 0, 4096, 0),
    "rows_do_not_tile":      (3 * 110 + 1, 110, 4096, 0),
    "row_larger_than_cap":   (2 * 840, 840, 839, 0),
    "used_beyond_cap":       (110, 110, 4096, 4097),
}


def run_driver(exe, work, cases, tag):
    inp = str(work / ("cases_%s.txt" % tag))
    with open(inp, "w") as f:
        for c in cases:
            f.write("%d %d %d %d\n" % c)
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines, plans, at = r.stdout.split("\n"), [], 0
    for _ in cases:
        tag_, n = lines[at].split(); at += 1
        assert tag_ == "plan"
        plans.append([tuple(int(v) for v in lines[at + i].split()) for i in range(int(n))]); at += int(n)
    return plans, r.stdout


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("load_plan")
    exe = str(work / "load_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    plans, out = run_driver(exe, work, list(CASES.values()), "good")
    return dict(work=work, exe=exe, plans=dict(zip(CASES, plans)), out=out)


def violations(plan, nbytes, row_bytes, cap, used):
    """the properties a plan [(file_off, row0, rows)] breaks; the planner's own row fields are not trusted for the byte checks"""
    bad = set()
    ends = [c[0] for c in plan[1:]] + [nbytes]
    at = 0
    for (off, row0, rows), end in zip(plan, ends):
        if off != at:
            bad.add("tiling")
        if end <= off or rows <= 0:
            bad.add("empty")
        if end - off > cap:
            bad.add("capacity")
        if off % row_bytes or end % row_bytes:
            bad.add("row boundary")
        if row0 * row_bytes != off or rows * row_bytes != end - off:
            bad.add("row fields")
        at = end
    if at != nbytes or not plan:
        bad.add("tiling")
    return bad


def bytewise_planner(nbytes, row_bytes, cap, used):
    """the wrong planner: fill what is left of the buffer, then whole buffers, wherever that cuts"""
    plan, at, room = [], 0, (cap - used) or cap
    while at < nbytes:
        n = min(room, nbytes - at)
        plan.append((at, at // row_bytes, max(1, n // row_bytes)))
        at, room = at + n, cap
    return plan


@pytest.mark.parametrize("name", list(CASES))
def test_chunks_tile_the_tensor_in_whole_rows(env, name):
    nbytes, row_bytes, cap, used = CASES[name]
    plan = env["plans"][name]
    assert not violations(plan, nbytes, row_bytes, cap, used), (plan[:4], violations(plan, nbytes, row_bytes, cap, used))
    # the first chunk takes what still fits behind `used`; it is sized for an empty buffer only when not one row fits there
    fits = (cap - used) // row_bytes
    n_rows = nbytes // row_bytes
    assert plan[0][2] == min(n_rows, fits if fits else cap // row_bytes)
    assert all(c[2] == cap // row_bytes for c in plan[1:-1])           # every middle chunk is as large as a buffer allows


def test_expected_plans(env):
    assert env["plans"]["smaller_than_a_chunk"] == [(0, 0, 3)]
    assert env["plans"]["exactly_one_chunk"] == [(0, 0, 8)]
    assert env["plans"]["one_byte_short_of_a_chunk"] == [(0, 0, 7), (7 * Q5_0_K192, 7, 1)]
    assert env["plans"]["rows_do_not_divide_cap"][:2] == [(0, 0, 7), (7 * Q5_0_K192, 7, 7)] and len(env["plans"]["rows_do_not_divide_cap"]) == 15
    assert env["plans"]["one_row_no_room_left"] == [(0, 0, 1)]
    assert env["plans"]["q3_k_behind_other_tensors"][:2] == [(0, 0, 9), (9 * 110, 9, 37)]
    assert len(env["plans"]["buffer_of_one_row_many_rows"]) == 51865
    assert env["plans"]["q6_k_one_row_per_chunk"] == [(i * Q6_K_K1024, i, 1) for i in range(7)]


def test_refusals(env):
    plans, _ = run_driver(env["exe"], env["work"], list(REFUSED.values()), "refused")
    assert plans == [[] for _ in REFUSED]


def test_bytewise_planner_fails_the_row_boundary_check():
    """the check is not vacuous: cutting where the buffer ends splits a row in every case whose rows do not divide the room"""
    caught = []
    for name, (nbytes, row_bytes, cap, used) in CASES.items():
        v = violations(bytewise_planner(nbytes, row_bytes, cap, used), nbytes, row_bytes, cap, used)
        if "row boundary" in v:
            caught.append(name)
    assert {"rows_do_not_divide_cap", "q3_k_rows_of_110", "q5_0_rows_of_176", "q5_0_rows_of_132", "q3_k_behind_other_tensors",
            "one_byte_short_of_a_chunk"} <= set(caught), caught
    # and it passes where nothing is cut: the check flags the cut, not the planner
    nbytes, row_bytes, cap, used = CASES["exactly_one_chunk"]
    assert not violations(bytewise_planner(nbytes, row_bytes, cap, used), nbytes, row_bytes, cap, used)


def test_sanitized_driver_runs_clean(env):
    exe = str(env["work"] / "load_plan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe])
    inp = str(env["work"] / "cases_good.txt")
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout == env["out"]

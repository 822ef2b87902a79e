"""The thread fan-out under every lock-step wave (whisper-rust_amd/csrc/wa_fanout.h through tests/native/wave_fanout.cpp, g++ alone: no HIP, no
device).

wa_fan_out(n, job, done, spawn): job(0) on the calling thread, job(1..n-1) on a thread each; done(i) exactly once for every i, on i's thread
after its job returned or threw, or - where thread k could not be started - on the calling thread before job(0) begins, for k and every later
member, whose jobs never run; -1 for a job that threw or never ran; every started thread joined.  The driver stands in for the batcher with a
mutex, a condition variable and a member count that `done` decrements: a job's steps return only when every member that has not left has
asked for one, so a missing `done` hangs the run (the timeout) and a doubled one shows in the counts.

Cases: n in {1, 2, 8}; plain, a job that throws (every index), a start failure at every k in 1..n-1, and both together.  The same driver built
with -fsanitize=thread, and with -fsanitize=address,undefined, runs clean as a stand-alone program.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "whisper-rust_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "wave_fanout.cpp")
TIMEOUT = 120       # seconds for all cases of one binary; they take well under one


def cases():
    out = []
    for n in (1, 2, 8):
        out.append((n, -1, -1))
        out += [(n, t, -1) for t in range(n)]
        out += [(n, -1, k) for k in range(1, n)]
        out += [(n, 1, k) for k in range(2, n)]
    return out


def expected(n, throw_at, fail_at):
    """the contract, restated: member i runs iff no start failed at or before it"""
    k = fail_at if fail_at >= 1 else n
    ran = [1 if i < k else 0 for i in range(n)]
    return dict(
        rcs=[100 + i if ran[i] and i != throw_at else -1 for i in range(n)],
        ran=ran,
        done=[1] * n,
        on_caller=[1 if i == 0 else 0 for i in range(n)],
        done_on_job_thread=ran,
        done_before_job0=[1 - r for r in ran],
        members_left=0,
    )


def build(work, name, flags):
    exe = str(work / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + CSRC] + flags + [SRC, "-o", exe])
    return exe


def run_all(exe, env=None):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    return r.returncode, r.stdout, r.stderr


def check_output(stdout):
    lines = [ln for ln in stdout.split("\n") if ln]
    want = cases()
    assert len(lines) == len(want)
    for ln, (n, throw_at, fail_at) in zip(lines, want):
        f = dict(kv.split("=") for kv in ln.split()[1:])
        assert (int(f["n"]), int(f["throw"]), int(f["fail"])) == (n, throw_at, fail_at)
        got = {key: [int(x) for x in f[key].split(",")] for key in ("rcs", "ran", "done", "on_caller", "done_on_job_thread", "done_before_job0")}
        got["members_left"] = int(f["members_left"])
        assert got == expected(n, throw_at, fail_at), ln


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    return tmp_path_factory.mktemp("wave_fanout")


def test_case_list_is_the_issue_s():
    c = cases()
    assert {n for n, _, _ in c} == {1, 2, 8}
    for n in (1, 2, 8):
        assert (n, -1, -1) in c
        assert all((n, t, -1) in c for t in range(n))               # a job that throws, every index, the calling thread's included
        assert all((n, -1, k) in c for k in range(1, n))            # a start failure at each k in 1..n-1


def test_header_compiles_alone(work):
    """wa_fanout.h with g++ and nothing else of the product: no HIP, no wa_internal.h."""
    src = work / "alone.cpp"
    src.write_text('#include "wa_fanout.h"\nint main() { auto rcs = wa_fan_out(3, [](int i) { return i; }, [](int) { }); '
                   'return rcs.size() == 3 && rcs[0] == 0 && rcs[1] == 1 && rcs[2] == 2 ? 0 : 1; }\n')
    exe = str(work / "alone")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + CSRC, str(src), "-o", exe])
    assert subprocess.run([exe], timeout=TIMEOUT).returncode == 0


def test_contract(work):
    rc, out, err = run_all(build(work, "wave_fanout", ["-O2"]))
    assert rc == 0 and err == "", err[-3000:]
    check_output(out)


def test_driver_under_address_and_undefined_sanitizers(work):
    exe = build(work, "wave_fanout_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    rc, out, err = run_all(exe)
    assert rc == 0 and err == "", err[-3000:]
    check_output(out)


def test_driver_under_thread_sanitizer(work):
    exe = build(work, "wave_fanout_tsan", ["-O1", "-g", "-fsanitize=thread"])
    rc, out, err = run_all(exe)
    if rc != 0 and out == "" and "FATAL: ThreadSanitizer" in err and ("memory mapping" in err or "memory layout" in err):
        pytest.skip("ThreadSanitizer cannot start here: " + err.strip().split("\n")[0])     # the address/undefined build above is still required
    assert rc == 0 and err == "", err[-3000:]
    check_output(out)

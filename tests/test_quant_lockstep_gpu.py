"""whisper_amd_batch_served (MI355X): how many of the passes a lock-step group formed DELIVERED their rows to the members - as one launch
(wa_rows.hip: F16, Q5_0, Q8_0) or through the launch sequence (F16) - beside `steps`, which counts every pass formed, whoever serves it.

Each case is one fresh process running tools/lockstep_check.py (the backend reads its switches once per process): four chunks through
whisper_amd_full_batch and then alone.  Checked: the group's segments equal the solo runs' (ids, token ids, times, p, plog as float32), members 0
and 1 equal the REFERENCE engine's committed goldens where the fixture has them, and the counter says what happened: one-launch passes and the
F16 launch-sequence passes count as served, a pass whose launch failed does not, and the formats whose members a group still sends away to decode
alone (Q5_1, Q4_1 and the K formats: their group pass is not in the tree) report no more served passes than formed ones.
Without the counter every test here fails: the symbol is missing."""
import json
import os
import subprocess
import sys

import pytest

import wsynth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "lockstep_check.py")
SWITCHES = ("WHISPER_AMD_NO_ROWS", "WHISPER_AMD_NO_GRAPH", "WHISPER_AMD_NO_FEW_ROWS", "WHISPER_AMD_TEST_FAIL_BATCH_LAUNCH", "WHISPER_AMD_NO_MEGA",
            "WHISPER_AMD_NO_BATCHER", "WHISPER_AMD_BATCH_GROUP", "WA_LIB")
_RUNS = {}


def run(model, env=None, extra=()):
    """One process of the tool, its JSON line; computed once per (model, switches, arguments) and shared by the tests."""
    key = (model, tuple(sorted((env or {}).items())), tuple(extra))
    if key not in _RUNS:
        if ":" in model:
            wsynth.quant_model_path(*model.split(":"))          # written once, here: not by the child
        else:
            wsynth.model_path(model)
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env or {})
        r = subprocess.run([sys.executable, TOOL, model, *extra], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (model, env, r.returncode, r.stderr[-2000:])
        _RUNS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _RUNS[key]


def n_tokens(segs):
    return sum(len(s["ids"]) for s in segs)


def check_served(out):
    """The group delivered at least one pass per two tokens of its shortest member, two rows or more each."""
    n_min = min(n_tokens(s) for s in out["solo"])
    print("steps %d rows %d one_launch %d served %d; solo tokens %r" % (out["steps"], out["rows"], out["one_launch"], out["served"], [n_tokens(s) for s in out["solo"]]))
    assert n_min > 0
    assert out["served"] >= n_min / 2, (out["served"], n_min)
    assert out["rows"] >= 2 * out["served"], (out["rows"], out["served"])
    assert out["served"] <= out["steps"], (out["served"], out["steps"])


@pytest.mark.parametrize("qt", ["q5_0", "q8_0"])
def test_one_launch_passes_count_as_served(qt):
    """s128 Q5_0 / Q8_0: the several-rows one-launch form serves the group; the group equals each member alone and members 0 and 1 equal the
    reference engine's goldens."""
    out = run("s128:" + qt)
    assert out["group"] == out["solo"], qt
    gold = json.load(open(os.path.join(GOLDEN, "s128_quant.json")))[qt]["full"]
    assert out["group"][0] == gold["greedy_seed0"] and out["group"][1] == gold["greedy_seed1"], qt
    assert out["one_launch"] > 0, out["one_launch"]
    check_served(out)


def test_launch_sequence_passes_of_an_f16_model_count_as_served():
    """s128 (F16) with the one-launch form switched off: the launch sequence with one K / V pointer set per row serves the group."""
    out = run("s128", {"WHISPER_AMD_NO_ROWS": "1"})
    assert out["group"] == out["solo"]
    assert out["one_launch"] == 0, out["one_launch"]
    check_served(out)


@pytest.mark.parametrize("model,fixture", [("s128:q5_1", "s128_quant1.json"), ("s256:q5_k", "s256_kquant.json")])
def test_members_sent_away_are_not_counted_twice(model, fixture):
    """A format without a group pass: the group forms its passes, the members decode alone; the result is each member's solo run and the
    reference engine's, no pass is one launch, and no more passes are reported served than were formed."""
    out = run(model)
    assert out["group"] == out["solo"], model
    gold = json.load(open(os.path.join(GOLDEN, fixture)))[model.split(":")[1]]["full"]
    assert out["group"][0] == gold["greedy_seed0"] and out["group"][1] == gold["greedy_seed1"], model
    assert out["one_launch"] == 0 and 0 <= out["served"] <= out["steps"], (out["one_launch"], out["served"], out["steps"])
    assert out["steps"] > 0


def test_few_rows_switch_leaves_the_result_alone():
    """WHISPER_AMD_NO_FEW_ROWS=1 (the general product kernel instead of the few-rows one, wa_quant.hip): the same segments."""
    base, out = run("s128:q5_1"), run("s128:q5_1", {"WHISPER_AMD_NO_FEW_ROWS": "1"})
    assert out["group"] == base["group"] and out["solo"] == base["solo"]


def test_failed_pass_is_not_served():
    """The host-side hook that fails every group launch (it faults nothing): every member decodes alone, the result is unchanged, no pass
    counts as served - for a model whose passes are served otherwise."""
    out = run("s128:q5_0", {"WHISPER_AMD_TEST_FAIL_BATCH_LAUNCH": "1"})
    assert out["group"] == out["solo"]
    assert out["group"] == run("s128:q5_0")["group"]
    assert out["served"] == 0, out["served"]


def test_full_parallel_sets_the_counters_too(wrs, ref_lib):
    """whisper_full_parallel with 2 processors on s128:q5_0: the stitched segments equal the reference engine's, run live on the same file and
    audio, and the two parts' shared passes are counted as for whisper_amd_full_batch."""
    out = run("s128:q5_0", extra=("--parallel", "2"))
    assert out["rc"] == 0
    mp = wsynth.quant_model_path("s128", "q5_0")
    rc = wrs.WhisperFullContext.new_with_params(mp, wrs.WhisperContextParameters(ref_lib, use_gpu=False), lib=ref_lib)
    assert rc.full_parallel(wrs.FullParams(ref_lib, 0, best_of=1, temperature_inc=0.0, n_threads=8), wsynth.synth_audio(960000, 4), 2) == 0
    want = [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"]) for s in rc.segments()]
    rc.free()
    assert want, "the reference produced no segment"
    assert out["parallel"] == want
    assert out["served"] > 0 and out["rows"] >= 2 * out["served"] and out["served"] <= out["steps"], (out["served"], out["rows"], out["steps"])

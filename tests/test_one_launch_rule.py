"""The device slot and the pause rule of the one-launch decode forms (whisper-rust_amd/csrc/wa_one_launch.h): the pause schedule after
hand-off time-outs, re-arming, the 9th time-out switching a form off; a slot that any thread may give back.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pause_rule_and_device_slot(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "one_launch_rule")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", os.path.join(ROOT, "tests", "native", "one_launch_rule.cpp"),
                           "-I", os.path.join(ROOT, "whisper-rust_amd", "csrc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "one_launch_rule: 0 failures" in out.stdout, out.stdout

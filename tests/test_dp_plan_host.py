"""The host plans of the sweep and band drivers (tracy_amd/csrc/dp_plan.h: order, chunk cut, offsets, runs, band launches, timer
credit; chunk_cut.h: the greedy cut every workspace plan uses) as a stand-alone program over the headers alone
(tests/cpp/dp_plan.cpp, its own main), built plain and with -fsanitize=address,undefined and run as a program.  No GPU, nothing
loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dp_plan.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_dp_plan_program(tmp_path, build):
    exe = tmp_path / ("dp_plan_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + FLAGS[build] + ["-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "dp_plan: ok" in r.stdout

"""The host plan of a wildtype job (tracy_amd/csrc/wildtype_plan.h: the two launch orders, the runs, the chunk cut) as a stand-alone
program over the header alone (tests/cpp/wildtype_plan.cpp, its own main), built plain and with -fsanitize=address,undefined and run
as a program.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "wildtype_plan.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_wildtype_plan_program(tmp_path, build):
    exe = tmp_path / ("wildtype_plan_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + FLAGS[build] + ["-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "wildtype_plan: ok" in r.stdout

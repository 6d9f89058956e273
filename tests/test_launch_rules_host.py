"""The launch sizing and timer-credit rules both paths share (tracy_amd/csrc/launch_rules.h: word bytes and credit of a banded pair,
code columns and LDS fit of band launches and pruned-sweep tiers, credit of tiers, sweeps and prefixes, the order of the sweeps) as a
stand-alone program over the headers alone (tests/cpp/launch_rules.cpp, its own main), built plain and with
-fsanitize=address,undefined and run as a program.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "launch_rules.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_launch_rules_program(tmp_path, build):
    exe = tmp_path / ("launch_rules_" + build)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + FLAGS[build] + ["-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "launch_rules: ok" in r.stdout

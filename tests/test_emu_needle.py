"""needle_body / needle_walk_one (tracy_amd/csrc/dp_kernels.h) and needle_step (dp_lane.h) on the host wave emulator against the oracle
(needle_str, needle_prof and the score-only forms), bit for bit, on the cases of tests/needle_cases.py: every strip height the host
chooses and both sides of every pass edge.  This is everything of the needle kernels but the __global__ wrappers, the DPP shift, the
barriers, the rounding intrinsics of SubProfD and the host driver -- those are tests/test_gpu_needle.py's.

Thinning (the emulator runs one fiber per lane): every case runs in every AlignConfig with a traceback and score-only, under one of
scorings 0 and 1 and, where needle_cases.cases_of_scoring admits the case, one of scorings 2 and 3; which one rotates with the case and
the config.  One case of every (strip height, one pass / several) class runs every config x scoring."""
import os
import sys

import pytest

import needle_cases as nc
import pyoracle as orc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402


def check(case, cfg, sc, K=None):
    """one case under one config and scoring at strip height K (default: the host's choice), traceback and score-only"""
    name, a, b = case
    prof = nc.is_prof(case)
    K = K or nc.strip_height(nc.shape(case)[0], prof)
    mode = emu.MODE_PROF if prof else emu.MODE_CHAR
    want = (orc.needle_prof if prof else orc.needle_str)(a, b, cfg[0], cfg[1], sc)
    assert (orc.needle_score_prof if prof else orc.needle_score_str)(a, b, cfg[0], cfg[1], sc) == want[0], (name, cfg, sc)
    got = emu.run(a, b, sc, cfg[0], cfg[1], mode, K, trace=True, needle=True)
    assert got[0] == want[0] and got[1] == want[1], (name, cfg, sc, K)
    assert emu.run(a, b, sc, cfg[0], cfg[1], mode, K, trace=False, needle=True)[0] == want[0], (name, cfg, sc, K)


def rotating(cases, ci):
    """(case, scoring index) for config CONFIGS[ci]: one of scorings 0 and 1, and one of 2 and 3 where the case is admitted"""
    tall_ok = {c[0] for c in nc.cases_of_scoring(cases, 2)}
    for j, case in enumerate(cases):
        yield case, (j + ci) % 2
        if case[0] in tall_ok:
            yield case, 2 + (j // 2 + ci) % 2


def test_the_cases_hold_every_kernel():
    nc.assert_every_kernel_is_reached()


@pytest.mark.parametrize("ci", range(4))
def test_strings_equal_the_oracle(ci):
    for case, si in rotating(nc.string_cases(), ci):
        check(case, nc.CONFIGS[ci], nc.SCORINGS[si])


@pytest.mark.parametrize("ci", range(4))
def test_profiles_equal_the_oracle(ci):
    for case, si in rotating(nc.profile_cases(), ci):
        check(case, nc.CONFIGS[ci], nc.SCORINGS[si])


@pytest.mark.parametrize("prof", [False, True])
def test_every_config_and_scoring_in_every_class(prof):
    reps = nc.representatives(nc.profile_cases() if prof else nc.string_cases())
    assert {nc.klass(c) for c in reps} == (nc.PROFILE_CLASSES if prof else nc.STRING_CLASSES)
    for case in reps:
        for cfg in nc.CONFIGS:
            for sc in nc.SCORINGS:
                check(case, cfg, sc)


def test_strips_of_eight_rows_in_one_pass():
    """K = 8 where the host would take 4: the strip height tests/test_emu_wave.py::test_needle leaves out"""
    picked = [c for c in nc.string_cases() if nc.shape(c) in ((5, 1), (64, 65), (255, 63), (256, 65))]
    picked += [c for c in nc.profile_cases() if nc.shape(c)[0] in (2, 65, 256)][::2]
    assert len(picked) >= 7 and all(nc.klass(c) == (4, False) for c in picked)
    for j, case in enumerate(picked):
        for ci, cfg in enumerate(nc.CONFIGS):
            check(case, cfg, nc.SCORINGS[(j + ci) % 4], K=8)

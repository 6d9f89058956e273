"""Generate tests/golden/launch_credit.json: what every kernel timer is credited (launches, cells, bytes) for the four calls of
tests/test_gpu_launch_credit.py, as the library in the tree computes them.  Needs a GPU.  Run it at a commit whose credits are
known to be right (the file in the repository was recorded at the commit before tracy_amd/csrc/launch_rules.h); the JSON is
committed (data, not source).  An argument names another file to write."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tracy_amd  # noqa: E402
from test_gpu_launch_credit import MUST_RUN, measure  # noqa: E402


def main():
    ctx = tracy_amd.Context(0)
    got = measure(ctx)
    ctx.close()
    out = {"note": "launches are those of the default options (b16_multi_max, side streams available); cells and bytes depend on the inputs alone",
           "compare_launches": True, "calls": {}, "stats": {}}
    for name, (res, stats, timers) in got.items():
        assert all(timers[t]["cells"] > 0 for t in MUST_RUN), (name, timers)
        out["calls"][name] = timers
        out["stats"][name] = {k: stats[k] for k in ("stream_ordered", "fallback_traces", "pruned", "pruned_uncertified", "prelim_banded", "final_banded")}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "launch_credit.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(json.dumps(out["stats"], sort_keys=True))
    print("wrote", path)


if __name__ == "__main__":
    main()

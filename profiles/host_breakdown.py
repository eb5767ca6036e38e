"""bench.py with the host side of a decode call broken down: runs bench.py's main() with the arguments given (one GPU) and
prints, behind bench.py's own line, a second JSON line -- per column lane the mean host microseconds per timed step of every part
of the call (capi.Context.lane_host_us: orcgpu_last_lane_host_us), in the order the parts run.

    python profiles/host_breakdown.py --gpus 1 --steps 20 --warmup 5 [--sf 1]

bench.py reads the lane statistics once per timed step; this reads the host parts at the same moment, so both lines are means
over the same steps.  profiles/host_plan_before.json and host_plan_after.json were written with it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from orc_rust_amd import capi  # noqa: E402

acc, steps = [], [0]
_lane_stats = capi.Context.lane_stats


def lane_stats(self):
    for k, parts in enumerate(self.lane_host_us()):
        if k == len(acc):
            acc.append(dict.fromkeys(capi.Context.HOST_PARTS, 0.0))
        for name, us in parts.items():
            acc[k][name] += us
    steps[0] += 1
    return _lane_stats(self)


capi.Context.lane_stats = lane_stats
bench.main()
n = max(1, steps[0])
lanes = []
for k, a in enumerate(acc):
    d = {name: round(us / n, 1) for name, us in a.items()}
    d["lane"] = k
    d["before_first_launch_us"] = round(sum(a[p] for p in ("lanes", "columns", "chunks", "layout")) / n, 1)
    d["tables_us"] = round(sum(a[p] for p in ("chunks", "fill", "upload")) / n, 1)  # planning, table fill and uploads together
    lanes.append(d)
print(json.dumps({"host_us_per_step": lanes, "steps": steps[0]}))

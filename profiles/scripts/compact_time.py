"""Time of sph_remove's compaction at BASELINE config 3 (16,777,216 particles), next to the sort's k_mm_move, which streams
the same arrays.  Run from the repo root under the kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/compact_time.py

and read k_edit_count / k_edit_scan / k_edit_compact / k_mm_move from OUT/p_kernel_stats.csv.  Three removals of different
share (a sphere ~3 %, a box 25 %, a half-space another 25 % of the dam) each after two merge-sorted steps; the printed line gives the
counts, so that a time can be read against the bytes its launch moved (36 B in per particle, 36 B out per survivor)."""
import json
import sys

import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

sys.path.insert(0, ".")
from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
regions = {
    "sphere": capi.Region.sphere((-10.0, -10.0, -10.0), 1.5),
    "box": capi.Region.box((-16.0, -16.0, -16.0), (-12.0, -12.0, 16.0)),
    "halfspace": capi.Region.halfspace((0.0, -12.0, 0.0), (0.0, 1.0, 0.0)),
}
out = {"particles": n}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.set_sort_mode(2)                     # the merge path whatever the mover count: k_mm_move runs in every sort but the first
    c.reset_lattice(cfg["lattice"])
    c.step(dt, 3)
    for name, reg in regions.items():
        before = c.n
        inside = c.count_in(reg)
        c.remove(reg, max_out=0)
        out[name] = {"before": before, "counted": inside, "removed": c.last_removed}
        c.step(dt, 2)
    c.sync()
    out["merges"] = c.sort_stats()["merges"]
print(json.dumps(out))

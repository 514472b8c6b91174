"""The one-block scans under the kernel trace: BASELINE config 3 (16,777,216 particles) as a lattice at rest, where every
step queues k_mm_tilescan (the mover count is wanted at the end of the step, so that the next sort can be skipped), and one
sph_remove, whose k_edit_scan takes 8192 tile counts.  Run from the repo root:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/scan_time.py [steps]

and read k_mm_tilescan / k_edit_scan from OUT/p_kernel_stats.csv (mean, standard deviation over the launches).  SPH_HIP_LIB picks
another build of the library (profiles/scan_unify_ab.txt: the parent commit's against this one's)."""
import json
import sys

import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

sys.path.insert(0, ".")
from gpufluidsimulator_amd import capi, ic  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=False)
    c.step(float(ic.DEFAULT_DT), steps)
    c.sync()
    stats = c.sort_stats()
    c.remove(capi.Region.sphere((-10.0, -10.0, -10.0), 1.5), max_out=0)
    print(json.dumps({"particles": n, "steps": steps, "sorts": stats["sorts"], "skips": stats["skips"], "removed": c.last_removed}))

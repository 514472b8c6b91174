"""Price of the obstacle pass (sph_obstacle_build, k_obstacle_push) at BASELINE config 3 (16,777,216 particles): the flowing dam
(6000 steps from the lattice) with a box pillar 8 cells wide standing in the fluid, on a local grid around it (the bounds
argument; spacing = the cell edge), stepped in 100-step windows that alternate between the context with the pillar and the same
context after sph_obstacle_clear.  (The two variants do not see the same bits: the pillar changes the flow around it.  The
windows alternate so that drift of the flow and of the clocks falls on both.)  Prints the six windows of each variant, their
medians, and how many particles sit within h of the pillar.  Run from the repo root; once plainly for the wall-clock medians, and
once under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/obstacle_time.py

for k_obstacle_push next to k_force in OUT/p_kernel_stats.csv."""
import json
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

sys.path.insert(0, ".")
from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
cell = cfg["box"][0] / cfg["grid"][0]
centre, half = (-11.0, -13.0, -12.0), (4.0 * cell, 3.0, 4.0 * cell)
pillar = [capi.Shape.box(centre, half)]
bounds = (tuple(c - h - 4.0 * cell for c, h in zip(centre, half)), tuple(c + h + 4.0 * cell for c, h in zip(centre, half)))
windows = {"pillar": [], "none": []}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, 6000)
    c.build_obstacle(pillar, cell, bounds)
    grid = c.obstacle()
    c.step(dt, 100)                                    # the pillar clears its place
    c.sync()
    for w in range(12):
        name = "none" if w % 2 else "pillar"
        if w % 2:
            c.clear_obstacle()
        else:
            c.build_obstacle(pillar, cell, bounds)
        c.step(dt, 5); c.sync()
        t0 = time.perf_counter()
        c.step(dt, 100); c.sync()
        windows[name].append(round((time.perf_counter() - t0) / 100 * 1e3, 4))
    pos = c.download(want=("pos",))["pos"]
q = np.abs(pos.astype(np.float64) - np.array(centre)) - np.array(half)
d = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)
print(json.dumps({"particles": n, "lattice": list(grid["dims"]), "spacing": float(grid["spacing"]), "ms_per_step": windows,
                  "median_ms": {k: statistics.median(v) for k, v in windows.items()},
                  "particles_within_h_of_the_pillar": int((d < 0.1).sum()), "deepest": float(d.min())}))

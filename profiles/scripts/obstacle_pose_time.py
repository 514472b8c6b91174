"""Price of the posed and of the sensing obstacle pass (sph_obstacle_set_pose, sph_obstacle_set_sensor: the instantiations of
k_obstacle_push, and k_obstacle_load) next to the plain one, at BASELINE config 3 (16,777,216 particles): the flowing dam with
the box pillar of profiles/scripts/obstacle_time.py on its local grid, stepped in 100-step windows that go round the variants
-- plain, posed (a pillar turned by 0.2 rad about its axis, omega = 0: it stays where it is), posed and sensing -- three
times.  Prints the windows' wall clock per step and the last load.  Run from the repo root under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/obstacle_pose_time.py

for the three k_obstacle_push instantiations and k_obstacle_load in OUT/p_kernel_stats.csv.  With a library of before the pose
(SPH_HIP_LIB=..., SPH_HIP_LIB_ALLOW_MISSING=1) only the plain variant runs: the parent's figure."""
import json
import math
import statistics
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

sys.path.insert(0, ".")
from gpufluidsimulator_amd import capi, ic  # noqa: E402

WARM = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
cell = cfg["box"][0] / cfg["grid"][0]
centre, half = (-11.0, -13.0, -12.0), (4.0 * cell, 3.0, 4.0 * cell)
pillar = [capi.Shape.box(centre, half)]
bounds = (tuple(c - h - 4.0 * cell for c, h in zip(centre, half)), tuple(c + h + 4.0 * cell for c, h in zip(centre, half)))
quat = (math.cos(0.1), 0.0, math.sin(0.1), 0.0)
has_pose = hasattr(capi.load(), "sph_obstacle_set_pose")
variants = ("plain", "posed", "posed_sensing") if has_pose else ("plain",)
windows = {v: [] for v in variants}
load = None
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, WARM)
    c.build_obstacle(pillar, cell, bounds)
    c.step(dt, 100)                                    # the pillar clears its place
    c.sync()
    for w in range(3 * len(variants)):
        name = variants[w % len(variants)]
        if has_pose:
            c.set_obstacle_pose(*((centre, quat) if name != "plain" else (None,)))
            c.set_obstacle_sensor(name == "posed_sensing")
        c.step(dt, 5); c.sync()
        t0 = time.perf_counter()
        c.step(dt, 100); c.sync()
        windows[name].append(round((time.perf_counter() - t0) / 100 * 1e3, 4))
        if name == "posed_sensing":
            load = c.obstacle_load()
print(json.dumps({"particles": n, "warm_steps": WARM, "ms_per_step": windows,
                  "median_ms": {k: statistics.median(v) for k, v in windows.items()},
                  "load": None if load is None else {"J": list(load["J"]), "L": list(load["L"]), "steps": load["steps"]}}))

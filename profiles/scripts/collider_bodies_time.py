"""Price of tracking the spheres' impulses (sph_set_collider_bodies) at BASELINE config 3 (16,777,216 particles): the flowing
dam (6000 steps from the lattice) with 8 spheres of 4 cells radius at rest in the fluid, stepped in 100-step windows that
alternate between the untracked context (the by-value kernels) and the tracked one with every mass 0 (the tracked kernels plus
k_spheres_step; the same bits in every particle, so both variants see the same flow).  Prints the six windows of each variant
and their medians.  Run from the repo root; once plainly for the wall-clock medians, and once under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/collider_bodies_time.py

for k_spheres_step and the two k_force instantiations in OUT/p_kernel_stats.csv."""
import json
import statistics
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

sys.path.insert(0, ".")
from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
R = 4.0 * cfg["box"][0] / cfg["grid"][0]
centers = [(-12.0 + sx, -12.5 + sy, -12.0 + sz) for sx in (-2.0, 2.0) for sy in (-1.5, 1.5) for sz in (-2.0, 2.0)]
windows = {"untracked": [], "tracked": []}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, 6000)
    c.set_colliders(centers, [R] * 8)
    c.step(dt, 100)                                    # the spheres clear their place
    c.sync()
    for w in range(12):
        name = "tracked" if w % 2 else "untracked"
        c.set_collider_bodies([0.0] * 8 if w % 2 else [])
        c.step(dt, 5); c.sync()
        t0 = time.perf_counter()
        c.step(dt, 100); c.sync()
        windows[name].append(round((time.perf_counter() - t0) / 100 * 1e3, 4))
    J, steps = c.collider_impulses()                   # (the last window was a tracked one)
    pos = c.download(want=("pos",))["pos"]
near = [int((((pos - ce) ** 2).sum(axis=1) < (R + 0.1) ** 2).sum()) for ce in centers]
print(json.dumps({"particles": n, "ms_per_step": windows, "median_ms": {k: statistics.median(v) for k, v in windows.items()},
                  "tracked_steps_last_window": steps, "J_last": [[float(x) for x in row] for row in J],
                  "particles_within_h_of_each_sphere": near}))

"""Time of one mesh voxelisation (sph_obstacle_build_mesh_dev) next to sph_obstacle_build of one analytic box on the same lattice,
the floor: both fill and install the same grid.

  pillar  the twelve-triangle box of profiles/scripts/obstacle_time.py on its 19 x 107 x 19 lattice (spacing = config 3's cell
          edge, the bounds argument), from device arrays
  c3      the mesh sph_mesh_extract gives for the flowing dam of BASELINE config 3 (16,777,216 particles, 6000 steps from the
          lattice) at spacing 1/15 (491^3 nodes, the finest the mesh limits allow in that box), fed through sph_mesh_dev's pointers
          and voxelised at band 3 over the whole box at spacing 0.063: 511^3 nodes, the largest lattice below SPH_OBSTACLE_MAX_NODES

Every build is timed as wall time between two synchronisations, over `--reps` builds, each of which replaces the obstacle of the
build before (so both sides pay the same release and allocation).  Without --case the script is the driver: it runs each case as
a child process under a time limit of its own, plainly and then under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python profiles/scripts/obstacle_mesh_time.py --case NAME

for the shares of k_obmesh_count / _scan / _distance / _cross / _finish and k_obstacle_bricks, stops at the first child that fails,
and writes profiles/obstacle_mesh_time.json.  Run from the repo root."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, ".")

ap = argparse.ArgumentParser()
ap.add_argument("--case", choices=("pillar", "c3"))
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--limit", type=int, default=420, help="seconds a child may run")
ap.add_argument("--out", default=os.path.join("profiles", "obstacle_mesh_time.json"))
args = ap.parse_args()


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def kernel_shares(directory):
    """name -> {calls, total_us} of the voxeliser's kernels and the bricks from the trace's p_kernel_stats.csv"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in ("k_obmesh_count", "k_obmesh_scan", "k_obmesh_distance", "k_obmesh_cross", "k_obmesh_finish", "k_obstacle_bricks",
                      "k_obstacle_raster"):
                if "::" + k + "(" in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "total_us": round(int(row["TotalDurationNs"]) / 1e3, 1),
                              "average_us": round(float(row["AverageNs"]) / 1e3, 2)}
    return out


if args.case is None:                                     # the driver: one child per GPU run, each under its own limit
    result = {}
    for case in ("pillar", "c3"):
        child = [sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps), "--flow-steps", str(args.flow_steps)]
        with tempfile.TemporaryDirectory() as d:
            runs = (("wall", ["timeout", "-k", "10", str(args.limit)] + child),
                    ("trace", ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
                               "-d", d, "-o", "p", "--"] + child))
            for what, cmd in runs:
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"{case} ({what}) ended with status {p.returncode}: stopping here")
                if what == "wall":
                    result[case] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                else:
                    result[case]["kernels_of_the_traced_run"] = kernel_shares(d)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    sys.exit(0)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
dt = float(ic.DEFAULT_DT)
cell = cfg["box"][0] / cfg["grid"][0]


def timed(c, build):
    ms = []
    for _ in range(args.reps):
        c.sync()
        t0 = time.perf_counter()
        build()
        c.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def box_mesh(lo, hi):
    v = np.array([[(hi if (q >> k) & 1 else lo)[k] for k in range(3)] for q in range(8)], np.float32)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    return v, np.array([(a, b, c) for a, b, c, d in quads] + [(a, c, d) for a, b, c, d in quads], np.int32)


out = {"case": args.case, "reps": args.reps}
if args.case == "pillar":
    centre, half = (-11.0, -13.0, -12.0), (4.0 * cell, 3.0, 4.0 * cell)
    lo, hi = tuple(c - h for c, h in zip(centre, half)), tuple(c + h for c, h in zip(centre, half))
    bounds = (tuple(x - 4.0 * cell for x in lo), tuple(x + 4.0 * cell for x in hi))
    v, t = box_mesh(lo, hi)
    dv, dtri = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    torch.cuda.synchronize()
    L = capi.load()
    with capi.Context(64, box=cfg["box"], grid=cfg["grid"]) as c:
        p = capi.ObstacleMeshParams(cell, 3, 0)
        blo, bhi = (C.c_float * 3)(*bounds[0]), (C.c_float * 3)(*bounds[1])

        def mesh():
            assert L.sph_obstacle_build_mesh_dev(c.h, C.byref(p), blo, bhi, len(v), dv.data_ptr(), len(t), dtri.data_ptr()) == 0

        mesh()
        out["dims"] = list(c.obstacle()["dims"])
        out["mesh_ms"] = timed(c, mesh)
        out["stats"] = c.obstacle_mesh_stats()
        out["analytic_box_ms"] = timed(c, lambda: c.build_obstacle([capi.Shape.box(centre, half)], cell, bounds))
        out["triangles"] = len(t)
else:
    n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
    spacing = 0.063
    with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
        c.reset_lattice(cfg["lattice"], jitter=True)
        c.step(dt, args.flow_steps)
        nv, nt = c.extract_mesh(capi.mesh_defaults(spacing=1.0 / 15.0))
        c.sync()
        c.build_obstacle_from_mesh(spacing, 3)
        out["dims"] = list(c.obstacle()["dims"])
        out["mesh_ms"] = timed(c, lambda: c.build_obstacle_from_mesh(spacing, 3))
        out["stats"] = c.obstacle_mesh_stats()
        out["analytic_box_ms"] = timed(c, lambda: c.build_obstacle([capi.Shape.box((-11.0, -13.0, -12.0), (0.5, 3.0, 0.5))], spacing))
        out["vertices"], out["triangles"], out["particles"] = nv, nt, n
print(json.dumps(out))

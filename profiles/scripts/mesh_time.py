"""Time of one mesh extraction (sph_mesh_extract) at BASELINE config 3 (16,777,216 particles): the flowing dam (6000 steps from
the lattice).  The defaults (spacing = the particle radius 1/64) give 2057 nodes per axis in the box of edge 32 -- beyond
SPH_MESH_MAX_DIM, so the call is refused (recorded); the extractions timed are the finest lattice the limits allow in that box
(spacing 1/15: 491^3 nodes -- fp32 3.0f * s over s rounds just above 3 there, so the reach is 4 and the pad 5) and a coarse one (spacing 1/8: 265^3), radius and iso at their defaults (three spacings, 0.5): a
particle touches ~113 nodes either way.  Per lattice: one extraction that allocates, then `--reps` extractions with one step of
the simulation between them, each timed as wall time between two synchronisations.  Prints one JSON line with the medians and the
spread.  `--scene box4` is the DEFAULT ratio of spacing to particle spacing instead, on a scene where the defaults are legal:
1,048,576 particles (a 128 x 64 x 128 lattice) in a box of edge 4 with config 3's cell width, 6000 steps, spacing = the particle
radius (265^3 nodes): there a workgroup's 256 cell-sorted particles reach more nodes than the splat's LDS tile holds.
Run from the repo root; once plainly, and once under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/mesh_time.py --lattices spacing_1_15

for the split between k_mesh_splat, k_mesh_count, k_mesh_scan_sums, k_mesh_vbase and k_mesh_generate in OUT/p_kernel_stats.csv.

The splat with every add sent straight to the field (no LDS tile) is a MEASURING build of the library (-DSPH_MESH_PLAIN_SPLAT),
timed the same way on the same box:

    python profiles/scripts/mesh_time.py --build-variant-libs          # no GPU needed: build/libsph_hip_plainsplat.so
    SPH_HIP_LIB=build/libsph_hip_plainsplat.so python profiles/scripts/mesh_time.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")

ap = argparse.ArgumentParser()
ap.add_argument("--build-variant-libs", action="store_true")
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--scene", default="c3", choices=("c3", "box4"))
ap.add_argument("--lattices", default=None, help="which of the lattices, by name (the kernel trace: one)")
args = ap.parse_args()

if args.build_variant_libs:
    from gpufluidsimulator_amd import build as b
    b.build()                                             # the product objects; only sph_mesh.hip depends on the macro
    os.makedirs("build", exist_ok=True)
    objs = [os.path.join(b.CSRC, os.path.splitext(s)[0] + ".o") for s in b.HIP_SOURCES + b.CXX_SOURCES if s != "sph_mesh.hip"]
    obj, lib = os.path.join("build", "sph_mesh_plainsplat.o"), os.path.join("build", "libsph_hip_plainsplat.so")
    subprocess.check_call([b.HIPCC] + b.FLAGS + ["-DSPH_MESH_PLAIN_SPLAT", "-x", "hip", "-c", os.path.join(b.CSRC, "sph_mesh.hip"), "-o", obj])
    subprocess.check_call([b.HIPCC, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + [obj, "-ldl"])
    print(lib)
    sys.exit(0)

import torch  # noqa: E402,F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

from gpufluidsimulator_amd import capi, ic  # noqa: E402

if args.scene == "c3":
    cfg = ic.CONFIGS["C3"]
    LATTICES = {"spacing_1_15": 1.0 / 15.0, "spacing_1_8": 1.0 / 8.0}
else:
    cfg = dict(lattice=(128, 64, 128), box=(4.0, 4.0, 4.0), grid=(64, 64, 64))
    LATTICES = {"defaults": 0.0, "spacing_1_32": 1.0 / 32.0}
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


out = {"scene": args.scene, "particles": n, "flow_steps": args.flow_steps, "reps": args.reps, "lib": os.environ.get("SPH_HIP_LIB", "product")}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, args.flow_steps)
    c.sync()
    try:
        out["at_the_defaults"] = {"dims": c.mesh_lattice()[0]}
    except capi.SphError as e:
        out["at_the_defaults"] = {"refused": str(e)}
    for name in (args.lattices.split(",") if args.lattices else LATTICES):
        s = LATTICES[name]
        mp = capi.mesh_defaults(spacing=s)
        dims, _ = c.mesh_lattice(mp)
        before = capi.memory_stats()[0]
        c.extract_mesh(mp)                                  # allocates
        c.sync()
        ms = []
        for _ in range(args.reps):
            c.step(dt, 1)
            c.sync()
            t0 = time.perf_counter()
            nv, nt = c.extract_mesh(mp)
            c.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        field = c.mesh_field()
        out[name] = {"dims": dims, "nodes": dims[0] * dims[1] * dims[2], "ms": spread(ms), "vertices": nv, "triangles": nt,
                     "device_bytes": capi.memory_stats()[0] - before, "count_max": int(field.max()),
                     "nodes_touched": int((field > 0).sum()), "count_total": int(field.astype("uint64").sum())}
print(json.dumps(out))

"""Time of one surface render (sph_render_surface) next to one sprite render (sph_render) in the same process: the scene and the
camera of profiles/scripts/render_time.py -- BASELINE config 3 (16,777,216 particles), the flowing dam (6000 steps from the
lattice), the reference's view scaled to the box (eye three half-edges back on +z, 60 degrees) -- at 1024x1024 and 1920x1080.
Per size and variant: 20 renders, one step of the simulation between them, each render between a pair of events on the
context's stream.  The variants: sph_render (the yardstick), sph_render_surface at its defaults (r 5, K 2, thickness on), with
the thickness pass off (absorb 0), and with r = 0 (no filter).  Prints one JSON line with the medians, the spread and the ratio
to sph_render.  Run from the repo root; once plainly, and once under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/surface_time.py

for the split between k_surface_splat, k_surface_depth, k_surface_filter and k_surface_shade in OUT/p_kernel_stats.csv.

The thickness in a walk of its own rather than in the walk of the depth keys is a MEASURING build of the library
(-DSPH_SURFACE_SPLIT_WALK), timed the same way:

    python profiles/scripts/surface_time.py --build-variant-libs          # no GPU needed: build/libsph_hip_splitwalk.so
    SPH_HIP_LIB=build/libsph_hip_splitwalk.so python profiles/scripts/surface_time.py
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, ".")
VARIANTS = {"splitwalk": "-DSPH_SURFACE_SPLIT_WALK"}

ap = argparse.ArgumentParser()
ap.add_argument("--build-variant-libs", action="store_true")
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--renders", type=int, default=20)
args = ap.parse_args()

if args.build_variant_libs:
    from gpufluidsimulator_amd import build as b
    b.build()                                             # the product objects; only sph_render.hip depends on the macro
    os.makedirs("build", exist_ok=True)
    objs = [os.path.join(b.CSRC, os.path.splitext(s)[0] + ".o") for s in b.HIP_SOURCES + b.CXX_SOURCES if s != "sph_render.hip"]
    for name, macro in VARIANTS.items():
        obj, lib = os.path.join("build", f"sph_render_{name}.o"), os.path.join("build", f"libsph_hip_{name}.so")
        subprocess.check_call([b.HIPCC] + b.FLAGS + [macro, "-x", "hip", "-c", os.path.join(b.CSRC, "sph_render.hip"), "-o", obj])
        subprocess.check_call([b.HIPCC, "--offload-arch=gfx950", "-shared", "-o", lib] + objs + [obj, "-ldl"])
        print(lib)
    sys.exit(0)

import torch  # noqa: E402  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
half = 0.5 * cfg["box"][0]
SIZES = ((1024, 1024), (1920, 1080))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


out = {"particles": n, "flow_steps": args.flow_steps, "lib": os.environ.get("SPH_HIP_LIB", "product")}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, args.flow_steps)
    c.sync()
    variants = {
        "sph_render": lambda cam: c.render(cam),
        "surface_defaults": lambda cam: c.render_surface(cam),
        "surface_no_thickness": lambda cam: c.render_surface(cam, capi.surface_defaults(absorb=(0.0, 0.0, 0.0))),
        "surface_no_filter": lambda cam: c.render_surface(cam, capi.surface_defaults(smooth_radius_px=0)),
        "surface_r16_K8": lambda cam: c.render_surface(cam, capi.surface_defaults(smooth_radius_px=16, smooth_iterations=8)),
    }
    for w, h in SIZES:
        # the reference's view (eye (0, 0, 3) for its box of edge 2), scaled to this box; far plane behind the box
        cam = capi.look_at(w, h, eye=(0.0, 0.0, 3.0 * half), target=(0.0, 0.0, 0.0), fovy_deg=60.0, near_z=0.1 * half, far_z=100.0 * half)
        for fn in variants.values():                       # allocates the image and the planes
            fn(cam)
        c.sync()
        ms = {name: [] for name in variants}
        for k in range(args.renders):
            for name, fn in variants.items():
                c.step(dt, 1)
                ms[name].append(timed(lambda: fn(cam)))
        c.render_surface(cam)
        _, ident, _ = c.read_image()
        _, thick, _ = c.read_surface()
        base = statistics.median(ms["sph_render"])
        out[f"{w}x{h}"] = {"ms": {name: spread(v) for name, v in ms.items()},
                           "ratio_to_sph_render": {name: round(statistics.median(v) / base, 2) for name, v in ms.items()},
                           "pixels_covered": round(float((ident != 0xFFFFFFFF).mean()), 4),
                           "thickness_counts_total": int(thick.astype("uint64").sum()), "thickness_count_max": int(thick.max())}
print(json.dumps(out))

"""Time of the device renders with the solids drawn (sph_render_set_solids) at BASELINE config 3 (16,777,216 particles), in the
manner of render_time.py: its flowing dam (6000 steps from the lattice) and its view, with a vessel in slot 0 -- the inverted box
of half edge 16.1 about the origin (its walls just outside the box's, so that the fluid never touches it), open, on a grid of
spacing 0.25 -- and a posed wheel in slot 1, a bar turning about z on a local grid.  Per size (1024x1024, 1920x1080) and per renderer (sph_render, sph_render_surface): 20 renders with the solids off and
20 with them on, one step of the simulation between two renders, each render between a pair of events on the context's stream.
Prints one JSON line with the medians and the spread, the share of pixels the solids win, and the share of rays whose march the
fluid's depth bounds (pixels a sprite covers that the solid does not win: sph_render's march leaves at the first free sample at or
behind that depth).  Run from the repo root.

With a library of the commit before the solids the same scene gives the figures to hold `off` against (its launches must be the
same):

    SPH_HIP_LIB=<that libsph_hip.so> SPH_HIP_LIB_ALLOW_MISSING=1 python profiles/scripts/solid_render_time.py --no-solids
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, ".")

ap = argparse.ArgumentParser()
ap.add_argument("--no-solids", action="store_true", help="time the renders without a style only (a library without sph_render_set_solids)")
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--renders", type=int, default=20)
args = ap.parse_args()

import torch  # noqa: E402  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
half = 0.5 * cfg["box"][0]
SIZES = ((1024, 1024), (1920, 1080))
CELL = 0.25


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


out = {"particles": n, "flow_steps": args.flow_steps, "library": os.path.relpath(capi.LIB_PATH)}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.build_obstacle([capi.Shape.box((0.0, 0.0, 0.0), (16.1, 16.1, 16.1), invert=True)], CELL, slot=0)
    c.build_obstacle([capi.Shape.box((0.0, -9.0, 0.0), (7.0, 0.75, 3.0))], CELL, ((-8.0, -17.0, -8.0), (8.0, -1.0, 8.0)), slot=1)
    c.set_obstacle_pose((0.0, -9.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 20.0), slot=1)
    c.step(dt, args.flow_steps)
    c.sync()
    style = None if args.no_solids else capi.solid_defaults(looks={0: dict(open=1), 1: dict(color=(0.85, 0.35, 0.25))})
    renderers = (("sph_render", lambda cam: c.render(cam)), ("sph_render_surface", lambda cam: c.render_surface(cam)))
    for w, h in SIZES:
        cam = capi.look_at(w, h, eye=(0.0, 0.0, 3.0 * half), target=(0.0, 0.0, 0.0), fovy_deg=60.0, near_z=0.1 * half, far_z=100.0 * half)
        row = {}
        for name, render in renderers:
            ids = {}
            for mode in ("off",) if args.no_solids else ("off", "on"):
                if not args.no_solids:
                    c.set_render_solids(style if mode == "on" else None)
                render(cam)                                # allocates the image and the planes
                c.sync()
                ms = []
                for k in range(args.renders):
                    c.step(dt, 1)
                    ms.append(timed(lambda: render(cam)))
                row[f"{name}_{mode}_ms"] = spread(ms)
                ids[mode] = c.read_image()[1]
            if "on" in ids:
                solid = (ids["on"] >= capi.RENDER_ID_SOLID) & (ids["on"] != 0xFFFFFFFF)
                fluid = ids["on"] < capi.RENDER_ID_SOLID
                row[f"{name}_pixels_solid"] = round(float(solid.mean()), 4)
                row[f"{name}_rays_bounded_by_fluid"] = round(float(fluid.mean()), 4)
        out[f"{w}x{h}"] = row
print(json.dumps(out))

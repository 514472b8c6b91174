"""Time of one device render (sph_render) at BASELINE config 3 (16,777,216 particles): the flowing dam (6000 steps from the
lattice), the reference's view scaled to the box (eye three half-edges back on +z, 60 degrees), `index` colouring, at
1024x1024 and 1920x1080.  Per size: 20 renders, one step of the simulation between them, each render between a pair of
events on the context's stream; and, as the yardstick, the step itself in alternating windows of the same process.  Prints
one JSON line with the medians and the spread.  Run from the repo root; once plainly, and once under the kernel trace

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- python profiles/scripts/render_time.py

for the split between k_render_clear, k_render_splat and k_render_resolve in OUT/p_kernel_stats.csv.

The share of fragments that pass the early-out load and reach the atomic comes from a MEASURING build of the library, whose
splat kernel counts them (-DSPH_RENDER_STATS; the product kernel has no counter):

    python profiles/scripts/render_time.py --build-stats-lib            # no GPU needed: build/libsph_hip_stats.so, ..._fresh.so
    SPH_HIP_LIB=build/libsph_hip_stats.so python profiles/scripts/render_time.py --fragments

The same step also builds build/libsph_hip_fresh.so and build/libsph_hip_stats_fresh.so, in which the early-out load is an
agent-scope atomic load that reads past the caches (-DSPH_RENDER_FRESH_LOAD): an experiment, timed and counted the same way.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, ".")
STATS_LIB = os.path.join("build", "libsph_hip_stats.so")

ap = argparse.ArgumentParser()
ap.add_argument("--build-stats-lib", action="store_true")
ap.add_argument("--fragments", action="store_true")
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--renders", type=int, default=20)
args = ap.parse_args()

if args.build_stats_lib:
    from gpufluidsimulator_amd import build as b
    b.build()                                             # the product objects; only sph_render.hip depends on the macro
    os.makedirs("build", exist_ok=True)
    objs = [os.path.join(b.CSRC, os.path.splitext(s)[0] + ".o") for s in b.HIP_SOURCES + b.CXX_SOURCES if s != "sph_render.hip"]
    for name, macros in (("stats", ["-DSPH_RENDER_STATS"]), ("fresh", ["-DSPH_RENDER_FRESH_LOAD"]),
                         ("stats_fresh", ["-DSPH_RENDER_STATS", "-DSPH_RENDER_FRESH_LOAD"])):
        obj = os.path.join("build", f"sph_render_{name}.o")
        subprocess.check_call([b.HIPCC] + b.FLAGS + macros + ["-x", "hip", "-c", os.path.join(b.CSRC, "sph_render.hip"), "-o", obj])
        subprocess.check_call([b.HIPCC, "--offload-arch=gfx950", "-shared", "-o", os.path.join("build", f"libsph_hip_{name}.so")] + objs + [obj, "-ldl"])
    print(STATS_LIB)
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


out = {"particles": n, "flow_steps": args.flow_steps}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.step(dt, args.flow_steps)
    c.sync()
    for w, h in SIZES:
        # the reference's view (eye (0, 0, 3) for its box of edge 2), scaled to this box; far plane behind the box
        cam = capi.look_at(w, h, eye=(0.0, 0.0, 3.0 * half), target=(0.0, 0.0, 0.0), fovy_deg=60.0, near_z=0.1 * half, far_z=100.0 * half)
        c.render(cam)                                      # allocates the image
        c.sync()
        if args.fragments:
            stats = (ctypes.c_uint64 * 2)()
            fn = c.L.sph_render_stats
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
            assert fn(c.h, stats) == 0                     # drop the counts of the warm-up render
            c.render(cam)
            assert fn(c.h, stats) == 0
            _, ident, _ = c.read_image()
            out[f"{w}x{h}"] = {"fragments_covered": int(stats[0]), "fragments_to_atomic": int(stats[1]),
                               "share_to_atomic": round(stats[1] / max(stats[0], 1), 5),
                               "pixels_covered": round(float((ident != 0xFFFFFFFF).mean()), 4)}
            continue
        render_ms, step_ms = [], []
        for k in range(args.renders):
            step_ms.append(timed(lambda: c.step(dt, 1)))
            render_ms.append(timed(lambda: c.render(cam)))
        _, ident, _ = c.read_image()
        out[f"{w}x{h}"] = {"render_ms": spread(render_ms), "step_ms_between_renders": spread(step_ms),
                           "pixels_covered": round(float((ident != 0xFFFFFFFF).mean()), 4)}
    if not args.fragments:                                 # the step on its own: windows that alternate with render windows
        alone, with_render = [], []
        cam = capi.look_at(1024, 1024, eye=(0.0, 0.0, 3.0 * half), target=(0.0, 0.0, 0.0), fovy_deg=60.0, near_z=0.1 * half, far_z=100.0 * half)
        c.render(cam)
        c.sync()

        def steps_and_renders():
            for _ in range(20):
                c.step(dt, 1)
                c.render(cam)
        for k in range(6):
            alone.append(timed(lambda: c.step(dt, 20)) / 20)
            with_render.append(timed(steps_and_renders) / 20)
        out["step_ms_windows"] = {"step_alone": spread(alone), "step_plus_render_1024": spread(with_render)}
print(json.dumps(out))

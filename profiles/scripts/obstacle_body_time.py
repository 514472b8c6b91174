"""Time per step of a wheel the fluid drives, at BASELINE config 3 (16,777,216 particles): the flowing dam, the vessel (slot 0)
and the wheel (slot 1) of solid_render_time.py, in ONE context, three ways of running the wheel, interleaved round by round so
that drift of the machine falls on all three alike (the measuring guide):

    (a) kinematic and sensing: sph_step(dt, K) -- the path of the commit before the bodies, unchanged
    (b) the same wheel as a HINGE body (sph_obstacle_set_body): sph_step(dt, K), the fluid drives it on the device
    (c) driven from the host: K times sph_step(dt, 1), sph_obstacle_get_load (a synchronisation), the hinge's scalar equation
        and the Cayley step in numpy, sph_obstacle_set_pose

Each sample is the wall clock of K steps between two synchronisations, divided by K.  Prints one JSON line with the medians and
the spread of the three.  Run from the repo root."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")

ap = argparse.ArgumentParser()
ap.add_argument("--flow-steps", type=int, default=6000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=40, help="K: steps per sample")
args = ap.parse_args()

import torch  # noqa: E402  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

from gpufluidsimulator_amd import capi, ic  # noqa: E402

cfg = ic.CONFIGS["C3"]
n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
dt = float(ic.DEFAULT_DT)
CELL = 0.25
PIVOT, AXIS, INERTIA = (0.0, -9.0, 0.0), (0.0, 0.0, 1.0), 5.0e7
K = args.steps


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def sample(c, work):
    c.sync()
    t0 = time.perf_counter()
    work()
    c.sync()
    return (time.perf_counter() - t0) * 1e3 / K


def host_driven(c):
    """the loop the header used to point a caller to: read the load, move the wheel, set the pose, every step"""
    ps = c.obstacle_pose(slot=1)
    q, w = ps["quat"].copy(), float(ps["omega"][2])
    for _ in range(K):
        c.step(dt, 1)
        w += float(c.obstacle_load(slot=1)["L"][2]) / INERTIA
        a = 0.5 * dt * w
        q = np.array([q[0] - a * q[3], q[1] + a * q[2], q[2] - a * q[1], q[3] + a * q[0]])
        q /= np.sqrt(q @ q)
        c.set_obstacle_pose(PIVOT, q, (0.0, 0.0, w), slot=1)


out = {"particles": n, "flow_steps": args.flow_steps, "rounds": args.rounds, "steps_per_sample": K, "library": os.path.relpath(capi.LIB_PATH)}
ms = {"kinematic_sensing": [], "hinge_body": [], "host_driven": []}
with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
    c.reset_lattice(cfg["lattice"], jitter=True)
    c.build_obstacle([capi.Shape.box((0.0, 0.0, 0.0), (16.1, 16.1, 16.1), invert=True)], CELL, slot=0)
    c.build_obstacle([capi.Shape.box((0.0, -9.0, 0.0), (7.0, 0.75, 3.0))], CELL, ((-8.0, -17.0, -8.0), (8.0, -1.0, 8.0)), slot=1)
    c.set_obstacle_pose(PIVOT, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 20.0), slot=1)
    c.set_obstacle_sensor(True, slot=1)
    c.step(dt, args.flow_steps)
    for r in range(args.rounds + 1):                       # (round 0 warms the three paths up and is not kept)
        got = {}
        got["kinematic_sensing"] = sample(c, lambda: c.step(dt, K))
        c.set_obstacle_body(slot=1, dof=capi.BODY_HINGE, inertia=(INERTIA, 0.0, 0.0), axis=AXIS)
        got["hinge_body"] = sample(c, lambda: c.step(dt, K))
        c.set_obstacle_body(None, slot=1)                  # kinematic again, from where the fluid left it
        got["host_driven"] = sample(c, lambda: host_driven(c))
        if r:
            for k, v in got.items():
                ms[k].append(v)
    out["omega_z_at_the_end"] = round(float(c.obstacle_pose(slot=1)["omega"][2]), 4)
for k, v in ms.items():
    out[k + "_ms_per_step"] = spread(v)
print(json.dumps(out))

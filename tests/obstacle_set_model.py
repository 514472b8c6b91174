"""numpy model of SEVERAL OBSTACLES (include/sph_hip.h: sph_obstacle_select and the section around it): the installed slots act
in ascending slot order, slot j on what slot j - 1 left, each by the rule of its kind -- tests/obstacle_model.py for an unposed
slot, tests/obstacle_pose_model.py for a posed one, both through obstacle_pose_model.push (ps None is the unposed rule) --, each
with its own wall rule, its own load (obstacle_pose_model.load_in_order) and its own advance.  Nothing here is new arithmetic:
the chain is the point."""
import numpy as np

import obstacle_model as om
import obstacle_pose_model as pm
from collider_body_model import WAVE

F = np.float32
MAX_OBSTACLES = 4
BRICK = 4                                          # cells per brick edge (csrc/sph_obstacle.hip: OBSTACLE_BRICK)
ZERO = (0.0, 0.0, 0.0)


def slot(grid, phi, off=ZERO, u=ZERO, pose=None):
    """One slot as the model passes it around; pose: obstacle_pose_model.pose(...) or None (unposed)."""
    return {"grid": grid, "phi": np.asarray(phi, F), "off": np.array(off, F), "u": np.array(u, F), "pose": pose}


def push(pos, vel, slots, box_min, box_max, eps=F(1e-5), damp=F(-0.75), mass=F(65.0)):
    """Every particle through the slots of `slots` ({k: slot}) in ascending k.  Returns (pos, vel, touched by any slot,
    {k: stats}); stats of a slot: "touched", "iterations", "kicked", "lane" (obstacle_pose_model.push) and "before", the positions
    that slot started from."""
    pos, vel = np.array(pos, F), np.array(vel, F)
    any_touched = np.zeros(pos.shape[0], bool)
    stats = {}
    for k in sorted(slots):
        assert 0 <= k < MAX_OBSTACLES
        sl, st = slots[k], {}
        st["before"] = pos.copy()
        pos, vel, touched = pm.push(pos, vel, sl["grid"], sl["phi"], sl["off"], sl["u"], sl["pose"], box_min, box_max, eps, damp, mass,
                                    stats=st)
        st["touched"] = touched
        any_touched |= touched
        stats[k] = st
    return pos, vel, any_touched, stats


def load(st, n):
    """(J, L) float64 of one slot's stats, in the device's order."""
    return pm.load_in_order(st["lane"], st["kicked"], n)


def advance(slots, dt, steps=1):
    """The slots after `steps` steps: every offset by obstacle_model.advance, every pose by obstacle_pose_model.advance."""
    out = {}
    for k, sl in slots.items():
        if sl["pose"] is None:
            out[k] = dict(sl, off=om.advance(sl["off"], sl["u"], dt, steps))
        else:
            ps, off = pm.advance(sl["pose"], sl["off"], sl["u"], dt, steps)
            out[k] = dict(sl, off=off, pose=ps)
    return out


# ---- the brick guard of csrc/sph_obstacle.hip, for choosing scenes (the model above needs none) ----------------------------------
def brick_minima(phi):
    """(nb_z, nb_y, nb_x): the minimum over the nodes [4 b, 4 b + 4] of every brick, clipped to the lattice"""
    nz, ny, nx = phi.shape
    nb = [-(-(n - 1) // BRICK) for n in (nz, ny, nx)]
    out = np.empty(nb, F)
    for k in range(nb[0]):
        for j in range(nb[1]):
            for i in range(nb[2]):
                out[k, j, i] = phi[4 * k:4 * k + 5, 4 * j:4 * j + 5, 4 * i:4 * i + 5].min()
    return out


def may_touch(sl, pos, eps=F(1e-5)):
    """(n,) bool: the particle is inside the slot's lattice and its brick's minimum is under the guard eps + 0.25 s -- what the
    push kernels look up before they sample.  The cell is the one the sample rule finds (posed: of the body-frame point)."""
    pos = np.asarray(pos, F)
    grid, ps = sl["grid"], sl["pose"]
    if ps is None:
        q, off = pos, sl["off"]
    else:
        P = pm.world_pivot(ps, sl["off"])
        d = (pos - P).astype(F)
        R, piv = pm.rot_of(ps["q"]), ps["pivot"]
        q = np.stack([((R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2]) + piv[k] for k in range(3)], axis=1).astype(F)
        off = np.zeros(3, F)
    o, s = np.asarray(grid["origin"], F), F(grid["spacing"])
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.stack([(((q[:, k] - off[k]) - o[k]) / s).astype(F) for k in range(3)], 1)
        inside = np.all((g >= 0) & (g < (np.array(grid["dims"], F) - F(1))), axis=1)
    out = np.zeros(pos.shape[0], bool)
    b = g[inside].astype(np.int64) // BRICK
    low = brick_minima(sl["phi"])
    guard = F(F(eps) + F(0.25) * s)
    out[inside] = low[b[:, 2], b[:, 1], b[:, 0]] < guard
    return out


def classes(pos, slots, stats, a, b, eps=F(1e-5)):
    """The particles of a pass by what slots a < b did to them: {"a_only", "b_only", "both", "none", "stale"} -> (n,) bool.
    "stale": slot a moved the particle, slot b then hit it, and at the position the pass STARTED from slot b's guard said "cannot
    touch" -- a kernel that keeps the first look-up leaves such a particle inside solid b."""
    ta, tb = stats[a]["touched"], stats[b]["touched"]
    hit_any = np.zeros(pos.shape[0], bool)
    for st in stats.values():
        hit_any |= st["touched"]
    return {"a_only": ta & ~tb, "b_only": tb & ~ta, "both": ta & tb, "none": ~hit_any,
            "stale": ta & tb & ~may_touch(slots[b], pos, eps)}


def waves_of(mask):
    return np.unique(np.nonzero(mask)[0] // WAVE)

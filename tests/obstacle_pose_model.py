"""numpy model of the posed obstacle and its load sensor (include/sph_hip.h: sph_obstacle_set_pose, sph_obstacle_set_sensor and
the calls next to them), on top of tests/obstacle_model.py: the quaternion's set, step and matrix in float64 with the header's
parentheses (python floats: one rounding per operation, no fusion, no sin or cos), the posed sample and push in float32, one
rounding per operation, and the load's terms with their sum in the order the header fixes -- iterations of a lane, kicked lanes
of a wave ascending, waves within runs of collider_body_model.run_length(n), the runs that hold a row ascending."""
import numpy as np

import obstacle_model as om
from collider_body_model import SUM_THREADS, WAVE, run_length
from collider_model import wall

F = np.float32
D = np.float64
ZERO = np.zeros(3, F)


# ---- the host state --------------------------------------------------------------------------------------------------------------
def _unit(q):
    w, x, y, z = (float(v) for v in q)
    n2 = ((w * w + x * x) + y * y) + z * z
    if not (n2 > 0.0) or not np.isfinite(n2):
        return None
    ln = float(np.sqrt(D(n2)))
    return np.array([w / ln, x / ln, y / ln, z / ln], D)


def quat_set(quat):
    """The unit quaternion (float64) the library keeps of a caller's float32 (w, x, y, z); None where it refuses."""
    return _unit(np.asarray(quat, F).astype(D))


def quat_step(q, omega, dt):
    """One Cayley step of dt (float32) with omega (float32, world axes)."""
    w, x, y, z = (float(v) for v in q)
    h = 0.5 * float(F(dt))
    a0, a1, a2 = (h * float(F(v)) for v in omega)
    return _unit((((w - a0 * x) - a1 * y) - a2 * z, ((x + a0 * w) + a1 * z) - a2 * y, ((y + a1 * w) + a2 * x) - a0 * z,
                  ((z + a2 * w) + a0 * y) - a1 * x))


def rot_of(q):
    """rot (3, 3) float32, body -> world: float64 as the header writes it, each entry rounded once."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], D).astype(F)


def pose(pivot, quat, omega=(0.0, 0.0, 0.0)):
    """A pose as the model passes it around: {"pivot" float32, "q" float64 unit, "omega" float32}."""
    return {"pivot": np.array(pivot, F), "q": quat_set(quat), "omega": np.array(omega, F)}


def advance(ps, off, u, dt, steps=1):
    """(pose, offset) after `steps` steps: the offset as obstacle_model.advance, the quaternion by quat_step."""
    q = ps["q"]
    for _ in range(steps):
        q = quat_step(q, ps["omega"], dt)
    return dict(ps, q=q), om.advance(off, u, dt, steps)


def world_pivot(ps, off):
    """P = pivot + off in float32; an unposed context (ps None): off."""
    off = np.asarray(off, F)
    return off.copy() if ps is None else (ps["pivot"] + off).astype(F)


# ---- the device rule ---------------------------------------------------------------------------------------------------------------
def sample(grid, phi, off, ps, points):
    """(phi (n,), WORLD normal (n, 3), inside (n,), d (n, 3)) at world points; ps None: the unposed rule (d = x - off)."""
    pts = np.asarray(points, F).reshape(-1, 3)
    P = world_pivot(ps, off)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (pts - P).astype(F)
        if ps is None:
            ph, nb, ins = om.sample(grid, phi, off, pts)
            return ph, nb, ins, d
        R, piv = rot_of(ps["q"]), ps["pivot"]
        q = np.stack([((R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2]) + piv[k] for k in range(3)], axis=1).astype(F)
        ph, nb, ins = om.sample(grid, phi, ZERO, q)                 # (q - 0 is q to the bit: the body-frame sample)
        nw = np.stack([(R[k, 0] * nb[:, 0] + R[k, 1] * nb[:, 1]) + R[k, 2] * nb[:, 2] for k in range(3)], axis=1).astype(F)
    nw[~ins] = 0
    return ph, nw, ins, d


def push(pos, vel, grid, phi, off, u, ps, box_min, box_max, eps=F(1e-5), damp=F(-0.75), mass=F(65.0), stats=None):
    """Every particle through the push of a posed (ps None: unposed) context: new pos, vel and the touched mask.  `stats`
    receives "iterations" (n,), "kicked" (n,) bool and "lane" (n, 6) float64: each particle's own sums of t and d x t over its
    iterations in order, from 0.0 (what a lane hands to its wave)."""
    pos, vel = np.array(pos, F), np.array(vel, F)
    u, eps, damp, mass = np.asarray(u, F), F(eps), F(damp), F(mass)
    om3 = ZERO if ps is None else ps["omega"]
    n = pos.shape[0]
    active = np.ones(n, bool)
    touched, kicked = np.zeros(n, bool), np.zeros(n, bool)
    iters = np.zeros(n, np.int32)
    lane = np.zeros((n, 6), D)
    for _ in range(om.ITERATIONS):
        idx = np.nonzero(active)[0]
        ph, nr, ins, d = sample(grid, phi, off, ps, pos[idx])
        go = ins & (ph < eps)
        active[idx[~go]] = False
        j = idx[go]
        if j.size == 0:
            break
        nr, ph, d, v, x = nr[go], ph[go], d[go], vel[j], pos[j]
        if ps is None:
            us = np.broadcast_to(u, v.shape)
        else:
            us = np.stack([u[0] + (om3[1] * d[:, 2] - om3[2] * d[:, 1]), u[1] + (om3[2] * d[:, 0] - om3[0] * d[:, 2]),
                           u[2] + (om3[0] * d[:, 1] - om3[1] * d[:, 0])], axis=1).astype(F)
        wn = ((v[:, 0] - us[:, 0]) * nr[:, 0] + (v[:, 1] - us[:, 1]) * nr[:, 1]) + (v[:, 2] - us[:, 2]) * nr[:, 2]
        kn = (((damp - F(1)) * wn)[:, None] * nr).astype(F)
        kick = wn < 0
        vel[j] = np.where(kick[:, None], v + kn, v)
        t = (-(mass * kn)).astype(F)
        td, dd = t.astype(D), d.astype(D)
        tau = np.stack([dd[:, 1] * td[:, 2] - dd[:, 2] * td[:, 1], dd[:, 2] * td[:, 0] - dd[:, 0] * td[:, 2],
                        dd[:, 0] * td[:, 1] - dd[:, 1] * td[:, 0]], axis=1)
        jk = j[kick]
        lane[jk] = lane[jk] + np.concatenate([td, tau], axis=1)[kick]
        kicked[jk] = True
        pos[j] = x + (eps - ph)[:, None] * nr
        touched[j] = True
        iters[j] += 1
    for i in np.nonzero(touched)[0]:
        for a in range(3):
            pos[i, a], vel[i, a] = wall(pos[i, a], vel[i, a], F(box_min[a]), F(box_max[a]), eps, damp)
    if stats is not None:
        stats.update(iterations=iters, kicked=kicked, lane=lane)
    assert pos.dtype == F and vel.dtype == F
    return pos, vel, touched


def load_in_order(lane, kicked, n, runs_descending=False):
    """(J (3,), L (3,)) float64 of the lanes' sums (n, 6) and kicked (n,), both in SLOT order, in the header's order: a wave's
    row is the sum from 0.0 of its kicked lanes ascending; run t = the waves [t K, (t + 1) K) adds its rows ascending from 0.0;
    the runs that hold a row are added ascending from 0.0 (collider_body_model.thread_sums with six columns).
    runs_descending: NOT the device's order -- for showing that the order can be seen."""
    lane, kicked, n = np.asarray(lane, D), np.asarray(kicked, bool), int(n)
    assert lane.shape == (n, 6) and kicked.shape == (n,)
    K = run_length(n)
    acc = np.zeros((SUM_THREADS, 6), D)
    found = np.zeros(SUM_THREADS, bool)
    for w in np.unique(np.nonzero(kicked)[0] // WAVE):
        lo, hi = int(w) * WAVE, min((int(w) + 1) * WAVE, n)
        row = np.zeros(6, D)
        for l in np.nonzero(kicked[lo:hi])[0]:
            row = row + lane[lo + l]
        t = int(w) // K
        assert t < SUM_THREADS
        acc[t] = acc[t] + row
        found[t] = True
    out = np.zeros(6, D)
    order = np.nonzero(found)[0]
    for t in (order[::-1] if runs_descending else order):
        out = out + acc[t]
    return out[:3], out[3:]

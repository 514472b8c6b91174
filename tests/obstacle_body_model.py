"""numpy model of a free obstacle body (include/sph_hip.h: THE BODY, sph_obstacle_set_body), on top of
tests/obstacle_pose_model.py: THE BODY STEP in python floats (float64, one rounding per operation, no fusion, sums left to right,
only + - * / sqrt) with the fp32 parts in numpy float32, one rounding per operation.  A state is what the device block holds:
{"off", "u", "pivot", "omega" float32 (3,), "q" float64 (4,) unit}; rot and P follow from it (rot_of, world_pivot)."""
import numpy as np

import obstacle_pose_model as pm
from collider_model import wall

F = np.float32
D = np.float64
FREE_X, FREE_Y, FREE_Z, SPIN, HINGE = 1, 2, 4, 8, 16
FREE_XYZ = FREE_X | FREE_Y | FREE_Z
ZERO3 = (0.0, 0.0, 0.0)


def body(dof=0, mass=0.0, inertia=ZERO3, axis=ZERO3, accel=ZERO3, torque=ZERO3, lo=ZERO3, hi=ZERO3):
    """The parameters as sph_obstacle_body holds them (float32)."""
    f3 = lambda v: np.array(v, F)
    return {"dof": int(dof), "mass": F(mass), "inertia": f3(inertia), "axis": f3(axis), "accel": f3(accel), "torque": f3(torque),
            "lo": f3(lo), "hi": f3(hi)}


def state(off, u, pivot, quat, omega):
    """The block of a slot whose motion and pose were just set (quat: the caller's float32 (w, x, y, z))."""
    return {"off": np.array(off, F), "u": np.array(u, F), "pivot": np.array(pivot, F), "omega": np.array(omega, F),
            "q": pm.quat_set(quat)}


def pose_of(st):
    """The state's pose as obstacle_pose_model passes it around."""
    return {"pivot": st["pivot"], "q": st["q"], "omega": st["omega"]}


def unit_axis(axis):
    """axis / |axis| in float64, as the host normalises it."""
    x, y, z = (float(F(v)) for v in axis)
    ln = float(np.sqrt(D((x * x + y * y) + z * z)))
    return x / ln, y / ln, z / ln


def rot_exact(q):
    """The nine float64 expressions of rot before their rounding (python floats, row-major rows)."""
    w, x, y, z = (float(v) for v in q)
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]


def step(st, bd, J, L, dt, damp=F(-0.75)):
    """The state after one body step with the load (J, L) (float64) of that integrate."""
    dt32, damp = F(dt), F(damp)
    ddt = float(dt32)
    off, u = st["off"].copy(), st["u"].copy()
    for a in range(3):
        if bd["dof"] & (1 << a):
            u[a] = F((float(u[a]) + float(J[a]) / float(bd["mass"])) + ddt * float(bd["accel"][a]))
            off[a], u[a] = wall(off[a], u[a], bd["lo"][a], bd["hi"][a], F(0), damp)
        off[a] = F(off[a] + F(dt32 * u[a]))
    T = [float(L[k]) + ddt * float(bd["torque"][k]) for k in range(3)]
    w = [float(v) for v in st["omega"]]
    omega = st["omega"].copy()
    if bd["dof"] & HINGE:
        e = unit_axis(bd["axis"])
        s = ((w[0] * e[0] + w[1] * e[1]) + w[2] * e[2]) + ((T[0] * e[0] + T[1] * e[1]) + T[2] * e[2]) / float(bd["inertia"][0])
        omega = np.array([s * e[0], s * e[1], s * e[2]], D).astype(F)
    elif bd["dof"] & SPIN:
        R = rot_exact(st["q"])
        I = [float(v) for v in bd["inertia"]]
        wb = [(R[0][k] * w[0] + R[1][k] * w[1]) + R[2][k] * w[2] for k in range(3)]
        Tb = [(R[0][k] * T[0] + R[1][k] * T[1]) + R[2][k] * T[2] for k in range(3)]
        h = [I[k] * wb[k] for k in range(3)]
        g = [wb[1] * h[2] - wb[2] * h[1], wb[2] * h[0] - wb[0] * h[2], wb[0] * h[1] - wb[1] * h[0]]
        wn = [wb[k] + (Tb[k] - ddt * g[k]) / I[k] for k in range(3)]
        omega = np.array([(R[k][0] * wn[0] + R[k][1] * wn[1]) + R[k][2] * wn[2] for k in range(3)], D).astype(F)
    q = pm.quat_step(st["q"], omega, dt32)
    return {"off": off, "u": u, "pivot": st["pivot"].copy(), "omega": omega, "q": st["q"].copy() if q is None else q}


def rot_of(st):
    return pm.rot_of(st["q"])


def world_pivot(st):
    return (st["pivot"] + st["off"]).astype(F)

"""numpy model of the obstacle rule of include/sph_hip.h (sph_obstacle_build and the calls next to it): the lattice of a build,
the rasterised shapes, the trilinear sample and the push that follows every integrate.  float32 throughout, one rounding per
operation, no multiply-add fusion, sums left to right: the order of the header's pseudo-code.  The model samples EVERY particle:
it knows nothing of the bricks the kernel skips work with."""
import numpy as np

from collider_model import wall

F = np.float32
SPHERE, BOX, CAPSULE, HALFSPACE = 0, 1, 2, 3
ITERATIONS = 4


def sphere(center, radius, invert=False):
    return {"kind": SPHERE, "invert": bool(invert), "a": np.array(center, F), "b": np.zeros(3, F), "r": F(radius)}


def box(center, half_extents, rounding=0.0, invert=False):
    return {"kind": BOX, "invert": bool(invert), "a": np.array(center, F), "b": np.array(half_extents, F), "r": F(rounding)}


def capsule(end_a, end_b, radius, invert=False):
    return {"kind": CAPSULE, "invert": bool(invert), "a": np.array(end_a, F), "b": np.array(end_b, F), "r": F(radius)}


def halfspace(point, normal, invert=False):
    """Solid on the side the normal points away from; the normal is normalised in float64 and rounded once."""
    return {"kind": HALFSPACE, "invert": bool(invert), "a": np.array(point, F), "b": np.array(normal, F), "r": F(0)}


def unit_normal(b):
    bd = np.asarray(b, F).astype(np.float64)
    ln = np.sqrt(bd[0] * bd[0] + bd[1] * bd[1] + bd[2] * bd[2])
    return (bd / ln).astype(F)


def lattice(spacing, lo, hi, particle_radius=F(1.0 / 64.0)):
    """The lattice of a build over the bounds [lo, hi]: float64, each result rounded once; the origin in float32."""
    s = F(spacing) if float(spacing) > 0 else F(2.0 * float(F(particle_radius)))
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    dims = tuple(int(np.ceil((float(hi[k]) - float(lo[k])) / float(s))) + 3 for k in range(3))
    return {"dims": dims, "origin": (lo - s).astype(F), "spacing": s}


def clamp_distance(grid):
    return F(grid["spacing"] * F(sum(grid["dims"])))


def node_positions(grid):
    """(px (n_x,), py (n_y,), pz (n_z,)): origin + (float)i * s."""
    s, o = F(grid["spacing"]), np.asarray(grid["origin"], F)
    return tuple((o[k] + np.arange(grid["dims"][k], dtype=F) * s).astype(F) for k in range(3))


def _shape_phi(sh, px, py, pz):
    a, b, r = sh["a"], sh["b"], F(sh["r"])
    if sh["kind"] == SPHERE:
        dx, dy, dz = px - a[0], py - a[1], pz - a[2]
        phi = np.sqrt((dx * dx + dy * dy) + dz * dz) - r
    elif sh["kind"] == BOX:
        qx, qy, qz = np.abs(px - a[0]) - b[0], np.abs(py - a[1]) - b[1], np.abs(pz - a[2]) - b[2]
        ox, oy, oz = np.maximum(qx, F(0)), np.maximum(qy, F(0)), np.maximum(qz, F(0))
        phi = (np.sqrt((ox * ox + oy * oy) + oz * oz) + np.minimum(np.maximum(qx, np.maximum(qy, qz)), F(0))) - r
    elif sh["kind"] == CAPSULE:
        pax, pay, paz = px - a[0], py - a[1], pz - a[2]
        bax, bay, baz = F(b[0] - a[0]), F(b[1] - a[1]), F(b[2] - a[2])
        t = ((pax * bax + pay * bay) + paz * baz) / F(F(bax * bax + bay * bay) + baz * baz)
        t = np.minimum(np.maximum(t, F(0)), F(1))
        dx, dy, dz = pax - t * bax, pay - t * bay, paz - t * baz
        phi = np.sqrt((dx * dx + dy * dy) + dz * dz) - r
    elif sh["kind"] == HALFSPACE:
        n = unit_normal(b)
        phi = ((px - a[0]) * n[0] + (py - a[1]) * n[1]) + (pz - a[2]) * n[2]
    else:
        raise ValueError(sh["kind"])
    phi = phi.astype(F)
    return -phi if sh["invert"] else phi


def rasterise(shapes, grid):
    """phi of shape (n_z, n_y, n_x): the union (minimum, in order) of the shapes at every node, clamped to [-D, D]."""
    x, y, z = node_positions(grid)
    px, py, pz = x[None, None, :], y[None, :, None], z[:, None, None]
    full = (grid["dims"][2], grid["dims"][1], grid["dims"][0])
    v = None
    for sh in shapes:
        p = np.broadcast_to(_shape_phi(sh, px, py, pz), full)
        v = p if v is None else np.minimum(v, p)
    D = clamp_distance(grid)
    return np.minimum(np.maximum(v, -D), D).astype(F)


def clamp(phi, grid):
    D = clamp_distance(grid)
    return np.minimum(np.maximum(np.asarray(phi, F), -D), D).astype(F)


def _lerp(p, q, t):
    return p + t * (q - p)


def sample(grid, phi, off, points):
    """(phi (n,), normal (n, 3), inside (n,) bool) at the points; +inf and a zero normal outside the grid."""
    pts = np.asarray(points, F).reshape(-1, 3)
    off, o, s = np.asarray(off, F), np.asarray(grid["origin"], F), F(grid["spacing"])
    n = pts.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        g = [(((pts[:, k] - off[k]) - o[k]) / s).astype(F) for k in range(3)]
        inside = np.ones(n, bool)
        for k in range(3):
            inside &= (g[k] >= F(0)) & (g[k] < F(grid["dims"][k] - 1))
    out_phi = np.full(n, np.inf, F)
    out_n = np.zeros((n, 3), F)
    j = np.nonzero(inside)[0]
    if j.size == 0:
        return out_phi, out_n, inside
    i = [g[k][j].astype(np.int32) for k in range(3)]
    fx, fy, fz = (g[k][j] - i[k].astype(F) for k in range(3))
    P = lambda a, b, c: phi[i[2] + c, i[1] + b, i[0] + a]
    P000, P100, P010, P110 = P(0, 0, 0), P(1, 0, 0), P(0, 1, 0), P(1, 1, 0)
    P001, P101, P011, P111 = P(0, 0, 1), P(1, 0, 1), P(0, 1, 1), P(1, 1, 1)
    ph = _lerp(_lerp(_lerp(P000, P100, fx), _lerp(P010, P110, fx), fy),
               _lerp(_lerp(P001, P101, fx), _lerp(P011, P111, fx), fy), fz)
    gx = _lerp(_lerp(P100 - P000, P110 - P010, fy), _lerp(P101 - P001, P111 - P011, fy), fz)
    gy = _lerp(_lerp(P010 - P000, P110 - P100, fx), _lerp(P011 - P001, P111 - P101, fx), fz)
    gz = _lerp(_lerp(P001 - P000, P101 - P100, fx), _lerp(P011 - P010, P111 - P110, fx), fy)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        len2 = (gx * gx + gy * gy) + gz * gz
        ok = np.isfinite(len2) & (len2 > 0)
        ln = np.sqrt(np.where(ok, len2, F(1)))
        nrm = np.stack([np.where(ok, gx / ln, F(0)), np.where(ok, gy / ln, F(1)), np.where(ok, gz / ln, F(0))], axis=1)
    assert ph.dtype == F and nrm.dtype == F
    out_phi[j] = ph
    out_n[j] = nrm
    return out_phi, out_n, inside


def push(pos, vel, grid, phi, off, u, box_min, box_max, eps=F(1e-5), damp=F(-0.75), stats=None):
    """Every particle through the push: (n, 3) float32 arrays -> new pos, vel and the mask of the particles the obstacle moved.
    `stats` (a dict) receives "iterations": how many times each particle was pushed."""
    pos, vel = np.array(pos, F), np.array(vel, F)
    u, eps, damp = np.asarray(u, F), F(eps), F(damp)
    n = pos.shape[0]
    active = np.ones(n, bool)
    touched = np.zeros(n, bool)
    iters = np.zeros(n, np.int32)
    for _ in range(ITERATIONS):
        idx = np.nonzero(active)[0]
        ph, nr, ins = sample(grid, phi, off, pos[idx])
        go = ins & (ph < eps)
        active[idx[~go]] = False
        j = idx[go]
        if j.size == 0:
            break
        nr, ph, v, x = nr[go], ph[go], vel[j], pos[j]
        wn = ((v[:, 0] - u[0]) * nr[:, 0] + (v[:, 1] - u[1]) * nr[:, 1]) + (v[:, 2] - u[2]) * nr[:, 2]
        k = (damp - F(1)) * wn
        vel[j] = np.where((wn < 0)[:, None], v + k[:, None] * nr, v)
        t = eps - ph
        pos[j] = x + t[:, None] * nr
        touched[j] = True
        iters[j] += 1
    for i in np.nonzero(touched)[0]:
        for a in range(3):
            pos[i, a], vel[i, a] = wall(pos[i, a], vel[i, a], F(box_min[a]), F(box_max[a]), eps, damp)
    if stats is not None:
        stats["iterations"] = iters
    assert pos.dtype == F and vel.dtype == F
    return pos, vel, touched


def advance(off, u, dt, steps):
    """The offset after `steps` steps: off = off + dt * u in float32, once per step."""
    off, u, dt = np.array(off, F), np.asarray(u, F), F(dt)
    for _ in range(steps):
        off = (off + dt * u).astype(F)
    return off


# ---- float64 distances of the same shapes (for the CPU tests: what the float32 arithmetic is held to) ----
def analytic(sh, p):
    """Signed distance in float64 of the points p (n, 3) to one shape (its float32 fields taken as they are)."""
    p = np.asarray(p, np.float64)
    a, b, r = sh["a"].astype(np.float64), sh["b"].astype(np.float64), float(sh["r"])
    if sh["kind"] == SPHERE:
        phi = np.linalg.norm(p - a, axis=1) - r
    elif sh["kind"] == BOX:
        q = np.abs(p - a) - b
        phi = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0) - r
    elif sh["kind"] == CAPSULE:
        pa, ba = p - a, b - a
        t = np.clip(pa @ ba / (ba @ ba), 0, 1)
        phi = np.linalg.norm(pa - t[:, None] * ba, axis=1) - r
    else:
        phi = (p - a) @ unit_normal(sh["b"]).astype(np.float64)
    return -phi if sh["invert"] else phi

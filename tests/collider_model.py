"""numpy model of the sphere-collider rule of include/sph_hip.h (sph_set_colliders), applied after the integrate and the
wall rule.  float32 throughout, one rounding per operation, sums left to right: the order of the header's pseudo-code."""
import numpy as np

F = np.float32


def wall(x, v, lo, hi, eps, damp):
    """The wall rule of one axis (csrc/sph_pairs.hip: wall): lower wall first."""
    if x - eps < lo:
        x, v = F(lo + eps), F(v * damp)
    if x + eps > hi:
        x, v = F(hi - eps), F(v * damp)
    return x, v


def push_one(x, v, centers, radii, velocities, box_min, box_max, eps=F(1e-5), damp=F(-0.75)):
    """One particle: x, v float32 (3,) -> new x, v and whether any sphere moved it."""
    x, v = np.array(x, F), np.array(v, F)
    eps, damp = F(eps), F(damp)
    hit = False
    for c, R, u in zip(np.asarray(centers, F), np.asarray(radii, F), np.asarray(velocities, F)):
        d = x - c
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        rp = F(R + eps)
        if r2 < rp * rp:
            nrm = d / np.sqrt(r2) if r2 > 0 else np.array([0, 1, 0], F)
            x = c + rp * nrm
            w = v - u
            wn = w[0] * nrm[0] + w[1] * nrm[1] + w[2] * nrm[2]
            if wn < 0:
                v = v + (damp - F(1)) * wn * nrm
            hit = True
    if hit:
        for a in range(3):
            x[a], v[a] = wall(x[a], v[a], F(box_min[a]), F(box_max[a]), eps, damp)
    return x, v, hit


def push(pos, vel, centers, radii, velocities, box_min, box_max, eps=F(1e-5), damp=F(-0.75)):
    """Every particle: (n, 3) float32 arrays -> new pos, vel and the mask of the particles a sphere moved."""
    pos, vel = np.array(pos, F), np.array(vel, F)
    centers = np.asarray(centers, F).reshape(-1, 3)
    radii = np.asarray(radii, F).reshape(-1)
    velocities = np.zeros_like(centers) if velocities is None else np.asarray(velocities, F).reshape(-1, 3)
    rp = (radii + F(eps)).astype(F)
    near = np.zeros(pos.shape[0], bool)
    for c, r in zip(centers, rp):                   # only particles near some sphere can move
        d = pos - c
        near |= (d * d).sum(axis=1) < F(1.01) * r * r
    touched = np.zeros(pos.shape[0], bool)
    for i in np.nonzero(near)[0]:
        pos[i], vel[i], touched[i] = push_one(pos[i], vel[i], centers, radii, velocities, box_min, box_max, eps, damp)
    return pos, vel, touched


def advance(centers, velocities, dt, steps):
    """The centres after `steps` steps: c = c + dt * u in float32, once per step."""
    c = np.array(centers, F)
    u, dt = np.asarray(velocities, F), F(dt)
    for _ in range(steps):
        c = (c + dt * u).astype(F)
    return c

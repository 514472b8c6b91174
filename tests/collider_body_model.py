"""numpy model of the tracked sphere colliders of include/sph_hip.h (sph_set_collider_bodies): the momentum every sphere takes
from the fluid in one integrate, and the once-per-step update of a free body.  The particle rule is tests/collider_model.py's
(push_one); this file adds, in the header's arithmetic, the per-particle terms t = -(mass * (k * nrm)) in float32 with their
float64 sum, and the body update (float64 velocity sum rounded once to float32, the wall rule, the float32 advance).
impulse_sum_in_order is that sum in the order the header fixes -- lanes, then waves within runs of run_length(n) waves, then
the runs -- which is the device's J to the bit; `impulses` adds the same terms in numpy's order, for the bounded checks."""
import numpy as np

from collider_model import push_one, wall

F = np.float32
D = np.float64


def terms_one(x, v, centers, radii, velocities, mass, box_min, box_max, eps=F(1e-5), damp=F(-0.75)):
    """One particle through the spheres in order, as push_one, and what each sphere took from it: returns new x, new v,
    terms float32 (nsph, 3), kicked bool (nsph,), hit (any sphere moved it) and walled (the wall pass behind the spheres
    changed it)."""
    x, v = np.array(x, F), np.array(v, F)
    eps, damp, mass = F(eps), F(damp), F(mass)
    centers = np.asarray(centers, F).reshape(-1, 3)
    terms = np.zeros((centers.shape[0], 3), F)
    kicked = np.zeros(centers.shape[0], bool)
    hit = False
    for j, (c, R, u) in enumerate(zip(centers, np.asarray(radii, F).reshape(-1), np.asarray(velocities, F).reshape(-1, 3))):
        d = x - c
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        rp = F(R + eps)
        if r2 < rp * rp:
            nrm = d / np.sqrt(r2) if r2 > 0 else np.array([0, 1, 0], F)
            x = c + rp * nrm
            w = v - u
            wn = w[0] * nrm[0] + w[1] * nrm[1] + w[2] * nrm[2]
            if wn < 0:
                kn = ((damp - F(1)) * wn) * nrm              # k * nrm, float32
                v = v + kn
                terms[j] = -(mass * kn)
                kicked[j] = True
            hit = True
    walled = False
    if hit:
        x0, v0 = x.copy(), v.copy()
        for a in range(3):
            x[a], v[a] = wall(x[a], v[a], F(box_min[a]), F(box_max[a]), eps, damp)
        walled = not (np.array_equal(x0, x) and np.array_equal(v0, v))
    return x, v, terms, kicked, hit, walled


def impulses(pos, vel, centers, radii, velocities, mass, box_min, box_max, eps=F(1e-5), damp=F(-0.75)):
    """Every particle: J float64 (nsph, 3) -- the float64 sum of the float32 terms --, the terms (n, nsph, 3), kicked
    (n, nsph), and the masks touched / walled (n,)."""
    pos, vel = np.asarray(pos, F), np.asarray(vel, F)
    centers = np.asarray(centers, F).reshape(-1, 3)
    radii = np.asarray(radii, F).reshape(-1)
    n, ns = pos.shape[0], centers.shape[0]
    terms = np.zeros((n, ns, 3), F)
    kicked = np.zeros((n, ns), bool)
    touched, walled = np.zeros(n, bool), np.zeros(n, bool)
    near = np.zeros(n, bool)
    for c, r in zip(centers, (radii + F(eps)).astype(F)):
        d = pos - c
        near |= (d * d).sum(axis=1) < F(1.01) * r * r
    for i in np.nonzero(near)[0]:
        _, _, terms[i], kicked[i], touched[i], walled[i] = terms_one(pos[i], vel[i], centers, radii, velocities, mass, box_min,
                                                                     box_max, eps, damp)
    return terms.astype(D).sum(axis=0), terms, kicked, touched, walled


def push_with_terms(pos, vel, centers, radii, velocities, mass, box_min, box_max, eps=F(1e-5), damp=F(-0.75)):
    """Every particle through terms_one: the new pos and vel (n, 3) float32, the terms (n, nsph, 3), kicked (n, nsph) and
    touched (n,).  Only the particles within 1.01 (R + eps)^2 of a sphere are visited; the others keep every bit."""
    pos, vel = np.array(pos, F), np.array(vel, F)
    centers = np.asarray(centers, F).reshape(-1, 3)
    radii = np.asarray(radii, F).reshape(-1)
    n, ns = pos.shape[0], centers.shape[0]
    terms = np.zeros((n, ns, 3), F)
    kicked = np.zeros((n, ns), bool)
    touched = np.zeros(n, bool)
    near = np.zeros(n, bool)
    for c, r in zip(centers, (radii + F(eps)).astype(F)):
        d = pos - c
        near |= (d * d).sum(axis=1) < F(1.01) * r * r
    for i in np.nonzero(near)[0]:
        pos[i], vel[i], terms[i], kicked[i], touched[i], _ = terms_one(pos[i], vel[i], centers, radii, velocities, mass,
                                                                       box_min, box_max, eps, damp)
    return pos, vel, terms, kicked, touched


def body_update(c, u, J, mass, accel, R, dt, box_min, box_max, damp=F(-0.75)):
    """One sphere after a step: centre c and velocity u (float32 (3,)), the step's impulse J (float64 (3,)).  mass > 0: the
    velocity takes J / mass + dt * accel in float64 with one rounding to float32, then the wall rule with eps = R; every
    sphere then advances, c = c + dt * u in float32 (mass 0: collider_model.advance)."""
    c, u = np.array(c, F), np.array(u, F)
    dt, mass, damp = F(dt), F(mass), F(damp)
    if mass > 0:
        for a in range(3):
            u[a] = F((D(u[a]) + D(J[a]) / D(mass)) + D(dt) * D(F(accel[a])))
            c[a], u[a] = wall(c[a], u[a], F(box_min[a]), F(box_max[a]), F(R), damp)
    c = (c + dt * u).astype(F)
    return c, u


WAVE = 64                 # slots per wave: one row of partial sums and one mask word each
SUM_THREADS = 256         # the one block that adds the rows (csrc/sph_pairs.hip: k_spheres_step)


def run_length(n):
    """Waves per thread of the summing block for n owned slots: ceil(waves / 256) rounded up to a multiple of 4."""
    n_waves = (int(n) + WAVE - 1) // WAVE
    return ((n_waves + SUM_THREADS - 1) // SUM_THREADS + 3) & ~3


def thread_sums(terms, kicked, n):
    """The summing block's per-thread state for n owned slots in slot order: acc float64 (256, nsph, 3) and found bool
    (256,).  row[w][j] is the float64 sum from 0.0 of wave w's kicked lanes' terms of sphere j in ascending lane order;
    thread t owns the waves [t K, min((t + 1) K, n_waves)), adds the rows they wrote in ascending wave order to an
    accumulator that starts at 0.0, and is found if any of its waves wrote any row.  A run that starts beyond n_waves is
    empty: nothing added, not found."""
    terms = np.asarray(terms, F)
    kicked = np.asarray(kicked, bool)
    n = int(n)
    assert terms.shape[0] == n and kicked.shape[0] == n and terms.shape[:2] == kicked.shape
    ns = kicked.shape[1]
    n_waves = (n + WAVE - 1) // WAVE
    K = run_length(n)
    acc = np.zeros((SUM_THREADS, ns, 3), D)
    found = np.zeros(SUM_THREADS, bool)
    for w in np.unique(np.nonzero(kicked.any(axis=1))[0] // WAVE):          # ascending: a thread's waves come in order
        t = int(w) // K
        assert t < SUM_THREADS and w < n_waves
        lo, hi = int(w) * WAVE, min((int(w) + 1) * WAVE, n)
        for j in range(ns):
            lanes = np.nonzero(kicked[lo:hi, j])[0]
            if lanes.size == 0:
                continue
            row = np.zeros(3, D)
            for l in lanes:                                                 # ascending lane order
                row = row + terms[lo + l, j].astype(D)
            acc[t, j] = acc[t, j] + row
        found[t] = True
    return acc, found


def impulse_sum_in_order(terms, kicked, n, runs_descending=False):
    """J float64 (nsph, 3) of terms float32 (n, nsph, 3) and kicked (n, nsph), both in slot order, in the order of
    include/sph_hip.h: lanes ascending within a wave, waves ascending within a run of run_length(n) waves (thread_sums),
    and then, from 0.0, the accumulators of the found threads in ascending thread order.  runs_descending adds them in
    descending thread order instead -- NOT the device's order; the tests use it to show that the order can be seen."""
    acc, found = thread_sums(terms, kicked, n)
    J = np.zeros(acc.shape[1:], D)
    order = np.nonzero(found)[0]
    for t in (order[::-1] if runs_descending else order):
        J = J + acc[t]
    return J


__all__ = ["terms_one", "impulses", "push_with_terms", "body_update", "push_one", "wall", "run_length", "thread_sums", "impulse_sum_in_order"]

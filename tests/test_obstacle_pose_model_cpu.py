"""CPU: the numpy model of the posed obstacle and its load (tests/obstacle_pose_model.py; include/sph_hip.h: sph_obstacle_set_pose,
sph_obstacle_set_sensor) held to float64 facts that do not depend on it: the analytic distance of the rotated shape, what a
push guarantees, the momentum balance, the speed a spinning plate gives a particle at rest, and the Cayley step's angle."""
import ctypes as C
import math

import numpy as np
import pytest

import collider_body_model as cbm
import obstacle_model as om
import obstacle_pose_model as pm

F = np.float32
D = np.float64
BOX_MIN, BOX_MAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
EPS, DAMP, MASS = F(1e-5), F(-0.75), F(65.0)
S = 1.0 / 16.0
GRID = om.lattice(S, BOX_MIN, BOX_MAX)                      # 67^3, the lattice of the GPU tests
SKEW = (0.8, 0.3, -0.4, 0.33)                               # (w, x, y, z), not normalised: about a skew axis by some 74 degrees
PIVOT, OFF = (0.1, -0.05, 0.0), (0.3, 0.2, -0.1)


def _exact_rot(q):
    """the rotation of the unit quaternion in float64 (no rounding to float32)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], D)


def _to_body(ps, off, pts):
    """float64: the body-frame points of world points"""
    P = ps["pivot"].astype(D) + np.asarray(off, F).astype(D)
    return (np.asarray(pts, D) - P) @ _exact_rot(ps["q"]) + ps["pivot"].astype(D)


def _to_world(ps, off, body):
    P = ps["pivot"].astype(D) + np.asarray(off, F).astype(D)
    return (np.asarray(body, D) - ps["pivot"].astype(D)) @ _exact_rot(ps["q"]).T + P


@pytest.mark.parametrize("shape", [om.box((0.1, -0.1, 0.05), (0.6, 0.1, 0.4)), om.capsule((-0.5, -0.4, 0.3), (0.6, 0.5, -0.2), 0.25)],
                         ids=["box", "capsule"])
def test_posed_phi_is_the_analytic_distance_of_the_rotated_shape(shape):
    """The points are the world images of lattice nodes: a trilinear interpolation reproduces a box's or a capsule's distance
    only there (between the nodes it is off by up to 0.4 s near a box's edges, s^2 / 8r beside a capsule), so the nodes are
    where the posed arithmetic -- d, R^T d + pivot, the cell, the lerps -- can be held to the bar of the tilted half-space in
    tests/test_obstacle_model_cpu.py, 16 spacings of D, against the float64 distance of the rotated shape AT THE fp32 POINT."""
    ps = pm.pose(PIVOT, SKEW)
    phi = om.rasterise([shape], GRID)
    rng = np.random.default_rng(23)
    ijk = rng.integers(8, 58, (4000, 3))                    # nodes within 1.6 of the centre: their images stay inside the grid
    x, y, z = om.node_positions(GRID)
    body = np.stack([x[ijk[:, 0]], y[ijk[:, 1]], z[ijk[:, 2]]], axis=1)
    pts = _to_world(ps, OFF, body).astype(F)
    got, nrm, inside, _ = pm.sample(GRID, phi, OFF, ps, pts)
    assert inside.all()
    want = om.analytic(shape, _to_body(ps, OFF, pts.astype(D)))
    bar = 16 * float(np.spacing(F(om.clamp_distance(GRID))))
    err = np.abs(got.astype(D) - want).max()
    print("max error", err, "bar", bar)
    assert err <= bar
    assert (want < 0).sum() > 20 and (want > 0.5).sum() > 20


def test_the_world_normal_is_the_rotated_body_normal():
    ps = pm.pose(PIVOT, SKEW)
    sh = om.halfspace((0.1, -0.3, 0.2), (0.3, 0.9, -0.2))
    phi = om.rasterise([sh], GRID)
    pts = np.random.default_rng(5).uniform(-1.0, 1.0, (2000, 3)).astype(F)
    got, nrm, inside, d = pm.sample(GRID, phi, OFF, ps, pts)
    assert inside.all()
    want_n = _exact_rot(ps["q"]) @ om.unit_normal(sh["b"]).astype(D)
    assert np.abs(nrm.astype(D) - want_n).max() <= 1e-4    # differences of phi ~ s: 1e-6 / 0.06, as for the unposed plane
    want = om.analytic(sh, _to_body(ps, OFF, pts.astype(D)))
    assert np.abs(got - want).max() <= 16 * float(np.spacing(F(om.clamp_distance(GRID))))
    assert np.array_equal(d, (pts - pm.world_pivot(ps, OFF)).astype(F))


def test_an_unposed_context_is_the_plain_model():
    sh = om.box((0.0, 0.0, 0.0), (0.5, 0.3, 0.4))
    phi = om.rasterise([sh], GRID)
    rng = np.random.default_rng(2)
    pts = rng.uniform(-1.0, 1.0, (5000, 3)).astype(F)
    vel = rng.normal(0, 100, pts.shape).astype(F)
    u = np.array([50.0, 0.0, -20.0], F)
    a = om.push(pts, vel, GRID, phi, OFF, u, BOX_MIN, BOX_MAX, EPS, DAMP)
    b = pm.push(pts, vel, GRID, phi, OFF, u, None, BOX_MIN, BOX_MAX, EPS, DAMP, MASS)
    assert a[2].sum() > 200                                  # (the box fills 6 % of the cloud)
    for p, q in zip(a, b):
        assert np.array_equal(p.view(np.uint8), q.view(np.uint8))


def _plate_scene(seed=31, n=20000):
    """a thick rotated plate (0.3 = 4.8 spacings) far wider than the cloud of particles around its middle: the cloud only meets
    the two large faces, where the field is a plane's but for the cells next to the middle plane"""
    ps = pm.pose(PIVOT, SKEW, (0.0, 0.0, 4000.0))
    plate = om.box((0.1, -0.05, 0.0), (1.2, 0.15, 1.2))
    phi = om.rasterise([plate], GRID)
    rng = np.random.default_rng(seed)
    body = rng.uniform(-0.45, 0.45, (n, 3)) + np.array([0.1, -0.05, 0.0])
    pts = _to_world(ps, OFF, body).astype(F)
    vel = rng.normal(0, 100, pts.shape).astype(F)
    return ps, plate, phi, pts, vel


def test_after_a_push_the_touched_particles_are_out_of_the_rotated_solid():
    ps, plate, phi, pts, vel = _plate_scene()
    u = np.array([50.0, 0.0, 0.0], F)
    st = {}
    p1, v1, touched = pm.push(pts, vel, GRID, phi, OFF, u, ps, BOX_MIN, BOX_MAX, EPS, DAMP, MASS, stats=st)
    assert touched.sum() > 3000 and np.isfinite(p1).all() and np.isfinite(v1).all()
    clear = touched & (np.abs(p1) < 1.99).all(axis=1)       # (not pushed against a wall afterwards)
    assert clear.sum() == touched.sum()
    dist = om.analytic(plate, _to_body(ps, OFF, p1[clear].astype(D)))
    print("iterations", np.bincount(st["iterations"]), "distance", dist.min(), dist.max())
    # on a face the field is a plane's and the last push lands on phi = eps: the bar of the unposed plane, plus the rounding
    # of the two frame changes at |x| ~ 1 (a few 1e-7)
    assert dist.min() >= float(EPS) - 1e-6 * 4.0 - 1e-6, dist.min()
    assert dist.min() >= -float(EPS)                         # in the issue's words: no deeper than eps
    assert np.array_equal(p1[~touched].view(np.uint32), pts[~touched].view(np.uint32))
    assert np.array_equal(v1[~touched].view(np.uint32), vel[~touched].view(np.uint32))


def test_the_load_balances_the_fluids_momentum():
    ps, plate, phi, pts, vel = _plate_scene(seed=37)       # (the cloud is 0.9 wide about the pivot: far from the walls)
    u = np.array([50.0, 0.0, 0.0], F)
    st = {}
    p1, v1, touched = pm.push(pts, vel, GRID, phi, OFF, u, ps, BOX_MIN, BOX_MAX, EPS, DAMP, MASS, stats=st)
    kicked = st["kicked"]
    assert kicked.sum() > 1000 and (kicked <= touched).all() and (np.abs(p1) < 1.9).all()
    J, L = pm.load_in_order(st["lane"], kicked, pts.shape[0])
    dv = (v1[kicked].astype(D) - vel[kicked].astype(D)) * float(MASS)
    rel = np.abs(dv.sum(axis=0) + J).max() / np.abs(st["lane"][:, :3]).sum()
    print("momentum balance", rel)
    assert rel <= 1e-6
    assert not st["lane"][~kicked].any()
    # L against float64: a particle kicked ONCE has d = x - P of its first position and t = -(mass dv) to fp32 rounding
    once = kicked & (st["iterations"] == 1)
    assert once.sum() > 500
    d = pts[once].astype(D) - pm.world_pivot(ps, OFF).astype(D)
    t = -(v1[once].astype(D) - vel[once].astype(D)) * float(MASS)
    tau = np.cross(d, t)
    assert np.abs(tau - st["lane"][once, 3:]).max() <= 1e-6 * np.abs(tau).max()
    # ... and the ordered sum against numpy's own order
    assert np.abs(L - st["lane"][:, 3:].sum(axis=0)).max() <= 1e-12 * np.abs(st["lane"][:, 3:]).sum()
    assert np.abs(J - st["lane"][:, :3].sum(axis=0)).max() <= 1e-12 * np.abs(st["lane"][:, :3]).sum()
    _, Ld = pm.load_in_order(st["lane"], kicked, pts.shape[0], runs_descending=True)
    assert not np.array_equal(Ld, L)                         # the order can be seen (in L: sums of fp32 terms are often exact)


def test_the_ordered_sum_is_the_tracked_spheres():
    """load_in_order is collider_body_model.impulse_sum_in_order for six columns: on float32 terms the two agree to the bit"""
    rng = np.random.default_rng(9)
    for n in (100, 3375, 70001):
        terms = rng.normal(0, 1, (n, 2, 3)).astype(F)
        kicked = rng.random(n) < 0.3
        terms[~kicked] = 0
        want = cbm.impulse_sum_in_order(terms, np.stack([kicked, kicked], axis=1), n)
        J, L = pm.load_in_order(terms.reshape(n, 6).astype(D), kicked, n)
        assert np.array_equal(J.view(np.uint64), want[0].view(np.uint64)) and np.array_equal(L.view(np.uint64), want[1].view(np.uint64))
    assert cbm.run_length(70001) == 8 and cbm.run_length(3375) == 4


def test_a_spinning_plate_gives_a_particle_at_rest_its_normal_speed():
    """v = 0, u = 0: wn = -(omega x d).n, so the particle leaves with v.n = (1 - damping) (omega x d).n |n|^2"""
    ps = pm.pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 40.0))
    plate = om.halfspace((0.0, 0.0, 0.0), (0.0, 1.0, 0.0))          # solid below y = 0 of the body frame, turning about z
    phi = om.rasterise([plate], GRID)
    r = np.linspace(0.2, 1.5, 40)
    pts = np.stack([r, np.full_like(r, -0.01), np.linspace(-0.5, 0.5, 40)], axis=1).astype(F)     # just inside, at distance r
    vel = np.zeros_like(pts)
    _, nrm, inside, d = pm.sample(GRID, phi, (0, 0, 0), ps, pts)
    p1, v1, touched = pm.push(pts, vel, GRID, phi, (0, 0, 0), (0, 0, 0), ps, BOX_MIN, BOX_MAX, EPS, DAMP, MASS)
    assert touched.all() and inside.all()
    n64, d64 = nrm.astype(D), d.astype(D)
    us = np.cross(np.array([0.0, 0.0, 40.0]), d64)
    want = (1.0 - float(DAMP)) * (us * n64).sum(axis=1) * (n64 * n64).sum(axis=1)
    got = (v1.astype(D) * n64).sum(axis=1)
    assert (want > 10.0).all()                               # 1.75 * 40 * r: the plate's face moves up towards them
    assert np.abs(got - want).max() <= 16 * 2.0 ** -24 * 1.75 * 40.0 * 1.6
    assert np.abs(want - 1.75 * 40.0 * pts[:, 0].astype(D)).max() <= 1e-3 * 1.75 * 40.0 * 1.5      # the normal is good to 1e-4


def test_the_quaternion_stays_unit_and_turns_by_the_cayley_angle():
    dt, omega = F(5e-7), np.array([1200.0, -2400.0, 3000.0], F)     # |omega| dt = 2e-3
    ps = pm.pose((0, 0, 0), (1.0, 0.0, 0.0, 0.0), omega)
    q, N = ps["q"], 20000
    for _ in range(N):
        q = pm.quat_step(q, omega, dt)
    assert abs(float(q @ q) - 1.0) <= 1e-7
    R = pm.rot_of(q).astype(D)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-7
    w = omega.astype(D)
    wl = float(np.sqrt(w @ w))
    step = 2.0 * math.atan(wl * float(dt) / 2.0)
    half = N * step / 2.0
    want = np.concatenate([[math.cos(half)], math.sin(half) * w / wl])
    assert min(np.abs(q - want).max(), np.abs(q + want).max()) <= 1e-9
    # the deficit against omega dt that the header states
    assert abs((wl * float(dt) - step) / (wl * float(dt)) - 3.3e-7) <= 0.1e-7
    assert pm.quat_set((0, 0, 0, 0)) is None and pm.quat_set((np.inf, 0, 0, 0)) is None
    assert np.array_equal(pm.rot_of(pm.quat_set((2.0, 0, 0, 0))), np.eye(3, dtype=F))


def test_the_four_symbols_are_exported_and_have_signatures():
    from gpufluidsimulator_amd import build, capi
    lib = C.CDLL(build.build())
    for name in ("sph_obstacle_set_pose", "sph_obstacle_get_pose", "sph_obstacle_set_sensor", "sph_obstacle_get_load"):
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    assert C.sizeof(capi.ObstaclePose) == 40
    assert all(hasattr(capi.Context, m) for m in ("set_obstacle_pose", "obstacle_pose", "set_obstacle_sensor", "obstacle_load"))

"""CPU: the numpy model of the obstacle rule (tests/obstacle_model.py, include/sph_hip.h: sph_obstacle_build) held to float64
facts that do not depend on it: analytic distances, a plane reproduced by the interpolation, what a push guarantees."""
import numpy as np
import pytest

import obstacle_model as om

F = np.float32
BOX_MIN, BOX_MAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
EPS, DAMP = F(1e-5), F(-0.75)
GRID = om.lattice(1.0 / 16.0, BOX_MIN, BOX_MAX)            # 67^3, the lattice of the GPU tests

SHAPES = {
    "sphere": om.sphere((0.3, -0.2, 0.1), 0.7),
    "box": om.box((-0.5, 0.25, 0.4), (0.3, 0.8, 0.45)),
    "round_box": om.box((0.5, -0.25, -0.4), (0.3, 0.5, 0.45), 0.1),
    "capsule": om.capsule((-1.0, -1.2, 0.3), (0.8, 0.9, -0.4), 0.25),
    "halfspace": om.halfspace((0.1, -0.3, 0.2), (0.3, 0.9, -0.2)),
    "bowl": om.sphere((0.0, 0.0, 0.0), 1.5, invert=True),
}


def test_the_lattice_formula():
    assert GRID["dims"] == (67, 67, 67) and GRID["spacing"] == F(0.0625)
    assert np.array_equal(GRID["origin"], np.full(3, -2.0625, F))
    g = om.lattice(0.0, BOX_MIN, BOX_MAX)                   # 0: the particle diameter, 1/32
    assert g["dims"] == (131, 131, 131) and g["spacing"] == F(1.0 / 32.0)
    lo, hi = (-0.3, -1.0, 0.15), (0.35, 0.1, 0.2)
    g = om.lattice(0.05, lo, hi)
    s = float(F(0.05))
    want = tuple(int(np.ceil((float(F(hi[k])) - float(F(lo[k]))) / s)) + 3 for k in range(3))
    assert g["dims"] == want == (16, 25, 4)
    assert np.array_equal(g["origin"], (np.array(lo, F) - F(0.05)).astype(F))
    # one spacing of margin on either side (to the rounding of the node positions): node 1 is lo, node n - 2 reaches hi
    x, y, z = om.node_positions(g)
    for k, ax in enumerate((x, y, z)):
        assert ax.size == g["dims"][k] and ax[0] < lo[k] and abs(float(ax[1]) - lo[k]) < 1e-6
        assert ax[-2] >= hi[k] - 1e-6 and ax[-1] > hi[k] and ax[-3] < hi[k]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_node_values_are_the_analytic_distance(name):
    sh = SHAPES[name]
    phi = om.rasterise([sh], GRID)
    assert phi.shape == (67, 67, 67) and phi.dtype == F
    x, y, z = om.node_positions(GRID)
    P = np.stack(np.meshgrid(z, y, x, indexing="ij")[::-1], axis=-1).reshape(-1, 3)
    want = om.analytic(sh, P).reshape(phi.shape)
    D = om.clamp_distance(GRID)
    assert np.abs(want).max() < D                           # the clamp is idle over the box
    err = np.abs(phi.astype(np.float64) - want).max()
    print(name, "max error", err, "in ulp of D", err / float(np.spacing(D)))
    assert err <= 2 * float(np.spacing(D))


def test_the_union_is_the_minimum_and_the_clamp_holds():
    shapes = [SHAPES[k] for k in ("sphere", "box", "capsule")]
    phi = om.rasterise(shapes, GRID)
    each = [om.rasterise([s], GRID) for s in shapes]
    assert np.array_equal(phi, np.minimum(np.minimum(each[0], each[1]), each[2]))
    g = om.lattice(1.0, (-40.0,) * 3, (40.0,) * 3)          # 83^3 nodes: D = 249 < the far corner's distance to the origin
    far = om.rasterise([om.sphere((0, 0, 0), 1000.0), om.sphere((0, 0, 0), 1.0, invert=True)], g)
    D = om.clamp_distance(g)
    assert D == F(249.0) and far.min() == -D and far.max() <= D


def test_a_tilted_halfspace_is_reproduced_to_rounding():
    """A plane is reproduced exactly by trilinear interpolation, so what is left is rounding; one push lands on phi = eps."""
    sh = SHAPES["halfspace"]
    phi = om.rasterise([sh], GRID)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.99, 1.99, (4000, 3)).astype(F)
    got, nrm, inside = om.sample(GRID, phi, (0, 0, 0), pts)
    assert inside.all()
    want = om.analytic(sh, pts)
    D = float(om.clamp_distance(GRID))
    assert np.abs(got - want).max() <= 16 * float(np.spacing(F(D)))
    assert np.abs(nrm.astype(np.float64) - om.unit_normal(sh["b"])).max() <= 1e-4        # differences of phi ~ s: 1e-6 / 0.06
    # one push: the particles below the plane land on phi = eps
    vel = rng.normal(0, 100, pts.shape).astype(F)
    p1, v1, touched = om.push(pts, vel, GRID, phi, (0, 0, 0), (0, 0, 0), BOX_MIN, BOX_MAX, EPS, DAMP)
    assert touched.sum() > 1000 and not touched[want > 1e-5].any() and touched[want < 0].all()
    clear = touched & (np.abs(p1) < 1.99).all(axis=1)       # (not pushed against a wall afterwards)
    assert clear.sum() > 1000
    assert np.abs(om.analytic(sh, p1[clear]) - float(EPS)).max() <= 1e-6 * 4.0
    # the velocity no longer approaches the plane faster than the damping leaves it
    n = om.unit_normal(sh["b"]).astype(np.float64)
    before, after = vel[clear].astype(np.float64) @ n, v1[clear].astype(np.float64) @ n
    assert np.abs(after - np.where(before < 0, -0.75 * before, before)).max() <= 0.1      # |v| ~ 100, the normal is good to 1e-4
    assert np.array_equal(p1[~touched].view(np.uint32), pts[~touched].view(np.uint32))
    assert np.array_equal(v1[~touched].view(np.uint32), vel[~touched].view(np.uint32))


def test_points_outside_and_nan_are_untouched():
    phi = om.rasterise([om.sphere((0, 0, 0), 5.0)], GRID)      # solid everywhere in the grid
    pts = np.array([[3.0, 0, 0], [0, -2.07, 0], [0, 0, 2.07], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
                    [2.07, 0, 0], [0.1, 0.2, 0.3]], F)
    got, nrm, inside = om.sample(GRID, phi, (0, 0, 0), pts)
    assert inside.tolist() == [False] * 7 + [True]             # (the last node plane is at 2.0625: the last cell ends there)
    vel = np.ones_like(pts)
    p1, v1, touched = om.push(pts, vel, GRID, phi, (0, 0, 0), (0, 0, 0), (-9, -9, -9), (9, 9, 9))
    assert touched.tolist() == [False] * 7 + [True]
    assert np.array_equal(p1[:7].view(np.uint32), pts[:7].view(np.uint32)) and np.array_equal(v1[:7], vel[:7])
    assert np.isinf(got[:7]).all() and not nrm[:7].any()
    # the offset moves the grid, not the points: the same point is inside again once the grid has followed it
    got, _, inside = om.sample(GRID, phi, (3.0, 0, 0), pts[:1])
    assert inside[0] and np.isfinite(got[0])


@pytest.mark.parametrize("name", ["sphere", "halfspace"])
def test_after_a_push_every_touched_particle_is_clear(name):
    sh = SHAPES[name]
    phi = om.rasterise([sh], GRID)
    rng = np.random.default_rng(11)
    pts = rng.uniform(-1.0, 1.0, (6000, 3)).astype(F)          # (a push from here ends inside the box: no wall puts a particle back)
    vel = rng.normal(0, 300, pts.shape).astype(F)
    u = np.array([50.0, -20.0, 10.0], F)
    p1, v1, touched = om.push(pts, vel, GRID, phi, (0, 0, 0), u, BOX_MIN, BOX_MAX, EPS, DAMP)
    assert touched.sum() > 500
    after, _, inside = om.sample(GRID, phi, (0, 0, 0), p1[touched])
    assert inside.all()
    assert after.min() >= float(EPS) - 1e-6 * 4.0, after.min()
    assert np.isfinite(v1).all() and np.isfinite(p1).all()


def test_advance_is_one_rounded_step_at_a_time():
    off = om.advance((0.1, 0.2, 0.3), (833.0, 0.0, -7.0), 5e-7, 300)
    o = np.array([0.1, 0.2, 0.3], F)
    for _ in range(300):
        o = (o + F(5e-7) * np.array([833.0, 0.0, -7.0], F)).astype(F)
    assert np.array_equal(off, o) and off.dtype == F
    assert abs(float(off[0]) - (0.1 + 300 * 5e-7 * 833.0)) < 1e-5

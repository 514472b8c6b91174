"""CPU: the inputs of tests/obstacle_cases.py reach the edges they are meant for -- the model of tests/obstacle_model.py alone, on
the particles as uploaded.  (The GPU tests assert the same conditions again on the obstacle-free twin's output.)"""
import numpy as np
import pytest

import obstacle_cases as oc
import obstacle_model as om

F = np.float32


def test_the_ramp_takes_particles_of_both_mover_tiles_to_other_cells():
    pos, vel = oc.two_tiles()
    grid = om.lattice(oc.S, oc.BMIN, oc.BMAX)
    after, _, touched = oc.push(pos, vel, grid, om.rasterise([oc.RAMP], grid))
    slot = oc.slots_of(oc.keys_of(pos))
    assert pos.shape[0] == 27000 and slot.max() // oc.MM_TILE == 1 and (slot // oc.MM_TILE == 1).sum() == 27000 - oc.MM_TILE
    per_tile = oc.movers_per_tile(pos, after, touched, slot)
    assert per_tile.tolist() == [4054, 2456]


def test_the_block_at_rest_is_pushed_into_other_cells():
    pos, vel = oc.rest_block()
    grid = om.lattice(oc.S, oc.BMIN, oc.BMAX)
    after, _, touched = oc.push(pos, vel, grid, om.rasterise([oc.REST_PILLAR], grid))
    movers = int((oc.keys_of(after) != oc.keys_of(pos)).sum())
    assert touched.sum() == 149 and movers == 97 and 50 <= movers <= oc.REST_N // 8
    # no particle of the lattice is near a cell face: at rest nothing changes cell by itself
    q = ((pos.astype(np.float64) + 2.0) * 16.0) % 1.0
    assert q.min() >= 0.25 and q.max() <= 0.75


def test_the_paddle_arrives_in_its_fifth_step_and_moves_cells_at_once():
    pos, vel = oc.rest_block()
    grid = om.lattice(oc.S, *oc.PADDLE_BOUNDS)
    phi = om.rasterise([oc.PADDLE], grid)
    off = np.zeros(3, F)
    for step in range(1, oc.PADDLE_CONTACT + 1):
        after, _, touched = oc.push(pos, vel, grid, phi, off, oc.PADDLE_U)
        assert touched.any() == (step == oc.PADDLE_CONTACT), step
        off = om.advance(off, oc.PADDLE_U, oc.REST_DT, 1)
    movers = int((oc.keys_of(after) != oc.keys_of(pos)).sum())
    assert 50 <= movers <= oc.REST_N // 8, movers
    # the lattice of the build covers the box wherever the solid has carried it
    assert grid["origin"][0] + off[0] < -2.0 and grid["origin"][0] + off[0] + grid["spacing"] * (grid["dims"][0] - 1) > 2.0


def _dam():
    from gpufluidsimulator_amd import ic
    return ic.dam_break_lattice((15, 15, 15), oc.BOX, jitter=True)


@pytest.mark.parametrize("name,want", [("amp0.2", 1082), ("amp3.0", 1643)])
def test_rough_fields_touch_many_particles_one_to_four_times(name, want):
    pos, vel = _dam()
    grid, phi = oc.rough_field(name, pos)
    st = {}
    _, _, touched = oc.push(pos, vel, grid, om.clamp(phi, grid), stats=st)
    assert touched.sum() == want >= 500
    assert np.bincount(st["iterations"], minlength=5)[1:].min() >= 1
    low = oc.brick_minima(om.clamp(phi, grid))
    assert (low < oc.guard_of(grid)).mean() > 0.99         # rough: nearly every brick must be sampled


def test_the_guard_field_sits_on_the_guard():
    pos, vel = _dam()
    grid, phi = oc.rough_field("guard", pos)
    phi = om.clamp(phi, grid)
    _, _, touched = oc.push(pos, vel, grid, phi)
    assert touched.sum() >= 500
    b, _ = oc.bricks_of(pos, grid)
    low = oc.brick_minima(phi)
    mins = np.array([low[z, y, x] for x, y, z in np.unique(b, axis=0)])
    guard = oc.guard_of(grid)
    assert guard == F(F(1e-5) + F(0.25) * F(oc.S))
    assert [int((mins == oc.ulps(guard, k)).sum()) for k in range(-4, 5)] == [2] * 9
    assert (mins < 0).sum() == 9 and mins.size == 27
    # in a brick whose minimum is on or over the guard the model touches nobody (what lets the kernel skip it)
    over = {tuple(u) for u, m in zip(np.unique(b, axis=0), mins) if m >= guard}
    assert len(over) == 10 and not touched[[tuple(r) in over for r in b]].any()


@pytest.mark.parametrize("name", list(oc.EDGE_LATTICES))
def test_edge_lattices_cut_through_the_block(name):
    grid, phi, off, pos, vel, probes = oc.edge_lattice(name)
    phi = om.clamp(phi, grid)
    _, _, touched = oc.push(pos, vel, grid, phi, off)
    _, _, inside = om.sample(grid, phi, off, pos)
    assert 500 < inside.sum() < pos.shape[0] - 500 and touched.sum() >= 500
    assert len(probes) == 12
    rows = np.array([r for _, r in probes])
    d = np.linalg.norm(pos[rows, None, :].astype(np.float64) - pos[None, :, :], axis=2)
    d[np.arange(12), rows] = np.inf
    assert d.min() > 0.1 + 1e-3                            # alone: further than h from every other particle
    for k in range(3):
        r = np.array([row for axis, row in probes if axis == k])
        assert (~inside[r]).sum() >= 1 and (inside[r] & touched[r]).sum() >= 1, k
    pts = oc.face_points(grid, off)
    _, _, pin = om.sample(grid, phi, off, pts)
    for k in range(6):
        assert 20 <= pin[2000 + 200 * k:2200 + 200 * k].sum() <= 180, k


def test_the_edge_lattices_are_the_edges():
    dims = {k: v[0] for k, v in oc.EDGE_LATTICES.items()}
    assert dims["one_cell"] == (2, 2, 2)
    assert all((n - 1) % oc.BRICK == 0 for n in dims["whole_bricks"]) and dims["whole_bricks_offset"] == dims["whole_bricks"]
    assert dims["two_cells_z"] == (6, 10, 3) and dims["non_dyadic"] == (23, 14, 9)
    off = np.array(oc.EDGE_LATTICES["whole_bricks_offset"][3])
    assert (np.abs(off / 0.13 - np.round(off / 0.13)) > 0.01).all()

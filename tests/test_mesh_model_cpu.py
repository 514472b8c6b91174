"""CPU: the numpy model of the mesh extraction (tests/mesh_model.py, include/sph_hip.h: sph_mesh_extract) held to facts that do
not depend on the kernels: a lone particle gives a closed, outward-oriented sphere of the right size; two give two; a particle in
the box's corner still gives a closed mesh; the case table is face-compatible on a random lattice."""
import math

import numpy as np
import pytest

import mesh_model as mm

F = np.float32
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def _mesh(pos, **kw):
    kw.setdefault("spacing", 1.0 / 16.0)
    kw.setdefault("radius", 3.0 / 16.0)
    return mm.mesh_of(np.array(pos, F).reshape(-1, 3), BOX[0], BOX[1], 1.0 / 64.0, **kw)


def _level_radius(r, iso):
    return r * math.sqrt(1.0 - iso ** (1.0 / 3.0))


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (0.013, -0.021, 0.034), (0.03125, 0.03125, 0.03125)])
@pytest.mark.parametrize("s,r", [(1.0 / 16.0, 3.0 / 16.0), (1.0 / 64.0, 8.0 / 64.0), (1.0 / 40.0, 0.11)])
def test_one_particle_is_a_closed_outward_sphere(centre, s, r):
    counts, origin, sp, pos, nrm, tri = _mesh([centre], spacing=s, radius=r)
    assert len(tri) > 0 and len(pos) > 0
    mm.check_closed_oriented(tri)
    assert mm.euler_characteristic(len(pos), tri) == 2
    vol = mm.signed_volume(pos, tri)
    assert vol > 0
    # every vertex sits on a lattice edge that straddles the level, and no lattice edge is longer than sqrt(3) s
    rho, slack = _level_radius(r, 0.5), math.sqrt(3.0) * s
    dist = np.linalg.norm(pos.astype(np.float64) - np.array(centre), axis=1)
    assert (np.abs(dist - rho) <= slack).all(), (dist.min(), dist.max(), rho, slack)
    ball = lambda a: 4.0 / 3.0 * math.pi * max(a, 0.0) ** 3
    assert ball(rho - slack) <= vol <= ball(rho + slack), (vol, ball(rho - slack), ball(rho + slack))
    # the normals point out of the fluid
    out = pos.astype(np.float64) - np.array(centre)
    assert (np.einsum("ij,ij->i", out, nrm.astype(np.float64)) > 0).all()
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the outermost nodes hold nothing
    for face in (counts[0], counts[-1], counts[:, 0], counts[:, -1], counts[:, :, 0], counts[:, :, -1]):
        assert not face.any()


def test_two_separate_particles_are_two_spheres():
    _, _, _, pos, _, tri = _mesh([(-0.25, 0.0, 0.0), (0.25, 0.05, -0.1)])
    mm.check_closed_oriented(tri)
    assert mm.euler_characteristic(len(pos), tri) == 4
    assert mm.signed_volume(pos, tri) > 0


@pytest.mark.parametrize("corner", [(-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5)])
def test_a_particle_in_the_corner_of_the_box_still_gives_a_closed_mesh(corner):
    counts, _, _, pos, _, tri = _mesh([corner])
    assert len(tri) > 0
    mm.check_closed_oriented(tri)
    assert mm.euler_characteristic(len(pos), tri) == 2
    assert mm.signed_volume(pos, tri) > 0
    for face in (counts[0], counts[-1], counts[:, 0], counts[:, -1], counts[:, :, 0], counts[:, :, -1]):
        assert not face.any()


def test_a_node_exactly_at_the_level_gives_coincident_vertices():
    """a particle on a node with iso = 1.0: that node's count is iso_q, its edges carry t = 0"""
    s, r, iso_q = mm.resolve(1.0 / 64.0, 1.0 / 16.0, 3.0 / 16.0, 1.0)
    dims, origin = mm.lattice(BOX[0], BOX[1], s, r)
    node = mm.node_coords(dims[0], origin[0], s)[12]
    counts, _, _, pos, nrm, tri = _mesh([(node, node, node)], iso=1.0)
    assert iso_q == 4096 and counts[12, 12, 12] == 4096 and (counts >= iso_q).sum() == 1
    assert len(pos) > 0 and (pos == node).all()
    mm.check_closed_oriented(tri)
    assert mm.euler_characteristic(len(pos), tri) == 2
    assert mm.signed_volume(pos, tri) == 0.0


def test_the_case_table_covers_the_sixteen_cases_with_the_right_counts():
    table = mm.case_table()
    assert len(mm.TETS) == 6 and sorted(set(mm.TETS)) == sorted([(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7),
                                                                  (0, 4, 6, 7)])
    assert mm.TETS == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
    for row in table:
        assert [len(row[c]) for c in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
        for c in range(1, 15):       # the complement case is the same surface seen from the other side
            flip = lambda tris: sorted(tuple(sorted(t)) for t in tris)
            assert flip(row[c]) == flip(row[15 - c])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_the_case_table_is_face_compatible_on_a_random_lattice(seed):
    """6^3 random inside / outside nodes (in a shell of outside nodes, so that the surface has no rim): every directed edge of
    every triangle is matched by its reverse exactly once -- across the faces between tetrahedra and between cubes alike"""
    rng = np.random.default_rng(seed)
    counts = np.zeros((8, 8, 8), np.uint32)
    counts[1:7, 1:7, 1:7] = rng.integers(0, 2, (6, 6, 6))
    pos, nrm, tri = mm.extract(counts, np.zeros(3, F), F(1.0), 1)
    assert len(tri) > 100
    mm.check_closed_oriented(tri)
    assert tri.max() == len(pos) - 1 and len(np.unique(tri)) == len(pos)       # every vertex is used
    # the volume is that of the inside nodes' neighbourhoods: positive, and every vertex at the middle of its edge
    assert mm.signed_volume(pos, tri) > 0
    assert np.isin(np.mod(pos * 2, 2), (0.0, 1.0)).all()


def test_the_lattice_formula():
    s, r, iso_q = mm.resolve(1.0 / 64.0)
    assert s == F(1.0 / 64.0) and r == F(3.0 / 64.0) and iso_q == 2048
    dims, origin = mm.lattice((-1.0, -0.25, 0.0), (1.0, 0.25, 2.0), F(0.07), F(0.21))
    pad = math.ceil(float(F(0.21)) / float(F(0.07))) + 1
    assert dims == tuple(math.ceil(e / float(F(0.07))) + 1 + 2 * pad for e in (2.0, 0.5, 2.0))
    assert origin[0] == F(-1.0) - F(pad) * F(0.07)
    assert mm.resolve(1.0, iso=1e30)[2] == 0xFFFFFFFF and mm.resolve(1.0, iso=1e-9)[2] == 1

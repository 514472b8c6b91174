"""GPU: the mesh extraction (sph_mesh_extract and the calls next to it) against the numpy model of tests/mesh_model.py, fed with
exactly the positions sph_download_owned returns.  Counts, vertex positions, normals and triangles are compared bit for bit: model
and device perform the same integer and IEEE fp32 operations, and the order of vertices and triangles is fixed by the rule."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_model as mm
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NOMEM, E_CAPACITY, E_STATE = -1, -3, -4, -5
F = np.float32
UNIT = dict(box=(1.0, 1.0, 1.0), grid=(8, 8, 8))
COARSE = dict(spacing=1.0 / 16.0, radius=3.0 / 16.0)
DAM = dict(box=(1.0, 0.5, 2.0), grid=(8, 4, 16))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _code(fn, *args, **kw):
    with pytest.raises(capi.SphError) as e:
        fn(*args, **kw)
    return int(str(e.value).split("error ")[1].split(":")[0])


def _want(c, **kw):
    """the model's lattice, counts and mesh of the context's particles as sph_download_owned returns them"""
    P = c.params
    s, r, iso_q = mm.resolve(P.particle_radius, kw.get("spacing", 0.0), kw.get("radius", 0.0), kw.get("iso", 0.0))
    dims, origin = mm.lattice(tuple(P.box_min), tuple(P.box_max), s, r)
    counts = mm.field(c.download_owned()[0], dims, origin, s, r)
    pos, nrm, tri = mm.extract(counts, origin, s, iso_q)
    return dict(dims=dims, origin=origin, counts=counts, pos=pos, nrm=nrm, tri=tri, iso_q=iso_q, s=s)


def _got(c, **kw):
    mp = capi.mesh_defaults(**kw)
    dims, origin = c.mesh_lattice(mp)
    nv, nt = c.extract_mesh(mp)
    pos, nrm, tri = c.read_mesh()
    assert pos.shape == (nv, 3) and nrm.shape == (nv, 3) and tri.shape == (nt, 3)
    return dict(dims=dims, origin=origin, counts=c.mesh_field(), pos=pos, nrm=nrm, tri=tri)


def _same(got, want, what=""):
    assert got["dims"] == want["dims"], what
    assert np.array_equal(_bits(got["origin"]), _bits(want["origin"])), what
    for k in ("counts", "pos", "nrm", "tri"):
        differ = int((_bits(got[k]) != _bits(want[k])).sum()) if got[k].shape == want[k].shape else -1
        print(f"{what}: {k}: shape {got[k].shape} / {want[k].shape}, {differ} words differ")
    for k in ("counts", "pos", "nrm", "tri"):
        assert got[k].shape == want[k].shape, f"{what}: {k}"
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k}"


def _check(c, what="", **kw):
    want = _want(c, **kw)
    _same(_got(c, **kw), want, what)
    return want


def _closed_sphere(m, spheres=1):
    mm.check_closed_oriented(m["tri"])
    assert mm.euler_characteristic(len(m["pos"]), m["tri"]) == 2 * spheres
    assert mm.signed_volume(m["pos"], m["tri"]) > 0


def test_one_particle_centred():
    with capi.Context(16, **UNIT) as c:
        c.upload(np.array([[0.013, -0.021, 0.034]], F), index=[5])
        want = _check(c, "one particle", **COARSE)
        assert want["dims"] == (25, 25, 25) and len(want["tri"]) > 8
        _closed_sphere(want)
        want = _check(c, "one particle, the defaults")          # s = 1/64, r = 3/64: a lattice of 73^3
        assert want["dims"] == (73, 73, 73)
        _closed_sphere(want)


def test_one_particle_on_a_node_at_the_level_gives_coincident_vertices():
    with capi.Context(16, **UNIT) as c:
        dims, origin = c.mesh_lattice(capi.mesh_defaults(**COARSE))
        node = mm.node_coords(dims[0], origin[0], F(1.0 / 16.0))[12]
        c.upload(np.array([[node, node, node]], F))
        want = _check(c, "on a node, iso 1", iso=1.0, **COARSE)
        assert want["iso_q"] == 4096 and want["counts"][12, 12, 12] == 4096 and (want["counts"] >= 4096).sum() == 1
        assert len(want["pos"]) > 0 and (want["pos"] == node).all()        # t = 0 on every edge of the one inside node
        mm.check_closed_oriented(want["tri"])
        assert mm.euler_characteristic(len(want["pos"]), want["tri"]) == 2


@pytest.mark.parametrize("corner", [(-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5)])
def test_one_particle_in_a_corner_of_the_box(corner):
    with capi.Context(16, **UNIT) as c:
        c.upload(np.array([corner], F))
        want = _check(c, f"corner {corner}", **COARSE)
        _closed_sphere(want)


@pytest.fixture(scope="module")
def dam():
    pos, vel = ic.dam_break_lattice((12, 12, 12), DAM["box"], jitter=True)
    return pos, vel


def test_a_dam_block_in_a_box_of_unequal_axes(dam):
    """s = 0.07 divides no edge of the box (1, 0.5, 2) and the three dimensions differ: a mixed-up stride cannot pass"""
    pos, vel = dam
    kw = dict(spacing=0.07)
    with capi.Context(len(pos), **DAM) as c:
        c.upload(pos, vel)
        want = _check(c, "dam before any step", **kw)
        assert len(set(want["dims"])) == 3 and len(want["tri"]) > 500
        mm.check_closed_oriented(want["tri"])
        assert mm.signed_volume(want["pos"], want["tri"]) > 0
        first = _got(c, **kw)
        _same(_got(c, **kw), first, "two extractions in a row")
        c.step(float(ic.DEFAULT_DT), 20)
        stepped = _check(c, "dam after 20 steps", **kw)
        mm.check_closed_oriented(stepped["tri"])
        assert mm.signed_volume(stepped["pos"], stepped["tri"]) > 0
        assert not np.array_equal(stepped["counts"], want["counts"])
        _check(c, "dam after 20 steps, the defaults")
    rng = np.random.default_rng(7)
    order = rng.permutation(len(pos))
    with capi.Context(len(pos), **DAM) as c:
        c.upload(pos[order], vel[order], index=order.astype(np.uint32))
        _same(_got(c, **kw), want, "the same particles in a shuffled order")


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "gpufluidsimulator_amd", "csrc", "sph_mesh.hip")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


def test_scan_boundaries():
    """More nodes than one first-level scan block (MESH_BLOCK) and more blocks than the second level takes at a time (MESH_SCAN2),
    with vertices and triangles in the first block, the last block, across block boundaries and on either side of the second
    level's boundary.  The first and the last block lie in the lattice's outermost layers, which only particles OUTSIDE the box
    reach: two of them sit there (the mesh is then open at the lattice's rim; the model says the same)."""
    block, scan2 = _kernel_constant("MESH_BLOCK"), _kernel_constant("MESH_SCAN2")
    assert (block, scan2) == (256, 1024)
    s, pad = 1.0 / 32.0, 3                                   # r = 1.5 s: pad = ceil(1.5) + 1
    dims = (64, 64, 66)                                      # block * scan2 = 64^3 nodes: the smallest cube beyond it, two layers deeper
    assert dims[0] * dims[1] * dims[2] > block * scan2 and dims[0] * dims[1] * (dims[2] - 2) == block * scan2
    box = tuple((n - 1 - 2 * pad) * s for n in dims)
    kw = dict(spacing=s, radius=1.5 * s)
    with capi.Context(64, box=box, grid=(16, 16, 16)) as c:
        got_dims, origin = c.mesh_lattice(capi.mesh_defaults(**kw))
        assert got_dims == dims
        node = lambda i, j, k: [origin[0] + F(i) * F(s), origin[1] + F(j) * F(s), origin[2] + F(k) * F(s)]
        shift = np.array([0.004, -0.003, 0.002], F)
        at = [node(2, 2, 0), node(61, 61, 65), node(10, 1, 64), node(40, 62, 63), node(31, 31, 33), node(33, 30, 31)]
        c.upload((np.array(at, F) + shift).astype(F))
        want = _check(c, "scan boundaries", **kw)
        nv, nt = mm.census(want["counts"], want["iso_q"])
        n_blocks = -(-len(nv) // block)
        assert n_blocks > scan2
        v_blocks, t_blocks = np.unique(np.nonzero(nv)[0] // block), np.unique(np.nonzero(nt)[0] // block)
        assert v_blocks[0] == 0 and t_blocks[0] == 0 and v_blocks[-1] == n_blocks - 1
        for blocks in (v_blocks, t_blocks):                  # on either side of the second level's boundary, and right at it
            assert (blocks < scan2).any() and (blocks >= scan2).any() and scan2 in blocks
            assert (np.diff(blocks) == 1).any()              # neighbouring blocks: a run of vertices / triangles across a boundary
        assert len(want["pos"]) == int(nv.sum()) > 0 and len(want["tri"]) == int(nt.sum()) > 0


def test_the_splat_on_either_side_of_its_tile():
    """A workgroup of the splat sums in LDS where the box of nodes its particles reach holds at most MESH_TILE_NODES nodes, and
    adds to the field directly beyond: two particles in one workgroup, r = 4 s and both in the middle of a cube, so each reaches
    8 nodes per axis, and D cubes apart along x: the box is (D + 8) x 8 x 8 -- exactly the tile, and one column more."""
    tile = _kernel_constant("MESH_TILE_NODES")
    assert tile == 8192
    s = 1.0 / 256.0
    kw = dict(spacing=s, radius=4.0 * s)
    with capi.Context(64, box=(1.0, 0.125, 0.125), grid=(8, 1, 1)) as c:
        dims, origin = c.mesh_lattice(capi.mesh_defaults(**kw))
        X = [mm.node_coords(dims[a], origin[a], F(s)) for a in range(3)]
        half = F(s) * F(0.5)
        for apart, fits in ((tile // 64 - 8, True), (tile // 64 - 7, False)):
            pos = np.array([[X[0][20] + half, X[1][20] + half, X[2][20] + half],
                            [X[0][20 + apart] + half, X[1][20] + half, X[2][20] + half]], F)
            r2 = F(4.0 * s) * F(4.0 * s)
            box = 1
            for a in range(3):                               # the box of the nodes that pass on each axis, as the kernel narrows it
                d = X[a][None, :] - pos[:, a:a + 1]
                reached = np.nonzero((d * d < r2).any(axis=0))[0]
                box *= int(reached[-1] - reached[0] + 1)
            assert (box <= tile) == fits and box == (apart + 8) * 64
            c.upload(pos)
            want = _check(c, f"two particles {apart} cubes apart: a box of {box} nodes", **kw)
            _closed_sphere(want, spheres=2)


def test_reach_at_both_ends():
    with capi.Context(64, **UNIT) as c:
        c.upload(np.array([[0.013, -0.021, 0.034], [0.2, 0.21, -0.3]], F))
        want = _check(c, "r = 8 s", spacing=1.0 / 32.0, radius=8.0 / 32.0)
        assert len(want["tri"]) > 1000
        mm.check_closed_oriented(want["tri"])
        # r = 0.75 s: a particle in the middle of a cube (0.866 s from its corners) reaches no node at all
        dims, origin = c.mesh_lattice(capi.mesh_defaults(spacing=1.0 / 16.0, radius=0.75 / 16.0))
        mid = mm.node_coords(dims[0], origin[0], F(1.0 / 16.0))[10] + F(1.0 / 32.0)
        c.upload(np.array([[mid, mid, mid]], F))
        want = _check(c, "r = 0.75 s, nothing reached", spacing=1.0 / 16.0, radius=0.75 / 16.0)
        assert not want["counts"].any() and want["pos"].shape == (0, 3) and want["tri"].shape == (0, 3)
        assert c.mesh_dev()[3:] == (0, 0)
        near = mid - F(1.0 / 32.0)                               # node 10 again
        c.upload(np.array([[near, near + F(0.01), near - F(0.01)]], F))
        want = _check(c, "r = 0.75 s, one node reached", spacing=1.0 / 16.0, radius=0.75 / 16.0)
        assert (want["counts"] > 0).sum() == 1 and len(want["tri"]) > 0


def test_particles_outside_the_lattice_are_skipped():
    with capi.Context(64, **UNIT) as c:
        c.upload(np.array([[0.1, 0.1, 0.1], [50.0, 0.0, 0.0], [0.0, -1e30, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],
                           [-0.73, 0.0, 0.0]], F))                    # (the last one: outside the box, inside the lattice's pad)
        want = _check(c, "far, NaN and infinite particles", **COARSE)
        assert len(want["tri"]) > 0


def test_an_empty_context_and_every_refusal():
    nan, inf = float("nan"), float("inf")
    with capi.Context(64, **UNIT) as c:
        assert _code(c.read_mesh) == E_STATE and _code(c.mesh_dev) == E_STATE and _code(c.save_obj, "/dev/null") == E_STATE
        assert c.L.sph_mesh_read(c.h, None, None, None) == E_STATE
        assert c.L.sph_mesh_field_read(c.h, np.zeros(8, np.uint32).ctypes.data) == E_STATE
        assert c.L.sph_mesh_field_dims(c.h, (ctypes.c_uint32 * 3)()) == E_STATE
        held = capi.memory_stats()
        for kw in (dict(spacing=-1.0), dict(spacing=nan), dict(spacing=inf), dict(radius=-0.1), dict(radius=nan), dict(radius=inf),
                   dict(iso=-0.5), dict(iso=nan), dict(iso=inf), dict(spacing=0.01, radius=0.0801), dict(radius=0.2),
                   dict(spacing=1e-30, radius=1e-30)):
            assert _code(c.extract_mesh, capi.mesh_defaults(**kw)) == E_INVALID, kw
            assert _code(c.mesh_lattice, capi.mesh_defaults(**kw)) == E_INVALID, kw
        for kw in (dict(spacing=1.0 / 2100.0), dict(spacing=1.0 / 600.0)):        # an axis beyond 2048 nodes; more than 2^27 nodes
            assert _code(c.extract_mesh, capi.mesh_defaults(**kw)) == E_CAPACITY, kw
            assert _code(c.mesh_lattice, capi.mesh_defaults(**kw)) == E_CAPACITY, kw
        assert c.L.sph_mesh_extract(None, None, None, None) == E_INVALID
        assert capi.memory_stats() == held and _code(c.read_mesh) == E_STATE      # nothing changed, nothing allocated
        assert c.extract_mesh(capi.mesh_defaults(**COARSE)) == (0, 0)            # a context that never held a particle
        pos, nrm, tri = c.read_mesh()
        assert pos.shape == (0, 3) and tri.shape == (0, 3) and not c.mesh_field().any()
        c.upload(np.array([[0.0, 0.0, 0.0]], F))
        nv, nt = c.extract_mesh(None)                                             # NULL parameters: the defaults
        assert nv > 0 and nt > 0
        before = c.read_mesh()
        assert _code(c.extract_mesh, capi.mesh_defaults(iso=nan)) == E_INVALID
        for x, y in zip(before, c.read_mesh()):                                   # the previous mesh: readable and unchanged
            assert np.array_equal(_bits(x), _bits(y))
        c.remove(capi.Region.box((-1, -1, -1), (1, 1, 1)))
        assert c.n == 0 and c.extract_mesh(None) == (0, 0)
    with capi.Context(64, slab=(0, 4), ghost_capacity=64, **UNIT) as s:
        assert _code(s.extract_mesh) == E_STATE and _code(s.read_mesh) == E_STATE


def test_meshing_is_invisible_to_the_simulation():
    """~2,000 particles, 10 phased steps with an extraction after every phase call, against 10 steps without"""
    pos, vel = ic.random_box(2000, DAM["box"], speed=20.0, fill=0.5)
    dt = float(ic.DEFAULT_DT)
    runs = []
    for mesh in (True, False):
        with capi.Context(len(pos), **DAM) as c:
            c.upload(pos, vel)
            for _ in range(10):
                for phase in (c.hash, c.sort, c.build_cells, c.density, c.force, c.collide, lambda: c.integrate(dt)):
                    phase()
                    if mesh:
                        assert c.extract_mesh(capi.mesh_defaults(spacing=0.05))[1] > 0
            runs.append((c.download_owned(), c.order(), c.download(want=("density", "pressure"))))
        if not mesh:
            with capi.Context(len(pos), **DAM) as c:
                c.upload(pos, vel)
                c.step_phased(dt, 10)
                runs.append((c.download_owned(), c.order(), c.download(want=("density", "pressure"))))
    for (a, oa, da), (b, ob, db) in ((runs[0], runs[1]), (runs[1], runs[2])):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(oa, ob)
        assert np.array_equal(_bits(da["density"]), _bits(db["density"])) and np.array_equal(_bits(da["pressure"]), _bits(db["pressure"]))


def test_memory_returns_to_its_base_and_every_allocation_may_fail(dam):
    import gc
    gc.collect()
    capi.fail_alloc(0)
    base = capi.memory_stats()
    pos, vel = dam
    small, large = dict(spacing=0.1), dict(spacing=0.07)
    with capi.Context(len(pos), **DAM) as c:
        created = capi.memory_stats()
        c.upload(pos, vel)
        c.step(float(ic.DEFAULT_DT), 2)
        assert capi.memory_stats() == created
        c.extract_mesh(capi.mesh_defaults(**small))
        first = capi.memory_stats()
        assert first[2] - created[2] == 6                        # counts, vertex bases, sums; positions, normals, triangles
        c.extract_mesh(capi.mesh_defaults(**small))
        assert capi.memory_stats() == first                      # nothing grows: nothing is allocated
        want = _check(c, "the larger lattice", **large)          # the buffers grow
        second = capi.memory_stats()
        assert second[2] == first[2] and second[0] > first[0]
        _check(c, "the smaller lattice in the larger buffers", **small)
        assert capi.memory_stats() == second
    assert capi.memory_stats() == base
    try:
        with capi.Context(len(pos), **DAM) as c:
            c.upload(pos, vel)
            created = capi.memory_stats()
            want = _want(c, **large)                                 # (before the hook is armed: a download allocates too)
            for k in range(1, 7):
                capi.fail_alloc(k)
                assert _code(c.extract_mesh, capi.mesh_defaults(**large)) == E_NOMEM, k
                capi.fail_alloc(0)
                assert capi.memory_stats() == created, k             # nothing extra is held
                assert _code(c.read_mesh) == E_STATE
            capi.fail_alloc(7)                                       # one more than an extraction allocates: it goes through
            _same(_got(c, **large), want, "after six failures")
            capi.fail_alloc(0)
            held = capi.memory_stats()
            capi.fail_alloc(1)                                       # a lattice that must grow and cannot: the mesh is given up
            assert _code(c.extract_mesh, capi.mesh_defaults(spacing=0.05)) == E_NOMEM
            capi.fail_alloc(0)
            assert capi.memory_stats() == created and held[2] - created[2] == 6
            _same(_got(c, **large), want, "after a failed growth")
    finally:
        capi.fail_alloc(0)
    assert capi.memory_stats() == base

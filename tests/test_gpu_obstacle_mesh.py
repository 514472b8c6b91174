"""GPU: obstacles from a triangle mesh (include/sph_hip.h: sph_obstacle_build_mesh and the calls next to it) against the numpy
model of tests/mesh_obstacle_model.py, BIT FOR BIT, on the inputs of tests/mesh_obstacle_cases.py: every case and its four
counters, the triangles in another order, the device-array path fed by sph_mesh_dev, a fused and a phased step against
obstacle_model.push on a bare twin's output, motion and replacement, the refusals with every allocation failing once, and the
triangles the device form skips; then lattices wider than a wave and work lists longer than a launch (mc.LARGE_CASES) and a triangle
list of more than 1024 blocks, nearly all skipped (mc.sparse_blocks)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_obstacle_cases as mc
import mesh_obstacle_model as mm
import obstacle_model as om
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
S = float(mc.S)
EPS, DAMP = F(1e-5), F(-0.75)
ZERO = (0.0, 0.0, 0.0)
INVALID, NOMEM, CAPACITY, STATE = -1, -3, -4, -5
WHOLE = (mc.BMIN, mc.BMAX)


def _ctx(cap=64):
    return capi.Context(cap, box=mc.BOX, grid=mc.GRID)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), (what, int((_bits(a) != _bits(b)).sum()))


def _build(c, name, permute=False, invert=False):
    v, t, band, bounds, _ = mc.permuted(name) if permute else mc.case(name)
    c.build_obstacle_mesh(v, t, S, band, invert, bounds or WHOLE)


# ---- 1. every case equals the model, counters included; the order of the triangles does not matter -----------------------------
@pytest.mark.parametrize("name", mc.CASES)
def test_build_equals_the_model(name):
    want, stats = mc.model(name)
    grid = mc.grid_of(name)
    with _ctx() as c:
        _build(c, name)
        ob = c.obstacle(read=True)
        assert ob["dims"] == grid["dims"] and ob["spacing"] == grid["spacing"]
        _same(ob["origin"], grid["origin"])
        _same(ob["phi"], want, name)
        assert c.obstacle_mesh_stats() == stats, (c.obstacle_mesh_stats(), stats)
        _build(c, name, permute=True)
        _same(c.obstacle(read=True)["phi"], want, name + " permuted")
        assert c.obstacle_mesh_stats() == stats


def test_invert_negates_bit_for_bit():
    want, _ = mc.model("free_box", True)
    with _ctx() as c:
        _build(c, "free_box", invert=True)
        _same(c.obstacle(read=True)["phi"], want)
    _same(want, -mc.model("free_box")[0])


# ---- 2. the device-array path ------------------------------------------------------------------------------------------------------
def test_the_extracted_mesh_comes_back_in_as_a_solid():
    pos = mc.blob_particles()
    with _ctx(512) as c:
        c.upload(pos, np.zeros_like(pos))
        nv, nt = c.extract_mesh(capi.mesh_defaults(spacing=S))
        assert nt > 1000
        c.build_obstacle_from_mesh(S, bounds=WHOLE)        # device pointers, the same stream, no host trip
        from_dev = c.obstacle(read=True)["phi"]
        stats = c.obstacle_mesh_stats()
        v, _, t = c.read_mesh()
        c.build_obstacle_mesh(v, t, S, bounds=WHOLE)
        _same(c.obstacle(read=True)["phi"], from_dev)
        assert c.obstacle_mesh_stats() == stats
    want, want_stats = mm.build(mc.grid_of("blob"), v, t)
    _same(from_dev, want)
    assert stats == want_stats and stats[0] == nt and stats[1:] == (0, 0, 0)


# ---- 3. stepping: A with the mesh-built obstacle is the model's push on the bare twin's output ---------------------------------------
def _flow():
    pos, vel = ic.dam_break_lattice((16, 16, 16), mc.BOX, jitter=True)       # fills [-1, -0.5]^3
    pos, vel = pos[:4000].copy(), vel[:4000].copy()
    pos += np.array([0.07, 0.75, 0.75], F)                                  # its +x end overlaps the sphere's -x cap
    vel[:, 0] = 300.0
    return pos, vel


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "phased"])
def test_a_step_with_the_icosphere_installed(fused):
    pos, vel = _flow()
    phi, _ = mc.model("ico_rotated")
    grid = mc.grid_of("ico_rotated")
    with _ctx(4000) as a, _ctx(4000) as b:
        _build(a, "ico_rotated")
        for c in (a, b):
            c.upload(pos, vel)
            c.step(DT, 1) if fused else c.step_phased(DT, 1)
        sa, sb = a.download(), b.download()
        p4 = a.positions4()
    want_p, want_v, touched = om.push(sb["pos"], sb["vel"], grid, phi, ZERO, ZERO, mc.BMIN, mc.BMAX, EPS, DAMP)
    assert touched.sum() >= 50, touched.sum()
    _same(sa["pos"], want_p, "pos")
    _same(sa["vel"], want_v, "vel")
    _same(sa["density"], sb["density"]); _same(sa["pressure"], sb["pressure"])
    _same(p4[:, :3], want_p, "positions by index")
    assert not np.array_equal(sa["pos"], sb["pos"])


# ---- 4. motion and replacement ---------------------------------------------------------------------------------------------------------
def test_motion_and_replacement():
    pos, vel = _flow()
    phi, stats = mc.model("ico_rotated")
    grid = mc.grid_of("ico_rotated")
    u = np.array([40.0, 0.0, -25.0], F)
    off = np.array([0.01, -0.02, 0.0], F)
    with _ctx(4000) as a, _ctx(4000) as b:
        before = capi.memory_stats()
        _build(a, "ico_rotated")
        assert capi.memory_stats()[2] == before[2] + 4      # phi, bricks, the work list, the marks
        a.set_obstacle_motion(offset=off, velocity=u)
        a.upload(pos, vel); b.upload(pos, vel)
        a.step(DT, 1); b.step(DT, 1)
        sa, sb = a.download(), b.download()
        want_p, want_v, touched = om.push(sb["pos"], sb["vel"], grid, phi, off, u, mc.BMIN, mc.BMAX, EPS, DAMP)
        assert touched.sum() >= 50
        _same(sa["pos"], want_p); _same(sa["vel"], want_v)
        _same(a.obstacle()["offset"], om.advance(off, u, DT, 1))
        # an analytic obstacle over the mesh-built one: the scratch leaves, the stats with it
        a.build_obstacle([capi.Shape.sphere((0.0, 0.0, 0.0), 0.3)], S, WHOLE)
        assert capi.memory_stats()[2] == before[2] + 2
        with pytest.raises(capi.SphError, match="error -5"):
            a.obstacle_mesh_stats()
        _same(a.obstacle(read=True)["phi"], om.rasterise([om.sphere((0.0, 0.0, 0.0), 0.3)], grid))
        # ... and the mesh over the analytic one
        _build(a, "ico_rotated")
        _same(a.obstacle(read=True)["phi"], phi)
        assert a.obstacle_mesh_stats() == stats
        _same(a.obstacle()["velocity"], u)                  # the motion belongs to the context
        a.clear_obstacle()
        assert a.obstacle() is None and capi.memory_stats() == before
        with pytest.raises(capi.SphError, match="error -5"):
            a.obstacle_mesh_stats()


# ---- 5. refusals change nothing; every allocation failing once ----------------------------------------------------------------------------
def test_refusals_change_nothing():
    L = capi.load()
    v, t, _, _, _ = mc.case("free_box")
    want, _ = mc.model("free_box")
    f3 = lambda *x: (C.c_float * 3)(*x)
    lo, hi = f3(*mc.BMIN), f3(*mc.BMAX)

    def host(c, verts=v, tris=t, band=0, nt=None, spacing=S, lo=lo, hi=hi):
        verts, tris = np.ascontiguousarray(verts, F), np.ascontiguousarray(tris, np.uint32)
        p = capi.ObstacleMeshParams(spacing, band, 0)
        return L.sph_obstacle_build_mesh(c.h, C.byref(p), lo, hi, len(verts), verts.ctypes.data, len(tris) if nt is None else nt,
                                         tris.ctypes.data)

    start = capi.memory_stats()
    with capi.Context(64, params=capi.default_params(mc.BOX, mc.GRID), slab=(0, mc.GRID[2]), ghost_capacity=64) as s:
        base = capi.memory_stats()
        assert host(s) == STATE
        assert L.sph_obstacle_build_obj(s.h, None, None, None, b"nowhere.obj") == STATE
        assert s.obstacle() is None and capi.memory_stats() == base
    with _ctx() as a:
        a.build_obstacle([capi.Shape.sphere((0.0, 0.0, 0.0), 0.3)], S, WHOLE)
        kept = a.obstacle(read=True)["phi"]
        base = capi.memory_stats()
        bad_index, nan_vertex = t.copy(), v.copy()
        bad_index[5, 1] = len(v)
        nan_vertex[3, 2] = np.nan
        assert host(a, band=17) == INVALID
        assert host(a, tris=bad_index) == INVALID
        assert host(a, verts=nan_vertex) == INVALID
        assert host(a, nt=0) == INVALID
        assert host(a, spacing=0.0005) == CAPACITY
        assert host(a, hi=f3(1.0, -2.0, 1.0)) == INVALID
        assert L.sph_obstacle_build_mesh(a.h, None, lo, hi, len(v), None, len(t), t.ctypes.data) == INVALID
        assert L.sph_obstacle_build_mesh_dev(a.h, None, lo, hi, len(v), None, len(t), None) == INVALID
        assert L.sph_obstacle_build_obj(a.h, None, lo, hi, b"/nonexistent/mesh.obj") == INVALID
        assert L.sph_obstacle_mesh_stats(a.h, (C.c_uint64 * 4)()) == STATE      # the installed obstacle is analytic
        assert capi.memory_stats() == base
        _same(a.obstacle(read=True)["phi"], kept)          # the previous obstacle is intact
        a.clear_obstacle()
        base = capi.memory_stats()
        for k in range(1, 7):                              # the two temporaries, phi, the bricks, the work list, the marks
            capi.fail_alloc(k)
            assert host(a) == NOMEM, k
            capi.fail_alloc(0)
            assert a.obstacle() is None and capi.memory_stats() == base, k
        capi.fail_alloc(7)                                 # one more than the call makes: it goes through
        assert host(a) == 0
        capi.fail_alloc(0)
        _same(a.obstacle(read=True)["phi"], want)
        capi.fail_alloc(4)                                 # over an installed obstacle: none is left
        assert host(a) == NOMEM
        capi.fail_alloc(0)
        assert a.obstacle() is None and capi.memory_stats() == base
        assert host(a) == 0
    assert capi.memory_stats() == start                    # after destroy: what the process held before create


# ---- 6. the device form skips what the host form refuses ------------------------------------------------------------------------------------
def test_the_device_form_skips_bad_triangles():
    v, t, band, _, _ = mc.case("ico_rotated")
    v, t = v.copy(), t.copy()
    v[17, 1] = np.nan                                      # every triangle round vertex 17 ...
    t[100, 2] = len(v)                                     # ... and one with an index out of range
    t[200, 0] = 0xFFFFFFFF
    ok = mm.good_triangles(v, t)
    assert 5 <= (~ok).sum() <= 9
    grid = mc.grid_of("ico_rotated")
    want, removed_stats = mm.build(grid, v, t[ok], band)   # the model with those triangles removed ...
    full, full_stats = mm.build(grid, v, t, band)          # ... is the model that skips them
    _same(full, want)
    assert removed_stats[0] == ok.sum() and removed_stats[3] > 0          # (the mesh is open now: odd columns)
    assert full_stats == (removed_stats[0], int((~ok).sum())) + removed_stats[2:]
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    L = capi.load()
    with _ctx() as c:
        p = capi.ObstacleMeshParams(S, band, 0)
        lo, hi = (C.c_float * 3)(*mc.BMIN), (C.c_float * 3)(*mc.BMAX)
        assert L.sph_obstacle_build_mesh_dev(c.h, C.byref(p), lo, hi, len(v), dv.data_ptr(), len(t), dt.data_ptr()) == 0
        _same(c.obstacle(read=True)["phi"], want)
        assert c.obstacle_mesh_stats() == full_stats


# ---- 7. the work list beyond one tile per triangle: chunks, row groups, mark words, the stride (tests/mesh_obstacle_cases.py:
#         LARGE_CASES; what each case reaches is asserted in tests/test_mesh_obstacle_model_cpu.py) ------------------------------------
def _build_large(c, case):
    v, t, band, bounds, _, s = case
    c.build_obstacle_mesh(v, t, float(s), band, False, bounds)
    return c.obstacle(read=True), c.obstacle_mesh_stats()


@pytest.mark.parametrize("name", mc.LARGE_CASES)
def test_large_lattices_equal_the_model(name):
    """phi and the four counters, bit for bit: as given, built a second time, and with the triangles in another order"""
    want, stats = mc.large_model(name)
    grid = mc.large_grid_of(name)
    with _ctx() as c:
        ob, got = _build_large(c, mc.large_case(name))
        assert ob["dims"] == grid["dims"] and ob["spacing"] == grid["spacing"]
        _same(ob["origin"], grid["origin"])
        _same(ob["phi"], want, name)
        assert got == stats, (got, stats)
        again, got = _build_large(c, mc.large_case(name))
        _same(again["phi"], ob["phi"], name + " built twice")
        assert got == stats
        ob, got = _build_large(c, mc.large_permuted(name))
        _same(ob["phi"], want, name + " permuted")
        assert got == stats


def test_the_device_form_with_a_thousand_skipped_blocks():
    """More blocks of 256 triangles than the second scan level takes at a time, nearly all without a tile (mc.sparse_blocks): the 320
    used triangles give the field and the counters of `ico_rotated` alone."""
    v, tri, at = mc.sparse_blocks()
    nt = len(tri)
    want, stats = mc.model("ico_rotated")
    band = mc.case("ico_rotated")[2]
    assert stats == (320, 0, 0, 0) and len(at) == 320
    dv, dt = torch.from_numpy(v).cuda(), torch.from_numpy(tri.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    L = capi.load()
    with _ctx() as c:
        p = capi.ObstacleMeshParams(S, band, 0)
        lo, hi = (C.c_float * 3)(*mc.BMIN), (C.c_float * 3)(*mc.BMAX)
        for _ in range(2):
            assert L.sph_obstacle_build_mesh_dev(c.h, C.byref(p), lo, hi, len(v), dv.data_ptr(), nt, dt.data_ptr()) == 0
            _same(c.obstacle(read=True)["phi"], want)
            assert c.obstacle_mesh_stats() == (320, nt - 320, 0, 0)

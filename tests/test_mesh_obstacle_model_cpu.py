"""CPU: the numpy model of the mesh voxeliser (tests/mesh_obstacle_model.py, include/sph_hip.h: sph_obstacle_build_mesh) held to a
float64 brute force written here -- Ericson's closest point on a triangle for the distance, the solid angle the mesh subtends for
the side -- and to the properties the rule promises: even columns for closed meshes, bits that do not depend on the order of the
triangles, a sign that does not depend on the winding, an exact negation under `invert`.  Also the binding."""
import ctypes as C

import numpy as np
import pytest

import mesh_model
import mesh_obstacle_cases as mc
import mesh_obstacle_model as mm
import obstacle_model as om
from gpufluidsimulator_amd import capi

F = np.float32
S = float(mc.S)
CLOSED = [n for n in mc.CASES if mc.case(n)[4]]
# ||phi| - float64 distance| over the nodes with |phi| < W, in spacings.  Worst cases measured on these inputs: 1.71e-6 (free_box
# at band 16, where distances reach 16 s), 5.45e-7 at band <= 3 (free_box; 8.9e-8 on aligned_box, 4.8e-7 on ico_rotated).  The
# bar is four times the worst.
DISTANCE_BAR = 4 * 1.71e-6


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _nodes(grid):
    x, y, z = om.node_positions(grid)
    return np.stack(np.meshgrid(z, y, x, indexing="ij")[::-1], -1).reshape(-1, 3).astype(np.float64)


def _closest_d2(P, a, b, c):
    """squared distance of the points P to the triangle a, b, c: the regions of Ericson, Real-Time Collision Detection 5.1.5"""
    ab, ac, ap, bp, cp = b - a, c - a, P - a, P - b, P - c
    d1, d2, d3, d4, d5, d6 = ap @ ab, ap @ ac, bp @ ab, bp @ ac, cp @ ab, cp @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    q = np.empty((len(P), 3))
    done = np.zeros(len(P), bool)

    def put(mask, point):
        mask = mask & ~done
        q[mask] = point[mask] if point.ndim == 2 else point
        done[mask] = True

    with np.errstate(all="ignore"):
        put((d1 <= 0) & (d2 <= 0), a)
        put((d3 >= 0) & (d4 <= d3), b)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[:, None] * ab)
        put((d6 >= 0) & (d5 <= d6), c)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[:, None] * ac)
        put((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (c - b))
        den = 1.0 / (va + vb + vc)
        put(np.ones(len(P), bool), a + ab * (vb * den)[:, None] + ac * (vc * den)[:, None])
    return ((P - q) ** 2).sum(axis=1)


def _truth(P, vertices, triangles):
    """(distance to the mesh, inside) of the points P in float64; inside from the winding number (van Oosterom and Strackee)"""
    V = vertices.astype(np.float64)
    d2, w = np.full(len(P), np.inf), np.zeros(len(P))
    for t in triangles.astype(np.int64):
        a, b, c = V[t[0]], V[t[1]], V[t[2]]
        if not np.cross(b - a, c - a).any():               # no area: its edges are its neighbours' too
            continue
        d2 = np.minimum(d2, _closest_d2(P, a, b, c))
        A, B, Cc = a - P, b - P, c - P
        la, lb, lc = (np.linalg.norm(x, axis=1) for x in (A, B, Cc))
        num = np.einsum("ij,ij->i", A, np.cross(B, Cc))
        den = la * lb * lc + (A * B).sum(1) * lc + (B * Cc).sum(1) * la + (Cc * A).sum(1) * lb
        w += 2.0 * np.arctan2(num, den)
    return np.sqrt(d2), np.abs(w) / (4.0 * np.pi) > 0.5


@pytest.mark.parametrize("name", CLOSED)
def test_the_model_against_float64(name):
    v, t, band, _, _ = mc.case(name)
    grid = mc.grid_of(name)
    phi = mc.model(name)[0].reshape(-1).astype(np.float64)
    W = float(F(F(band) * mc.S))
    in_band = np.nonzero(np.abs(phi) < W)[0]
    rest = np.nonzero(np.abs(phi) >= W)[0]
    rng = np.random.default_rng(1)
    if len(t) > 1000:                                      # the large meshes: a sample of the band
        in_band = rng.choice(in_band, 800, replace=False)
    rest = rng.choice(rest, min(len(rest), 1500), replace=False)
    assert len(in_band) >= 800
    sel = np.concatenate([in_band, rest])
    d, inside = _truth(_nodes(grid)[sel], v, t)
    m = np.arange(len(sel)) < len(in_band)
    worst = float(np.abs(np.abs(phi[sel]) - d)[m].max()) / S
    print(f"{name}: worst distance error {worst:.3g} spacings over {m.sum()} nodes")
    assert worst <= DISTANCE_BAR, worst
    assert (d[~m] >= W * (1 - 1e-6)).all()                 # flat at +-W only where the surface is that far
    far = d > 0.25 * S
    assert far.sum() > 0.8 * len(sel)
    assert np.array_equal((phi[sel] < 0)[far], inside[far]), int(((phi[sel] < 0) != inside)[far].sum())
    assert 100 < inside.sum() < len(sel) - 100


@pytest.mark.parametrize("name,lo,hi", [("aligned_box", (-0.5, -0.375, -0.25), (0.25, 0.5, 0.375)),
                                       ("free_box", (-0.53, -0.41, -0.27), (0.29, 0.47, 0.36))])
def test_the_boxes_against_the_analytic_box(name, lo, hi):
    lo, hi = np.array(lo, F).astype(np.float64), np.array(hi, F).astype(np.float64)
    sh = {"kind": om.BOX, "invert": False, "a": (lo + hi) / 2, "b": (hi - lo) / 2, "r": 0.0}       # (the mesh's corners, in float64)
    assert np.array_equal(sh["a"] - sh["b"], lo) and np.array_equal(sh["a"] + sh["b"], hi)
    grid = mc.grid_of(name)
    want = om.analytic(sh, _nodes(grid))
    phi = mc.model(name)[0].reshape(-1).astype(np.float64)
    W = 3 * S
    m = np.abs(phi) < W
    assert m.sum() > 4000
    # outside, the analytic distance is the distance to the surface; inside a box it is too (the nearest face)
    assert np.abs(phi[m] - want[m]).max() / S <= DISTANCE_BAR
    far = np.abs(want) > 0.25 * S
    assert np.array_equal((phi < 0)[far], (want < 0)[far])
    assert (np.abs(want[~m]) >= W * (1 - 1e-6)).all()


@pytest.mark.parametrize("name", mc.CASES)
def test_closed_meshes_have_even_columns(name):
    v, t, _, _, closed = mc.case(name)
    used, skipped, lost, odd = mc.model(name)[1]
    assert used == len(t) and skipped == 0
    if closed:
        assert mesh_model.check_closed_oriented(t) is None or name == "ico_snapped"
        assert (lost, odd) == (0, 0)
    else:
        assert odd > 0


def test_the_cases_exercise_what_they_are_for():
    # aligned_box: every vertex on a node plane of every axis
    v = mc.case("aligned_box")[0]
    assert np.array_equal(v * 16, np.round(v * 16))
    v = mc.case("free_box")[0]
    assert (np.abs(v * 16 - np.round(v * 16)) > 0.05).all()
    # ico_snapped: triangles edge-on to the ray (n.x = 0) or without area
    v, t, _, _, _ = mc.case("ico_snapped")
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert (n[:, 0] == 0).sum() >= 1
    # mixed_sizes: triangles of very different sizes share one work list
    v, t, band, _, _ = mc.case("mixed_sizes")
    tiles = mm.distance_tiles(mc.grid_of("mixed_sizes"), v, t, band)
    assert (tiles > 1).sum() >= 1 and (tiles == 1).sum() >= 4000, np.bincount(tiles)
    # clipped: the lattice cuts the mesh on either side in x, and crossings land in the overflow mark
    grid = mc.grid_of("clipped")
    x = om.node_positions(grid)[0]
    v, t, band, _, _ = mc.case("clipped")
    assert v[:, 0].min() < x[0] and v[:, 0].max() > x[-1] and max(grid["dims"]) <= 35
    marks = mm.raw(grid, v, t, band)[1]
    assert marks[:, :, 0].sum() > 50 and marks[:, :, grid["dims"][0]].sum() > 50
    # the bands at both ends of the range
    assert mm.MAX_BAND == capi.OBSTACLE_MESH_MAX_BAND == 16 and mc.case("free_box_band16")[2] == 16 and mc.case("free_box_band1")[2] == 1
    for name in mc.CASES:
        assert max(mc.grid_of(name)["dims"]) <= 35


@pytest.mark.parametrize("name", ["aligned_box", "free_box", "ico_rotated", "ico_snapped", "clipped", "open_box", "mixed_sizes"])
def test_the_order_of_the_triangles_does_not_matter(name):
    v, t, band, _, _ = mc.permuted(name)
    assert not np.array_equal(t, mc.case(name)[1])
    phi, stats = mm.build(mc.grid_of(name), v, t, band)
    want, want_stats = mc.model(name)
    assert np.array_equal(_bits(phi), _bits(want)) and stats == want_stats


@pytest.mark.parametrize("name", ["aligned_box", "free_box", "ico_rotated", "ico_snapped", "clipped", "open_box"])
def test_the_winding_does_not_matter(name):
    """Reversed triangles (A, C, B): n becomes -n exactly, so the plane term, every crossing and every mark keep their bits.  A
    reversed triangle walks its segments from their other ends -- which is how its neighbour across each edge walked them before:
    in a closed, consistently wound mesh the minimum runs over the same set of directed segments, and the field keeps every bit.
    The rim of an open mesh has no such neighbour: there the side is held exactly and the distance to the rounding bar."""
    v, t, band, _, closed = mc.case(name)
    grid = mc.grid_of(name)
    phi, stats = mm.build(grid, v, t[:, [0, 2, 1]], band)
    want, want_stats = mc.model(name)
    assert stats == want_stats
    assert np.array_equal(mm.raw(grid, v, t, band)[1], mm.raw(grid, v, t[:, [0, 2, 1]], band)[1])
    if closed:
        assert np.array_equal(_bits(phi), _bits(want))
    else:
        assert np.array_equal(np.signbit(phi), np.signbit(want))
        assert np.abs(phi.astype(np.float64) - want).max() / S <= DISTANCE_BAR


def test_invert_negates_bit_for_bit():
    for name in ("free_box", "ico_snapped"):
        a, sa = mc.model(name)
        b, sb = mc.model(name, True)
        assert np.array_equal(_bits(b), _bits(-a)) and sa == sb
        assert (a < 0).sum() > 1000 and (b < 0).sum() > (a < 0).sum()


def test_bad_triangles_are_skipped_and_counted():
    v, t, band, _, _ = mc.case("free_box")
    v, t = v.copy(), np.concatenate([t, [[0, 1, 8], [2, 0xFFFFFFFF, 3]]]).astype(np.uint32)
    v = np.concatenate([v, [[np.inf, 0.0, 0.0]]]).astype(F)
    t = np.concatenate([t, [[8, 1, 2]]]).astype(np.uint32)
    phi, stats = mm.build(mc.grid_of("free_box"), v, t, band)
    assert stats == (12, 3, 0, 0)
    assert np.array_equal(_bits(phi), _bits(mc.model("free_box")[0]))


def test_binding_carries_the_struct_and_the_four_calls():
    """sph_obstacle_mesh_params is 12 bytes, field for field; the library exports the four entry points with these signatures."""
    assert C.sizeof(capi.ObstacleMeshParams) == 12
    assert [f[0] for f in capi.ObstacleMeshParams._fields_] == ["spacing", "band", "invert"]
    assert capi.ObstacleMeshParams.band.offset == 4 and capi.ObstacleMeshParams.invert.offset == 8
    lib = capi.load()
    for name in ("sph_obstacle_build_mesh", "sph_obstacle_build_mesh_dev", "sph_obstacle_build_obj", "sph_obstacle_mesh_stats"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    for name in ("build_obstacle_mesh", "build_obstacle_from_mesh", "build_obstacle_obj", "obstacle_mesh_stats"):
        assert callable(getattr(capi.Context, name))
    # a null context is refused before anything touches a device
    out = (C.c_uint64 * 4)()
    assert lib.sph_obstacle_mesh_stats(None, out) == -1
    assert lib.sph_obstacle_build_mesh(None, None, None, None, 0, None, 0, None) == -1
    assert lib.sph_obstacle_build_mesh_dev(None, None, None, None, 0, None, 0, None) == -1
    assert lib.sph_obstacle_build_obj(None, None, None, None, None) == -1

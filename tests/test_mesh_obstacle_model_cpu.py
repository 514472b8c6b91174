"""CPU: the numpy model of the mesh voxeliser (tests/mesh_obstacle_model.py, include/sph_hip.h: sph_obstacle_build_mesh) held to a
float64 brute force written here -- Ericson's closest point on a triangle for the distance, the solid angle the mesh subtends for
the side -- and to the properties the rule promises: even columns for closed meshes, bits that do not depend on the order of the
triangles, a sign that does not depend on the winding, an exact negation under `invert`.  Also the binding."""
import ctypes as C
import os
import re

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
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpufluidsimulator_amd", "csrc")
# ||phi| - float64 distance| over the nodes with |phi| < W, in spacings.  Worst cases measured on these inputs: 1.71e-6 (free_box
# at band 16, where distances reach 16 s), 5.45e-7 at band <= 3 (free_box; 8.9e-8 on aligned_box, 4.8e-7 on ico_rotated).  The
# bar is four times the worst.
DISTANCE_BAR = 4 * 1.71e-6
# The large lattices (mc.LARGE_CASES) have bars of their own: the rounding error follows the size of the coordinates and not the
# spacing, so in spacings it grows as s shrinks.  Worst cases measured over every node of the band (many_tiles: over 8000 of its
# 11,470), in spacings (and in absolute units): long_x, s = 1/64, band 3: 4.54e-7 (7.1e-9); wide_yz, s = 1/80, band 3, faces of
# 1.1 x 1.9: 6.33e-6 (7.9e-8); many_tiles, s = 1/64, band 1, where no distance exceeds s: 5.96e-8 (9.3e-10, an ulp of s / 2).
# Each case is held to four times its own worst.
LARGE_WORST = {"long_x": 4.54e-7, "wide_yz": 6.33e-6, "many_tiles": 5.96e-8}


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


def _against_float64(name, v, t, band, grid, phi, bar, most=None):
    """the model's phi of a closed mesh against _truth: the distance in the band to `bar` spacings, the side beyond a quarter
    spacing exactly.  Meshes of more than 1000 triangles: a sample of 800 band nodes; `most`: a sample of smaller meshes' too."""
    s = float(grid["spacing"])
    phi = phi.reshape(-1).astype(np.float64)
    W = float(F(F(band) * grid["spacing"]))
    in_band = np.nonzero(np.abs(phi) < W)[0]
    rest = np.nonzero(np.abs(phi) >= W)[0]
    rng = np.random.default_rng(1)
    if len(t) > 1000:                                      # the large meshes: a sample of the band
        in_band = rng.choice(in_band, 800, replace=False)
    elif most is not None and len(in_band) > most:         # the large lattices
        in_band = rng.choice(in_band, most, replace=False)
    rest = rng.choice(rest, min(len(rest), 1500), replace=False)
    assert len(in_band) >= 800
    sel = np.concatenate([in_band, rest])
    d, inside = _truth(_nodes(grid)[sel], v, t)
    m = np.arange(len(sel)) < len(in_band)
    worst = float(np.abs(np.abs(phi[sel]) - d)[m].max()) / s
    print(f"{name}: worst distance error {worst:.3g} spacings ({worst * s:.3g}) over {m.sum()} nodes")
    assert worst <= bar, worst
    assert (d[~m] >= W * (1 - 1e-6)).all()                 # flat at +-W only where the surface is that far
    far = d > 0.25 * s
    assert far.sum() > 0.8 * len(sel)
    assert np.array_equal((phi[sel] < 0)[far], inside[far]), int(((phi[sel] < 0) != inside)[far].sum())
    assert 100 < inside.sum() < len(sel) - 100


@pytest.mark.parametrize("name", CLOSED)
def test_the_model_against_float64(name):
    v, t, band, _, _ = mc.case(name)
    _against_float64(name, v, t, band, mc.grid_of(name), mc.model(name)[0], DISTANCE_BAR)


@pytest.mark.parametrize("name", sorted(LARGE_WORST))
def test_the_model_against_float64_on_the_large_lattices(name):
    """node coordinates (float)i * s with i beyond 128, at s = 1/64 and 1/80"""
    v, t, band, _, _, _ = mc.large_case(name)
    _against_float64(name, v, t, band, mc.large_grid_of(name), mc.large_model(name)[0], 4 * LARGE_WORST[name], most=6000)


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


@pytest.mark.parametrize("name", mc.LARGE_CASES)
def test_the_large_cases_are_closed_and_have_even_columns(name):
    v, t, _, _, closed, _ = mc.large_case(name)
    assert closed and mesh_model.check_closed_oriented(t) is None
    assert mc.large_model(name)[1] == (len(t), 0, 0, 0)
    assert np.prod(mc.large_grid_of(name)["dims"]) < 500_000


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


def _constants():
    """the constants of the voxeliser's work list, from the source text: a case below that a changed constant no longer sends down
    its path fails its condition here instead of passing on the device for nothing"""
    src = open(os.path.join(CSRC, "sph_obstacle_mesh.hip")).read()
    k = {n: int(re.search(r"constexpr uint32_t OBMESH_%s = (\d+);" % n, src).group(1)) for n in ("THREADS", "TILE_ROWS", "SCAN2", "MAX_BLOCKS")}
    k["WAVE"] = int(re.search(r"constexpr int WAVE = (\d+);", open(os.path.join(CSRC, "sph_common.hpp")).read()).group(1))
    assert re.search(r"constexpr uint32_t OBMESH_WAVES = OBMESH_THREADS / WAVE;", src)
    assert re.search(r"L\.words = ceil_div\(G\.dims\[0\] \+ 1u, 32u\);", src)
    return k


def _ceil_div(a, b):
    return -(-a // b)


def _extents(name):
    v, t, band, _, _, _ = mc.large_case(name)
    return mm.tile_extents(mc.large_grid_of(name), v, t, band)


def test_the_large_cases_reach_the_paths_they_are_for():
    """Each condition is read off the model's index boxes (mm.tile_extents: the `across` and `rows` of k_obmesh_count) and the
    constants of csrc/sph_obstacle_mesh.hip.  No kernel is altered to see a test bite: a wrong decode of a tile writes out of bounds."""
    K = _constants()
    wave, rows, waves = K["WAVE"], K["TILE_ROWS"], K["THREADS"] // K["WAVE"]
    assert (mm.TILE_X, mm.TILE_ROWS) == (wave, rows)
    # long_x: a triangle of three chunks along x (3 tells `local % chunks` from `local / chunks` where 2 might not), and
    # triangles of one chunk in the same list
    e = _extents("long_x")
    chunks = _ceil_div(e[:, 0], wave)
    assert chunks.max() >= 3 and (chunks == 1).sum() >= 10, np.bincount(chunks)
    # the exact edges of a chunk: every lane of one chunk active; a second chunk with one active lane
    for name, across in (("across_64", wave), ("across_65", wave + 1)):
        assert mc.large_grid_of(name)["dims"][0] == across and _extents(name)[:, 0].max() == across, name
    # wide_yz: one triangle with two chunks of columns AND two row groups in the crossing pass, and over a hundred row groups
    # in the distance pass
    e = _extents("wide_yz")
    both = (_ceil_div(e[:, 2], wave) >= 2) & (_ceil_div(e[:, 3], rows) >= 2)
    assert both.any() and _ceil_div(e[both, 1], rows).max() > 100, e
    # ... and the exact edges of a row group, in both passes, under a triangle that covers every column
    for name, n in (("rows_128", rows), ("rows_129", rows + 1)):
        d = mc.large_grid_of(name)["dims"]
        assert d[1] * d[2] == n and _extents(name)[:, 1].max() == n, name
    for name, n in (("cross_rows_128", rows), ("cross_rows_129", rows + 1)):
        assert mc.large_grid_of(name)["dims"][2] == n and _extents(name)[:, 3].max() == n, name
    # many_tiles: either pass has more tiles than the largest launch has waves, so `tile += stride` is taken; the launch is the
    # largest (`blocks` of obmesh_build_dev); in the first block of triangles the counts are unequal
    launch_waves = K["MAX_BLOCKS"] * K["THREADS"] // wave
    v, t, band, _, _, _ = mc.large_case("many_tiles")
    grid = mc.large_grid_of("many_tiles")
    td, tx = mm.distance_tiles(grid, v, t, band), mm.crossing_tiles(grid, v, t, band)
    assert td.sum() > launch_waves and tx.sum() > launch_waves, (td.sum(), tx.sum())
    nx, ny, nz = grid["dims"]
    most = len(t) * _ceil_div(nx, wave) * _ceil_div(ny * nz, rows)
    assert min(K["MAX_BLOCKS"], _ceil_div(most, waves)) == K["MAX_BLOCKS"]
    first = slice(0, K["THREADS"])
    assert td[first].max() >= 6 and (td[first] == 1).sum() > 100 and tx[first].max() >= 2 and (tx[first] == 1).sum() > 100
    e = _extents("many_tiles")                              # (the slab: three chunks and two row groups in one triangle; two chunks)
    assert ((_ceil_div(e[:, 0], wave) >= 3) & (_ceil_div(e[:, 1], rows) >= 2)).any() and _ceil_div(e[:, 2], wave).max() >= 2
    # the mark words: crossings in the overflow mark n_x of every lattice, a crossing in the first word of columns that are
    # inside at i >= 64, i.e. two whole words and more behind it, wherever n_x allows; every word count from 1 to 4
    words = []
    for nx in mc.MARK_NX:
        name = "marks_%d" % nx
        v, t, band, _, _, _ = mc.large_case(name)
        grid = mc.large_grid_of(name)
        assert grid["dims"][0] == nx and v[:, 0].max() > om.node_positions(grid)[0][-1] + 0.1
        marks = mm.raw(grid, v, t, band)[1]
        assert marks[:, :, nx].sum() > 50, (name, marks[:, :, nx].sum())
        first = marks[:, :, :32].any(axis=2)
        assert first.sum() > 5
        if nx > 64:
            inside = mc.large_model(name)[0][:, :, 64:] < 0
            assert inside.sum() > 50 and (inside.any(axis=2) & first).sum() > 5, name
        words.append(_ceil_div(nx + 1, 32))
    assert words == [1, 2, 2, 2, 3, 3, 3, 4, 4]


def test_the_sparse_list_has_its_blocks_where_the_scan_turns():
    """sparse_blocks(): used triangles in blocks below and at or above OBMESH_SCAN2 (the second level's carry), a long run of blocks
    without a tile (equal bases in obmesh_find's first search), a partial last block, blocks that begin and end with skipped
    triangles -- and the model of the whole list is the model of `ico_rotated`."""
    K = _constants()
    block, scan2 = K["THREADS"], K["SCAN2"]
    assert block == mc.SPARSE_BLOCK
    v, tri, at = mc.sparse_blocks()
    nt = len(tri)
    ok = mm.good_triangles(v, tri)
    assert nt == mc.SPARSE_NT and nt % block != 0 and _ceil_div(nt, block) > scan2 + 1
    assert np.array_equal(np.nonzero(ok)[0], at) and len(at) == 320
    used = np.bincount(at // block, minlength=_ceil_div(nt, block))
    assert used[0] > 0 and used[scan2 - 1] > 0 and used[scan2] > 0 and used[-1] > 0 and used[:scan2].sum() > 0 < used[scan2:].sum()
    assert (used[1:101] == 0).all() and (used == 0).sum() > scan2 - 10            # a run of a hundred empty blocks, and more
    assert not ok[0] and not ok[block - 1]                                         # block 0 begins and ends with skipped ones
    assert ok[scan2 * block - 1] and ok[scan2 * block] and ok[nt - 1]              # used on both sides of the boundary; the end
    for kind in ((tri >= len(v)).any(axis=1), (tri == 0xFFFFFFFF).any(axis=1)):    # every way of being skipped, many times
        assert kind.sum() > 1000
    fin = np.isfinite(v).all(axis=1)
    assert (~fin).sum() == 2 and np.isnan(v).any() and np.isinf(v).any()
    in_range = (tri < len(v)).all(axis=1)
    assert (in_range & ~ok).sum() > 1000
    _, t, band, _, _ = mc.case("ico_rotated")
    assert np.array_equal(tri[at], t)
    phi, stats = mm.build(mc.grid_of("ico_rotated"), v, tri, band)
    want, _ = mc.model("ico_rotated")
    assert np.array_equal(_bits(phi), _bits(want)) and stats == (320, nt - 320, 0, 0)


# many_tiles is left out: its model takes four seconds a build, and the device is given its permuted twin (tests/test_gpu_obstacle_mesh.py)
@pytest.mark.parametrize("name", [n for n in mc.LARGE_CASES if n != "many_tiles"])
def test_the_order_of_the_triangles_does_not_matter_on_the_large_lattices(name):
    v, t, band, _, _, _ = mc.large_permuted(name)
    assert not np.array_equal(t, mc.large_case(name)[1])
    phi, stats = mm.build(mc.large_grid_of(name), v, t, band)
    want, want_stats = mc.large_model(name)
    assert np.array_equal(_bits(phi), _bits(want)) and stats == want_stats


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

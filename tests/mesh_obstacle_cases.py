"""The inputs of the mesh-obstacle tests (tests/test_mesh_obstacle_model_cpu.py, tests/test_gpu_obstacle_mesh.py): triangle meshes
in a box of edge 2.  Each case is (vertices float32[nv, 3], triangles uint32[nt, 3], band, bounds); `closed` says whether every
column must come out even.  The model's result of a case is computed once and shared.

CASES: lattices of at most 35^3 nodes at s = 1/16 -- the arithmetic of the rule on one tile per triangle and two mark words.
LARGE_CASES: lattices of up to 163 nodes on an axis at s = 1/16 .. 1/80 (a case of these carries its spacing) -- the work list
of csrc/sph_obstacle_mesh.hip beyond one tile per triangle: several 64-node chunks and 128-row groups in both passes and their
exact edges, one to four mark words, more tiles than a launch has waves.  sparse_blocks(): a triangle list of more than 1024
blocks of 256, nearly all skipped, for the device form.  What each of them reaches is asserted from the model's index boxes in
tests/test_mesh_obstacle_model_cpu.py."""
import functools

import numpy as np

import mesh_model
import mesh_obstacle_model as mm

F = np.float32
S = F(1.0 / 16.0)
BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)          # the context: cell edge 1/16
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
CLIP_BOUNDS = ((-0.3, -0.4, -1.0), (0.4, 1.0, 0.3))


def box_mesh(lo, hi):
    """12 triangles, outward wound"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)], F)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    t = [(a, b, c) for a, b, c, d in quads] + [(a, c, d) for a, b, c, d in quads]
    return v, np.array(t, np.uint32)


def icosphere(level, radius, centre, rotation_seed=None):
    """20 * 4^level triangles, outward wound; rotated by a seeded random rotation"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, t2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            t2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = t2
    v = np.array(v)
    if rotation_seed is not None:
        q, r = np.linalg.qr(np.random.default_rng(rotation_seed).normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        v = v @ q.T
    return (v * radius + np.asarray(centre, np.float64)).astype(F), np.array(t, np.uint32)


def split_box(lo, hi, n=32):
    """a closed box whose two x faces are n x n squares of two triangles each; the four side faces are strips that share every
    vertex of the fine faces' rims (no T-junction: each edge belongs to exactly two triangles)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ys, zs = np.linspace(lo[1], hi[1], n + 1), np.linspace(lo[2], hi[2], n + 1)
    verts, tris = [], []
    face = {}
    for side, x in ((0, lo[0]), (1, hi[0])):
        for a in range(n + 1):
            for b in range(n + 1):
                face[side, a, b] = len(verts)
                verts.append((x, ys[a], zs[b]))
        for a in range(n):
            for b in range(n):
                p, q, r, s = face[side, a, b], face[side, a + 1, b], face[side, a + 1, b + 1], face[side, a, b + 1]
                tris += [(p, s, r), (p, r, q)] if side == 0 else [(p, q, r), (p, r, s)]
    rim = [(a, 0) for a in range(n)] + [(n, b) for b in range(n)] + [(a, n) for a in range(n, 0, -1)] + [(0, b) for b in range(n, 0, -1)]
    for k in range(len(rim)):                          # a strip round the box between the two rims
        (a0, b0), (a1, b1) = rim[k], rim[(k + 1) % len(rim)]
        p, q, r, s = face[0, a0, b0], face[0, a1, b1], face[1, a1, b1], face[1, a0, b0]
        tris += [(p, q, r), (p, r, s)]
    return np.array(verts, F), np.array(tris, np.uint32)


def join(*meshes):
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + np.uint32(base))
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts)


@functools.lru_cache(maxsize=None)
def blob_particles():
    return np.random.default_rng(500).uniform(-0.28, 0.28, (500, 3)).astype(F)


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, triangles, band, bounds, closed)"""
    free = box_mesh((-0.53, -0.41, -0.27), (0.29, 0.47, 0.36))
    if name == "aligned_box":
        return box_mesh((-0.5, -0.375, -0.25), (0.25, 0.5, 0.375)) + (3, None, True)
    if name == "free_box":
        return free + (3, None, True)
    if name in ("free_box_band1", "free_box_band16"):
        return free + (int(name[13:]), None, True)
    if name == "ico_rotated":
        return icosphere(2, 0.6, (0.03, -0.05, 0.02), 7) + (3, None, True)
    if name == "ico_snapped":
        v, t = icosphere(2, 0.6, (0.03, -0.05, 0.02), 7)
        return (np.round(v.astype(np.float64) * 32.0) / 32.0).astype(F), t, 3, None, True
    if name == "blob":
        _, _, _, v, _, t = mesh_model.mesh_of(blob_particles(), BMIN, BMAX, F(1.0 / 64.0), spacing=float(S))
        return v, t, 3, None, True
    if name == "mixed_sizes":
        v, t = join(split_box((-0.83, -0.31, -0.29), (-0.17, 0.33, 0.27)), box_mesh((0.13, -0.31, -0.29), (0.79, 0.33, 0.27)))
        return v, t, 3, None, True
    if name == "clipped":
        return icosphere(2, 0.6, (0.03, -0.05, 0.02), 7) + (3, CLIP_BOUNDS, True)
    if name == "open_box":
        return free[0], free[1][1:].copy(), 3, None, False       # (without a triangle of the x = lo face)
    raise KeyError(name)


CASES = ("aligned_box", "free_box", "ico_rotated", "ico_snapped", "blob", "mixed_sizes", "clipped", "open_box", "free_box_band1",
         "free_box_band16")


def grid_of(name):
    lo, hi = case(name)[3] or (BMIN, BMAX)
    return mm.lattice(S, lo, hi)


@functools.lru_cache(maxsize=None)
def model(name, invert=False):
    """(phi, stats) of the case by the model; shared and left unchanged"""
    v, t, band, _, _ = case(name)
    phi, stats = mm.build(grid_of(name), v, t, band, invert)
    phi.setflags(write=False)
    return phi, stats


def permuted(name, seed=11):
    v, t, band, bounds, closed = case(name)
    return v, t[np.random.default_rng(seed).permutation(len(t))], band, bounds, closed


# ---- the large lattices: (vertices, triangles, band, bounds, closed, spacing) ----------------------------------------------------------
MARK_NX = (31, 32, 33, 63, 64, 65, 95, 96, 97)          # 1, 2, 2, 2, 3, 3, 3, 4, 4 mark words
S64 = F(1.0 / 64.0)
SLAB = ((-0.97, -0.02, -0.16), (0.97, 0.99, 0.15))       # at s = 1/64: more than 128 nodes along x, more than 64 columns along y


def _marks_bounds(nx):
    """the lattice of s = 1/32 with nx nodes along x from x = -1 - s on, and 32 along y and z"""
    return (-1.0, -0.45, -0.45), (-1.0 + (nx - 3) / 32.0, 0.45, 0.45)


@functools.lru_cache(maxsize=None)
def large_case(name):
    """(vertices, triangles, band, bounds, closed, spacing)"""
    if name == "long_x":
        # a box of three 64-node chunks along x and, in the same work list, its two x faces and a small sphere of one chunk
        v, t = join(box_mesh((-0.97, -0.15, -0.06), (0.97, -0.03, 0.05)), icosphere(1, 0.07, (0.31, 0.09, 0.0), 3))
        return v, t, 3, ((-1.0, -0.2, -0.1), (1.0, 0.2, 0.1)), True, S64
    if name in ("across_64", "across_65"):
        # n_x = 64 and 65, and a box through both x ends of the lattice: the banded range is the whole axis
        hi_x = -0.5 + (int(name[7:]) - 3) / 64.0
        return box_mesh((-0.7, -0.05, -0.04), (0.7, 0.06, 0.05)) + (3, ((-0.5, -0.1, -0.1), (hi_x, 0.1, 0.1)), True, S64)
    if name == "wide_yz":
        # x faces of more than 64 columns and more than 128 rows in the crossing pass, over a hundred row groups in the distance pass
        return box_mesh((-0.04, -0.55, -0.95), (0.05, 0.54, 0.93)) + (3, ((-0.1, -0.6, -1.0), (0.1, 0.6, 1.0)), True, F(1.0 / 80.0))
    if name == "rows_128":
        # 8 x 16 columns; the box's x faces cover every one of them: 128 rows in the distance pass
        return box_mesh((-0.3, -0.9, -0.9), (0.3, 0.9, 0.9)) + (3, ((-0.5, -0.15, -0.4), (0.5, 0.15, 0.4)), True, S)
    if name == "rows_129":
        # 3 x 43 columns: 129 rows
        return box_mesh((-0.3, -0.5, -1.5), (0.3, 0.5, 1.5)) + (3, ((-0.5, 0.0, -1.25), (0.5, 0.0, 1.25)), True, S)
    if name in ("cross_rows_128", "cross_rows_129"):
        # n_z = 128 and 129 under x faces that cover every column: 128 and 129 rows in the crossing pass
        hi_z = -1.0 + (int(name[11:]) - 3) / 64.0
        return box_mesh((-0.05, -0.3, -1.2), (0.06, 0.3, 1.2)) + (3, ((-0.1, -0.1, -1.0), (0.1, 0.1, hi_z)), True, S64)
    if name.startswith("marks_"):
        # a sphere and a thin bar, both cut by the +x end of the lattice; the bar starts in the first mark word
        lo, hi = _marks_bounds(int(name[6:]))
        v, t = join(icosphere(1, 0.35, (hi[0] - 0.2, 0.03, -0.05), 5), box_mesh((-0.83, -0.41, 0.31), (hi[0] + 0.3, -0.33, 0.4)))
        return v, t, 3, (lo, hi), True, F(1.0 / 32.0)
    if name == "many_tiles":
        # 8,460 small triangles of one tile or a few each, and the twelve of a slab with several chunks in either pass: band 1 keeps
        # the model quick
        v, t = join(box_mesh(*SLAB), split_box((-0.83, -0.22, -0.16), (-0.41, -0.06, 0.17), n=45))
        return v, t, 1, ((-1.0, -0.25, -0.2), (1.0, 1.0, 0.2)), True, S64
    raise KeyError(name)


EDGE_CASES = ("across_64", "across_65", "rows_128", "rows_129", "cross_rows_128", "cross_rows_129")
MARK_CASES = tuple("marks_%d" % n for n in MARK_NX)
LARGE_CASES = ("long_x", "wide_yz", "many_tiles") + EDGE_CASES + MARK_CASES


def large_grid_of(name):
    _, _, _, (lo, hi), _, s = large_case(name)
    return mm.lattice(s, lo, hi)


@functools.lru_cache(maxsize=None)
def large_model(name):
    """(phi, stats) of the large case by the model; shared and left unchanged"""
    v, t, band, _, _, _ = large_case(name)
    phi, stats = mm.build(large_grid_of(name), v, t, band)
    phi.setflags(write=False)
    return phi, stats


def large_permuted(name, seed=11):
    v, t, band, bounds, closed, s = large_case(name)
    return v, t[np.random.default_rng(seed).permutation(len(t))], band, bounds, closed, s


# ---- more than 1024 blocks of 256 triangles, nearly all of them skipped -----------------------------------------------------------------
SPARSE_BLOCK = 256
SPARSE_NT = 1027 * SPARSE_BLOCK - 100
# where the 320 triangles of `ico_rotated` go, as (first position, how many): in block 0 behind five skipped ones; across the
# boundary of blocks 700 and 701, after 699 wholly skipped blocks; across the boundary of blocks 1023 and 1024; the last 100
# positions, which are the end of the partial block 1026
SPARSE_RUNS = ((5, 40), (700 * SPARSE_BLOCK + 200, 100), (1024 * SPARSE_BLOCK - 30, 80), (SPARSE_NT - 100, 100))


@functools.lru_cache(maxsize=None)
def sparse_blocks():
    """(vertices, triangles, positions of the used triangles): the mesh of `ico_rotated` scattered through SPARSE_NT triangles that
    the device form skips -- an index equal to and far beyond the vertex count, 0xFFFFFFFF, a NaN and an infinite vertex"""
    v, t, _, _, _ = case("ico_rotated")
    nv = len(v) + 2
    v = np.concatenate([v, np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0]], F)])
    bad = np.array([[0, 1, nv], [nv - 2, 2, 3], [4, 0xFFFFFFFF, 5], [6, 7, nv - 1], [nv + 1000, 8, 9]], np.uint32)
    tri = bad[np.arange(SPARSE_NT) % len(bad)]
    at = np.concatenate([np.arange(a, a + n) for a, n in SPARSE_RUNS])
    assert len(at) == len(t) == 320
    tri[at] = t
    return v, np.ascontiguousarray(tri), at

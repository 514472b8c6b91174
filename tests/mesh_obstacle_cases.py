"""The inputs of the mesh-obstacle tests (tests/test_mesh_obstacle_model_cpu.py, tests/test_gpu_obstacle_mesh.py): triangle meshes
on lattices of at most 35^3 nodes at s = 1/16 in a box of edge 2.  Each case is (vertices float32[nv, 3], triangles uint32[nt, 3],
band, bounds); `closed` says whether every column must come out even.  The model's result of a case is computed once and shared."""
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

"""The rule of sph_mesh_extract (include/sph_hip.h) in numpy: the same fp32 operations in the same order, so that the counts, the
vertex positions, the normals and the triangles of the device come out bit for bit.  Also the checker of what a mesh must be:
closed, consistently oriented, its Euler characteristic and its signed volume.

Arrays of the lattice are indexed [k, j, i] (x fastest), as the device's linear index (k*n_y + j)*n_x + i."""
import itertools
import math

import numpy as np

F = np.float32
MAX_REACH, MAX_DIM, MAX_NODES = 8, 2048, 1 << 27

# the six Kuhn tetrahedra of a cube, as the corners (0, e_a, e_a | e_b, 7) of the axis orders xyz, xzy, yxz, yzx, zxy, zyx
TETS = [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in itertools.permutations(range(3))]


def resolve(particle_radius, spacing=0.0, radius=0.0, iso=0.0):
    """(s, r, iso_q) of the parameters, zeros replaced by their defaults"""
    s = F(spacing) if spacing > 0 else F(particle_radius)
    r = F(radius) if radius > 0 else F(3.0) * s
    iso = F(iso) if iso > 0 else F(0.5)
    v = iso * F(4096.0) + F(0.5)
    q = int(v) if v < F(4294967296.0) else 0xFFFFFFFF
    return s, r, max(1, q)


def lattice(box_min, box_max, s, r):
    """(dims (n_x, n_y, n_z), origin float32[3]): in double, each result rounded once; the origin's two operations in fp32"""
    pad = math.ceil(float(r) / float(s)) + 1
    dims = tuple(int(math.ceil((float(F(box_max[k])) - float(F(box_min[k]))) / float(s))) + 1 + 2 * pad for k in range(3))
    origin = np.array([F(box_min[k]) - F(pad) * F(s) for k in range(3)], F)
    return dims, origin


def node_coords(n, origin_k, s):
    return (F(origin_k) + np.arange(n, dtype=np.uint32).astype(F) * F(s)).astype(F)


def field(pos, dims, origin, s, r):
    """The counts: every particle against every node of a box of nodes around it that is wider than the kernel's walk (so the
    kernel's walk is held to be a superset of the nodes that pass)."""
    nx, ny, nz = dims
    s, r = F(s), F(r)
    r2 = r * r
    X = [node_coords(dims[k], origin[k], s) for k in range(3)]
    counts = np.zeros(nx * ny * nz, np.uint32)
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    reach = int(math.ceil(float(r) / float(s))) + 3
    off = np.arange(-reach, reach + 1)
    oz, oy, ox = np.meshgrid(off, off, off, indexing="ij")
    ox, oy, oz = ox.ravel(), oy.ravel(), oz.ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        centre = np.rint((pos.astype(np.float64) - origin.astype(np.float64)) / float(s))
    chunk = max(1, 4_000_000 // len(ox))
    for lo in range(0, len(pos), chunk):
        p = pos[lo:lo + chunk]
        c = centre[lo:lo + chunk]
        good = np.isfinite(c).all(axis=1) & (np.abs(c) < 1e6).all(axis=1)
        p, c = p[good], c[good].astype(np.int64)
        i, j, k = c[:, :1] + ox, c[:, 1:2] + oy, c[:, 2:3] + oz
        ok = (i >= 0) & (i < nx) & (j >= 0) & (j < ny) & (k >= 0) & (k < nz)
        ic, jc, kc = np.clip(i, 0, nx - 1), np.clip(j, 0, ny - 1), np.clip(k, 0, nz - 1)
        dx, dy, dz = X[0][ic] - p[:, :1], X[1][jc] - p[:, 1:2], X[2][kc] - p[:, 2:3]
        d2 = (dx * dx + dy * dy) + dz * dz
        hit = ok & (d2 < r2)
        t = F(1.0) - d2[hit] / r2
        w = (t * t) * t
        q = (w * F(4096.0) + F(0.5)).astype(np.uint32)
        np.add.at(counts, ((kc[hit] * ny + jc[hit]) * nx + ic[hit]), q)
    return counts.reshape(nz, ny, nx)


def _unit(v):
    return np.array([(v >> 0) & 1, (v >> 1) & 1, (v >> 2) & 1], float)


def case_table():
    """table[m][case] = the triangles of tetrahedron m whose corner t is inside iff bit t of case: each triangle three edges,
    each edge the positions (p, q), p < q, of its corners in the tetrahedron.  The winding comes from the geometry: every vertex
    at its edge's midpoint, the normal held against (centroid of the outside corners - centroid of the inside corners)."""
    table = []
    for tet in TETS:
        P = [_unit(c) for c in tet]
        row = []
        for case in range(16):
            ins = [t for t in range(4) if (case >> t) & 1]
            out = [t for t in range(4) if not (case >> t) & 1]
            e = lambda x, y: (min(x, y), max(x, y))
            if len(ins) in (1, 3):
                a = ins[0] if len(ins) == 1 else out[0]
                b, c, d = out if len(ins) == 1 else ins
                tris = [[e(a, b), e(a, c), e(a, d)]]
            elif len(ins) == 2:
                (a, b), (c, d) = ins, out
                tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
            else:
                tris = []
            if tris:
                direction = np.mean([P[t] for t in out], axis=0) - np.mean([P[t] for t in ins], axis=0)
            fixed = []
            for tri in tris:
                m = [0.5 * (P[p] + P[q]) for p, q in tri]
                sign = np.dot(np.cross(m[1] - m[0], m[2] - m[0]), direction)
                assert sign != 0
                fixed.append(tri if sign > 0 else [tri[0], tri[2], tri[1]])
            row.append(fixed)
        table.append(row)
    return table


def _shift(a, d, fill):
    """a[k + dz, j + dy, i + dx] for the direction bits d, `fill` where that leaves the lattice"""
    out = np.full_like(a, fill)
    dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
    nz, ny, nx = a.shape
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def _gradient(counts):
    """G per node [k, j, i, 3]: (float)((int64)C(+1) - (int64)C(-1)) per axis, outside the lattice counting 0"""
    c = np.pad(counts.astype(np.int64), 1)
    g = np.stack([c[1:-1, 1:-1, 2:] - c[1:-1, 1:-1, :-2], c[1:-1, 2:, 1:-1] - c[1:-1, :-2, 1:-1], c[2:, 1:-1, 1:-1] - c[:-2, 1:-1, 1:-1]],
                 axis=-1)
    return g.astype(F)


def extract(counts, origin, s, iso_q):
    """(pos[nv, 3] float32, normal[nv, 3] float32, tri[nt, 3] uint32) of the counts [n_z, n_y, n_x], in the rule's order"""
    nz, ny, nx = counts.shape
    s = F(s)
    inside = counts >= np.uint32(iso_q)
    exists = np.ones(counts.shape, bool)
    # the vertices: per node the mask of its seven directions
    owns = []
    mask = np.zeros(counts.shape, np.uint32)
    for d in range(1, 8):
        o = _shift(exists, d, False) & (_shift(inside, d, False) != inside)
        owns.append(o)
        mask |= o.astype(np.uint32) << np.uint32(d - 1)
    per_node = sum(o.astype(np.int64) for o in owns).ravel()
    vbase = np.concatenate([[0], np.cumsum(per_node)[:-1]]).reshape(counts.shape)
    nv = int(per_node.sum())
    pos, nrm = np.zeros((nv, 3), F), np.zeros((nv, 3), F)
    X = [node_coords(n, origin[a], s) for a, n in enumerate((nx, ny, nz))]
    G = _gradient(counts)
    level = F(np.uint32(iso_q))
    below = np.zeros(counts.shape, np.int64)              # vertices of the node on the directions below d
    vid = {}
    for d in range(1, 8):
        k, j, i = np.nonzero(owns[d - 1])
        kb, jb, ib = k + (d >> 2), j + ((d >> 1) & 1), i + (d & 1)
        v = vbase[k, j, i] + below[k, j, i]
        vid[d] = vbase + below                            # (the number the edge (node, d) would have; read only where it owns one)
        ca, cb = counts[k, j, i].astype(F), counts[kb, jb, ib].astype(F)
        t = (level - ca) / (cb - ca)
        for a, (na, nb) in enumerate(((i, ib), (j, jb), (k, kb))):
            xa, xb = X[a][na], X[a][nb]
            pos[v, a] = xa + t * (xb - xa)
        ga, gb = G[k, j, i], G[kb, jb, ib]
        g = ga + t[:, None] * (gb - ga)
        len2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        ok = np.isfinite(len2) & (len2 > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = (-g) / np.sqrt(len2)[:, None]
        nrm[v] = np.where(ok[:, None], n, F(0.0))
        below = below + owns[d - 1]
    # the triangles: per cube, per tetrahedron, per case
    table = case_table()
    corner_in = [_shift(inside, c, False) for c in range(8)]
    cube = np.zeros(counts.shape, bool)
    cube[:nz - 1, :ny - 1, :nx - 1] = True
    n_in = sum(c.astype(np.int64) for c in corner_in)
    active = np.nonzero((cube & (n_in > 0) & (n_in < 8)).ravel())[0]          # ascending linear index
    k, rem = np.divmod(active, ny * nx)
    j, i = np.divmod(rem, nx)
    rows = []          # (cube rank, m, position in the tetrahedron's list, three vertex numbers)
    for m, tet in enumerate(TETS):
        case = sum(corner_in[c][k, j, i].astype(np.int64) << t for t, c in enumerate(tet))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if not len(sel):
                continue
            for q, tri in enumerate(table[m][cs]):
                verts = []
                for p0, p1 in tri:
                    cu, cv = tet[p0], tet[p1]
                    d = cu ^ cv
                    ka, ja, ia = k[sel] + (cu >> 2), j[sel] + ((cu >> 1) & 1), i[sel] + (cu & 1)
                    assert owns[d - 1][ka, ja, ia].all()
                    verts.append(vid[d][ka, ja, ia])
                rows.append(np.stack([sel, np.full(len(sel), m), np.full(len(sel), q)] + verts, axis=1))
    if not rows:
        return pos, nrm, np.zeros((0, 3), np.uint32)
    rows = np.concatenate(rows)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    return pos, nrm, rows[order, 3:].astype(np.uint32)


def mesh_of(pos, box_min, box_max, particle_radius, spacing=0.0, radius=0.0, iso=0.0):
    """the whole rule: (counts, origin, s, mesh positions, normals, triangles) of particles in a box"""
    s, r, iso_q = resolve(particle_radius, spacing, radius, iso)
    dims, origin = lattice(box_min, box_max, s, r)
    counts = field(pos, dims, origin, s, r)
    return (counts, origin, s) + extract(counts, origin, s, iso_q)


# ---- what a mesh must be ----------------------------------------------------------------------------------------------------------

def directed_edges(tri):
    t = np.asarray(tri, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def check_closed_oriented(tri):
    """every directed edge occurs exactly once, and so does its reverse"""
    e = directed_edges(tri)
    if not len(e):
        return
    big = int(e.max()) + 1
    key, rev = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), "a directed edge occurs %d times" % cnt.max()
    assert np.array_equal(uniq, np.unique(rev)), "a directed edge without its reverse"


def euler_characteristic(n_vertices, tri):
    e = np.sort(directed_edges(tri), axis=1)
    n_edges = len(np.unique(e, axis=0))
    return n_vertices - n_edges + len(tri)


def signed_volume(pos, tri):
    p = np.asarray(pos, np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def census(counts, iso_q):
    """(vertices owned per node, triangles per cube) in lattice order, flattened; a node that is no cube's base gives 0"""
    inside = counts >= np.uint32(iso_q)
    nz, ny, nx = counts.shape
    exists = np.ones(counts.shape, bool)
    vertices = sum((_shift(exists, d, False) & (_shift(inside, d, False) != inside)).astype(np.int64) for d in range(1, 8))
    corner_in = [_shift(inside, c, False).astype(np.int64) for c in range(8)]
    triangles = np.zeros(counts.shape, np.int64)
    for tet in TETS:
        n_in = sum(corner_in[c] for c in tet)
        triangles += np.where(n_in == 2, 2, np.where((n_in == 1) | (n_in == 3), 1, 0))
    cube = np.zeros(counts.shape, bool)
    cube[:nz - 1, :ny - 1, :nx - 1] = True
    return vertices.ravel(), np.where(cube, triangles, 0).ravel()

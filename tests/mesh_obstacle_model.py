"""numpy model of the mesh voxeliser of include/sph_hip.h (sph_obstacle_build_mesh and the calls next to it): a triangle mesh
becomes the truncated signed-distance grid the obstacle pass reads.  float32 throughout, one rounding per operation, no
multiply-add fusion, sums left to right: the order of the header's pseudo-code.  The lattice, the clamp and F are those of
tests/obstacle_model.py.  One triangle at a time, every node of its index box at once.

Arrays of the lattice are indexed [k, j, i] (x fastest), as the device's linear index (k*n_y + j)*n_x + i."""
import numpy as np

from obstacle_model import F, clamp, lattice, node_positions

assert lattice          # (re-exported: the lattice of a mesh build is the lattice of sph_obstacle_build)
MAX_BAND, DEFAULT_BAND = 16, 3
TILE_X, TILE_ROWS = 64, 128          # a tile of the device's work list: 64 consecutive x nodes (or y columns), 128 rows


def resolve_band(band):
    return int(band) if int(band) else DEFAULT_BAND


def index_range(lo, hi, origin_k, s, n_k):
    """[a, b] of one axis: floorf((lo - origin) / s) .. ceilf((hi - origin) / s), each clamped as a float to [0, n - 1]"""
    with np.errstate(all="ignore"):
        a = np.floor(F(F(F(lo) - F(origin_k)) / F(s)))
        b = np.ceil(F(F(F(hi) - F(origin_k)) / F(s)))
    a = np.fmin(np.fmax(F(a), F(0)), F(n_k - 1))
    b = np.fmin(np.fmax(F(b), F(0)), F(n_k - 1))
    return int(a), int(b)


def good_triangles(vertices, triangles):
    """mask of the triangles the device uses: every index < n_vertices and every vertex finite"""
    V = np.asarray(vertices, F).reshape(-1, 3)
    T = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    ok = (T < len(V)).all(axis=1)
    fin = np.isfinite(V).all(axis=1)
    ok[ok] &= fin[T[ok]].all(axis=1)
    return ok


def _cross(u, v):
    return (F(F(u[1] * v[2]) - F(u[2] * v[1])), F(F(u[2] * v[0]) - F(u[0] * v[2])), F(F(u[0] * v[1]) - F(u[1] * v[0])))


def _seg(a, b, px, py, pz):
    """the capsule's arithmetic without the radius: squared distance of the nodes to the segment a-b"""
    pax, pay, paz = px - a[0], py - a[1], pz - a[2]
    bax, bay, baz = F(b[0] - a[0]), F(b[1] - a[1]), F(b[2] - a[2])
    bb = F(F(bax * bax + bay * bay) + baz * baz)
    if np.isfinite(bb) and bb > 0:
        t = ((pax * bax + pay * bay) + paz * baz) / bb
        t = np.fmin(np.fmax(t, F(0)), F(1))
    else:
        t = F(0)
    dx, dy, dz = pax - t * bax, pay - t * bay, paz - t * baz
    return (dx * dx + dy * dy) + dz * dz


def _boxes(A, B, C, W, grid):
    o, s, n = np.asarray(grid["origin"], F), F(grid["spacing"]), grid["dims"]
    lo, hi = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
    with np.errstate(all="ignore"):
        dist = [index_range(F(lo[k] - W), F(hi[k] + W), o[k], s, n[k]) for k in range(3)]
    cols = [index_range(lo[k], hi[k], o[k], s, n[k]) for k in (1, 2)]
    return dist, cols


def _canonical(p, q):
    """the two ends of an edge, smaller z first, on equal z smaller y first"""
    return (q, p) if (q[2] < p[2]) or (q[2] == p[2] and q[1] < p[1]) else (p, q)


def raw(grid, vertices, triangles, band=0):
    """(d2 float32[n_z, n_y, n_x], marks bool[n_z, n_y, n_x + 1], used, skipped, lost): the two accumulations of the rule"""
    V = np.asarray(vertices, F).reshape(-1, 3)
    T = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    nx, ny, nz = grid["dims"]
    s, o = F(grid["spacing"]), np.asarray(grid["origin"], F)
    W = F(F(resolve_band(band)) * s)
    X, Y, Z = node_positions(grid)
    d2 = np.full((nz, ny, nx), np.inf, F)
    d2u = d2.view(np.uint32)
    marks = np.zeros((nz, ny, nx + 1), bool)
    ok = good_triangles(V, T)
    lost = 0
    with np.errstate(all="ignore"):
        for t in T[ok]:
            A, B, C = V[t[0]], V[t[1]], V[t[2]]
            (i0, i1), (j0, j1), (k0, k1) = _boxes(A, B, C, W, grid)[0]
            px, py, pz = X[None, None, i0:i1 + 1], Y[None, j0:j1 + 1, None], Z[k0:k1 + 1, None, None]
            cand = np.fmin(np.fmin(_seg(A, B, px, py, pz), _seg(B, C, px, py, pz)), _seg(C, A, px, py, pz))
            n = _cross(B - A, C - A)
            nn = F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if np.isfinite(nn) and nn > 0:
                within = np.ones(cand.shape, bool)
                for a, b in ((A, B), (B, C), (C, A)):
                    c = _cross(b - a, n)
                    within &= (((px - a[0]) * c[0] + (py - a[1]) * c[1]) + (pz - a[2]) * c[2]) <= 0
                h = ((px - A[0]) * n[0] + (py - A[1]) * n[1]) + (pz - A[2]) * n[2]
                cand = np.where(within, np.fmin(cand, (h * h) / nn), cand)
            assert cand.dtype == F
            view = d2u[k0:k1 + 1, j0:j1 + 1, i0:i1 + 1]
            np.minimum(view, np.ascontiguousarray(cand).view(np.uint32), out=view)      # (the bits of a non-negative float)
            # the sign: the columns of the y and z extents
            (j0, j1), (k0, k1) = _boxes(A, B, C, W, grid)[1]
            qy, qz = Y[None, j0:j1 + 1], Z[k0:k1 + 1, None]
            odd = np.zeros((k1 - k0 + 1, j1 - j0 + 1), bool)
            for p, q in ((A, B), (B, C), (C, A)):
                l, u = _canonical(p, q)
                straddle = (l[2] <= qz) & ~(u[2] <= qz)
                E = F(u[1] - l[1]) * (qz - l[2]) - F(u[2] - l[2]) * (qy - l[1])
                odd ^= straddle & (E > 0)
            xc = A[0] + ((n[1] * (A[1] - qy)) + n[2] * (A[2] - qz)) / n[0]
            g = ((xc - o[0]) / s).astype(F)
            fin = np.isfinite(g)
            lost += int((odd & ~fin).sum())
            gi = np.where(fin, g, F(0))
            m = np.where(gi <= 0, 0, np.where(gi > F(nx - 1), nx, np.ceil(np.fmin(gi, F(nx - 1))).astype(np.int64)))
            kk, jj = np.nonzero(odd & fin)
            marks[k0 + kk, j0 + jj, m[kk, jj]] ^= True
    return d2, marks, int(ok.sum()), int((~ok).sum()), lost


def build(grid, vertices, triangles, band=0, invert=False):
    """(phi float32[n_z, n_y, n_x], (used, skipped, lost crossings, odd columns)): what sph_obstacle_build_mesh installs and
    what sph_obstacle_mesh_stats reports"""
    d2, marks, used, skipped, lost = raw(grid, vertices, triangles, band)
    nx = grid["dims"][0]
    W = F(F(resolve_band(band)) * F(grid["spacing"]))
    parity = np.logical_xor.accumulate(marks, axis=2)
    with np.errstate(all="ignore"):
        phi = np.fmin(np.sqrt(d2), W).astype(F)
    phi = np.where(parity[:, :, :nx], -phi, phi)
    if invert:
        phi = -phi
    return clamp(phi, grid), (used, skipped, lost, int(parity[:, :, nx].sum()))


def tile_extents(grid, vertices, triangles, band=0):
    """int64[n_used, 4]: per used triangle (across, rows) of the distance pass -- the nodes of its banded x range, the (j, k) rows of
    its banded y and z ranges -- and (across, rows) of the crossing pass -- the columns of its y range, the rows of its z range"""
    V = np.asarray(vertices, F).reshape(-1, 3)
    T = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    W = F(F(resolve_band(band)) * F(grid["spacing"]))
    out = []
    with np.errstate(all="ignore"):
        for t in T[good_triangles(V, T)]:
            ((i0, i1), (j0, j1), (k0, k1)), ((cj0, cj1), (ck0, ck1)) = _boxes(V[t[0]], V[t[1]], V[t[2]], W, grid)
            out.append((i1 - i0 + 1, (j1 - j0 + 1) * (k1 - k0 + 1), cj1 - cj0 + 1, ck1 - ck0 + 1))
    return np.array(out, np.int64).reshape(-1, 4)


def crossing_tiles(grid, vertices, triangles, band=0):
    """tiles of the crossing pass per used triangle: 64-column chunks of its y range times 128-row groups of its z range"""
    e = tile_extents(grid, vertices, triangles, band)
    return -(-e[:, 2] // TILE_X) * -(-e[:, 3] // TILE_ROWS)


def distance_tiles(grid, vertices, triangles, band=0):
    """tiles of the distance pass per used triangle: 64-node chunks of its x range times 128-row groups of its (j, k) rows"""
    V = np.asarray(vertices, F).reshape(-1, 3)
    T = np.asarray(triangles, np.uint32).reshape(-1, 3).astype(np.int64)
    W = F(F(resolve_band(band)) * F(grid["spacing"]))
    out = []
    with np.errstate(all="ignore"):
        for t in T[good_triangles(V, T)]:
            (i0, i1), (j0, j1), (k0, k1) = _boxes(V[t[0]], V[t[1]], V[t[2]], W, grid)[0]
            out.append(-(-(i1 - i0 + 1) // TILE_X) * -(-((j1 - j0 + 1) * (k1 - k0 + 1)) // TILE_ROWS))
    return np.array(out, np.int64)

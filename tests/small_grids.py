"""Tiny and degenerate grids: the case table and numpy-only generators -- TEST INFRASTRUCTURE, no GPU code.

Every other GPU test runs on grids of at least 18 cells per axis with a cell edge of about h.  There a candidate kept from across
a face is more than h away and adds exactly zero, a one-pass radix plan never runs and a slab always has an interior.  The grids
below are the ones where those things show: 1, 2 and 3 cells per axis, a cell edge below h, key widths of 1, 8 and 9 bits.
tests/test_small_grids_cpu.py checks that the table reaches what it claims; tests/test_gpu_small_grids.py runs it.
"""
import numpy as np

import sph_model

F = np.float32
H = 0.1
R = F(1 / 64)                       # the reference's particle radius; lattice spacing 2R

# id -> (grid, box edges, box_min or None = centred on the origin)
GRIDS = {
    "g111": ((1, 1, 1), (2.0, 2.0, 2.0), None),            # key_bits 1; every mask at once; power-of-two decode with shift 0
    "g222": ((2, 2, 2), (0.25, 0.25, 0.25), None),         # exact-scaling hash; every cell at a face on every axis
    "g222d": ((2, 2, 2), (0.3, 0.3, 0.3), (0.1, -0.2, 1.0)),   # division hash; box off the origin
    "g333": ((3, 3, 3), (0.27, 0.27, 0.27), None),         # cell edge 0.09 < h: a wrapped cell is within reach; generic decode
    "g171": ((1, 7, 1), (0.2, 0.63, 0.2), None),           # gx a power of two, gy not (generic branch); row offsets +-1
    "g511": ((5, 1, 1), (0.45, 0.2, 0.2), None),           # x only: every dy and dz row is masked
    "g116": ((1, 1, 6), (0.2, 0.2, 0.54), None),           # z only: the dz rows are key +- 1
    "g213": ((2, 1, 3), (0.3, 0.2, 0.5), None),            # mixed
    "g888": ((8, 8, 8), (0.5, 0.5, 0.5), None),            # key_bits 9: the 1 x 9 plan
    "g1644": ((16, 4, 4), (1.0, 0.25, 0.25), None),        # key_bits 8: the 1 x 8 plan at its widest
}
# the sort also runs on two cells in a row (key_bits 1 with both keys in use)
SORT_GRIDS = {"g888": GRIDS["g888"][:2], "g1644": GRIDS["g1644"][:2], "g111": GRIDS["g111"][:2],
              "g211": ((2, 1, 1), (0.125, 0.0625, 0.0625))}


def bounds(gid):
    """(box_min, box_max) float32 (3,) of a row of GRIDS, as sph_default_params makes them for a centred box."""
    grid, box, lo = GRIDS[gid]
    box = np.asarray(box, F)
    if lo is None:
        return (-box / F(2)).astype(F), (box / F(2)).astype(F)
    lo = np.asarray(lo, F)
    return lo, (lo + box).astype(F)


def set_bounds(p, gid):
    """Write the row's box into a parameter object (capi.Params or the namespace below) and return it."""
    lo, hi = bounds(gid)
    for a in range(3):
        p.box_min[a], p.box_max[a] = float(lo[a]), float(hi[a])
    return p


def model_params(gid):
    """The reference's constants on the row's box and grid, without the library."""
    grid, box, _ = GRIDS[gid]
    return set_bounds(sph_model.reference_params(box, grid), gid)


# ---- what the library derives from a grid (csrc/sph_capi.hip: derive; sph_sort.hip: radix_sort_pairs; sph_pairs.hip) -----------
def key_bits(grid):
    nc, b = int(np.prod([int(g) for g in grid])), 1
    while (1 << b) < nc:
        b += 1
    return b


def radix_plan(bits):
    """(digit bits, passes): 9-bit digits where they save a pass over 8-bit ones."""
    p8, p9 = (bits + 7) // 8, (bits + 8) // 9
    return (9, p9) if p9 < p8 else (8, p8)


def decode_branch(grid):
    """Which key decode lane_rows takes: shifts where gx and gy are powers of two, else divisions."""
    gx, gy = int(grid[0]), int(grid[1])
    return "pow2" if ((gx & (gx - 1)) | (gy & (gy - 1))) == 0 else "generic"


def hash_branches(gid):
    """Per axis, which cell_coord the row takes: "scale" where the float32 box edge is a power of two, else "divide"."""
    lo, hi = bounds(gid)
    m, _ = np.frexp((hi - lo).astype(F))
    return ["scale" if v == 0.5 else "divide" for v in m]


# ---- the hash in numpy (sph_model.Model.cells; _np_cell of tests/test_gpu_edge_cases.py) -------------------------------------
def np_cells(pos, lo, hi, grid, clamp=True):
    """floor(((p - bmin) / bdim) * g) in float32, clipped to [0, g - 1] (clamp=False: as floor leaves it)."""
    g = np.asarray(grid, np.int64)
    q = ((np.asarray(pos, F) - lo) / (hi - lo).astype(F)) * g.astype(F)
    c = np.floor(q).astype(np.int64)
    return np.clip(c, 0, g - 1) if clamp else c


def np_keys(pos, lo, hi, grid):
    c = np_cells(pos, lo, hi, grid)
    return ((c[:, 2] * int(grid[1]) + c[:, 1]) * int(grid[0]) + c[:, 0]).astype(np.uint32)


FACE_ULPS = (-16, -2, -1, 0, 1, 2, 16)      # nextafter steps around a face; axis_probes adds steps of the box edge's ulp


def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def axis_probes(gid, a):
    """The coordinates of axis a that decide a cell: {"face": {k: [...]}, "lo": [...], "hi": [...], "centre": [...]}.
    face k lies between cells k - 1 and k, as the float32 bmin + k * edge; lo / hi: the walls and up to one cell edge outside."""
    grid = GRIDS[gid][0]
    lo, hi = bounds(gid)
    g = int(grid[a])
    edge = F((hi[a] - lo[a]) / F(g))
    out = {"face": {}, "centre": [F(lo[a] + (F(k) + F(0.5)) * edge) for k in range(g)]}
    step = np.spacing(F(hi[a] - lo[a]))                     # where a face is at 0, nextafter is a denormal: p - bmin swallows it
    for k in range(1, g):
        f = F(lo[a] + F(k) * edge)
        out["face"][k] = [_ulps(f, u) for u in FACE_ULPS] + [F(f + F(m) * step) for m in (-16, -2, -1, 1, 2, 16)]
    out["lo"] = [lo[a], _ulps(lo[a], 1), _ulps(lo[a], -1), F(lo[a] - F(0.3) * edge), F(lo[a] - edge)]
    out["hi"] = [hi[a], _ulps(hi[a], -1), _ulps(hi[a], 1), F(hi[a] + F(0.3) * edge), F(hi[a] + edge)]
    return out


def hash_positions(gid, n_total=2000, seed=5):
    """About 2,000 float32 positions: on every axis every probe of axis_probes (three rows each, the other two coordinates
    drawn from the probes of their axes or from the interior), then random interior points up to n_total (at least 400)."""
    lo, hi = bounds(gid)
    rng = np.random.default_rng(seed)
    flat = []
    for a in range(3):
        pr = axis_probes(gid, a)
        flat.append(np.array(pr["centre"] + pr["lo"] + pr["hi"] + [v for vs in pr["face"].values() for v in vs], F))
    rows = []
    for a in range(3):
        for v in flat[a]:
            for rep in range(3):
                p = (lo + rng.random(3, F) * (hi - lo)).astype(F)
                for b in range(3):
                    if b != a and rep > 0 and rng.random() < 0.5:
                        p[b] = rng.choice(flat[b])
                p[a] = v
                rows.append(p)
    rows.append(lo.copy()); rows.append(hi.copy())
    inner = (lo + rng.random((max(n_total - len(rows), 400), 3), F) * (hi - lo)).astype(F)
    return np.concatenate([np.array(rows, F), inner]).astype(F)


def moving_cloud(gid, n=600, seed=9):
    """A small cloud over the whole box, fast enough that some particles change cell or reach a wall in one step of 5e-7."""
    lo, hi = bounds(gid)
    rng = np.random.default_rng(seed)
    pos = (lo + (F(0.002) + F(0.996) * rng.random((n, 3), F)) * (hi - lo)).astype(F)
    vel = ((rng.random((n, 3), F) - F(0.5)) * (F(2 * 0.02 / 5e-7) * (hi - lo))).astype(F)      # up to 2 % of the edge per step
    return pos, vel


# ---- part C: what the pair kernels are given ------------------------------------------------------------------------------------
MAX_PAIR_PARTICLES = 1536           # the model holds every candidate pair; in g111 every pair is one
N_WALL = 24


def _block_counts(dims):
    """Lattice points per axis: spacing 2R from R inside the min corner, the last centre within 80 % of the edge, at most
    MAX_PAIR_PARTICLES - N_WALL in all (the longest axis gives way first)."""
    n = [int(np.floor((0.8 * float(d) - float(R)) / (2 * float(R)))) + 1 for d in dims]
    n = [max(v, 1) for v in n]
    while n[0] * n[1] * n[2] > MAX_PAIR_PARTICLES - N_WALL:
        n[int(np.argmax(n))] -= 1
    return n


def _clump_extent(dims):
    """Edges of the cuboid in the min corner that holds the clump: the whole box where twice the lattice's number density
    gives no more than the particle budget, else the budget's volume as a cube clipped to the box."""
    rho = 2.0 / (2 * float(R)) ** 3
    dims = np.asarray(dims, np.float64)
    vol = (MAX_PAIR_PARTICLES - N_WALL) / rho
    if dims.prod() <= vol:
        return dims, int(rho * dims.prod())
    ext, free = dims.copy(), [True, True, True]
    for _ in range(3):
        fixed = np.prod([ext[a] for a in range(3) if not free[a]]) if not all(free) else 1.0
        s = (vol / fixed) ** (1.0 / sum(free))
        over = [a for a in range(3) if free[a] and dims[a] <= s]
        if not over:
            for a in range(3):
                if free[a]:
                    ext[a] = s
            break
        for a in over:
            free[a] = False
    return ext, MAX_PAIR_PARTICLES - N_WALL


def pair_case(gid, kind, seed=11):
    """(pos, vel) float32: a jittered lattice block ("block") or a random clump at twice its number density ("clump"), plus 24
    particles 1e-6 inside the six walls, moving outward (both wall branches of the integrate)."""
    lo, hi = bounds(gid)
    dims = (hi - lo).astype(F)
    rng = np.random.default_rng(seed)
    if kind == "block":
        nx, ny, nz = _block_counts(dims)
        i = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(F)
        pos = (lo + R + F(2) * R * i + (rng.random(i.shape, F) - F(0.5)) * F(0.02) * R).astype(F)
        vel = ((rng.random(i.shape, F) - F(0.5)) * F(1.0)).astype(F)
        ext = (pos.max(axis=0) - lo).astype(F)
    elif kind == "clump":
        ext, n = _clump_extent(dims)
        ext = ext.astype(F)
        pos = (lo + (F(0.002) + F(0.996) * rng.random((n, 3), F)) * ext).astype(F)
        vel = ((rng.random((n, 3), F) - F(0.5)) * F(2 * 200.0)).astype(F)
    else:
        raise KeyError(kind)
    wp = (lo + rng.random((N_WALL, 3), F) * ext).astype(F)
    wv = ((rng.random((N_WALL, 3), F) - F(0.5)) * F(10.0)).astype(F)
    for k in range(N_WALL):
        a, upper = k % 3, (k // 3) % 2
        wp[k, a] = (hi[a] - F(1e-6)) if upper else (lo[a] + F(1e-6))
        wv[k, a] = F(3000.0) if upper else F(-3000.0)
    return np.concatenate([pos, wp]).astype(F), np.concatenate([vel, wv]).astype(F)


def brute_pairs(pos, lo, hi, grid):
    """(i, j) of every pair whose cells differ by at most one on every axis, self pairs included: the 27-cell stencil stated
    without a cell table, a sort or a key.  Sorted by (i, j)."""
    c = np_cells(pos, lo, hi, grid)
    near = np.all(np.abs(c[:, None, :] - c[None, :, :]) <= 1, axis=2)
    i, j = np.nonzero(near)
    return i, j


def neighbour_directions(pos, lo, hi, grid, h=H):
    """Cell offsets (dx, dy, dz) at which some particle has another particle closer than h."""
    c = np_cells(pos, lo, hi, grid)
    i, j = brute_pairs(pos, lo, hi, grid)
    x = np.asarray(pos, np.float64)
    keep = (i != j) & (((x[i] - x[j]) ** 2).sum(axis=1) < h * h)
    return {tuple(int(v) for v in d) for d in np.unique(c[j[keep]] - c[i[keep]], axis=0)}


def existing_directions(grid):
    """The offsets of the 27 that some cell of the grid has a neighbour cell at."""
    per_axis = [(-1, 0, 1) if int(g) > 1 else (0,) for g in grid]
    return {(dx, dy, dz) for dx in per_axis[0] for dy in per_axis[1] for dz in per_axis[2]}


# ---- part B: key distributions that tests/sort_reference.py does not have ------------------------------------------------------
def every_cell(n, grid, seed):
    """Every cell occupied (n >= the number of cells), in a random upload order."""
    import sort_reference as sr
    nc = int(np.prod([int(g) for g in grid]))
    assert n >= nc
    keys = np.random.default_rng(seed).permutation(np.arange(n) % nc)
    return sr.cells_of(keys, grid)


def only_first(n, grid, seed):
    return np.zeros((n, 3), np.int64)


def only_last(n, grid, seed):
    return np.tile(np.array([int(g) - 1 for g in grid], np.int64), (n, 1))


# ---- part D: thin slabs ------------------------------------------------------------------------------------------------------
# (grid, slabs, layers per slab the balanced cuts must give)
SLAB_CASES = {
    "1x1x8 in 4 slabs of two layers": ((1, 1, 8), 4),
    "1x1x8 in 2 slabs of four layers": ((1, 1, 8), 2),
    "1x5x12 in 3 slabs": ((1, 5, 12), 3),
    "4x1x9 in 3 slabs": ((4, 1, 9), 3),
    "8x8x8 in 4 slabs of two layers": ((8, 8, 8), 4),
}


def slab_box(grid):
    return tuple(int(g) / 16.0 for g in grid)      # cell edge 1/16: faces are exact in float32


def slab_particles(grid, n=3000, seed=21, vz=4000.0):
    """n particles, the same number in every cell layer (the count-balanced cuts then are the even ones), half of them moving up
    and half down: 0.002 per step of 5e-7, a third of a cell edge in 12 steps."""
    box = np.asarray(slab_box(grid), F)
    rng = np.random.default_rng(seed)
    gz = int(grid[2])
    layer = np.arange(n) % gz
    u = F(0.02) + F(0.96) * rng.random((n, 3), F)
    pos = np.empty((n, 3), F)
    pos[:, :2] = -box[:2] / F(2) + u[:, :2] * box[:2]
    pos[:, 2] = -box[2] / F(2) + (layer.astype(F) + u[:, 2]) * F(1 / 16)
    vel = ((rng.random((n, 3), F) - F(0.5)) * F(20.0)).astype(F)
    vel[:, 2] = np.where(rng.random(n) < 0.5, F(vz), F(-vz))    # both ways across every cut
    return pos.astype(F), vel


# ---- part E: the reference's seam at gridDim 1, 2 and 4 ----------------------------------------------------------------------
SEAM_BOX, SEAM_N, SEAM_SEED = 0.5, 700, 8837      # the first seed of seam_particles that gives the counts below
SEAM_EXPECT = {1: dict(cells=1, fullest=700, bprime=22), 2: dict(cells=8, fullest=92, bprime=24),
               4: dict(cells=56, fullest=64, bprime=64)}


def seam_particles(seed=None):
    """700 particles in a 0.3 cube around the origin of the 0.5 box, random velocities."""
    rng = np.random.default_rng(SEAM_SEED if seed is None else seed)
    pos = ((rng.random((SEAM_N, 3)) - 0.5) * 0.3).astype(F)
    vel = ((rng.random((SEAM_N, 3)) - 0.5) * 400.0).astype(F)
    return pos, vel


def seam_counts(pos, g):
    """(occupied cells, fullest cell, 32-particle chunks) of the positions on a g^3 grid over the seam's box."""
    lo, hi = np.full(3, -SEAM_BOX / 2, F), np.full(3, SEAM_BOX / 2, F)
    _, cnt = np.unique(np_keys(pos, lo, hi, (g, g, g)), return_counts=True)
    return dict(cells=int(cnt.size), fullest=int(cnt.max()), bprime=int(((cnt + 31) // 32).sum()))

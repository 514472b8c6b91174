"""Inputs for the mixed-precision density pass (`k_density_h`, csrc/sph_pairs.hip), and numpy restatements of what the kernel
documents about its walks -- TEST INFRASTRUCTURE, imports without a GPU.

tests/test_mixed_cases_cpu.py shows on the CPU that the bars the GPU tests use are reachable and that the cases reach the
walks they are meant for; tests/test_gpu_mixed_walks.py runs them on the device, tests/test_gpu_slabs_mixed.py the moving
tower (d_tower) inside the z-slab step.

DYADIC cases -- why the packed fp16 arithmetic is EXACT on them, and the bar is therefore the fp32 one (1e-5):
h = 0.125, box_min = (-2, -2, -2), and every particle sits on a site box_min + (k + 0.5) h/2 without jitter.  Hence
  * every coordinate difference is a multiple of h/2, so every (p - ref) / h the kernel forms is a multiple of 1/2 below 64 (the
    box is at most 36 h wide): exact in fp32 and in fp16;
  * the coarse x part (a multiple of 1/2) is the whole x, the fine part is 0;
  * a candidate within h has |dx|, |dy|, |dz| in {0, 1/2}, so every 1 - r'^2 that is not clamped to 0 is a multiple of 1/4,
    and every (1 - r'^2)^3 a multiple of 1/64 that is at most 1 (a far candidate's 1 - r'^2 may round, but stays negative and
    is clamped);
  * at most the 27 sites of a 3 x 3 x 3 cube lie within h, so a row sum is a multiple of 1/64 below 32: exact in fp16's 11 bits.
So, apart from the fp32 roundings of the final scale m POLY6 h^6, a correct mixed result EQUALS the float64 model, whichever
walk produced it; one dropped or doubled candidate is an error of at least 1/64 in ~10, i.e. > 1e-3.

GENERIC cases are jittered fp32 positions, held to the mixed mode's documented bar (2e-2 max, 4e-3 rms).
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import sph_model

F = np.float32
H16 = np.float16

WAVE, PIECE = 64, 128                                   # csrc/sph_common.hpp: lanes of a wave, staged slots per piece
MIXED_PASSES, MIXED_SPAN, MIXED_XSPAN = 3, 6.0, 1000.0  # csrc/sph_pairs.hip: SPH_MIXED_PASSES, _SPAN, _XSPAN
GATHER = MIXED_PASSES + 1                               # "pass" number of the lanes left to the fp32 gather

DY_H = 0.125
DY_MIN = -2.0


def params(box_min, box_max, grid, h, particle_radius=None):
    """The reference's constants (sph_model.reference_params) with another box, grid, h and radius."""
    p = sph_model.reference_params((1, 1, 1), grid)
    p.box_min = [F(v) for v in np.broadcast_to(np.asarray(box_min, F), 3)]
    p.box_max = [F(v) for v in np.broadcast_to(np.asarray(box_max, F), 3)]
    p.h = F(h)
    p.particle_radius = F(0.15625 * h if particle_radius is None else particle_radius)
    return p


def _case(name, pos, p, **extra):
    pos = np.ascontiguousarray(pos, F)
    pos.setflags(write=False)
    return SimpleNamespace(name=name, pos=pos, params=p, **extra)


# ---- dyadic cases -----------------------------------------------------------------------------------------------------------
def _sites(k):
    """Site indices (n, 3) -> float32 positions; exact."""
    return (F(DY_MIN) + (np.asarray(k, F) + F(0.5)) * F(DY_H / 2)).astype(F)


def _thinned_block(start, shape, keep, seed):
    k = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3) + np.asarray(start)
    rng = np.random.default_rng(seed)
    return k[rng.random(k.shape[0]) < keep]


def _dyadic_params(grid, wide=False):
    # wide: 3 x 3 x 3 cells of exactly 12 h (1.5) -- the widest cell include/sph_hip.h admits for the mixed mode
    return params(DY_MIN, DY_MIN + (4.5 if wide else 4.0), grid, DY_H)


@lru_cache(maxsize=None)
def d_block():
    """24 x 10 x 10 sites thinned to ~60 %, cells of edge h (2 sites per axis, 0..8 particles): row ranges of 0..24 slots
    that start at even and odd slots, with odd and even lengths, many shorter than one unrolled group of 8."""
    return _case("D-block", _sites(_thinned_block((7, 21, 33), (24, 10, 10), 0.6, 102)), _dyadic_params((32, 32, 32)))


@lru_cache(maxsize=None)
def d_wide(edge_h):
    """16 x 16 x 16 sites (8 h wide) thinned to ~2500, across a cell corner of a grid with cells 4 h or 12 h wide.  12 h:
    the block is cut 7|9 in x, 14|2 in y and 13|3 in z, so the longest row holds ~1750 candidates: 14 staged pieces, every lane's
    range across all of their edges and ending inside the last one (the lanes of a cell share their ranges; a wave across two
    cells has ranges that begin inside a piece); 4 h: the block covers a half, a whole and a half cell per axis."""
    if edge_h == 4:
        return _case("D-wide-4h", _sites(_thinned_block((12, 20, 28), (16, 16, 16), 0.61, 107)), _dyadic_params((8, 8, 8)))
    assert edge_h == 12
    return _case("D-wide-12h", _sites(_thinned_block((48 - 7, 48 - 14, 48 - 13), (16, 16, 16), 0.61, 103)),
                 _dyadic_params((3, 3, 3), wide=True))


def _droplet_sites():
    """120 droplets of 6..14 sites out of a 3 x 3 x 2 site block each, the two sites of the block's middle column always
    among them (they lie within h of every other site of the block: no particle is alone).  A droplet's (y, z) cell column is its own: five y
    positions 7.5 h apart (the nearest particles of two of them are 6.5 h apart: never served by one reference point) in
    each of 24 z cell layers, at scattered x.  In the cell-key order (z, then y, then x) a wave of 64 therefore runs through
    six or seven droplets that lie far apart in y; the droplets of the next z layers are close in z but far down the order."""
    rng = np.random.default_rng(104)
    out = []
    block = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    middle = (block[:, 0] == 1) & (block[:, 1] == 1)
    block = np.concatenate([block[middle], block[~middle]])
    for layer in range(24):
        for col in range(5):
            start = np.array([rng.integers(0, 62), 1 + 15 * col, 2 * (4 + layer)])
            m = int(rng.integers(6, 15))
            out.append(np.concatenate([block[:2], block[2 + rng.permutation(block.shape[0] - 2)[:m - 2]]]) + start)
    return np.concatenate(out)


@lru_cache(maxsize=None)
def d_droplets():
    return _case("D-droplets", _sites(_droplet_sites()), _dyadic_params((32, 32, 32)))


TOWER_SHIFTS = 12                      # d_tower(0) .. d_tower(12): the block stays 2 sites and more below the top wall
TOWER_VEL = (0.0, 0.0, 64.0)           # every particle's velocity; with TOWER_DT one step moves every particle one site up
TOWER_DT = 2.0 ** -10


@lru_cache(maxsize=None)
def d_tower(shift=0):
    """A dyadic case that MOVES and stays dyadic: 16 x 16 x 72 sites thinned to ~60 % (11,167 particles, the same ones for
    every shift) in a box 48 cell layers of edge h tall, `shift` sites above its start.  No gravity, and a rest density above
    every density of the case, so every pressure is 0.  With the velocity TOWER_VEL on every particle a step of TOWER_DT is a
    rigid translation by exactly one site (h/2 in z): pressure terms are 0 times finite values, viscous terms are 0 (no
    relative velocity), no collision has r.v < 0, a = 0, and x += 2^-10 * 64 is exact in fp32 on multiples of 2^-5.  So
    the state after k steps from d_tower(0) is d_tower(k), bit for bit, and the block crosses a cell layer every second step.
    The box is 48 h tall, not 36: (p - ref) / h stays below 64 all the same."""
    p = params(DY_MIN, (2, 2, 4), (32, 32, 48), DY_H)
    p.gravity_y = F(0)
    p.rest_density = F(2 ** 19)
    assert 0 <= shift <= TOWER_SHIFTS
    return _case(f"D-tower+{shift}", _sites(_thinned_block((24, 24, 8 + shift), (16, 16, 72), 0.6, 111)), p, shift=shift)


def tower_velocity(n):
    return np.tile(np.asarray(TOWER_VEL, F), (n, 1))


DYADIC = {"D-block": d_block, "D-wide-4h": lambda: d_wide(4), "D-wide-12h": lambda: d_wide(12), "D-droplets": d_droplets}


# ---- generic cases ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def g_droplets():
    """D-droplets, every particle moved by up to 0.1 h per axis: still in its cell (sites lie h/4 from the cell faces), so the
    order, the waves and the pass each lane is served in are those of D-droplets."""
    d = d_droplets()
    rng = np.random.default_rng(105)
    pos = (d.pos + ((rng.random(d.pos.shape, F) - F(0.5)) * F(0.2 * DY_H))).astype(F)
    return _case("G-droplets", pos, d.params)


WIDE_EDGES = (1.25, 2, 4, 6, 8, 12)            # cell edges in h; 12 is the documented limit
_WIDE_GRID = {1.25: 32, 2: 16, 4: 8, 6: 6, 8: 4, 12: 3}


@lru_cache(maxsize=None)
def g_wide(edge_h):
    """A 20 x 10 x 10 dam lattice at spacing 0.3125 h (2 R) with 1 % jitter, h = 0.1, across an inner cell corner (cut
    45|55, 35|65 and 55|45 per cent) of a grid whose cells are `edge_h` h wide."""
    h, g = 0.1, _WIDE_GRID[edge_h]
    edge = edge_h * h
    p = params(-0.5 * g * edge, 0.5 * g * edge, (g, g, g), h)
    R = F(p.particle_radius)
    corner = F(-0.5 * g * edge + max(1, g // 2) * edge)
    i = np.stack(np.meshgrid(np.arange(20), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(F)
    extent = F(2) * R * np.array([20, 10, 10], F)
    rng = np.random.default_rng(106)
    pos = (corner - np.array([0.45, 0.35, 0.55], F) * extent + R + F(2) * R * i
           + (rng.random(i.shape, F) - F(0.5)) * F(0.02) * R).astype(F)
    return _case(f"G-wide-{edge_h}h", pos, p)


@lru_cache(maxsize=None)
def g_heavy():
    """600 particles in ONE cell 0.625 h wide: tests/test_gpu_edge_cases.py::test_everything_in_one_cell's generator, restated
    (same seed, same draws).  Nearly every pair is within h: a row sums to a few hundred."""
    rng = np.random.default_rng(3)
    pos = (np.float32([0.1, -0.4, 0.3]) + rng.uniform(0.001, 0.061, (600, 3))).astype(np.float32)
    pos = (np.floor((pos + 1.0) / 0.0625)[0] * 0.0625 - 1.0 + rng.uniform(0.002, 0.060, (600, 3))).astype(np.float32)
    return _case("G-heavy", pos, params(-1.0, 1.0, (32, 32, 32), 0.1, 1 / 64))


# ---- the float64 reference, once per case -----------------------------------------------------------------------------------
_MODEL_RHO = {}


def model_density(case):
    """float64 density of tests/sph_model.py; computed once per case and read-only."""
    if case.name not in _MODEL_RHO:
        rho = sph_model.Model(case.params).density(case.pos)[0]
        rho.setflags(write=False)
        _MODEL_RHO[case.name] = rho
    return _MODEL_RHO[case.name]


# ---- what the device does with a case: order, row ranges, passes ---------------------------------------------------------------
def layout(case):
    """The sorted layout of a whole-domain context: `order` (creation index per slot, the STABLE cell-key order), the cell
    coordinates per slot, and the nine row ranges [lo, hi) per slot in (dz, dy) order as csrc/sph_pairs.hip: lane_rows forms
    them (the slots of the cells cx-1 .. cx+1 of row (cy+dy, cz+dz); lo = hi where the row lies outside the grid or is empty)."""
    if not hasattr(case, "_layout"):
        m = sph_model.Model(case.params)
        c = m.cells(case.pos)
        gx, gy, gz = (int(v) for v in m.grid)
        key = (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0]
        order = np.argsort(key, kind="stable")
        skey, cs = key[order], c[order]
        n = order.size
        lo, hi = np.zeros((n, 9), np.int64), np.zeros((n, 9), np.int64)
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                r = (dz + 1) * 3 + (dy + 1)
                y, z = cs[:, 1] + dy, cs[:, 2] + dz
                ok = (y >= 0) & (y < gy) & (z >= 0) & (z < gz)
                base = (z * gy + y) * gx
                a = np.searchsorted(skey, base + np.maximum(cs[:, 0] - 1, 0), "left")
                b = np.searchsorted(skey, base + np.minimum(cs[:, 0] + 1, gx - 1), "right")
                lo[:, r] = np.where(ok & (b > a), a, 0)
                hi[:, r] = np.where(ok & (b > a), b, 0)
        case._layout = SimpleNamespace(order=order, keys=skey, cells=cs, lo=lo, hi=hi, pos=case.pos[order])
    return case._layout


def passes(case):
    """The pass rule of k_density_h over the waves [64 w, 64 w + 64) of the sorted slots, in the kernel's fp32 arithmetic:
    the first lane not yet served gives the reference; a waiting lane within MIXED_SPAN h of it in y and z and MIXED_XSPAN h
    in x is served by this pass; after MIXED_PASSES passes the rest gathers in fp32.
    Returns per SLOT: pass_no (1..3, or GATHER) and ref (the slot of the reference point; the slot itself for GATHER)."""
    if not hasattr(case, "_passes"):
        L = layout(case)
        n = L.order.size
        inv_h = F(1.0) / F(case.params.h)
        pass_no, ref = np.zeros(n, np.int64), np.arange(n)
        for w0 in range(0, n, WAVE):
            s = np.arange(w0, min(w0 + WAVE, n))
            p = L.pos[s]
            todo = np.ones(s.size, bool)
            for k in range(1, MIXED_PASSES + 1):
                if not todo.any():
                    break
                lead = int(np.argmax(todo))
                far = np.maximum(np.abs(p[:, 1] - p[lead, 1]), np.abs(p[:, 2] - p[lead, 2])) * inv_h
                take = todo & (far <= F(MIXED_SPAN)) & (np.abs(p[:, 0] - p[lead, 0]) * inv_h <= F(MIXED_XSPAN))
                pass_no[s[take]], ref[s[take]] = k, s[lead]
                todo &= ~take
            pass_no[s[todo]] = GATHER
        case._passes = (pass_no, ref)
    return case._passes


def by_creation_index(case, per_slot):
    """A per-slot array as a per-particle one (the order of case.pos and of Context.download)."""
    out = np.empty_like(per_slot)
    out[layout(case).order] = per_slot
    return out


def neighbours_within_h(case):
    """Per particle (creation order): candidates of the stencil closer than h, the particle itself not counted."""
    m = sph_model.Model(case.params)
    i, j = m.pairs(case.pos)
    x = case.pos.astype(np.float64)
    near = (((x[i] - x[j]) ** 2).sum(axis=1) < m.h * m.h) & (i != j)
    return np.bincount(i[near], minlength=x.shape[0])


def staged_segments(case):
    """What the STAGED walk of every pass hands to a lane: the hull of row r of a pass is cut into pieces of PIECE slots from
    its first slot A, and a lane walks [max(lo, a), min(hi, b)) of every piece [a, b).  Returns the arrays (rel, length,
    pass_no) of every non-empty segment -- rel = its first slot relative to the piece, whose parity picks the staged copy --
    and per (slot, row) of a served lane with a non-empty range the number of piece edges strictly inside it (`edges`)."""
    L = layout(case)
    pass_no, ref = passes(case)
    n = L.order.size
    rel, length, seg_pass, edges = [], [], [], []
    for w0 in range(0, n, WAVE):
        s = np.arange(w0, min(w0 + WAVE, n))
        for k in range(1, MIXED_PASSES + 1):
            lanes = s[pass_no[s] == k]
            for r in range(9):
                lo, hi = L.lo[lanes, r], L.hi[lanes, r]
                has = hi > lo
                if not has.any():
                    continue
                lo, hi = lo[has], hi[has]
                A, B = int(lo[0]), int(hi[-1])            # wave_hulls: the first and the last lane that have a range
                assert (np.diff(lo) >= 0).all() and (np.diff(hi) >= 0).all()
                cuts = np.arange(A + PIECE, B, PIECE)
                edges.append(((cuts[None, :] > lo[:, None]) & (cuts[None, :] < hi[:, None])).sum(axis=1))
                for a in range(A, B, PIECE):
                    l0, l1 = np.maximum(lo, a), np.minimum(hi, min(a + PIECE, B))
                    m = l1 > l0
                    rel.append(l0[m] - a); length.append((l1 - l0)[m]); seg_pass.append(np.full(int(m.sum()), k))
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(rel), cat(length), cat(seg_pass), cat(edges)


# ---- the documented per-pair arithmetic in numpy float16 -------------------------------------------------------------------------
def packed_f16_sums(case):
    """Sum over a particle's nine rows of the NORMALISED kernel (1 - r'^2)^3 in the arithmetic k_density_h documents, every
    operation rounded to fp16 (numpy float16): coordinates relative to the lane's reference point (passes()) in units of h,
    x as a coarse part (a multiple of 1/2) plus a fine part, 1 - dx^2 - dy^2 - dz^2, clamp at 0, cube, and the row summed in
    two fp16 accumulators (even and odd candidates) over the WHOLE row, as the direct walk does; rows added up exactly.
    Returns (sum per slot as float64, the largest row sum, the largest |staged coordinate|, the largest |fine x part|)."""
    if hasattr(case, "_f16"):
        return case._f16
    L = layout(case)
    _, ref = passes(case)
    n = L.order.size
    inv_h = F(1.0) / F(case.params.h)
    P, Rf = L.pos, L.pos[ref]

    def x_parts(x, rx):
        v = (x - rx) * inv_h
        c = (np.rint(v + v) * F(0.5)).astype(F)
        return c.astype(H16), (v - c).astype(H16)

    tx, txl = x_parts(P[:, 0], Rf[:, 0])
    ty, tz = ((P[:, 1] - Rf[:, 1]) * inv_h).astype(H16), ((P[:, 2] - Rf[:, 2]) * inv_h).astype(H16)
    one, zero = H16(1), H16(0)
    total = np.zeros(n, np.float64)
    row_max = coord_max = fine_max = 0.0
    idx = np.arange(n)
    for r in range(9):
        lo, ln = L.lo[:, r], L.hi[:, r] - L.lo[:, r]
        acc = np.zeros((2, n), H16)
        for t in range(int(ln.max(initial=0))):
            live = idx[ln > t]
            j = lo[live] + t
            x, xl = x_parts(P[j, 0], Rf[live, 0])
            y = ((P[j, 1] - Rf[live, 1]) * inv_h).astype(H16)
            z = ((P[j, 2] - Rf[live, 2]) * inv_h).astype(H16)
            dx, dy, dz = (tx[live] - x) + (txl[live] - xl), ty[live] - y, tz[live] - z
            w = one - dx * dx
            w = w - dy * dy
            w = np.maximum(w - dz * dz, zero)
            acc[t & 1, live] = acc[t & 1, live] + (w * w) * w
            coord_max = max(coord_max, float(np.abs(np.stack([x, y, z]).astype(F)).max()))
            fine_max = max(fine_max, float(np.abs(xl.astype(F)).max()))
        assert acc.dtype == H16
        row_max = max(row_max, float(acc.astype(F).max(initial=0)))
        total += acc[0].astype(np.float64) + acc[1].astype(np.float64)
    total.setflags(write=False)
    case._f16 = (total, row_max, coord_max, fine_max)
    return case._f16


def scale64(case):
    """m POLY6 h^6 of the float64 model: density = scale64 * sum of the normalised kernel."""
    m = sph_model.Model(case.params)
    return m.mass * 315.0 / (65.0 * np.pi * m.h ** 3)

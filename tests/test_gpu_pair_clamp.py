"""GPU: the two forms of the pair loops' r < h cut, and the collision work-off as a divergent loop.

The hot launches (`k_density`, the fused `k_force` without colliders; csrc/sph_pairs.hip) cut h - r and h^2 - r^2 below zero
with the clamp modifier of the fma that computes them, which also caps at 1: right only while h <= 1, so the host picks the
form per launch (pair_clamp) and SPH_PAIR_CLAMP=0 at create time forces the v_max_f32 form.  Both forms must give the same
bits wherever the clamp form is taken, a context with h > 1 must not take it, and the drain of the collision bit masks must
count what the model counts when one lane of a wave has several bits and its neighbours none."""
import numpy as np
import pytest

import sph_model
from conftest import bits, load_golden
from gpufluidsimulator_amd import capi
from phase_checks import FORCE_REL_TOL, POS_TOL_PER_BOX, REL_TOL, close, phases_vs_model

pytestmark = pytest.mark.gpu

F = np.float32
DT = 5e-7
KEYS = ("pos", "vel", "density", "pressure")


def _fused(monkeypatch, clamp_env, n, steps, direct=False, setup=None, **ctx_kw):
    """`steps` fused steps in a context created with SPH_PAIR_CLAMP unset (None) or set to clamp_env."""
    if clamp_env is None:
        monkeypatch.delenv("SPH_PAIR_CLAMP", raising=False)
    else:
        monkeypatch.setenv("SPH_PAIR_CLAMP", clamp_env)
    with capi.Context(n, **ctx_kw) as c:
        if direct:
            c.set_direct_hull(0)
        setup(c)
        c.step(DT, steps)
        return c.download()


@pytest.mark.parametrize("direct", [False, True], ids=["staged", "direct"])
def test_clamp_and_max_forms_agree_bit_for_bit(monkeypatch, direct):
    """Developed flow with collisions (c1_flow, 4,096 particles), 5 fused steps: the context that keeps v_max_f32 and the
    default one give the same bits -- under the staged walk and with every wave on the direct walk."""
    g = load_golden("c1_flow")
    pos, vel = g["pos"], g["vel"]
    kw = dict(box=g["box"], grid=g["grid"], setup=lambda c: c.upload(pos, vel), direct=direct)
    want = _fused(monkeypatch, "0", pos.shape[0], 5, **kw)
    got = _fused(monkeypatch, None, pos.shape[0], 5, **kw)
    assert np.isfinite(got["vel"]).all() and float(np.abs(got["vel"]).max()) > 0
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), k


# ---- the boundary h = 1 ---------------------------------------------------------------------------------------------------
def _scaled(h):
    """The default configuration scaled by s = h / 0.1: box, particle radius and lattice spacing times s, the mass times s^3
    (the densities stay those of the default dam, so the pressures are not all zero).  A jittered 16 x 16 x 12 lattice."""
    h = F(h)
    s = float(h) / 0.1
    p = capi.default_params((2.0 * s, 2.0 * s, 2.0 * s), (32, 32, 32))
    p.h = h
    p.particle_radius = F(float(h) * 0.15625)
    p.mass = F(65.0 * s ** 3)
    lo, R = np.array(p.box_min[:], F), F(p.particle_radius)
    rng = np.random.default_rng(5)
    i = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(F)
    pos = (lo + R + F(2) * R * i + (rng.random(i.shape, F) - F(0.5)) * F(0.02) * R).astype(F)
    vel = ((rng.random(i.shape, F) - F(0.5)) * F(s)).astype(F)           # not uniform: see tests/test_gpu_physics_params.py
    return p, pos, vel


@pytest.mark.parametrize("h", [1.0, float(np.nextafter(F(1), F(2))), 1.25], ids=["h1", "h1_next", "h1.25"])
def test_h_at_and_above_one_against_the_model(monkeypatch, h):
    """Every particle's own pair contributes d = h^2: at h = 1 exactly the clamp's cap, above it a clamp form chosen by
    mistake would cut the self term (and h - r of every close pair).  One step: density, pressure, forces and the integrate
    phase by phase against the float64 model, then the FUSED step's density, pressure, velocity and position against the
    model fed the GPU's phase outputs -- the bars of tests/test_gpu_physics_params.py."""
    p, pos, vel = _scaled(h)
    assert F(p.h) == F(h) and (F(p.h) > 1) == (h > 1.0)
    n = pos.shape[0]
    monkeypatch.delenv("SPH_PAIR_CLAMP", raising=False)
    with capi.Context(n, params=p) as c:
        c.upload(pos, vel)
        for _ in phases_vs_model(c, p, None, DT, steps=1):
            pass
    m = sph_model.Model(p)
    with capi.Context(n, params=p) as c:
        c.upload(pos, vel)
        c.hash(); c.sort(); c.build_cells(); c.density(); c.force(); c.collide()
        st, f = c.download(want=("density", "pressure")), c.download_forces()
    out = m.integrate(pos, vel, st["density"], f["fpress"].astype(np.float64) + f["fvisc"], f["dv"], DT)
    rho, pr = m.density(pos)
    assert float(pr.max()) > 0, "the case has pressure"
    setup = lambda c: c.upload(pos, vel)                                # noqa: E731
    got = _fused(monkeypatch, None, n, 1, params=p, setup=setup)
    close("fused density", got["density"], rho, REL_TOL)
    close("fused pressure", got["pressure"], pr, REL_TOL)
    box = float(np.max(np.array(p.box_max[:]) - np.array(p.box_min[:])))
    bad = sph_model.integrate_mismatch(out, got["pos"], got["vel"], POS_TOL_PER_BOX * box, REL_TOL * float(np.abs(out[1]).max()))
    assert bad.size == 0, ("fused step", bad.size, bad[:8])
    if h > 1.0:          # both contexts take the v_max_f32 form
        off = _fused(monkeypatch, "0", n, 1, params=p, setup=setup)
        for k in KEYS:
            assert np.array_equal(bits(got[k]), bits(off[k])), k
        direct = _fused(monkeypatch, None, n, 1, params=p, setup=setup, direct=True)
        for k in KEYS:
            assert np.array_equal(bits(got[k]), bits(direct[k])), ("direct", k)


# ---- uneven drains --------------------------------------------------------------------------------------------------------
PER_CELL, CELLS, CX0, CYZ = 16, 12, 10, 16


def _uneven_clump(where):
    """One x-row of 12 cells, 16 particles in each: three waves of four cells, every lane's (dz, dy) = (0, 0) row holds 48
    candidates (two chunks of the 32-candidate walk, the second one partial) and its other eight rows are empty.  Everything
    is at rest but three partners, which fly at one particle `P` from the next cell, all four within 2R of each other:
      first:  P is at the low x face of cell 4 (the wave of cells 4..7), the partners in cell 3 -- candidates 0..15 of P's row;
      second: P is at the high x face of cell 7, the partners in cell 8 -- candidates 32..47, the second chunk.
    P's lane has three bits to work off in one chunk, the 63 other lanes of its wave none; in the partners' wave three lanes
    have one bit each.  The other particles keep more than 2R from the partners."""
    p = capi.default_params((2.0, 2.0, 2.0), (32, 32, 32))
    edge, R = 2.0 / 32, float(p.particle_radius)
    rng = np.random.default_rng(17)
    x_lo = lambda cell: -1.0 + (CX0 + cell) * edge                       # noqa: E731
    y0 = z0 = -1.0 + CYZ * edge
    pc, nc, face, sign = (4, 3, x_lo(4), 1.0) if where == "first" else (7, 8, x_lo(8), -1.0)
    pos = np.empty((CELLS * PER_CELL, 3), np.float64)
    for cell in range(CELLS):
        blk = pos[cell * PER_CELL:(cell + 1) * PER_CELL]
        # the two cells at the face keep 0.56 of a cell (> 2R = half a cell, plus the partners' 0.004) clear of it
        a, b = 0.05, 0.95
        if cell == pc: a, b = (0.62, 0.95) if sign > 0 else (0.05, 0.38)
        if cell == nc: a, b = (0.05, 0.38) if sign > 0 else (0.62, 0.95)
        blk[:, 0] = x_lo(cell) + rng.uniform(a, b, PER_CELL) * edge
        blk[:, 1] = y0 + rng.uniform(0.05, 0.95, PER_CELL) * edge
        blk[:, 2] = z0 + rng.uniform(0.05, 0.95, PER_CELL) * edge
    vel = np.zeros_like(pos)
    P = pc * PER_CELL
    pos[P] = (face + sign * 0.002, y0 + 0.5 * edge, z0 + 0.5 * edge)
    partners = nc * PER_CELL + np.arange(3)
    for k, (dy, dz) in zip(partners, ((0.012, 0.0), (-0.012, 0.0), (0.0, 0.012))):
        pos[k] = (face - sign * 0.004, y0 + 0.5 * edge + dy, z0 + 0.5 * edge + dz)
        vel[k, 0] = sign * 100.0
    assert 2 * R == 0.03125
    return p, pos.astype(F), vel.astype(F), P, partners


@pytest.mark.parametrize("where", ["first", "second"])
def test_one_lane_drains_three_bits_while_its_wave_has_none(monkeypatch, where):
    monkeypatch.delenv("SPH_PAIR_CLAMP", raising=False)
    p, pos, vel, P, partners = _uneven_clump(where)
    n = pos.shape[0]
    m = sph_model.Model(p)
    cells = m.cells(pos)
    assert (cells[:, 1] == CYZ).all() and (cells[:, 2] == CYZ).all()
    assert np.array_equal(cells[:, 0], CX0 + np.arange(n) // PER_CELL), "every particle in the cell it was made for"
    wave = (cells[:, 0] - CX0) // 4                                      # 64 sorted slots = 4 cells of this row
    want = m.collide(pos, vel)[1]
    assert want[P] == 3 and (want[partners] == 1).all() and int(want.sum()) == 6
    assert (want[(wave == wave[P]) & (np.arange(n) != P)] == 0).all() and (wave[partners] != wave[P]).all()
    res = {}
    for direct in (False, True):
        with capi.Context(n, params=p) as c:
            if direct:
                c.set_direct_hull(0)
            c.upload(pos, vel)
            c.hash(); c.sort(); c.build_cells(); c.density(); c.force(); c.collide()
            res[direct] = c.download_forces()
            c.step(DT, 2)                                                # the fused pass: the same drain with the sums beside it
            res[direct].update({k + "_2": v for k, v in c.download().items()})
    for direct in (False, True):
        assert np.array_equal(res[direct]["count"], want), ("direct" if direct else "staged", res[direct]["count"][[P, *partners]])
    dv = m.collide(pos, vel)[0]
    close("delta_v", res[False]["dv"], dv, FORCE_REL_TOL, float(np.abs(dv).max()))
    for k, a in res[False].items():
        b = res[True][k]
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b), ("staged vs direct", k)

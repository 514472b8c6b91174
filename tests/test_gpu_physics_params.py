"""GPU: the step at NON-DEFAULT physics parameters against the float64 model of tests/sph_model.py.

Every other numeric test compares with the oracle, which bakes in the reference's constants; here each row of PARAM_ROWS
changes some of the eleven physics fields of sph_params and the GPU is held to the reference's formulas at those values.
Each phase is fed the GPU's own inputs for that phase (hash -> integrate), so errors do not compound.  Bars are those of
tests/test_gpu_parity.py (fp32) and tests/test_gpu_mixed_precision.py (mixed density); collision counts are exact.
"""
import threading

import numpy as np
import pytest

import sph_model
from conftest import bits
from gpufluidsimulator_amd import capi, slab
from phase_checks import REL_TOL, close as _close, phases_vs_model as _phases_vs_model      # shared with the state walk

pytestmark = pytest.mark.gpu

RHO_MAX, RHO_RMS = 2e-2, 4e-3                                         # tests/test_gpu_mixed_precision.py
FUSED_POS, FUSED_VEL = 1e-7, 2e-6                                     # tests/test_gpu_parity.py: fused vs phased
DT = 5e-7

F = np.float32
R0 = F(1 / 64)                      # the reference's particle radius; spacing 2R = 0.3125 h at h = 0.1


def _row(name):
    """(Params, colliders or None, dt) of one row; the lattice spacing 2R scales with the radius."""
    box, grid = (2.0, 2.0, 2.0), (32, 32, 32)
    kw, coll, dt = {}, None, DT
    if name == "P1":                # h-powers of derive(); cell edge 1/16 >= h
        kw = dict(h=0.05, particle_radius=0.05 * 0.15625)
    elif name == "P2":              # h 0.2 on cells of 1/8: the stencil truncates
        box, grid = (4.0, 4.0, 4.0), (32, 32, 32)
        kw = dict(h=0.2, particle_radius=0.2 * 0.15625)
    elif name == "P3":              # the ratio cp_scale
        kw = dict(mass=1.0, rest_density=500.0, gas_constant=50.0)
    elif name == "P4-visc0":
        kw = dict(viscosity=0.0)
    elif name == "P4-visc1e4":
        kw = dict(viscosity=1e4)
    elif name == "P5":
        kw = dict(gas_constant=0.0)
    elif name in ("P6-g0", "P6-gup"):   # many collisions; collision range 3R = 0.094 > the cell edge 1/16
        kw = dict(gravity_y=0.0 if name == "P6-g0" else 5e4, restitution=1.0, collision_param=1.5, particle_radius=2 * float(R0))
    elif name in ("P7-damp0", "P7-damp-1"):   # walls of a box off the origin, non-power-of-two edges; two moving spheres
        kw = dict(wall_eps=0.0, wall_damping=0.0 if name == "P7-damp0" else -1.0)
        p = capi.default_params((2, 2, 2), (32, 32, 32))
        lo, edge = (0.3, -1.1, 2.0), (1.7, 1.3, 1.1)
        grid = (27, 21, 18)
        for a in range(3):
            p.box_min[a], p.box_max[a], p.grid[a] = lo[a], lo[a] + edge[a], grid[a]
        for k, v in kw.items():
            setattr(p, k, v)
        c = np.array([[0.55, -0.95, 2.15], [0.75, -0.85, 2.35]], F)
        coll = (c, np.array([0.08, 0.05], F), np.array([[2000.0, 0, 0], [0, -1500.0, 3000.0]], F))
        return p, coll, dt
    elif name != "P0":
        raise KeyError(name)
    p = capi.default_params(box, grid)
    for k, v in kw.items():
        setattr(p, k, v)
    return p, coll, dt


PARAM_ROWS = ["P0", "P1", "P2", "P3", "P4-visc0", "P4-visc1e4", "P5", "P6-g0", "P6-gup", "P7-damp0", "P7-damp-1"]


def _case(p, kind):
    """A jittered dam lattice (spacing 2R, from the min corner) or a dense random clump with random velocities and a few
    particles on every wall, moving outward."""
    lo, hi = np.array(p.box_min[:], F), np.array(p.box_max[:], F)
    R = F(p.particle_radius)
    rng = np.random.default_rng(11)
    if kind == "dam":
        nx, ny, nz = 16, 16, 12
        i = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(F)
        pos = (lo + R + F(2) * R * i + (rng.random(i.shape, F) - F(0.5)) * F(0.02) * R).astype(F)
        # a velocity field that is not uniform: from rest, the second step's velocities are all g dt, and the viscous force
        # is then ~0 -- below what k_force resolves (it sums w_j v_j - v_i sum w_j: an absolute error of ~1e-7 |v| sum w_j,
        # DESIGN.md section 4), which at gas_constant = 0 is the largest force of the step
        return pos, ((rng.random(i.shape, F) - F(0.5)) * F(1.0)).astype(F)
    n = 4000
    side = F((n * 0.5) ** (1 / 3)) * F(2) * R                        # twice the lattice's number density
    pos = (lo + rng.random((n, 3), F) * side).astype(F)
    vel = ((rng.random((n, 3), F) - F(0.5)) * F(2 * 200.0)).astype(F)
    for k in range(24):                                              # on the walls, outward: both wall branches
        a, upper = k % 3, (k // 3) % 2
        pos[k, a] = (hi[a] - F(1e-6)) if upper else (lo[a] + F(1e-6))
        vel[k, a] = F(3000.0) if upper else F(-3000.0)
    return pos, vel


def _ctx(p, coll, n):
    c = capi.Context(n, params=p)
    if coll is not None:
        c.set_colliders(*coll)
    return c


@pytest.mark.parametrize("kind", ["dam", "clump"])
@pytest.mark.parametrize("row", PARAM_ROWS)
def test_row_against_the_model(row, kind):
    p, coll, dt = _row(row)
    pos, vel = _case(p, kind)
    n = pos.shape[0]
    # phases, each against the model
    with _ctx(p, coll, n) as c:
        c.upload(pos, vel)
        counts = sum(int(k.sum()) for k in _phases_vs_model(c, p, coll, dt))
    if kind == "clump":
        assert counts > 0, "the clump collides"
    # fused vs phased, and the direct-rows walk against the staged walk
    res = {}
    for mode in ("fused", "phased", "direct"):
        with _ctx(p, coll, n) as c:
            if mode == "direct":
                c.set_direct_hull(0)
            c.upload(pos, vel)
            (c.step_phased if mode == "phased" else c.step)(dt, 3)
            res[mode] = c.download()
    a, b = res["fused"], res["phased"]
    box = float(np.max(np.array(p.box_max[:]) - np.array(p.box_min[:])))
    assert np.isfinite(a["vel"]).all() and np.isfinite(a["density"]).all()
    assert np.abs(a["pos"] - b["pos"]).max() <= FUSED_POS * box
    _close("fused vs phased velocity", a["vel"], b["vel"], FUSED_VEL)
    assert np.array_equal(a["density"], b["density"])
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(bits(res["direct"][k]), bits(a[k])), f"direct rows: {k}"
    # mixed-precision density against the model
    with _ctx(p, coll, n) as c:
        c.set_precision(True)
        c.upload(pos, vel)
        c.hash(); c.sort(); c.build_cells(); c.density()
        rho16 = c.download(want=("density",))["density"]
    rel = rho16 / sph_model.Model(p).density(pos)[0] - 1
    assert np.abs(rel).max() <= RHO_MAX and np.sqrt(np.mean(rel ** 2)) <= RHO_RMS, (np.abs(rel).max(), np.sqrt(np.mean(rel ** 2)))


def test_set_params_between_steps():
    """P0 -> P3 -> P4 (viscosity 0) on one context: every step follows the parameters in force at that step."""
    pos, vel = _case(_row("P0")[0], "clump")
    with capi.Context(pos.shape[0], params=_row("P0")[0]) as c:
        c.upload(pos, vel)
        for row in ("P0", "P3", "P4-visc0"):
            p, coll, dt = _row(row)
            c.set_params(p)
            for _ in _phases_vs_model(c, p, coll, dt, steps=1):
                pass
        got = capi.Params()
        capi._check(c.L.sph_get_params(c.h, got))
        assert bytes(got) == bytes(p) and got.viscosity == 0.0


def test_snapshot_keeps_non_default_parameters(tmp_path):
    p, coll, dt = _row("P6-gup")
    pos, vel = _case(p, "clump")
    n = pos.shape[0]
    path = str(tmp_path / "p6.snap")
    with capi.Context(n, params=p) as a:
        a.upload(pos, vel)
        a.step(dt, 2)
        a.save(path)
        a.step(dt, 3)
        want = a.download()
    n_saved, q = capi.Context.snapshot_info(path)
    assert n_saved == n and bytes(q) == bytes(p)
    d = capi.default_params((2, 2, 2), (32, 32, 32))
    with capi.Context(n, params=d) as b:
        b.load_snapshot(path)
        got_p = capi.Params()
        capi._check(b.L.sph_get_params(b.h, got_p))
        assert bytes(got_p) == bytes(p)
        b.step(dt, 3)
        got = b.download()
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("protocol", [3, 1])
def test_non_default_row_in_four_slabs(protocol):
    """P3's physics (mass, rest density, gas constant) in 4 z-slabs on the local transport, particles crossing the cuts: the
    bits of one context under the same parameters (sph_params reaches every rank's context)."""
    from slab_oracle_engine import make_case
    pos, vel, box, grid = make_case("tall_up")
    p = capi.default_params(box, grid)
    p.mass, p.rest_density, p.gas_constant = 1.0, 500.0, 50.0
    world, steps = 4, 16
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=60)
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            comm = slab.LocalComm(hub, r)
            comm.local_hub = dev_hub
            sim = slab.NativeSlabSimulation(comm, box, grid, device_index=0, transport="local", particles=(pos, vel),
                                            protocol=protocol, params=p)
            sim.run(DT, steps)
            sim.sync()
            results[r] = sim.gather_state()
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=300)
    dev_hub.close()
    assert not errors, errors
    with capi.Context(pos.shape[0], params=p) as c:
        c.upload(pos, vel)
        c.step(DT, steps)
        ref = c.download()
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(bits(results[0][k]), bits(ref[k])), k


def test_mixed_density_in_fluid_longer_than_1024_h():
    """fp16 holds every multiple of h/2 only below 1024 h: the coarse x part of the mixed density pass must not be taken
    relative to a reference point farther away than that.  Four x-rows of 3500 particles (1094 h each at h = 0.01, spacing
    0.3125 h), each in its own (y, z) cell, so that waves straddle the rows' ends; cell edge 1.17 h."""
    h, R = 0.01, 0.01 / 6.4
    p = capi.default_params((12.0, 0.08, 0.08), (1024, 8, 8))
    p.h, p.particle_radius = h, R
    nx = 3500
    x = np.float32(-6.0) + F(R) + F(2 * R) * np.arange(nx, dtype=F)
    rows = []
    for yy in (-R, R):                 # either side of the cell boundary at 0 in y and in z
        for zz in (-R, R):
            rows.append(np.stack([x, np.full(nx, yy, F), np.full(nx, zz, F)], 1))
    pos = np.concatenate(rows).astype(F)
    pos += ((np.random.default_rng(3).random(pos.shape, F) - F(0.5)) * F(0.02 * R)).astype(F)
    want = sph_model.Model(p).density(pos)[0]
    res = {}
    with capi.Context(pos.shape[0], params=p) as c:
        for mixed in (False, True):
            c.set_precision(mixed)
            c.upload(pos, np.zeros_like(pos))
            c.hash(); c.sort(); c.build_cells(); c.density()
            res[mixed] = c.download(want=("density",))["density"]
    _close("fp32 density", res[False], want, REL_TOL)
    rel = res[True] / want - 1
    assert np.abs(rel).max() <= RHO_MAX and np.sqrt(np.mean(rel ** 2)) <= RHO_RMS, (np.abs(rel).max(), np.sqrt(np.mean(rel ** 2)))

"""GPU: the mixed-precision density pass (`k_density_h`, csrc/sph_pairs.hip) INSIDE the z-slab step (csrc/sph_slab.hip).

`bench.py --gpus N --precision mixed` runs the two together; tests/test_gpu_mixed_walks.py holds every walk of the kernel to
the float64 model, but through sph_density on a whole-domain context, which is ONE launch form.  A slab never launches the
pass over its whole owned range: it launches a range given in device memory in front of the host's wait (the deep interior,
plain block order, waves beyond the range leave early), a range with a hole whose start is rounded up to a wave (everything
that is not deep), and ranges that do not start at the first slot -- with ghost slots in front of and behind the targets
that are candidates and not targets.  The mixed result depends on which 64 slots share a wave, so the bit-for-bit bar of the
fp32 slab tests does not carry over.  What does:

  * the TOWER (tests/mixed_cases.py: d_tower) is a dyadic case that moves: packed fp16 arithmetic is exact on it at every
    step, so EVERY density equals the float64 model to the fp32 bar 1e-5 whichever wave, walk, launch form or rank produced
    it, and one dropped, doubled or stale candidate is an error above 1e-3 (tests/test_mixed_cases_cpu.py shows all of that on
    the CPU).  Every step is a rigid translation by one site: positions are known bit for bit, half of the particles change
    cell layer in every step, so slabs see migrants, in-place merges and the early force launch at that bar;
  * generic input (`tall_up`) at the documented mixed bars of tests/test_gpu_mixed_precision.py, against the float64 model
    and the fp32 whole-domain run, with a whole-domain mixed context as the control.

Under the one-message protocol (sph_slab_set_protocol(s, 1)) the receiver RECOMPUTES the densities of its inner ghost layer.
The tower shows that such a ghost density is the owner's value wherever the arithmetic is exact; `tall_up` that it is within
the mixed bar otherwise (include/sph_hip.h).
"""
import threading
from functools import lru_cache

import numpy as np
import pytest

import mixed_cases as mc
import sph_model
from conftest import bits
from gpufluidsimulator_amd import capi, slab
from slab_oracle_engine import make_case

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5                                   # tests/test_gpu_mixed_walks.py: the fp32 bar against the float64 model
RHO_MAX, RHO_RMS, VEL_TOL_20, POS_TOL_20 = 2e-2, 4e-3, 5e-3, 2e-6      # tests/test_gpu_mixed_precision.py
STAGED, DEFAULT, DIRECT = 0xFFFFFFFF, 512, 0     # sph_set_direct_hull
TOWER_STEPS = 10
FIELDS = ("h", "mass", "rest_density", "gas_constant", "viscosity", "gravity_y", "wall_eps", "wall_damping", "restitution",
          "collision_param", "particle_radius")


def _params(case):
    p = capi.default_params((1, 1, 1), case.params.grid)
    for a in range(3):
        p.box_min[a], p.box_max[a], p.grid[a] = float(case.params.box_min[a]), float(case.params.box_max[a]), int(case.params.grid[a])
    for k in FIELDS:
        setattr(p, k, float(getattr(case.params, k)))
    return p


def _with_ranks(world, body, timeout_s=120):
    """`body(make_sim, r)` on `world` threads that share one GPU over the device-to-device transport; every wait is bounded."""
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=60)
    out, errors = [None] * world, [None] * world

    def rank_main(r):
        try:
            comm = slab.LocalComm(hub, r)
            comm.local_hub = dev_hub
            out[r] = body(lambda **kw: slab.NativeSlabSimulation(comm, device_index=0, transport="local", **kw), r)
        except BaseException as e:     # noqa: BLE001
            errors[r] = e
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=timeout_s)
    dev_hub.close()
    assert errors == [None] * world, errors
    return out


# ---- the tower -----------------------------------------------------------------------------------------------------------------
def _tower_layers(shift):
    """Global cell layer of every particle of d_tower(shift), by creation index (float32 cell coordinates, as the device's)."""
    case = mc.d_tower(shift)
    return sph_model.Model(case.params).cells(case.pos)[:, 2]


def _where(owned, step):
    """What decides how a particle's density was computed in `step` of a slab run: its rank, its slot in that rank's owned
    range, whether its cell layer is one of the rank's two boundary layers, and whether the slot lies within 64 slots of an edge
    of the deep range (owned layers three and more from either cut, the start rounded up to a whole wave: the hole of the
    launches over everything else).  `owned`: per rank (z_lo, z_hi, creation index per owned slot after the step -- the
    integrate leaves every particle in its slot)."""
    layer = _tower_layers(step - 1)                   # where the particles stood when the step computed its densities
    n = layer.size
    rank, slot = np.full(n, -1), np.full(n, -1)
    boundary, near_edge = np.zeros(n, bool), np.zeros(n, bool)
    for r, (z_lo, z_hi, idx) in enumerate(owned):
        idx = idx.astype(np.int64)
        rank[idx], slot[idx] = r, np.arange(idx.size)
        lay = layer[idx]
        boundary[idx] = (lay <= z_lo) | (lay >= z_hi - 1)
        if z_hi - z_lo >= 7:
            first = int(np.searchsorted(lay, z_lo)), int(np.searchsorted(lay, z_hi))
            d0 = first[0] + ((int(np.searchsorted(lay, z_lo + 3)) - first[0] + 63) & ~63)
            d1 = max(int(np.searchsorted(lay, z_hi - 3)), d0)
            s = np.arange(idx.size)
            near_edge[idx] = (np.abs(s - d0) <= 64) | (np.abs(s - d1) <= 64)
    return rank, slot, boundary, near_edge


def _worst(rel, where=None, k=8):
    rows = []
    for i in np.argsort(-np.abs(rel))[:k]:
        row = [int(i), f"{rel[i]:+.2e}"]
        if where is not None:
            rank, slot, boundary, near_edge = where
            row += ["rank", int(rank[i]), "slot", int(slot[i]), "boundary layer" if boundary[i] else "inner layer",
                    "within 64 slots of a hole edge" if near_edge[i] else "away from the hole edges"]
        rows.append(tuple(row))
    return rows


def _check_tower_step(st, step, what, where=None):
    """The state after `step` steps from d_tower(0) under TOWER_VEL: the density the step computed is the model's (the same
    array for every shift: tests/test_mixed_cases_cpu.py), no pressure, the sites of d_tower(step), the velocity untouched.
    `where`: a callable that says where each particle was computed, for the report.  Returns the largest density error."""
    want = mc.model_density(mc.d_tower(0))
    assert np.isfinite(st["density"]).all(), (what, step)
    rel = st["density"].astype(np.float64) / want - 1
    err = float(np.abs(rel).max())
    print(f"{what}: step {step}: density max {err:.3e}, particles beyond 1e-5: {np.count_nonzero(np.abs(rel) > REL_TOL)}")
    assert err <= REL_TOL, (what, "step", step, err, np.count_nonzero(np.abs(rel) > REL_TOL), _worst(rel, where() if where else None))
    assert not st["pressure"].any(), (what, "step", step, "pressure", np.abs(st["pressure"]).max())
    sites = mc.d_tower(step).pos
    bad = np.nonzero((bits(st["pos"]) != bits(sites)).any(axis=1))[0]
    assert bad.size == 0, (what, "step", step, "positions", bad.size, bad[:6], st["pos"][bad[:3]], sites[bad[:3]])
    vel = mc.tower_velocity(sites.shape[0])
    bad = np.nonzero((bits(st["vel"]) != bits(vel)).any(axis=1))[0]
    assert bad.size == 0, (what, "step", step, "velocities", bad.size, bad[:6], st["vel"][bad[:3]])
    return err


@pytest.mark.parametrize("early", [True, False], ids=["early", "late"])
@pytest.mark.parametrize("protocol", [3, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_tower_in_slabs_is_exact(world, protocol, early):
    """The tower in 2 and 3 slabs, both protocols, the early force launch on and off, one step at a time: after EVERY step
    every density within 1e-5 of the float64 model (no outlier clause), pressure 0, positions and velocities bit for bit.  The
    run's own counters show that particles migrated, arrivals were merged in place, the early launch was used and the
    one-message protocol was spoken.  Measured on an MI355X: the largest density error is 7.4e-8 in each of the eight runs (the
    fp32 rounding of the final scale), as in one context."""
    case = mc.d_tower(0)
    p = _params(case)
    pos, vel = case.pos, mc.tower_velocity(case.pos.shape[0])
    box = tuple(float(b - a) for a, b in zip(case.params.box_min, case.params.box_max))

    def body(make, r):
        sim = make(box=box, grid=tuple(case.params.grid), particles=(pos, vel), protocol=protocol, params=p, early_force=early)
        try:
            sim.engine.ctx.set_precision(True)
            states, owned = [], []
            for _ in range(TOWER_STEPS):
                sim.step(mc.TOWER_DT)
                sim.sync()
                states.append(sim.gather_state())
                owned.append((sim.z_lo, sim.z_hi, sim.engine.download_owned()[2]))
            return states, owned, dict(sim.stats), list(sim.cuts)
        finally:
            sim.close()

    out = _with_ranks(world, body)
    stats, cuts = [o[2] for o in out], out[0][3]
    what = f"tower, {world} slabs {cuts}, protocol {protocol}, early force {'on' if early else 'off'}"
    worst = 0.0
    for k in range(1, TOWER_STEPS + 1):
        worst = max(worst, _check_tower_step(out[0][0][k - 1], k, what, lambda k=k: _where([o[1][k - 1] for o in out], k)))
    keys = ("migrants", "in_place_merges", "early_force_launches", "early_force_used", "one_message_steps")
    print(f"{what}: largest density error {worst:.3e}; " + ", ".join(f"{key} {[s[key] for s in stats]}" for key in keys))
    assert sum(s["migrants"] for s in stats) > 0, stats
    assert sum(s["in_place_merges"] for s in stats) > 0, stats
    if early:
        assert any(s["early_force_launches"] > 0 and s["early_force_used"] > 0 for s in stats), stats
    else:
        assert all(s["early_force_launches"] == 0 and s["early_force_used"] == 0 for s in stats), stats
    if protocol == 1:
        assert all(s["one_message_steps"] > 0 for s in stats), stats
    else:
        assert all(s["one_message_steps"] == 0 for s in stats), stats


@pytest.mark.parametrize("hull", [STAGED, DEFAULT, DIRECT], ids=["staged", "default", "direct"])
@pytest.mark.parametrize("sort", ["default", "merge"])
@pytest.mark.parametrize("stepper", ["step", "step_phased"])
def test_tower_in_one_context_is_exact(stepper, sort, hull):
    """The same motion through sph_step (the fused step) and sph_step_phased on a whole-domain context, under the staged walk,
    the default and the direct walk: the same per-step assertions.  Half of the particles change cell in every step, which
    the default sort mode answers with a full radix sort; "merge" (sph_set_sort_mode 2) makes the sort of the movers and its
    merge feed the mixed density pass in every step but the first."""
    case = mc.d_tower(0)
    what = f"tower, one context, {stepper}, {sort} sort, direct hull {hull:#x}"
    with capi.Context(case.pos.shape[0], params=_params(case)) as c:
        c.set_precision(True)
        c.set_direct_hull(hull)
        if sort == "merge":
            c.set_sort_mode(2)
        c.upload(case.pos, mc.tower_velocity(case.pos.shape[0]))
        worst = 0.0
        for k in range(1, TOWER_STEPS + 1):
            getattr(c, stepper)(mc.TOWER_DT, 1)
            worst = max(worst, _check_tower_step(c.download(), k, what))
        stats = c.sort_stats()
        print(f"{what}: largest density error {worst:.3e}; sorts {stats}")
        if sort == "merge":
            assert stats["merges"] >= TOWER_STEPS - 1 and stats["movers_total"] > 4000 * (TOWER_STEPS - 1), stats


# ---- generic input at the documented bars ------------------------------------------------------------------------------------------
GENERIC_DT, GENERIC_STEPS = 5e-7, 20


@lru_cache(maxsize=None)
def _tall_up():
    """`tall_up` (6,912 particles, 24 cell layers, moving up across the cuts) and what the slab runs are compared with, once:
    the float64 model's density of the initial positions, the fp32 whole-domain run, and the CONTROL -- a whole-domain mixed
    context, held to the same bars."""
    pos, vel, box, grid = make_case("tall_up")
    model_rho = sph_model.Model(capi.default_params(box, grid)).density(pos)[0]
    runs = {}
    for mixed in (False, True):
        with capi.Context(pos.shape[0], box=box, grid=grid) as c:
            c.set_precision(mixed)
            c.upload(pos, vel)
            c.step(GENERIC_DT, 1)
            rho1 = c.download(want=("density",))["density"]
            c.step(GENERIC_DT, GENERIC_STEPS - 1)
            runs[mixed] = (rho1, c.download())
    for a in [model_rho] + [v for rho1, end in runs.values() for v in (rho1, *end.values())]:
        a.setflags(write=False)
    return pos, vel, box, grid, model_rho, runs


def _generic_figures(rho1, end, model_rho, fp32_end, box):
    rel = rho1.astype(np.float64) / model_rho - 1
    return (float(np.abs(rel).max()), float(np.sqrt(np.mean(rel ** 2))),
            float(np.abs(end["vel"] - fp32_end["vel"]).max() / np.abs(fp32_end["vel"]).max()),
            float(np.abs(end["pos"] - fp32_end["pos"]).max() / max(box)))


@pytest.mark.parametrize("protocol", [3, 1])
@pytest.mark.parametrize("world", [2, 4])
def test_generic_fluid_in_mixed_slabs_meets_the_documented_bars(world, protocol):
    """Jittered input, 2 and 4 slabs, both protocols: the density of step 1 against the float64 model within 2e-2 max and 4e-3
    rms; after 20 steps velocities within 5e-3 of |v|max and positions within 2e-6 of the box edge of the fp32 whole-domain
    run.  The whole-domain mixed context is the control: where it meets a bar that a slab run misses, the slab step is at
    fault; where neither does, the bar is."""
    pos, vel, box, grid, model_rho, runs = _tall_up()
    assert np.abs(runs[False][0].astype(np.float64) / model_rho - 1).max() <= REL_TOL, "the fp32 run itself, against the model"

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), protocol=protocol)
        try:
            sim.engine.ctx.set_precision(True)
            sim.step(GENERIC_DT); sim.sync()
            rho1 = sim.gather_state()["density"]
            sim.run(GENERIC_DT, GENERIC_STEPS - 1); sim.sync()
            return rho1, sim.gather_state(), dict(sim.stats), list(sim.cuts)
        finally:
            sim.close()

    out = _with_ranks(world, body)
    stats = [o[2] for o in out]
    control = _generic_figures(runs[True][0], runs[True][1], model_rho, runs[False][1], box)
    got = _generic_figures(out[0][0], out[0][1], model_rho, runs[False][1], box)
    names = ("density max", "density rms", "velocity / |v|max after 20 steps", "position / box after 20 steps")
    for name, g, ctl, bar in zip(names, got, control, (RHO_MAX, RHO_RMS, VEL_TOL_20, POS_TOL_20)):
        print(f"tall_up, {world} slabs {out[0][3]}, protocol {protocol}: {name}: slabs {g:.3e}, one mixed context {ctl:.3e}, bar {bar:.0e}")
    assert np.isfinite(out[0][1]["density"]).all() and np.isfinite(out[0][1]["vel"]).all()
    assert sum(s["migrants"] for s in stats) > 0, stats
    if protocol == 1:
        assert all(s["one_message_steps"] > 0 for s in stats), stats
    for name, g, ctl, bar in zip(names, got, control, (RHO_MAX, RHO_RMS, VEL_TOL_20, POS_TOL_20)):
        assert ctl <= bar, ("the control misses the bar: a finding about the bar", name, ctl, bar)
        assert g <= bar, ("the slab run misses a bar the control meets: a finding about the slab step", name, g, ctl, bar)

"""GPU: the z-slab path through its product entry point, sph_slab_step (csrc/sph_slab.hip, C ABI): one call per rank
and step queues sort, migrants, halo A, density, halo B and the fused force pass on two HIP streams.  Several slabs
share the one GPU of the test box as in-process ranks (one thread each).  Two transports:
  * "local": DEVICE pointers, copies queued on the comm stream behind the sender's event (sph_local_transport_create)
    -- the product branch of slab_exchange (host_buffers = 0), the one RCCL takes on an N-GPU node: nothing drains a
    stream inside an exchange, so a missing event edge between the two streams shows up as a wrong result here;
  * "host": pinned host buffers handed to a Python callback (LocalComm) -- the branch the multi-process rehearsal over
    gloo uses.
The RCCL neighbour exchange itself needs >= 2 GPUs and has not run (only its one-rank self-send test below)."""
import threading

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic, slab
from conftest import bits
from slab_oracle_engine import far_case as _far_case, make_case

pytestmark = pytest.mark.gpu
DT = 5e-7


def _comm(hub, dev_hub, r):
    comm = slab.LocalComm(hub, r)
    comm.local_hub = dev_hub
    return comm


def _run_slabs(world, box, grid, steps, particles=None, lattice=None, transport="local", rebalance_every=0, expect_error=False,
               early_force="auto", protocol=None):
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=60) if transport == "local" else None
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), box, grid, device_index=0, transport=transport,
                                            particles=particles, lattice=lattice, early_force=early_force, protocol=protocol)
            cuts0 = list(sim.cuts)
            handles0 = (sim.engine.ctx.h.value, sim._slab.value)
            sim.run(DT, steps, rebalance_every=rebalance_every)
            sim.sync()
            kept = handles0 == (sim.engine.ctx.h.value, sim._slab.value)       # same sph_ctx, same sph_slab (re-cuts keep both)
            results[r] = (sim.gather_state(), dict(sim.stats, sort_forms=sim.engine.ctx.sort_forms(), kept=kept), sim.cuts, sim.engine.n,
                          cuts0)
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=900)
    if dev_hub is not None:
        dev_hub.close()
    if expect_error:
        return errors
    assert not errors, errors
    return results


def _exchanges_ok(stats):
    """Transport calls of a run under either protocol: three per three-group step, one per one-message step, + the second
    (exact-size) message of a burst in either."""
    return stats["exchanges"] == (3 * (stats["steps"] - stats["one_message_steps"]) + stats["rest_messages"] + stats["one_message_steps"] +
                                  stats["one_message_rests"])


def _same_bits(st, ref):
    """An N-slab run holds every cell in the order of the one-context run (arrivals from below in front of the residents
    of their cell, from above behind them: csrc/sph_slab.hip k_slab_insert, sph_sort.hip Front), so every neighbour sum
    adds the same terms in the same order: positions, velocities, densities and pressures agree in EVERY BIT.  Any
    stream/event race, stale ghost or mis-sized message shows as a bit difference instead of hiding under a tolerance."""
    for k in ("pos", "vel", "density", "pressure"):
        a, b = bits(st[k]), bits(ref[k])
        bad = np.nonzero(a != b)[0] if a.ndim == 1 else np.nonzero((a != b).any(axis=1))[0]
        assert bad.size == 0, (k, bad.size, bad[:8], st[k][bad[:4]], ref[k][bad[:4]])


def _whole_domain(pos, vel, box, grid, steps):
    with capi.Context(pos.shape[0], box=box, grid=grid) as c:
        c.upload(pos, vel)
        c.step(DT, steps)
        return c.download()


@pytest.mark.parametrize("case,world,transport", [("up", 3, "local"), ("shear", 4, "local"), ("up", 3, "host"),
                                                  ("tall_up", 2, "local"), ("tall_up", 2, "host")])
def test_slabs_with_migration_match_whole_domain(case, world, transport):
    pos, vel, box, grid = make_case(case)
    steps = 24
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), transport=transport, early_force=(case == "tall_up"))
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert sum(r[1]["migrants"] for r in res) > 0
    assert sum(r[3] for r in res) == pos.shape[0]
    assert all(r[1]["host_waits"] == steps for r in res), "one host wait per step and rank"
    # three transport calls per step (migrants, halo A, halo B), a fourth only when a side has > 255 leavers
    assert all(r[1]["exchanges"] == 3 * steps + r[1]["rest_messages"] for r in res), [r[1] for r in res]
    arrivals, in_place = sum(r[1]["resorts"] for r in res), sum(r[1]["in_place_merges"] for r in res)
    assert arrivals > 0 and in_place == arrivals, "arrivals join their boundary layer in place (k_slab_insert)"
    if case == "tall_up":        # slabs of 12 owned layers: the innermost layers' force pass runs in front of the wait, arrivals or not
        assert all(r[1]["early_force_used"] == steps for r in res), [r[1] for r in res]
    _same_bits(st, ref)


def test_slab_at_rest_skips_its_sort_and_matches():
    """A slab at rest skips its sort like a whole-domain context does (sph_sort.hip: sort_skip_if_still).  Its hash has left the
    cells of the old ghosts to that sort, which then has no k_mm_compact to clear them in: the skip clears them with a kernel
    of its own, the one place where that happens.  Three slabs (the middle one has ghosts on both sides), the block of
    make_case with no velocity field, one step per call with a sync in between -- a host in lockstep with the device, which is
    what a skip needs; then a kick through set_by_index on slabs and whole-domain twin alike, and six steps of flow: 0.036 in
    all, more than the lattice's layer spacing of half a cell (0.03125), so a layer crosses every cut inside the fluid and there
    are migrants.  A ghost cell the skip forgot, or cleared wrongly, shows in the bits."""
    pos, vel, box, grid = make_case("at rest")                 # (any name but a flow's: the lattice with zero velocities)
    kick = vel.copy()
    kick[:, 2] = 12000.0
    world, rest_steps, flow_steps = 3, 12, 6
    hub, dev_hub = slab.LocalComm.Hub(world), capi.LocalHub(world, timeout_s=60)
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), box, grid, device_index=0, transport="local", particles=(pos, vel))
            for _ in range(rest_steps):
                sim.run(DT, 1)
                sim.sync()
            skips = sim.engine.ctx.sort_stats()["skips"]
            sim.engine.ctx.set_by_index(0, vel=kick)
            for _ in range(flow_steps):
                sim.run(DT, 1)
                sim.sync()
            results[r] = (sim.gather_state(), skips, dict(sim.stats))
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=300)
    dev_hub.close()
    assert not errors, errors
    with capi.Context(pos.shape[0], box=box, grid=grid) as c:
        c.upload(pos, vel)
        c.step(DT, rest_steps)
        c.set_by_index(0, vel=kick)
        c.step(DT, flow_steps)
        ref = c.download()
    print("skips per rank", [r[1] for r in results], "migrants", [r[2]["migrants"] for r in results])
    assert results[1][1] > 0, "the middle slab never skipped a sort"
    assert sum(r[2]["migrants"] for r in results) > 0
    _same_bits(results[0][0], ref)


@pytest.mark.parametrize("case,world,transport", [("up", 3, "local"), ("shear", 3, "local"), ("down", 3, "local"), ("up", 3, "host"),
                                                  ("tall_up", 2, "local"), ("tall_up", 2, "host")])
def test_one_message_step_matches_whole_domain_bit_for_bit(case, world, transport):
    """The ONE-MESSAGE protocol (sph_slab_set_protocol(s, 1); SURVEY.md section 8e "a 2-layer halo, ghost densities recomputed
    locally (one message)"): header, leavers and the residents of two layers per side in one group per step, the receiver merges
    its own leavers into its copy of the neighbour's layers and computes the inner ghost layer's densities itself -- same
    candidates, same order, so still the bits of the one-context run.  The first step learns the message sizes under the
    three-group protocol; every later step is one transport call (+ one when a message outgrew the size fixed in advance)."""
    pos, vel, box, grid = make_case(case)
    steps = 24
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), transport=transport, early_force=(case == "tall_up"), protocol=1)
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert sum(r[1]["migrants"] for r in res) > 0 and sum(r[3] for r in res) == pos.shape[0]
    assert all(r[1]["protocol"] == 1 and r[1]["one_message_steps"] == steps - 1 for r in res), [r[1] for r in res]
    assert all(r[1]["host_waits"] == steps for r in res), "one host wait per step and rank"
    assert all(r[1]["exchanges"] == 3 + r[1]["rest_messages"] + (steps - 1) + r[1]["one_message_rests"] for r in res), [r[1] for r in res]
    assert sum(r[1]["resorts"] for r in res) > 0
    if case == "tall_up":
        assert all(r[1]["early_force_used"] == steps for r in res), [r[1] for r in res]
    _same_bits(st, ref)


def test_python_driven_protocol_still_matches():
    """SlabSimulation.step (the Python statement of the protocol that the CPU tests run with the oracle engine) with
    the product engine: same physics as the native step."""
    pos, vel, box, grid = make_case("up")
    steps, world = 12, 3
    hub = slab.LocalComm.Hub(world)
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            sim = slab.SlabSimulation(slab.LocalComm(hub, r), lambda cap, gcap, p, z0, z1: slab.HipEngine(cap, gcap, p, z0, z1, 0),
                                      box, grid, particles=(pos, vel))
            sim.run(DT, steps)
            results[r] = sim.gather_state()
            sim.engine.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=900)
    assert not errors, errors
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert np.abs(results[0]["vel"] - ref["vel"]).max() <= 1e-5 * np.abs(ref["vel"]).max()
    assert np.abs(results[0]["density"] / ref["density"] - 1).max() <= 1e-5


def test_c2_in_four_slabs_matches_whole_domain():
    """BASELINE config 2 (262144 particles) generated slab by slab from the lattice description."""
    cfg = ic.CONFIGS["C2"]
    steps = 3
    res = _run_slabs(4, cfg["box"], cfg["grid"], steps, lattice=cfg["lattice"])
    st, _, cuts, _, _ = res[0]
    counts = [r[3] for r in res]
    assert sum(counts) == 262144 and max(counts) - min(counts) <= 2 * 64 * 64 * 2, counts
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True)
    ref = _whole_domain(pos, vel, cfg["box"], cfg["grid"], steps)
    _same_bits(st, ref)


def test_weak_scaling_geometry_in_four_slabs():
    """The bench's N-GPU layout in small: a lattice stretched along z in a box stretched along z
    (ic.weak_scaling_config), jitter scaled by the per-GPU box, count-balanced cuts with the last slab
    owning the empty three quarters of the box."""
    cfg = ic.weak_scaling_config(4, per_gpu=(32, 32, 32))
    hub_world, steps = 4, 3
    hub = slab.LocalComm.Hub(hub_world)
    dev_hub = capi.LocalHub(hub_world, timeout_s=60)
    results, errors = [None] * hub_world, []

    def rank_main(r):
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), cfg["box"], cfg["grid"], device_index=0, transport="local",
                                            lattice=cfg["lattice"], jitter=True, jitter_dims=cfg["jitter_dims"])
            sim.run(DT, steps)
            results[r] = (sim.gather_state(), sim.cuts, sim.engine.n)
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(hub_world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=900)
    dev_hub.close()
    assert not errors, errors
    st, cuts, _ = results[0]
    assert cuts == [0, 16, 32, 48, cfg["grid"][2]]
    assert [r[2] for r in results] == [32 * 32 * 32] * 4
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True, jitter_dims=cfg["jitter_dims"])
    ref = _whole_domain(pos, vel, cfg["box"], cfg["grid"], steps)
    _same_bits(st, ref)


def test_slab_entry_points_directly():
    """sph_slab_counts / sph_migrants_* / sph_halo_* / sph_layer_histogram on one slab context, against
    numpy on the same particles (no communication involved)."""
    import torch
    pos, vel, box, grid = make_case("shear")
    gz = grid[2]
    layers = slab.cell_layer_of(pos[:, 2], box[2], gz)
    z_lo, z_hi = 3, 9                                   # owns layers 3..8; the case fills layers 0..11
    mine = np.nonzero((layers >= z_lo - 1) & (layers <= z_hi))[0]       # include both would-be ghost layers
    p = capi.default_params(box, grid)
    with capi.Context(len(mine) + 100, params=p, slab=(z_lo, z_hi), ghost_capacity=4096) as c:
        c.upload(pos[mine], vel[mine], mine.astype(np.uint32))
        c.hash(); c.sort()
        lay = layers[mine]
        want = (int((lay == z_lo - 1).sum()), int((lay == z_lo).sum()), int((lay == z_hi - 1).sum()), int((lay == z_hi).sum()))
        assert c.slab_counts() == want
        assert c.migrants_count() == (want[0], want[3])
        hist = c.layer_histogram()
        assert np.array_equal(hist, np.bincount(lay, minlength=gz).astype(np.uint32))
        dev = torch.device("cuda", 0)
        lo = torch.zeros((4096, 8), dtype=torch.float32, device=dev); hi = torch.zeros_like(lo)
        c.migrants_pack(lo.data_ptr(), hi.data_ptr(), 4096)
        assert c.n == len(mine) - want[0] - want[3]
        rec_lo, rec_hi = lo[:want[0]].cpu().numpy(), hi[:want[3]].cpu().numpy()
        idx_lo = np.ascontiguousarray(rec_lo[:, 3]).view(np.uint32)
        assert set(idx_lo.tolist()) == set(mine[lay == z_lo - 1].tolist())
        assert np.array_equal(rec_lo[:, 0:3], pos[idx_lo]) and np.array_equal(rec_hi[:, 4:7], vel[np.ascontiguousarray(rec_hi[:, 3]).view(np.uint32)])
        assert c.halo_count() == (want[1], want[2])
        # ghosts: give the departed particles back as ghost layers, the table must then cover everything
        c.halo_unpack(lo.data_ptr(), want[0], hi.data_ptr(), want[3])
        c.build_cells()
        k, s, cnt = c.cells()
        assert int(cnt.sum()) == len(mine)
        c.density()
        # appended migrants are owned again after hash + sort
        c.migrants_append(lo.data_ptr(), want[0])
        c.hash(); c.sort()
        assert c.n == len(mine) - want[3] and c.slab_counts()[0] == want[0]


@pytest.mark.parametrize("local_layers", [30, 31, 60, 61, 64])
def test_layer_histogram_past_one_chunk_of_targets(local_layers):
    """sph_layer_histogram finds the layers' ends 30 targets at a time and carries the last end of a chunk into the next: 30
    local layers are one full chunk, 31 one layer more, 60 two full chunks, 61 and 64 a third.  A whole-domain context, slab
    contexts over the whole grid with one and two ghost layers per side (their lowest ghost layer is global layer -1 or -2,
    their highest gz or gz + 1: neither has an entry in the histogram) and a slab in the middle of a taller grid whose ghost
    layers hold leavers; particles in every layer but a random fifth of them, which stay empty.  The integers of np.bincount
    over the float32 cell layers."""
    L = local_layers
    kinds = {"whole": (L, None, 1), "slab, 1 ghost layer": (L - 2, (0, L - 2), 1), "slab, 2 ghost layers": (L - 4, (0, L - 4), 2),
             "middle slab": (L + 6, (4, 4 + L - 2), 1)}
    for k, (what, (gz, zs, ghost_layers)) in enumerate(kinds.items()):
        box, grid = (1.0, 1.0, gz / 8.0), (8, 8, gz)
        rng = np.random.default_rng(1000 * L + k)
        pos = ((rng.random((3000, 3)) - 0.5) * np.array(box) * 0.999).astype(np.float32)
        layers = slab.cell_layer_of(pos[:, 2], box[2], gz)
        # a slab context is given the particles of its would-be ghost layers too (leavers: counted in their global layer)
        lo, hi = (max(zs[0] - 1, 0), min(zs[1], gz - 1)) if zs else (0, gz - 1)
        empty = lo + rng.permutation(hi - lo + 1)[:(hi - lo + 1) // 5]
        keep = ~np.isin(layers, empty) & (layers >= lo) & (layers <= hi)
        pos, layers = pos[keep], layers[keep]
        want = np.bincount(layers, minlength=gz).astype(np.uint32)
        assert np.count_nonzero(want[lo:hi + 1] == 0) == empty.size >= 5 and want.sum() == pos.shape[0], what
        with capi.Context(pos.shape[0] + 64, params=capi.default_params(box, grid), slab=zs, ghost_capacity=1024 if zs else 0,
                          ghost_layers=ghost_layers) as c:
            c.upload(pos, np.zeros_like(pos))
            c.hash(); c.sort()
            got = c.layer_histogram()
        assert got.dtype == np.uint32 and got.shape == (gz,)
        assert np.array_equal(got, want), (what, L, np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])


@pytest.mark.parametrize("transport,protocol", [("local", 3), ("host", 3), ("local", 1)])
def test_rebalance_on_gpu_engines(transport, protocol):
    """slab.SlabSimulation.rebalance() with the product engine: the fluid drifts out of its slabs, the
    cuts follow, whole layers change owner, the physics matches the whole-domain context."""
    pos, vel, box, grid = make_case("up")
    vel[:, 2] = 12000.0
    world, steps = 3, 65
    results = _run_slabs(world, box, grid, steps, particles=(pos, vel), transport=transport, rebalance_every=20, protocol=protocol)
    st, stats, cuts1, _, cuts0 = results[0]
    assert stats.get("rebalances", 0) >= 1 and cuts1 != cuts0
    # the re-cut happens on the device (sph_slab_recut): no rank got a new context or a new slab object, and the step
    # counters ran on through it (one host wait and three messages per step, re-cut traffic not counted)
    assert all(r[1]["kept"] for r in results)
    assert all(r[1]["steps"] == steps and r[1]["host_waits"] == steps + r[1]["far_steps"] for r in results), [r[1] for r in results]
    assert all(_exchanges_ok(r[1]) for r in results), [r[1] for r in results]
    if protocol == 1:       # every step but the first and the one after each re-cut (those learn the message sizes) is ONE message
        assert all(r[1]["protocol"] == 1 and steps - 1 - r[1].get("rebalances", 0) * 8 <= r[1]["one_message_steps"] < steps for r in results), \
            [r[1] for r in results]
    owned = [r[3] for r in results]
    assert sum(owned) == pos.shape[0] and max(owned) <= 1.35 * pos.shape[0] / world, owned
    ref = _whole_domain(pos, vel, box, grid, steps)
    _same_bits(st, ref)


@pytest.mark.parametrize("direction", ["up", "down"])
def test_particle_crossing_two_layers_in_one_step(direction):
    """The slab twin of test_gpu_edge_cases.py::test_faster_than_one_cell_per_step.  A leaver that crossed MORE than
    one cell layer does not land in the neighbour's boundary layer: its sender counts it as `far` in the migrant
    header, the receiver then takes the step's arrivals in through the pass over all particles (any key is fine
    there) instead of merging them into the boundary layer in place, counts its layers again (one more wait on that
    step only), and both sides size their ghost messages accordingly.  Result: the whole-domain physics.  "down": the same
    from the bottom layer of slab 2 into slab 1 -- the sender's far count towards rank - 1, the receiver's from rank + 1."""
    pos, vel, box, grid, fast = _far_case(direction)
    steps, world = 4, 3
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel))
    assert res[0][2] == [0, 4, 8, 64]
    far = sum(r[1]["far_steps"] for r in res)
    assert far >= 1, [r[1] for r in res]
    for r in res:
        assert r[1]["host_waits"] == steps + r[1]["far_steps"], r[1]
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert np.abs(ref["pos"][fast, 2] - pos[fast, 2]).min() > 0.14         # more than two cell layers (viscosity brakes them fast)
    _same_bits(st, ref)


@pytest.mark.parametrize("direction", ["up", "down"])
def test_one_message_step_with_particles_crossing_two_layers_and_refusing_three(direction):
    """The one-message step keeps TWO ghost layers, so a particle that crosses into the neighbour's second layer in one step is
    still inside the copy this rank holds of that layer: the sender merges it into its ghost copy where the neighbour will put
    it, the receiver takes it through the pass over all particles as ever -- whole-domain bits.  One that flies FURTHER is in
    nobody's copy: SPH_E_STATE on the ranks that see it, SPH_E_PEER on the others (the three-group protocol takes such a
    particle as long as it lands in an interior layer: test_particle_crossing_two_layers_in_one_step).  "down": the mirror
    image, from 8.25 / 8.75 cells (the bottom layer of slab 2) into the last and the second-last layer of slab 1."""
    # 0.1 = 1.6 cell layers per step: from 3.25 / 3.75 cells (the top layer of slab 0) to 4.85 / 5.35, i.e. into the FIRST and
    # the SECOND layer of slab 1
    pos, vel, box, grid, fast = _far_case(direction, 2.0e5)
    steps, world = 4, 3
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), protocol=1)
    assert res[0][2] == [0, 4, 8, 64]
    assert sum(r[1]["far_steps"] for r in res) >= 1 and all(r[1]["one_message_steps"] == steps - 1 for r in res), [r[1] for r in res]
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert np.abs(ref["pos"][fast, 2] - pos[fast, 2]).min() > 0.0625
    _same_bits(res[0][0], ref)
    pos, vel, box, grid, fast = _far_case(direction, 3.4e5)      # 2.72 layers per step: from 3.75 to 6.47 cells, the THIRD layer of slab 1
    errors = _run_slabs(world, box, grid, steps, particles=(pos, vel), protocol=1, expect_error=True)
    assert errors and any("more than TWO cell layers" in str(e) for e in errors), errors


def test_a_stopped_neighbour_is_an_error_not_a_hang():
    """Rank 1 never steps.  Rank 0's exchange (and with it the step's one wait) is bounded: it returns an error that
    names the missing message instead of spinning for ever."""
    pos, vel, box, grid = make_case("up")
    world = 2
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=2.0)
    ready = threading.Barrier(world)
    errors = [None] * world

    def rank_main(r):
        sim = None
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), box, grid, device_index=0, transport="local",
                                            particles=(pos, vel))
            capi._check(capi.load().sph_slab_set_wait_timeout(sim._slab, 2.0))
            ready.wait()
            if r == 0:
                sim.run(DT, 1)
        except BaseException as e:     # noqa: BLE001
            errors[r] = e
        finally:
            if r == 0:
                done.set()
            else:
                done.wait(timeout=60)          # rank 1 keeps its slab alive until rank 0 has given up
            if sim is not None:
                sim.close()

    done = threading.Event()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=120)
    dev_hub.close()
    assert errors[1] is None, errors
    assert isinstance(errors[0], capi.SphError) and ("never sent" in str(errors[0]) or "no migrant header" in str(errors[0])), errors


def test_eight_slabs_on_one_gpu():
    """The 8-rank layout of the metric's strong-scaling point in small (BASELINE config 2 cut into 8 slabs of 4 cell
    layers): every slab keeps >= 2 layers, counts are balanced, the result is the whole-domain result."""
    cfg = ic.CONFIGS["C2"]
    steps = 3
    res = _run_slabs(8, cfg["box"], cfg["grid"], steps, lattice=cfg["lattice"])
    st, _, cuts, _, _ = res[0]
    assert len(cuts) == 9 and all(b - a >= slab.MIN_SLAB_LAYERS for a, b in zip(cuts, cuts[1:])), cuts
    counts = [r[3] for r in res]
    assert sum(counts) == 262144 and max(counts) - min(counts) <= 2 * 64 * 64, counts
    assert all(r[1]["host_waits"] == steps for r in res)
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True)
    ref = _whole_domain(pos, vel, cfg["box"], cfg["grid"], steps)
    _same_bits(st, ref)


def test_a_burst_of_leavers_takes_the_second_migrant_message():
    """More than 255 particles cross one cut in one step: the fixed-size migrant message carries the first 255, the
    rest follows in an exact-size message (both ends know both counts from the headers)."""
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    steps, world = 3, 3
    # a 24 x 24 x 24 block: 576 particles per lattice layer.  The lattice layers just under the two cuts (cell layers 4
    # and 8: lattice layers 7 and 15 sit at 3.75 / 7.75 cells) move 0.32 cells per step: they cross at the first step
    pos2, vel2 = ic.dam_break_lattice((24, 24, 24), box, jitter=True)
    iz2 = np.arange(pos2.shape[0]) // (24 * 24)
    vel2[(iz2 == 7) | (iz2 == 15), 2] = 4.0e4
    res = _run_slabs(world, box, grid, steps, particles=(pos2, vel2))
    assert sum(r[1]["rest_messages"] for r in res) >= 2, [r[1] for r in res]
    assert sum(r[1]["migrants"] for r in res) >= 2 * 576
    st = res[0][0]
    ref = _whole_domain(pos2, vel2, box, grid, steps)
    _same_bits(st, ref)


def test_one_message_step_burst_outgrows_the_size_fixed_in_advance():
    """The one message of a step is sized from the counts of the step BEFORE (+ 1/16 + 1024 records); when a whole lattice layer
    crosses a cut at once the message outgrows that and the rest follows in a second, exact message -- on that step only."""
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    steps, world = 8, 2
    # (Leavers alone never outgrow it: they come out of the residents the message already carried.  What does is fluid reaching
    # layers that were EMPTY:) a 48 x 48 x 8 block = 2304 particles per lattice plane in cell layers 0..3, all of slab 0 of two
    # (slabs of >= 4 layers: cuts [0, 4, 64]); the block rises 0.1 cells per step, its top plane (3.75 cells) enters slab 1 at the
    # third step -- slab 1's boundary layer goes from 0 to 2304 residents at once, against the 1024 records its message was sized for
    pos2, vel2 = ic.dam_break_lattice((48, 48, 8), box, jitter=True)
    vel2[:, 2] = 1.25e4
    res = _run_slabs(world, box, grid, steps, particles=(pos2, vel2), protocol=1)
    assert res[0][2] == [0, 4, 64], res[0][2]
    assert all(r[1]["one_message_rests"] >= 1 for r in res), [r[1] for r in res]
    assert sum(r[1]["migrants"] for r in res) >= 2304 and all(_exchanges_ok(r[1]) for r in res)
    assert all(r[1]["one_message_steps"] == steps - 1 for r in res)
    _same_bits(res[0][0], _whole_domain(pos2, vel2, box, grid, steps))


def test_rccl_binding_moves_real_bytes_on_one_rank():
    """The product transport's librccl binding (dlopen, by-value ncclUniqueId, ncclSend/ncclRecv in one group) with real
    traffic: a one-rank communicator sends two messages to itself and compares what arrives (csrc/sph_slab.hip:
    sph_rccl_transport_selftest).  The neighbour exchange itself needs >= 2 GPUs (RCCL refuses two ranks on one device)."""
    tr = slab.rccl_transport(0, 1, 0, lambda raw: raw)
    try:
        L = capi.load()
        for nbytes in (16, 4 << 10, 4 << 20):
            capi._check(L.sph_rccl_transport_selftest(tr, nbytes))
    finally:
        capi.load().sph_rccl_transport_destroy(tr)


@pytest.mark.parametrize("protocol", [3, 1])
def test_slabs_under_heavy_two_way_migration(protocol):
    """Stress of the step's rarely taken branches together: random z velocities both ways (a particle crosses a cell layer
    every ~4 steps), thin 3-layer slabs next to a thick one, arrivals on both sides of a slab in the same step, steps with
    arrivals next to steps without (the halo work switches between the comm-stream form and the main-stream form).
    The result is the whole-domain result."""
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    pos, vel = ic.dam_break_lattice((24, 24, 24), box, jitter=True)
    rng = np.random.default_rng(5)
    vel[:, 2] = rng.uniform(-30000.0, 30000.0, pos.shape[0]).astype(np.float32)
    steps, world = 12, 4
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), protocol=protocol)
    stats = [r[1] for r in res]
    assert all(_exchanges_ok(s) and s["one_message_steps"] == (steps - 1 if protocol == 1 else 0) for s in stats), stats
    assert sum(s["migrants"] for s in stats) > (1500 if protocol == 3 else 800), stats          # (viscosity brakes the random motion within a few steps)
    assert sum(s["resorts"] for s in stats) >= steps, stats
    assert all(s["host_waits"] == steps + s["far_steps"] for s in stats)
    assert sum(r[3] for r in res) == pos.shape[0]
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    _same_bits(st, ref)


def test_mid_size_slabs_with_deep_interiors_and_migration():
    """857,375 particles (a 95 x 95 x 95 block in BASELINE config 2's box) in 2 slabs of 24 cell layers, moving up through
    the cut: both slabs have a deep interior (its density pass is queued before the step's host wait, the rest of the halo
    work runs on the comm stream), the upper slab has no neighbour above (its force launch for the 'boundary' chunks reaches
    into deep slots: the event that orders it behind the deep density was missing in the first version and showed only at
    sizes where kernels take tens of microseconds), and neither slab's particle count is a multiple of 64.  Kernels here
    run 50-300 us, so the two streams of a rank really overlap.  40 steps, against the whole-domain context."""
    cfg = ic.CONFIGS["C2"]
    pos, vel = ic.dam_break_lattice((95, 95, 95), cfg["box"], jitter=True)
    vel[:, 2] = 4000.0
    steps = 40
    res = _run_slabs(2, cfg["box"], cfg["grid"], steps, particles=(pos, vel))
    stats = [r[1] for r in res]
    assert sum(s["migrants"] for s in stats) > 5000 and all(s["far_steps"] == 0 for s in stats), stats
    assert all(r[3] % 64 for r in res), [r[3] for r in res]
    assert sum(r[3] for r in res) == pos.shape[0]
    st = res[0][0]
    ref = _whole_domain(pos, vel, cfg["box"], cfg["grid"], steps)
    assert np.isfinite(st["vel"]).all() and np.isfinite(st["density"]).all()
    _same_bits(st, ref)


@pytest.mark.parametrize("protocol", [3, 1])
def test_nearly_empty_slabs(protocol):
    """Ragged input for the slab step: 40 particles in a 64^3 grid cut into 3 slabs -- two ranks own nothing at first, then a
    few particles wander into one of them (arrivals into an EMPTY slab: no boundary layer to merge into, no cell table yet),
    and an isolated particle sits alone in its layer.  Every kernel of the step must cope with zero-length ranges."""
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    rng = np.random.default_rng(11)
    pos = np.zeros((40, 3), np.float32)
    pos[:, 0:2] = rng.uniform(-0.3, 0.3, (40, 2)).astype(np.float32)
    pos[:, 2] = rng.uniform(-0.05, 0.05, 40).astype(np.float32)          # a pancake around z = 0: cell layers 31 and 32
    pos[0] = (1.5, 1.5, 1.9)                                             # alone near the ceiling
    vel = np.zeros_like(pos)
    vel[:, 2] = np.where(np.arange(40) % 2 == 0, 9000.0, -9000.0)       # half go up, half go down: ~14 steps per layer
    steps, world = 45, 3
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), protocol=protocol)
    owned = [r[3] for r in res]
    assert sum(owned) == 40
    assert sum(r[1]["migrants"] for r in res) > 0
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    _same_bits(st, ref)


@pytest.mark.parametrize("seed", [100, 101, 104, 105, 107, 109, 119, 122, 124, 129,
                                  1031, 1072, 1174, 1186, 1194, 2008, 2039, 2226, 2257])
def test_slab_fuzz(seed):
    """Randomised slab runs (2-5 ranks, random block, four kinds of velocity field, 5-39 steps, local or host transport)
    against the whole-domain context, bit for bit.  Round 3 swept 580 such cases (profiles/scripts/fuzz_slabs.py, seeds
    100..129, 1000..1249, 2000..2299) at a tolerance: no failure of the step, but 9 cases beyond the bar -- random
    z-velocity fields after 27+ steps (density 1.0-2.3e-5, seed 1174 with flipped collision counts).  Cause: a particle
    that crossed a cut was put BEHIND the residents of its new cell, whereas the one-context stable sort puts an
    arrival from below in front of them; the ~1e-7 of a re-ordered fp32 sum grew from there.  With the whole-domain
    order restored at the cuts (round 4) the comparison is array_equal; those 9 seeds are the last nine here."""
    rng = np.random.default_rng(seed)
    world = int(rng.integers(2, 6))
    nx, ny = int(rng.integers(8, 40)), int(rng.integers(8, 40))
    nz = int(rng.integers(2 * world * 2, 110))
    box, grid = (8.0, 8.0, 8.0), (128, 128, 128)
    pos, vel = ic.dam_break_lattice((nx, ny, nz), box, jitter=True)
    mode = int(rng.integers(0, 4))
    if mode == 0:
        vel[:, 2] = float(rng.uniform(-9000, 9000))
    elif mode == 1:
        vel[:, 2] = rng.uniform(-20000, 20000, pos.shape[0]).astype(np.float32)
    elif mode == 2:
        vel[:, 2] = np.where(pos[:, 2] > np.median(pos[:, 2]), 6000.0, -6000.0)
    else:
        vel[:] = rng.uniform(-3000, 3000, pos.shape).astype(np.float32)
    steps = int(rng.integers(5, 40))
    transport = "local" if rng.random() < 0.8 else "host"
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), transport=transport)
    st = res[0][0]
    ref = _whole_domain(pos, vel, box, grid, steps)
    assert sum(r[3] for r in res) == pos.shape[0]
    assert all(r[1]["host_waits"] == steps + r[1]["far_steps"] for r in res)
    _same_bits(st, ref)


@pytest.mark.parametrize("seed", [100, 104, 109, 122, 1031, 1174, 2008, 2257, 3001, 3002, 3003, 3004])
def test_slab_fuzz_one_message_step(seed):
    """The same randomised runs under the one-message protocol (slabs of >= 4 layers: choose_cuts sees to it), bit for bit."""
    rng = np.random.default_rng(seed)
    world = int(rng.integers(2, 6))
    nx, ny = int(rng.integers(8, 40)), int(rng.integers(8, 40))
    nz = int(rng.integers(2 * world * 2, 110))
    box, grid = (8.0, 8.0, 8.0), (128, 128, 128)
    pos, vel = ic.dam_break_lattice((nx, ny, nz), box, jitter=True)
    mode = int(rng.integers(0, 4))
    if mode == 0:
        vel[:, 2] = float(rng.uniform(-9000, 9000))
    elif mode == 1:
        vel[:, 2] = rng.uniform(-20000, 20000, pos.shape[0]).astype(np.float32)
    elif mode == 2:
        vel[:, 2] = np.where(pos[:, 2] > np.median(pos[:, 2]), 6000.0, -6000.0)
    else:
        vel[:] = rng.uniform(-3000, 3000, pos.shape).astype(np.float32)
    steps = int(rng.integers(5, 40))
    transport = "local" if rng.random() < 0.8 else "host"
    res = _run_slabs(world, box, grid, steps, particles=(pos, vel), transport=transport, protocol=1,
                     rebalance_every=7 if seed >= 3000 else 0, early_force=True if seed % 2 else "auto")
    assert sum(r[3] for r in res) == pos.shape[0]
    assert all(r[1]["host_waits"] == steps + r[1]["far_steps"] and _exchanges_ok(r[1]) and r[1]["one_message_steps"] > 0 for r in res), \
        [r[1] for r in res]
    fields = ("pos", "vel") if seed >= 3000 and steps % 7 == 0 else ("pos", "vel", "density", "pressure")    # (a re-cut on the last step: densities are the next step's)
    ref = _whole_domain(pos, vel, box, grid, steps)
    for k in fields:
        assert np.array_equal(bits(res[0][0][k]), bits(ref[k])), k


@pytest.mark.parametrize("case", ["burst", "ramp"])
def test_movers_sort_forms_in_a_slab(case):
    """A slab's host knows the mover count of the PREVIOUS sort and launches only the sort form that count asks for
    (csrc/sph_sort.hip: radix_sort_bits).  "burst": nothing moves for three steps, then half of all particles change
    cell in ONE step (every other lattice plane in x crosses its cell face): 65,536 movers per slab reach a one-block
    sort that was launched alone for "at most 8192" -- it sorts them all the same (tile by tile, `alone`).  "ramp": half
    of the particles cross over four steps, 10,000 - 16,000 per slab and step: the multi-block passes launched alone.
    Bit for bit the whole-domain result."""
    cfg = ic.CONFIGS["C2"]
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=False)
    if case == "burst":
        vel[:, 0] = 8000.0                               # 0.004 per step: the planes 0.0156 below a face cross in step 4
    else:
        idx = np.arange(pos.shape[0])
        ix, iz = idx % 64, idx // (64 * 64)
        rng = np.random.default_rng(2)
        sel = ix % 2 == 1
        vel[sel, 0] = rng.uniform(3906.0, 8000.0, int(sel.sum())).astype(np.float32)
    # (ramp: viscosity brakes them; measured on the device, the whole domain has 20,825 / 32,271 / 28,817 / 22,672 movers
    # in steps 9 .. 12 -- per slab between 8192 and the 16,384 beyond which the next sort is a full radix sort)
    steps = 8 if case == "burst" else 13
    res = _run_slabs(2, cfg["box"], cfg["grid"], steps, particles=(pos, vel))
    forms = [r[1]["sort_forms"] for r in res]
    assert all(f[0] == 0 for f in forms), forms          # a slab never launches both forms
    if case == "burst":
        assert all(f[1] >= 3 for f in forms), forms
    else:
        assert all(f[1] >= 1 and f[2] >= 1 for f in forms), forms
    with capi.Context(pos.shape[0], box=cfg["box"], grid=cfg["grid"]) as c:
        c.upload(pos, vel)
        c.step(DT, 3)
        q0 = c.sort_stats()
        c.step(DT, 2)
        q1 = c.sort_stats()
        c.step(DT, steps - 5)
        ref = c.download()
    if case == "burst":
        assert q1["movers_total"] - q0["movers_total"] >= 100000, (q0, q1)      # the burst is what the docstring says
    _same_bits(res[0][0], ref)


@pytest.mark.parametrize("protocol", [3, 1])
def test_a_failure_on_one_rank_reaches_every_rank_within_steps_not_timeouts(protocol):
    """The top rank of three has room for exactly the particles it starts with; the fluid moves up, so the first lattice
    layer that arrives overflows it: SPH_E_CAPACITY there -- and only there, its neighbours cannot know.  The failing rank
    still exchanges what the step owes (so nobody is left waiting for a halo), then sends "abort" in its next migrant
    header: the middle rank returns SPH_E_PEER one step later, the bottom rank the step after that.  All timeouts are 60 s;
    the three ranks are done in a fraction of that, and every slab closes (nothing stays queued on a stream)."""
    import time
    pos, vel, box, grid = make_case("up")
    world = 3
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=60)
    errors, steps_done, t_end = [None] * world, [0] * world, [0.0] * world
    t0 = time.perf_counter()

    def rank_main(r):
        sim = None
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), box, grid, device_index=0, transport="local", particles=(pos, vel),
                                            capacity_factor=1.0 if r == world - 1 else 1.5, capacity_slack=0 if r == world - 1 else 4096,
                                            protocol=protocol)
            for k in range(60):
                sim.run(DT, 1)
                steps_done[r] = k + 1
        except BaseException as e:     # noqa: BLE001
            errors[r] = e
        finally:
            t_end[r] = time.perf_counter() - t0
            if sim is not None:
                failed = capi.load().sph_slab_failed(sim._slab)
                errors[r] = (errors[r], failed)
                sim.close()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=300)
    dev_hub.close()
    assert all(isinstance(e, tuple) and isinstance(e[0], capi.SphError) for e in errors), errors
    assert errors[2][1] == -4 and "exceed the capacity" in str(errors[2][0]), errors           # SPH_E_CAPACITY, the cause
    assert errors[1][1] == -6 and "upper neighbour reported a failure" in str(errors[1][0]), errors
    assert errors[0][1] == -6 and "upper neighbour reported a failure" in str(errors[0][0]), errors
    assert steps_done[1] == steps_done[2] + 1 and steps_done[0] == steps_done[2] + 2, steps_done
    assert max(t_end) < 30.0, t_end                                                          # nobody sat out a 60 s timeout


def test_long_flowing_run_in_four_slabs_bit_for_bit():
    """BASELINE config 2's dam (262,144 particles) for 3,100 steps -- from rest through the first lattice planes crossing cell
    faces into a flow with bursts of movers, leavers and arrivals at every cut, re-balancing checks every 500 steps -- in
    four slabs against one context: the same bits after thousands of steps, not just after the few dozen of the fuzz."""
    cfg = ic.CONFIGS["C2"]
    steps = 3100
    res = _run_slabs(4, cfg["box"], cfg["grid"], steps, lattice=cfg["lattice"], rebalance_every=500)
    st = res[0][0]
    stats = [r[1] for r in res]
    assert sum(s["migrants"] for s in stats) > 0 and all(s["host_waits"] == s["steps"] + s["far_steps"] for s in stats), stats
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True)
    with capi.Context(pos.shape[0], box=cfg["box"], grid=cfg["grid"]) as c:
        c.upload(pos, vel)
        c.step(DT, steps)
        ref = c.download()
        movers = c.sort_stats()["movers_total"]
    assert movers > 100 * pos.shape[0] // 100, movers            # a flowing state: every particle changed cell on average
    _same_bits(st, ref)


def _with_ranks(world, body, timeout_s=60, hub_timeout=60):
    """`body(sim_factory, r)` on `world` threads sharing one GPU over the device-to-device transport."""
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=hub_timeout)
    out, errors = [None] * world, [None] * world

    def rank_main(r):
        try:
            out[r] = body(lambda **kw: slab.NativeSlabSimulation(_comm(hub, dev_hub, r), device_index=0, transport="local", **kw), r)
        except BaseException as e:     # noqa: BLE001
            errors[r] = e
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=timeout_s)
    dev_hub.close()
    return out, errors


def test_neighbour_ping_checks_sender_direction_and_size():
    """The preflight of a multi-rank run (sph_slab_ping, called by NativeSlabSimulation._bind before the first step): one
    exchange-shaped group to rank - 1 and rank + 1 at the step's three message sizes through the slab's own transport,
    comm stream and buffers; every word is checked for its sender, direction and round.  Here over the device-to-device
    transport (RCCL refuses two ranks on one device); the RCCL transport takes the same code path on an N-GPU node.  The
    step counters do not count the ping, a size beyond the halo buffer is SPH_E_INVALID, and a rank whose neighbour does
    not take part gets an error that names the ping, not a hang."""
    import ctypes as C
    pos, vel, box, grid = make_case("up")

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel))
        try:
            L = capi.load()
            ping = dict(sim.ping)
            ex0 = int(L.sph_slab_exchanges(sim._slab))
            res = (C.c_double * 3)()
            capi._check(L.sph_slab_ping(sim._slab, 4096, 4, res))
            bad = L.sph_slab_ping(sim._slab, (sim.ghost_capacity + 2) * 32, 1, res)
            sim.run(DT, 2)
            sim.sync()
            return ping, ex0, tuple(res), bad, int(L.sph_slab_exchanges(sim._slab)), sim.message_sizes()
        finally:
            sim.close()

    out, errors = _with_ranks(3, body)
    assert errors == [None] * 3, errors
    for r, (ping, ex0, res, bad, ex1, sizes) in enumerate(out):
        assert set(ping) == {"migrants", "halo_a", "halo_b"} and ping["migrants"]["bytes"] == 8192
        assert {k: v["bytes"] for k, v in ping.items()} == sizes
        assert all(v["mean_us"] > 0.0 and v["max_us"] >= v["mean_us"] for v in ping.values()), ping
        assert ex0 == 0 and ex1 == 6, (ex0, ex1)               # two steps, three groups each: the pings are not counted
        assert res[0] > 0.0 and res[2] == 0.0
        assert bad == -1                                       # SPH_E_INVALID

    # a neighbour that never pings: bounded, and the error says what was being waited for
    def lonely(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), ping_reps=0)
        try:
            capi._check(capi.load().sph_slab_set_wait_timeout(sim._slab, 2.0))
            if r == 0:
                res = (C.c_double * 3)()
                capi._check(capi.load().sph_slab_ping(sim._slab, 4096, 1, res))
        finally:
            if r == 1:
                gone.wait(timeout=30)
            else:
                gone.set()
            sim.close()

    gone = threading.Event()
    out, errors = _with_ranks(2, lonely, hub_timeout=2.0)
    assert errors[1] is None and isinstance(errors[0], capi.SphError), errors
    assert "never sent" in str(errors[0]) or "ping" in str(errors[0]), errors


@pytest.mark.parametrize("protocol", [3, 1])
def test_slab_timing_reports_every_message_group(protocol):
    """sph_slab_timing_*: host-side step timing is always on; with timing enabled every transport call of a step is
    bracketed by an event pair on the comm stream -- three groups per step (+ the rest message on a burst), or the one group
    of the one-message step."""
    pos, vel, box, grid = make_case("up")
    steps = 12

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), protocol=protocol)
        try:
            sim.run(DT, 3)
            sim.slab_timing_reset(); sim.slab_timing_enable(True)
            sim.run(DT, steps); sim.sync()
            t = sim.slab_timing()
            sim.slab_timing_enable(False); sim.slab_timing_reset()
            sim.run(DT, 2); sim.sync()
            return t, sim.slab_timing(), dict(sim.stats)
        finally:
            sim.close()

    out, errors = _with_ranks(3, body)
    assert errors == [None] * 3, errors
    for t, t_off, stats in out:
        assert t["steps"] == steps and 0 <= t["waits_ready"] <= steps
        for k in ("host_wait_us", "host_pre_us", "host_post_us", "host_step_us"):
            assert 0.0 < t[k]["mean"] <= t[k]["max"], (k, t[k])
        assert t["host_step_us"]["mean"] >= t["host_wait_us"]["mean"]
        for g in ("migrants", "halo_a", "halo_b") if protocol == 3 else ("one",):
            e = t["exchange_us_" + g]
            assert e["calls"] == steps and 0.0 < e["mean"] <= e["max"], (g, e)
        for g in ("one", "one_rest") if protocol == 3 else ("migrants", "halo_a", "halo_b"):
            assert t["exchange_us_" + g]["calls"] == 0, (g, t["exchange_us_" + g])
        assert t["exchange_us_migrants_rest"]["calls"] == 0
        assert t_off["steps"] == 2 and all(t_off["exchange_us_" + g]["calls"] == 0 for g in ("migrants", "halo_a", "halo_b", "one"))


@pytest.mark.parametrize("protocol", [3, 1])
def test_a_failure_before_the_migrant_message_reaches_the_neighbours_in_the_same_step(protocol):
    """a step that fails BEFORE it has posted its migrant message (a device-side flag of the previous step's
    insert kernel, the sort, a launch) used to send nothing -- the neighbours then sat out the whole wait time-out.  Now the
    abort header travels as that step's migrant message: the middle rank of three raises the sticky 'arrival outside its
    boundary layer' flag by hand after 5 steps (sph_slab_test_raise_flag), fails at its next step with SPH_E_STATE, and BOTH
    neighbours return SPH_E_PEER from that same step -- with 60 s time-outs everybody is done in seconds and every slab closes."""
    import time
    pos, vel, box, grid = make_case("up")
    t0 = time.perf_counter()

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), protocol=protocol)
        done, err = 0, None
        try:
            for k in range(20):
                if r == 1 and k == 5:
                    capi._check(capi.load().sph_slab_test_raise_flag(sim._slab, 0))
                sim.run(DT, 1)
                done = k + 1
        except capi.SphError as e:
            err = e
        finally:
            failed = capi.load().sph_slab_failed(sim._slab)
            sim.close()
        return done, failed, str(err), time.perf_counter() - t0

    out, errors = _with_ranks(3, body, timeout_s=200)
    assert errors == [None] * 3, errors
    assert [o[0] for o in out] == [5, 5, 5], out                      # the same step on every rank
    assert out[1][1] == -5 and "boundary layer" in out[1][2], out     # SPH_E_STATE, the cause
    assert out[0][1] == -6 and out[2][1] == -6, out                   # SPH_E_PEER on both neighbours
    assert max(o[3] for o in out) < 30.0, out


@pytest.mark.parametrize("protocol", [3, 1])
def test_a_failure_on_the_last_step_still_lets_every_slab_close(protocol):
    """a rank that fails queues an "abort" migrant message for its neighbours' NEXT step.  When there is no next
    step (the failure came on the last one) that message is never matched: closing the slab must give up after the wait
    time-out (here 2 s; over RCCL the same bound ends in ncclCommAbort) instead of blocking in a stream synchronise."""
    import time
    pos, vel, box, grid = make_case("up")

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), capacity_factor=1.0 if r == 2 else 1.5,
                   capacity_slack=0 if r == 2 else 4096, protocol=protocol)
        capi._check(capi.load().sph_slab_set_wait_timeout(sim._slab, 2.0))
        done, err = 0, None
        try:
            for k in range(60):
                gate.wait(timeout=60)                                 # in lockstep: nobody starts step k + 1 before everybody
                if stop.is_set():                                     # is through step k -- or has failed in it
                    break
                sim.run(DT, 1)
                done = k + 1
        except capi.SphError as e:
            err = e
            stop.set()
            gate.wait(timeout=60)                                     # release the others: they take no further step
        t0 = time.perf_counter()
        try:
            sim.sync()
        except capi.SphError:
            pass
        sim.close()
        return done, str(err), time.perf_counter() - t0

    stop, gate = threading.Event(), threading.Barrier(3)
    out, errors = _with_ranks(3, body, timeout_s=200, hub_timeout=2.0)
    assert errors == [None] * 3, errors
    assert "exceed the capacity" in out[2][1], out
    assert out[0][0] == out[1][0] == out[2][0] + 1, out               # the neighbours finished the step the top rank failed in
    assert max(o[2] for o in out) < 20.0, out


def test_recut_by_several_layers_in_hops_and_into_an_empty_slab():
    """sph_slab_recut beyond the easy case: the cuts are set BY HAND far from where they were -- a cut jumps past its
    neighbour's old position (taken in several single-hop re-cuts), a slab is emptied completely and later refilled, the
    layer range of a slab grows beyond the cell table it was created with (the table is replaced, the context kept) --
    with steps in between; the state stays bit for bit the one-context run's, capacity permitting."""
    pos, vel, box, grid = make_case("shear")
    world, gz = 4, grid[2]
    plans = [[0, 2, 4, 6, gz], [0, 13, 15, 17, gz], [0, 5, 9, 11, gz], [0, 3, 6, 9, gz], [0, 8, 10, 12, gz]]

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), capacity_factor=4.2)
        try:
            h0 = (sim.engine.ctx.h.value, sim._slab.value)
            owned = []
            for cuts in plans:
                sim.run(DT, 5)
                moved = sim.rebalance(cuts=cuts)
                owned.append((moved, sim.engine.n, list(sim.cuts)))
            sim.run(DT, 5)
            sim.sync()
            import ctypes as C
            rs = (C.c_uint64 * 2)()
            capi._check(capi.load().sph_slab_recut_stats(sim._slab, rs))
            return sim.gather_state(), owned, h0 == (sim.engine.ctx.h.value, sim._slab.value), (int(rs[0]), int(rs[1])), dict(sim.stats)
        finally:
            sim.close()

    out, errors = _with_ranks(world, body, timeout_s=300)
    assert errors == [None] * world, errors
    ref = _whole_domain(pos, vel, box, grid, 5 * (len(plans) + 1))
    _same_bits(out[0][0], ref)
    assert all(o[2] for o in out), "context and slab object are kept across re-cuts"
    for k, cuts in enumerate(plans):
        assert all(o[1][k][2] == cuts for o in out) and sum(o[1][k][1] for o in out) == pos.shape[0]
    assert sum(o[3][1] for o in out) > pos.shape[0] // 2 and max(o[3][0] for o in out) >= len(plans)     # whole layers moved, in several hops
    assert all(o[4]["host_waits"] == o[4]["steps"] + o[4]["far_steps"] for o in out)


def test_recut_of_slabs_past_one_chunk_of_the_block_scan():
    """sph_slab_recut partitions a rank's owned range in blocks of 1024 slots and scans the per-block {down, up} counts in one
    workgroup, 1024 blocks at a time.  Two slabs of 36 cell layers x 32,768 particles = 1,179,648 each, 1152 blocks: the
    second chunk of the scan starts at the carry of the first.  A slab has ONE neighbour here, so the two directions take two
    re-cuts: the cut goes up by three layers (slab 1 sends down, from its first blocks: the carry is all of them), then
    down by five (slab 0, now 1248 blocks, sends up, from its last blocks).  Bit for bit the one-context run."""
    cfg = ic.CONFIGS["C2"]
    box, grid, lattice = cfg["box"], cfg["grid"], (128, 128, 144)
    moves = [3, -5]

    def body(make, r):
        sim = make(box=box, grid=grid, lattice=lattice)
        try:
            cut0, owned = sim.cuts[1], [sim.engine.n]
            for k in range(len(moves)):
                sim.run(DT, 2)
                assert sim.rebalance(cuts=[0, cut0 + sum(moves[:k + 1]), grid[2]])
                owned.append(sim.engine.n)
            sim.run(DT, 2)
            sim.sync()
            return sim.gather_state(), owned, cut0
        finally:
            sim.close()

    out, errors = _with_ranks(2, body, timeout_s=300)
    assert errors == [None] * 2, errors
    total, (below, above) = 128 * 128 * 144, (out[0][1], out[1][1])
    assert all(a + b == total for a, b in zip(below, above)) and below[0] < below[1] > below[2], (below, above)
    assert above[0] > 1024 * 1024 and below[1] > 1024 * 1024, "the slab that sends has more than 1024 blocks"
    pos, vel = ic.dam_break_lattice(lattice, box, jitter=True)
    _same_bits(out[0][0], _whole_domain(pos, vel, box, grid, 2 * (len(moves) + 1)))


def test_recut_under_the_one_message_step():
    """sph_slab_recut with the one-message protocol: cuts moved by hand (slabs of >= 4 layers: a thinner one is SPH_E_INVALID
    there), steps in between -- each re-cut is followed by one three-group step that learns the message sizes again."""
    pos, vel, box, grid = make_case("shear")
    world, gz = 3, grid[2]
    plans = [[0, 4, 8, gz], [0, 6, 10, gz], [0, 4, 8, gz]]

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), capacity_factor=3.2, protocol=1)
        try:
            for cuts in plans:
                sim.run(DT, 5)
                sim.rebalance(cuts=cuts)
            sim.run(DT, 5)
            sim.sync()
            bad = capi.load().sph_slab_recut(sim._slab, 0, 2) if r == 0 else 0       # (not collective: refused before anything is sent)
            return sim.gather_state(), dict(sim.stats), bad
        finally:
            sim.close()

    out, errors = _with_ranks(world, body, timeout_s=300)
    assert errors == [None] * world, errors
    _same_bits(out[0][0], _whole_domain(pos, vel, box, grid, 5 * (len(plans) + 1)))
    assert out[0][2] == -1                                                         # SPH_E_INVALID: two layers
    assert all(o[1]["one_message_steps"] == 20 - 1 - 2 and _exchanges_ok(o[1]) for o in out), [o[1] for o in out]


@pytest.mark.parametrize("protocol", [3, 1])
def test_one_slab_between_its_periodic_images_matches_three_stacked_copies(protocol):
    """The loop transport (sph_loop_transport_create; `bench.py --force-slab --periodic-z`): one slab whose neighbours are its own
    images shifted by the slab height does ALL the work of a rank between two neighbours -- migrants in both directions,
    both halo messages, ghost unpack, boundary launches -- on one device.  Physics check: the same slice stacked THREE times
    in one whole-domain context; for a few steps (before the free outer faces of the outer copies are felt: one cell layer
    per step) the middle copy lives between two copies of itself, i.e. in the periodic slab's world.  Positions modulo the
    slab height, velocities and densities agree to rounding (the images are shifted positions, the copies evolve on their
    own: not the same bits)."""
    import ctypes as C
    box, grid, layers = (4.0, 4.0, 4.0), (64, 64, 64), 8
    H = np.float32(layers * 4.0 / 64)                                     # 0.5
    nx = ny = 12
    nz = 2 * layers
    n = nx * ny * nz
    P, _ = ic.dam_break_lattice((nx, ny, 64), box, jitter=True, start=nx * ny * 48, count=n)      # cell layers 24 .. 31
    rng = np.random.default_rng(8)
    V = np.zeros_like(P)
    V[:, 2] = rng.uniform(-12000, 12000, n).astype(np.float32)
    steps = 5
    z_lo, z_hi = 24, 32
    L = capi.load()
    with capi.Context(2 * n + 1024, params=capi.default_params(box, grid), slab=(z_lo, z_hi), ghost_capacity=8 * nx * ny + 1024,
                      ghost_layers=2 if protocol == 1 else 1) as c:
        c.upload(P, V)
        tr = C.POINTER(capi.Transport)()
        capi._check(L.sph_loop_transport_create(C.byref(tr), float(H), 0.0, 0.0))
        h = C.c_void_p()
        capi._check(L.sph_slab_create(C.byref(h), c.h, 1, 3, tr, 0))
        if protocol == 1:
            capi._check(L.sph_slab_set_protocol(h, 1))
        try:
            capi._check(L.sph_slab_step(h, DT, steps))
            capi._check(L.sph_slab_sync(h))
            cnt = (C.c_uint64 * 8)()
            capi._check(L.sph_slab_counters(h, cnt))
            got = c.download(count=n)
            owned, exchanges = c.n, int(L.sph_slab_exchanges(h))
        finally:
            L.sph_slab_destroy(h)
            L.sph_loop_transport_destroy(tr)
    assert owned == n and int(cnt[1]) > 0 and int(cnt[4]) == steps            # nobody lost, some wrapped around, one wait per step
    assert exchanges == (3 * steps if protocol == 3 else 3 + steps - 1) + int(cnt[7])
    lo, hi = P.copy(), P.copy()
    lo[:, 2] = P[:, 2] - H; hi[:, 2] = P[:, 2] + H                        # the images' fp32 positions, as the transport makes them
    ref = _whole_domain(np.concatenate([lo, P, hi]), np.concatenate([V, V, V]), box, grid, steps)
    mid = slice(n, 2 * n)
    zb = np.float32(-2.0 + z_lo * 0.0625)
    wrap = lambda z: np.mod(z - zb, H)                                    # noqa: E731
    dz = np.abs(wrap(got["pos"][:, 2]) - wrap(ref["pos"][mid, 2]))
    dz = np.minimum(dz, H - dz)
    assert np.abs(got["pos"][:, :2] - ref["pos"][mid, :2]).max() <= 1e-6 * 4.0 and dz.max() <= 1e-6 * 4.0
    assert np.abs(got["vel"] - ref["vel"][mid]).max() <= 1e-5 * np.abs(ref["vel"]).max()
    assert np.abs(got["density"] / ref["density"][mid] - 1).max() <= 1e-5


@pytest.mark.parametrize("early", [True, False, 700])
def test_early_force_launch_gives_the_same_bits(early):
    """sph_slab_set_early_force: the fused force pass of a slab's innermost layers (six layers and more from either cut) is
    queued in front of the step's host wait -- keys by absolute slot, movers marked afterwards (k_slab_early_finish).  A dam
    slice 40 cell layers tall in two and three slabs, particles crossing the cuts both ways and changing cell inside the
    early range every step, the merge path of the sort consuming the marks: bit for bit the one-context run, switched on
    and off; on, every step uses the early result (the in-place merges of arrivals do not disturb it).  700: on, the
    launch capped at 700 slots (it then ends in the middle of a cell layer; the library's cap is 2^20)."""
    box, grid = (4.0, 4.0, 4.0), (64, 64, 64)
    pos, vel = ic.dam_break_lattice((10, 10, 80), box, jitter=True)
    rng = np.random.default_rng(4)
    vel[:] = rng.uniform(-9000, 9000, pos.shape).astype(np.float32)
    steps = 30
    for world in (2, 3):
        def body(make, r):
            sim = make(box=box, grid=grid, particles=(pos, vel))
            try:
                sim.set_early_force(early)
                sim.run(DT, steps); sim.sync()
                return sim.gather_state(), dict(sim.stats), sim.engine.ctx.sort_stats()
            finally:
                sim.close()
        out, errors = _with_ranks(world, body, timeout_s=300)
        assert errors == [None] * world, errors
        ref = _whole_domain(pos, vel, box, grid, steps)
        _same_bits(out[0][0], ref)
        assert sum(o[1]["migrants"] for o in out) > 0 and all(o[2]["merges"] >= steps - 2 for o in out), [o[1] for o in out]
        used = [o[1]["early_force_used"] for o in out]
        assert used == ([steps] * world if early else [0] * world), used

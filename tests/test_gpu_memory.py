"""GPU: what the library allocates is freed, once, on every path -- the paths that fail included.

Every device and pinned buffer of a context, a slab and the compat seam belongs to one owner (csrc/sph_common.hpp: Buffers), which
counts what it holds: sph_memory_stats reports the live device bytes, live pinned bytes and live buffers of this process's library
(hipMemGetInfo on a shared card sees everybody's processes and cannot carry an exact check).  sph_test_fail_alloc(k) makes the k-th
allocation from now return the ordinary SPH_E_NOMEM -- a host-side return taken before any HIP call -- so that a create that fails
at its 30th buffer, a refused image and a table that cannot grow each run once here.  A real out-of-memory of the device is not
covered: it would have to fill a card other people are using.

Everything runs at capacity 4096 on a 16^3 grid with 1792 particles and images of at most 96 x 64."""
import ctypes as C
import gc

import numpy as np
import pytest

import render_model as rm
from gpufluidsimulator_amd import capi, ic
from test_gpu_slabs import _same_bits, _whole_domain, _with_ranks

pytestmark = pytest.mark.gpu
CAP, GCAP, BOX, GRID = 4096, 1024, (1.0, 1.0, 1.0), (16, 16, 16)
DT = 5e-7
E_INVALID, E_NOMEM, E_STATE = -1, -3, -5
# sph_create: 12 particle arrays (posi velr posi2 velr2 keyS keyS2 dp cw fpress fvisc dvel pos_out) and 23 buffers of the sorts
# (k0 v0 k1 v1, 7 x os_*, mm_tileL mm_tileA, 9 x mm_*, the mapped word block); the table and the scratch pair come on top
N_CREATE_AT_LEAST = 12 + 23
BG = (10, 20, 30, 255)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _baseline():
    gc.collect()                     # (a context an earlier test dropped without closing must not go away half-way through this one)
    capi.fail_alloc(0)
    return capi.memory_stats()


def _code(fn, *args, **kw):
    with pytest.raises(capi.SphError) as e:
        fn(*args, **kw)
    return int(str(e.value).split("error ")[1].split(":")[0])


def _ctx(**kw):
    return capi.Context(CAP, box=BOX, grid=GRID, **kw)


def _same_state(a, b):
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


@pytest.fixture(scope="module")
def fluid():
    """8 x 8 x 28 lattice: 14 of the 16 cell layers, 128 particles each; moving up, a layer every ~8 steps."""
    pos, vel = ic.dam_break_lattice((8, 8, 28), BOX, jitter=True)
    vel[:, 2] = 4000.0
    return pos, vel


CAM_SMALL = dict(eye=(0.0, 0.0, 2.0))


def _cam(w, h):
    return capi.look_at(w, h, **CAM_SMALL)


def _life_cycle(pos, vel):
    with _ctx() as c:
        created = capi.memory_stats()
        c.upload(pos, vel)
        c.step(DT, 2)
        c.render(_cam(64, 48))
        c.render(_cam(96, 64))                             # the resize
        c.render_surface(_cam(96, 64))                     # (the default style has the thickness pass on)
        assert c.read_surface()[1].any()
        c.set_colliders([[0.2, 0.0, 0.0]], [0.1])
        c.set_collider_bodies([1.0])                       # first tracking
        c.step(DT, 1)
        c.emit(pos[:50] + np.array([0.5, 0.0, 0.0], np.float32), vel[:50])
        gone = c.remove([capi.Region.sphere(pos[0], 0.1)])
        assert len(gone) > 0
        c.step(DT, 1)
        c.sync()
        full = capi.memory_stats()
    return created, full


def test_whole_domain_life_cycle_twice_returns_every_byte(fluid):
    base = _baseline()
    first = _life_cycle(*fluid)
    assert capi.memory_stats() == base
    second = _life_cycle(*fluid)
    assert capi.memory_stats() == base
    assert first == second, "the same calls hold the same bytes"
    created, full = first
    print("after create:", [c - b for c, b in zip(created, base)], "with image, surface and tracking:", [c - b for c, b in zip(full, base)])
    assert created[2] - base[2] >= N_CREATE_AT_LEAST and full[2] - created[2] == 4 + 4 + 4      # image, planes, tracking


def test_slab_life_cycle_with_a_table_that_grows(fluid):
    """Two ranks in one process, two ghost layers, two steps of each protocol, a re-cut that gives rank 0 more cell layers than its
    table holds (the table is replaced), two more steps: the counters return to the baseline and the state is the one-context
    run's in every bit."""
    base = _baseline()
    pos, vel = fluid
    L = capi.load()
    new_cut = 11

    def body(make, r):
        sim = make(box=BOX, grid=GRID, particles=(pos, vel), protocol=1, capacity_factor=0.0, capacity_slack=CAP, ghost_factor=0.0)
        try:
            assert (sim.capacity, sim.ghost_capacity) == (CAP, GCAP)
            capi._check(L.sph_slab_set_protocol(sim._slab, 3))
            sim.run(DT, 2)
            capi._check(L.sph_slab_set_protocol(sim._slab, 1))
            sim.run(DT, 2)
            sim.sync()
            cut0 = sim.cuts[1]
            sim.comm.barrier()
            before = capi.memory_stats()
            sim.comm.barrier()
            sim.rebalance(cuts=[0, new_cut, GRID[2]])
            sim.sync()
            sim.comm.barrier()
            after = capi.memory_stats()
            sim.comm.barrier()
            sim.run(DT, 2)
            sim.sync()
            return sim.gather_state(), cut0, before, after, dict(sim.stats)
        finally:
            sim.close()

    out, errors = _with_ranks(2, body)
    assert errors == [None] * 2, errors
    assert capi.memory_stats() == base
    state, cut0, before, after, stats = out[0]
    _same_bits(state, _whole_domain(pos, vel, BOX, GRID, 6))
    # rank 0's table: (owned layers + 2 x 2 ghost layers) x 16 x 16 cells of 8 bytes (+ 2 guards, before and after); and the first
    # re-cut allocates each rank's block counts: 2 x (4096 / 1024 + 1) words
    assert new_cut > cut0 and stats["one_message_steps"] >= 1
    assert after[0] - before[0] == (new_cut - cut0) * 16 * 16 * 8 + 2 * 2 * 5 * 4 and after[2] - before[2] == 2
    assert after[1] == before[1]


def test_refused_calls_allocate_nothing(fluid):
    base = _baseline()
    L = capi.load()
    bad = capi.default_params(BOX, GRID)
    bad.grid[0] = 0
    h = capi._P()
    assert L.sph_create(C.byref(h), 0, CAP, C.byref(bad)) == E_INVALID and not h.value
    assert capi.memory_stats() == base
    with _ctx() as c:
        c.upload(*fluid)
        c.set_colliders([[0.2, 0.0, 0.0]], [0.1])
        held = capi.memory_stats()
        cam = _cam(64, 48)
        cam.focal_px = float("nan")
        assert _code(c.render, cam) == E_INVALID
        assert _code(c.render_surface, _cam(64, 48), capi.surface_defaults(smooth_radius_px=1000)) == E_INVALID
        assert _code(c.set_collider_bodies, [-1.0]) == E_INVALID
        assert capi.memory_stats() == held
    assert capi.memory_stats() == base


# ---- every allocation failure is clean ---------------------------------------------------------------------------------------
def _fail_each(attempt, after_failure):
    """attempt() with the k-th allocation failing, k = 1, 2, ... (none skipped) until it goes through; returns how many failed.
    attempt returns the call's code; after_failure(k) checks what a failure must leave."""
    k = 1
    while True:
        capi.fail_alloc(k)
        rc = attempt()
        if rc >= 0:
            capi.fail_alloc(0)          # (the hook was armed beyond the call's last allocation)
            return k - 1
        assert rc == E_NOMEM, (k, rc, capi.load().sph_last_error())
        after_failure(k)
        k += 1
        assert k < 200


def _create_failures(base):
    L = capi.load()
    params = capi.default_params(BOX, GRID)
    with _ctx():
        n_create = capi.memory_stats()[2] - base[2]
    assert n_create >= N_CREATE_AT_LEAST
    for k in range(1, n_create + 1):
        capi.fail_alloc(k)
        h = capi._P()
        assert L.sph_create(C.byref(h), 0, CAP, C.byref(params)) == E_NOMEM, k
        assert not h.value and capi.memory_stats() == base, k
    capi.fail_alloc(n_create + 1)       # one more than a create makes: it goes through (and leaves the hook armed: disarm)
    with _ctx():
        capi.fail_alloc(0)
    return n_create


def _slab_create_failures(fluid):
    L = capi.load()
    hub = capi.LocalHub(1)
    tr = hub.transport(0)
    with capi.Context(CAP, params=capi.default_params(BOX, GRID), slab=(0, GRID[2]), ghost_capacity=GCAP, ghost_layers=2) as c:
        c.upload(*fluid)
        held = capi.memory_stats()
        h = capi._P()

        def after(k):
            assert not h.value and capi.memory_stats() == held, k

        failed = _fail_each(lambda: L.sph_slab_create(C.byref(h), c.h, 0, 1, tr, 0), after)     # the last attempt went through
        n_slab = capi.memory_stats()[2] - held[2]
        # dev, host, 2 x 6 message buffers, and hop_mem where the write / wait-value probe accepts it (released where it does not)
        assert n_slab >= 14 and failed in (n_slab, n_slab + 1), (failed, n_slab)
        capi._check(L.sph_slab_step(h, DT, 2))                   # the slab the context got in the end works
        capi._check(L.sph_slab_sync(h))
        moved = c.download_owned()[0]
        assert moved.shape == fluid[0].shape and np.isfinite(moved).all() and moved[:, 2].mean() > fluid[0][:, 2].mean()
        L.sph_slab_destroy(h)
        assert capi.memory_stats() == held
    L.sph_local_transport_destroy(tr)
    hub.close()


def _tracking_failures(fluid):
    with _ctx() as c, _ctx() as ref:
        for x in (c, ref):
            x.upload(*fluid)
            x.set_colliders([[-0.4, -0.4, -0.3]], [0.05])          # inside the fluid
        held = capi.memory_stats()

        def attempt():
            try:
                c.set_collider_bodies([1.0])
                return 0
            except capi.SphError as e:
                return int(str(e).split("error ")[1].split(":")[0])

        def after(k):
            assert capi.memory_stats() == held, k
            assert c.collider_impulses()[0].shape == (0, 3)      # untracked ...
            c.step(DT, 1)                                        # ... and still steps
            ref.step(DT, 1)

        assert _fail_each(attempt, after) == 4                   # table, partial sums, masks, J
        assert capi.memory_stats()[2] - held[2] == 4
        ref.set_collider_bodies([1.0])
        for x in (c, ref):
            x.step(DT, 1)
        assert c.collider_impulses()[0].shape == (1, 3)
        assert np.array_equal(c.collider_impulses()[0], ref.collider_impulses()[0])
        _same_state(c.download(), ref.download())


def _render_failures(fluid):
    cam = _cam(96, 64)
    with _ctx() as never:
        never_code = _code(never.read_image)
    assert never_code == E_STATE
    with _ctx() as c:
        c.upload(*fluid)
        held = capi.memory_stats()

        def attempt():
            try:
                c.render(cam, background=BG)
                return 0
            except capi.SphError as e:
                return int(str(e).split("error ")[1].split(":")[0])

        def after(k):
            assert capi.memory_stats() == held, k
            assert _code(c.read_image) == never_code

        assert _fail_each(attempt, after) == 4                   # keys, rgba, id, depth
        pos, vel, idx = c.download_owned()
        want = rm.render(pos, cam, vel=vel, index=idx, background=BG, radius=c.params.particle_radius)
        got = c.read_image()
        assert (want[1] != rm.NO_ID).any()
        assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(got[0], want[0])


def _surface_failures(fluid):
    cam = _cam(96, 64)
    with _ctx() as c, _ctx() as ref:
        for x in (c, ref):
            x.upload(*fluid)
        held = capi.memory_stats()

        def attempt():
            try:
                c.render_surface(cam)
                return 0
            except capi.SphError as e:
                return int(str(e).split("error ")[1].split(":")[0])

        def after(k):
            assert capi.memory_stats() == held, k                # (a failure among the planes takes the image with it)
            assert _code(c.read_image) == E_STATE and _code(c.read_surface) == E_STATE

        assert _fail_each(attempt, after) == 8                   # the image and the four planes
        ref.render_surface(cam)
        for a, b in zip(c.read_image() + c.read_surface(), ref.read_image() + ref.read_surface()):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)
        assert c.read_surface()[1].any()


def _recut_failure(fluid):
    """Two ranks; the cut goes 7 -> 6 -> 7 first, so that each rank has its block counts and rank 1 a table to spare; then
    7 -> 8 needs a larger table on rank 0 and nothing else: the one allocation of that re-cut fails (the hook counts the allocations
    of the whole process, so a re-cut in which both ranks allocate could not say which of them fails)."""
    pos, vel = fluid
    L = capi.load()

    def body(make, r):
        sim = make(box=BOX, grid=GRID, particles=(pos, vel), protocol=1, capacity_factor=0.0, capacity_slack=CAP, ghost_factor=0.0)
        try:
            sim.run(DT, 1)
            cut = sim.cuts[1]
            sim.rebalance(cuts=[0, cut - 1, GRID[2]])
            sim.run(DT, 1)
            sim.rebalance(cuts=[0, cut, GRID[2]])
            sim.sync()
            sim.comm.barrier()
            held = capi.memory_stats()
            if r == 0:
                capi.fail_alloc(1)
            sim.comm.barrier()
            new = [0, cut + 1, GRID[2]]
            rc = L.sph_slab_recut(sim._slab, new[r], new[r + 1])
            sim.comm.barrier()
            capi.fail_alloc(0)
            after = capi.memory_stats()
            failed = L.sph_slab_failed(sim._slab)
            n_owned = sim.engine.ctx.download_owned()[0].shape[0]       # the context is still there, table and all
            sim.comm.barrier()
            return rc, failed, held, after, n_owned
        finally:
            sim.close()

    out, errors = _with_ranks(2, body)
    assert errors == [None] * 2, errors
    assert (out[0][0], out[0][1]) == (E_NOMEM, E_NOMEM) and (out[1][0], out[1][1]) == (0, 0), out
    assert out[0][2] == out[0][3], "the old table is still there, the new one is not"
    assert out[0][4] + out[1][4] == pos.shape[0]


def test_every_allocation_failure_is_clean(fluid):
    base = _baseline()
    with _ctx() as before:
        before.upload(*fluid)
        before.step(DT, 3)
        want = before.download()
    assert capi.memory_stats() == base
    n_create = _create_failures(base)
    print("buffers of a create:", n_create)
    for part in (_slab_create_failures, _tracking_failures, _render_failures, _surface_failures, _recut_failure):
        part(fluid)
        assert capi.memory_stats() == base, part.__name__
    with _ctx() as c:
        c.upload(*fluid)
        c.step(DT, 3)
        _same_state(c.download(), want)
    assert capi.memory_stats() == base


def test_the_hook_fails_once_and_disarms():
    base = _baseline()
    L = capi.load()
    params = capi.default_params(BOX, GRID)

    def create():
        h = capi._P()
        rc = L.sph_create(C.byref(h), 0, CAP, C.byref(params))
        if h.value:
            L.sph_destroy(h)
        return rc

    assert create() == 0
    capi.fail_alloc(3)
    assert create() == E_NOMEM and create() == 0                 # once, with no re-arming
    capi.fail_alloc(10000)                                       # beyond what a create allocates: nothing fails
    assert create() == 0
    capi.fail_alloc(0)
    capi.fail_alloc(2)
    capi.fail_alloc(0)                                           # disarms the armed hook
    assert create() == 0
    assert capi.memory_stats() == base

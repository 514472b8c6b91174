"""GPU: several obstacles per context (include/sph_hip.h: SEVERAL OBSTACLES, sph_obstacle_select) against the chain of numpy models
of tests/obstacle_set_model.py, BIT FOR BIT.  The method is tests/test_gpu_obstacle_pose.py's: a twin context without obstacles
gives the integrate's output, and the models pushed on that, slot after slot, must equal the context with the slots in position,
velocity, by-index row and next keys; every slot's load equals the model's ordered sums of that slot's iterations, and every
slot's offset and pose the model's advance."""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest

import obstacle_cases as oc
import obstacle_model as om
import obstacle_pose_model as pm
import obstacle_set_cases as sc
import obstacle_set_model as sm
from collider_body_model import run_length
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
BOX, GRID, BMIN, BMAX = sc.BOX, sc.GRID, sc.BMIN, sc.BMAX
EPS, DAMP, MASS = sc.EPS, sc.DAMP, sc.MASS
ZERO = sc.ZERO
N = sc.N
BAND = 4096


def _ctx(cap=N):
    return capi.Context(cap, box=BOX, grid=GRID)


def _shape(sh):
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    return capi.Shape(int(sh["kind"]), int(sh["invert"]), f3(sh["a"]), f3(sh["b"]), float(sh["r"]))


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b, what=""):
    assert np.array_equal(_u32(a), _u32(b)), (what, int((_u32(a) != _u32(b)).sum()))


def _install(c, k, solid, posed=None, sensor=None):
    """`solid` (tests/obstacle_set_cases.py) into slot k through the slot= keyword: the selection is left where it was."""
    posed = solid["pivot"] is not None if posed is None else posed
    c.build_obstacle([_shape(s) for s in solid["shapes"]], solid["spacing"], solid["bounds"], slot=k)
    c.set_obstacle_motion(offset=solid["off"], velocity=solid["u"], slot=k)
    if posed:
        c.set_obstacle_pose(solid["pivot"], solid["quat"], solid["omega"], slot=k)
    c.set_obstacle_sensor(solid["sensor"] if sensor is None else sensor, slot=k)


def _install_scene(c, scene):
    for k in sorted(scene, reverse=True):                     # (the order of installation is not the order of action)
        _install(c, k, scene[k])


def _fused(c, install):
    install()
    c.step(DT, 1)


def _phased(c, install):
    install()
    c.step_phased(DT, 1)


def _mid_step(c, install):
    c.hash(); c.sort(); c.build_cells(); c.density()
    install()                                              # between sph_density and sph_force: this step's integrate uses it
    c.force(); c.collide(); c.integrate(DT)


def _check_pair(a, b, scene, fused=True, steps_before=0, classes=None):
    """a (with the slots of `scene`) and b (without) have just taken ONE step from the same particles.  Returns the model's
    per-slot stats."""
    pa, va, ia = a.download_owned()
    pb, vb, ib = b.download_owned()
    n = pb.shape[0]
    assert a.n == b.n == n and np.array_equal(ia, ib)
    assert a.installed_obstacles() == (len(scene), sum(1 << k for k in scene))
    slots = {}
    for k, solid in scene.items():
        ob = a.obstacle(read=True, slot=k)
        slots[k] = sc.model_slot(solid, {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}, ob["phi"])
    want_p, want_v, touched, st = sc.push(pb, vb, slots)
    print({k: (int(s["touched"].sum()), int(s["kicked"].sum())) for k, s in st.items()})
    if classes is not None:                                   # the scene's conditions, on the twin's output
        cls = sm.classes(pb, slots, st, *classes)
        counts = {k: int(m.sum()) for k, m in cls.items()}
        print(counts)
        assert all(v > 0 for v in counts.values()), counts
    _same(pa, want_p, "pos")
    _same(va, want_v, "vel")
    assert touched.sum() > 0 and not np.array_equal(pa, pb)
    p4 = a.positions4()
    _same(p4[ia, :3], want_p, "positions by index")
    assert (p4[:, 3] == 1.0).all()
    nxt = sm.advance(slots, DT, 1)
    for k, solid in scene.items():
        ob = a.obstacle(slot=k)
        _same(ob["offset"], nxt[k]["off"], ("offset", k))
        got = a.obstacle_pose(slot=k)
        if slots[k]["pose"] is None:
            assert got is None
        else:
            assert np.array_equal(_u64(got["quat"]), _u64(nxt[k]["pose"]["q"])), k
            _same(got["rot"], pm.rot_of(nxt[k]["pose"]["q"]), k)
        load = a.obstacle_load(slot=k)
        if solid["sensor"]:
            J, L = sm.load(st[k], n)
            assert np.array_equal(_u64(load["J"]), _u64(J)), (k, load["J"], J)
            assert np.array_equal(_u64(load["L"]), _u64(L)), (k, load["L"], L)
            _same(load["about"], pm.world_pivot(slots[k]["pose"], slots[k]["off"]), k)
            assert load["steps"] == steps_before + 1
            assert st[k]["kicked"].sum() > 0 and np.abs(J).max() > 0 and np.abs(L).max() > 0
        else:
            assert load["steps"] == 0 and not load["J"].any() and not load["L"].any()
    a.hash()                                               # the NEXT hash: after a fused step it takes the keys the pass left
    keys = a.keys()
    slot_pos, _, _ = a.download_owned()
    assert np.array_equal(keys, oc.keys_of(slot_pos)), int((keys != oc.keys_of(slot_pos)).sum())
    if fused:                                              # (so the key fix is exercised: the push took particles to other cells)
        assert ((oc.keys_of(want_p) != oc.keys_of(pb)) & touched).sum() > 0
    return st


def _one_step(scene, stepper, fused, pos_vel=None, cap=N, configure=None, classes=None):
    pos, vel = pos_vel if pos_vel is not None else sc.dam()
    with _ctx(cap) as a, _ctx(cap) as b:
        for c in (a, b):
            if configure:
                configure(c)
            c.upload(pos, vel)
        stepper(a, lambda: _install_scene(a, scene))
        stepper(b, lambda: None)
        assert a.selected_obstacle() == 0
        return _check_pair(a, b, scene, fused, classes=classes)


# ---- 1: one step equals the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stepper,fused", [(_fused, True), (_phased, False), (_mid_step, False)], ids=["fused", "phased", "mid_step"])
def test_one_step_is_the_chain_of_models_on_the_twins_output(stepper, fused):
    """slot 0 a static ramp, slot 1 a spinning sensed paddle on a local lattice, slot 3 a translating sensed bar; slot 2 empty"""
    st = _one_step(sc.SCENE, stepper, fused, classes=(0, 1))
    assert all(s["touched"].sum() >= 100 for s in st.values())


# ---- 2: a slot alone behaves as slot 0 does ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posed", [False, True], ids=["unposed", "posed"])
@pytest.mark.parametrize("sensor", [False, True], ids=["plain", "sensed"])
def test_a_solid_alone_in_slot_2_is_the_solid_in_slot_0(posed, sensor):
    """slot 2 alone runs the set kernel, slot 0 alone the kernel of one obstacle: the same bits, so each rule kept its arithmetic"""
    pos, vel = sc.dam()
    out = []
    for k in (0, 2):
        with _ctx() as c:
            _install(c, k, sc.PADDLE, posed=posed, sensor=sensor)
            c.upload(pos, vel)
            c.step(DT, 2)
            c.step_phased(DT, 1)
            assert c.installed_obstacles() == (1, 1 << k)
            out.append((c.download_owned(), c.positions4(), c.obstacle_load(slot=k), c.obstacle(slot=k), c.obstacle_pose(slot=k)))
            c.hash()
            out[-1] += (c.keys(),)
    (da, p4a, la, oa, qa, ka), (db, p4b, lb, ob, qb, kb) = out
    for x, y in zip(da, db):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    _same(p4a, p4b)
    assert np.array_equal(ka, kb)
    assert np.array_equal(_u64(la["J"]), _u64(lb["J"])) and np.array_equal(_u64(la["L"]), _u64(lb["L"]))
    assert la["steps"] == lb["steps"] == (3 if sensor else 0) and (np.abs(la["J"]).max() > 0) == sensor
    _same(la["about"], lb["about"]); _same(oa["offset"], ob["offset"])
    assert (qa is None) == (not posed) and (qb is None) == (not posed)
    if posed:
        assert np.array_equal(_u64(qa["quat"]), _u64(qb["quat"]))


def test_the_identity_pose_is_not_the_unposed_rule_in_the_set_kernel_either():
    """a posed slot with quat (1, 0, 0, 0) goes through d = x - P and d + pivot: with a pivot far from the solid (coarser
    roundings: tests/test_obstacle_set_model_cpu.py counts the particles) the bits are the posed model's, not the unposed rule's"""
    pos, vel = sc.dam()
    st = _one_step({2: sc.IDENTITY_POSED}, _fused, True)
    out = []
    for posed in (False, True):
        with _ctx() as c:
            _install(c, 2, sc.IDENTITY_POSED, posed=posed)
            c.upload(pos, vel); c.step(DT, 1)
            out.append(c.download_owned())
    assert st[2]["touched"].sum() > 100 and (_u32(out[0][0]) != _u32(out[1][0])).any(axis=1).sum() > 20


# ---- 3: order ---------------------------------------------------------------------------------------------------------------------------
def test_each_order_of_two_overlapping_solids_is_its_model_and_they_differ():
    pos, vel = sc.dam()
    out = []
    for scene in ({0: sc.OVERLAP_A, 1: sc.OVERLAP_B}, {0: sc.OVERLAP_B, 1: sc.OVERLAP_A}):
        with _ctx() as a, _ctx() as b:
            a.upload(pos, vel); b.upload(pos, vel)
            _install_scene(a, scene)
            a.step(DT, 1); b.step(DT, 1)
            st = _check_pair(a, b, scene)
            assert (st[0]["touched"] & st[1]["touched"]).sum() > 0
            out.append(a.download_owned())
    assert not np.array_equal(_u32(out[0][0]), _u32(out[1][0])) and not np.array_equal(_u32(out[0][1]), _u32(out[1][1]))


# ---- 4: the movers' marks past one tile -----------------------------------------------------------------------------------------------
TILES_SCENE = {0: sc.RAMP, 2: dict(sc.BAR, shapes=[om.box((-1.5, -1.5, -1.3), (0.3, 0.1, 0.25))], spacing=sc.S,
                                   bounds=((-1.9, -1.7, -1.65), (-1.1, -1.3, -0.95)), off=ZERO, u=(0.0, 0.0, 200.0))}


def test_the_merge_sort_sees_the_marks_of_a_set_push_in_both_tiles():
    """27 000 particles, two tiles of the movers' marks.  After a fused step with two slots, the context that merges (it trusts
    the marks the set push put right) and the one that sorts everything from the keys hold the same keys, order and table, and
    stay the same particles through the steps that follow."""
    pos, vel = (x.copy() for x in oc.two_tiles())
    n = pos.shape[0]
    slot = oc.slots_of(oc.keys_of(pos))
    assert n == 27000 and slot.max() // oc.MM_TILE == 1

    def sorted_state(c):
        st0 = c.sort_stats()
        c.hash(); c.sort(); c.sync(); c.build_cells()
        st1 = c.sort_stats()
        assert np.array_equal(c.keys(), oc.keys_of(c.download_owned()[0])), "the keys of the slots' positions"
        return {"keys": c.keys(), "order": c.order(), "cells": c.cells(), "movers": st1["last_movers"],
                "merges": st1["merges"] - st0["merges"]}

    with _ctx(n) as a, _ctx(n) as z, _ctx(n) as b:
        for c, mode in ((a, 2), (z, 0), (b, 2)):
            c.set_sort_mode(mode)
            if c is not b:
                _install_scene(c, TILES_SCENE)
            c.upload(pos, vel)
            c.step(DT, 1)
        sb = b.download()
        slots = {}
        for k, solid in TILES_SCENE.items():
            ob = a.obstacle(read=True, slot=k)
            slots[k] = sc.model_slot(solid, {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}, ob["phi"])
        want_p, want_v, touched, st = sc.push(sb["pos"], sb["vel"], slots)
        per_tile = oc.movers_per_tile(sb["pos"], want_p, touched, slot)
        assert per_tile.shape == (2,) and per_tile.min() >= 200, per_tile
        assert (st[0]["touched"] & st[2]["touched"]).sum() > 0
        sa = a.download()
        _same(sa["pos"], want_p, "pos"); _same(sa["vel"], want_v, "vel")
        ga, gz = sorted_state(a), sorted_state(z)
        new_keys, keys0 = oc.keys_of(want_p), oc.keys_of(pos)
        assert ga["merges"] == 1 and gz["merges"] == 0
        assert ga["movers"] == int((new_keys != keys0).sum()), (ga["movers"], int((new_keys != keys0).sum()))
        for f in ("keys", "order"):
            assert np.array_equal(ga[f], gz[f]), f
        for x, y in zip(ga["cells"], gz["cells"]):
            assert np.array_equal(x, y)
        a.step(DT, 3); z.step(DT, 3)
        sa, sz = a.download(), z.download()
        for f in ("pos", "vel", "density", "pressure"):
            _same(sa[f], sz[f], f)
        assert a.sort_stats()["merges"] >= 2 and z.sort_stats()["merges"] == 0


# ---- 5: lockstep ---------------------------------------------------------------------------------------------------------------------------
def test_fifty_steps_of_two_moving_slots_in_lockstep():
    scene = {1: sc.PADDLE, 3: sc.BAR}
    pos, vel = sc.dam()
    slots = sc.model_slots(scene)
    with _ctx() as c:
        _install_scene(c, scene)
        c.upload(pos, vel)
        for step in range(50):
            if step % 2:
                c.step_phased(DT, 1)
            else:
                c.step(DT, 1)
            slots = sm.advance(slots, DT, 1)
            for k in scene:
                _same(c.obstacle(slot=k)["offset"], slots[k]["off"], (step, k))
            got = c.obstacle_pose(slot=1)
            assert np.array_equal(_u64(got["quat"]), _u64(slots[1]["pose"]["q"])), step
            _same(got["rot"], pm.rot_of(slots[1]["pose"]["q"]), step)
            assert c.obstacle_pose(slot=3) is None
        before = sm.advance(sc.model_slots(scene), DT, 49)
        for k in scene:
            load = c.obstacle_load(slot=k)
            assert load["steps"] == 50
            _same(load["about"], pm.world_pivot(before[k]["pose"], before[k]["off"]), k)
        assert c.obstacle(slot=0) is None and c.obstacle(slot=2) is None


# ---- 6: two sensing slots past 1024 waves -------------------------------------------------------------------------------------------------
BIG_N = 70001
BIG_A = dict(shapes=[om.halfspace((-1.0, -1.5, -1.4), (0.4, 1.0, -0.3))], spacing=sc.S, bounds=None, pivot=(-1.0, -1.5, -1.4),
             quat=(0.95, -0.1, 0.15, 0.2), omega=(100.0, -2000.0, 300.0), off=(0.01, 0.02, -0.01), u=(20.0, -10.0, 0.0), sensor=True)
BIG_B = dict(shapes=[om.halfspace((-1.0, -1.5, -1.5), (-0.3, 0.2, 1.0))], spacing=sc.S, bounds=None, pivot=None, off=(0.0, 0.01, 0.02),
             u=(0.0, 30.0, -15.0), sensor=True)


def test_two_loads_past_1024_waves_do_not_leak_into_each_other():
    """70 001 particles, 1094 waves, runs of 8, a last wave of 49 lanes (tests/test_gpu_obstacle_pose.py), cut by two half-spaces
    in slots 1 and 2 that kick different but overlapping sets of waves: each slot's J and L are the sums of ITS rows"""
    pos, _ = ic.dam_break_lattice((64, 32, 35), BOX, jitter=True, count=BIG_N)
    vel = np.random.default_rng(43).normal(0, 100, pos.shape).astype(F)
    st = _one_step({1: BIG_A, 2: BIG_B}, _fused, True, pos_vel=(pos, vel), cap=BIG_N)
    assert (BIG_N + 63) // 64 == 1094 and run_length(BIG_N) == 8
    wa, wb = sm.waves_of(st[1]["kicked"]), sm.waves_of(st[2]["kicked"])
    assert wa.size > 200 and wb.size > 200
    assert np.intersect1d(wa, wb).size > 20 and np.setdiff1d(wa, wb).size > 20 and np.setdiff1d(wb, wa).size > 20


# ---- 7: bookkeeping ---------------------------------------------------------------------------------------------------------------------
def test_selection_clear_and_the_installed_mask():
    pos, vel = sc.dam()
    with _ctx() as c:
        assert c.selected_obstacle() == 0 and c.installed_obstacles() == (0, 0)
        _install_scene(c, sc.SCENE)
        assert c.selected_obstacle() == 0 and c.installed_obstacles() == (3, 0b1011)
        c.upload(pos, vel)
        c.step(DT, 2)
        keep = {k: (c.obstacle(read=True, slot=k), c.obstacle_pose(slot=k), c.obstacle_load(slot=k)) for k in (0, 3)}
        c.select_obstacle(1)
        assert c.selected_obstacle() == 1 and c.obstacle_load()["steps"] == 2
        c.clear_obstacle()                                  # the selected slot alone
        assert c.obstacle() is None and c.obstacle_pose() is None and c.obstacle_load()["steps"] == 0
        assert c.installed_obstacles() == (2, 0b1001) and c.selected_obstacle() == 1
        for k in (0, 3):
            ob, ps, load = c.obstacle(read=True, slot=k), c.obstacle_pose(slot=k), c.obstacle_load(slot=k)
            for f in ("origin", "offset", "velocity", "phi"):
                _same(ob[f], keep[k][0][f], (k, f))
            assert ob["dims"] == keep[k][0]["dims"] and ps is None and keep[k][1] is None
            assert np.array_equal(_u64(load["J"]), _u64(keep[k][2]["J"])) and load["steps"] == keep[k][2]["steps"]
        assert c.selected_obstacle() == 1                   # (slot= restored it)
        # installing over a slot keeps its motion and pose
        c.select_obstacle(0)
        _install(c, 2, sc.PADDLE)
        q = c.obstacle_pose(slot=2)
        c.build_obstacle([_shape(om.sphere((-1.7, -1.7, -1.7), 0.2))], sc.S, slot=2)
        got = c.obstacle_pose(slot=2)
        assert np.array_equal(_u64(got["quat"]), _u64(q["quat"])) and c.installed_obstacles() == (3, 0b1101)
        _same(c.obstacle(slot=2)["offset"], np.array(sc.PADDLE["off"], F)); _same(c.obstacle(slot=2)["velocity"], np.array(sc.PADDLE["u"], F))
        assert c.obstacle(slot=2)["dims"] != c.obstacle(slot=3)["dims"]
        c.step(DT, 1)                                       # the set {0, 2, 3} still steps
        c.select_obstacle(3)
        c.clear_obstacles_all()
        assert c.installed_obstacles() == (0, 0) and c.selected_obstacle() == 0
        for k in range(capi.MAX_OBSTACLES):
            assert c.obstacle(slot=k) is None and c.obstacle_pose(slot=k) is None and c.obstacle_load(slot=k)["steps"] == 0
        c.step(DT, 1)


def test_refusals_change_nothing_and_allocate_nothing():
    L = capi.load()
    INVALID, STATE = -1, -5
    with capi.Context(N, params=capi.default_params(BOX, GRID), slab=(0, GRID[2]), ghost_capacity=256) as s:
        base = capi.memory_stats()
        for k in (0, 1, 3, 4):
            assert L.sph_obstacle_select(s.h, k) == STATE
        assert L.sph_obstacle_clear_all(s.h) == STATE
        assert L.sph_obstacle_selected(s.h) == 0 and L.sph_obstacle_installed(s.h, None) == 0
        assert capi.memory_stats() == base
    with _ctx() as c:
        _install(c, 1, sc.BAR)
        c.select_obstacle(1)
        base = capi.memory_stats()
        for k in (4, 5, 64, 2 ** 32 - 1):
            assert L.sph_obstacle_select(c.h, k) == INVALID, k
            assert c.selected_obstacle() == 1 and c.installed_obstacles() == (1, 0b10) and capi.memory_stats() == base
        with pytest.raises(capi.SphError):
            c.obstacle(slot=4)
        assert c.selected_obstacle() == 1 and c.obstacle() is not None


def test_a_life_cycle_returns_every_byte_with_the_sensors_of_two_slots():
    base = capi.memory_stats()
    pos, vel = sc.dam()
    waves = (N + 63) // 64
    sensor_bytes = 48 * waves + 4 * (((waves + 3) & ~3) + 4) + 72
    with _ctx() as c:
        created = capi.memory_stats()
        _install(c, 1, sc.PADDLE, sensor=False)
        _install(c, 3, sc.BAR, sensor=False)
        built = capi.memory_stats()
        c.set_obstacle_sensor(True, slot=3)
        one = capi.memory_stats()
        assert one[2] == built[2] + 3 and one[0] - built[0] == sensor_bytes     # slot 3's buffers alone
        c.set_obstacle_sensor(True, slot=1)
        two = capi.memory_stats()
        assert two[2] == one[2] + 3 and two[0] - one[0] == sensor_bytes
        c.set_obstacle_sensor(False, slot=1); c.set_obstacle_sensor(True, slot=1)          # allocated once
        assert capi.memory_stats() == two
        c.upload(pos, vel); c.step(DT, 2)
        c.clear_obstacle(slot=1)
        after = capi.memory_stats()
        assert after[0] < two[0] and c.installed_obstacles() == (1, 0b1000)
        c.clear_obstacles_all()
        assert capi.memory_stats()[0] == created[0] + 2 * sensor_bytes          # the sensors' buffers stay until sph_destroy
    assert capi.memory_stats() == base


# ---- 8: guarded allocations ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _guard(fill):
    gc.collect()
    capi.guard(BAND, fill)
    try:
        yield
    finally:
        capi.guard(0)
        last = capi.guard_check()
    assert last[0] > 0 and last[1] == 0, last


def _guarded_run(fill, pos, vel):
    n = pos.shape[0]
    with _guard(fill):
        with _ctx(n) as c:
            _install_scene(c, sc.SCENE)
            c.upload(pos, vel)
            c.step(DT, 1)
            r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
            fused = (c.download_owned(), [c.obstacle_load(slot=k) for k in (1, 3)])
            c.step_phased(DT, 1)
            r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
            phased = (c.download_owned(), [c.obstacle_load(slot=k) for k in (1, 3)])
    return fused, phased


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_guarded_set_steps_write_inside_their_buffers_and_ignore_fresh_memory(n):
    """three slots, two of them sensing, at sizes around a wave: no store outside a buffer, and the same bits whether fresh
    allocations hold zeros or a pattern.  The particles are those nearest the paddle's pivot, so every size touches a solid."""
    pos, _ = ic.dam_break_lattice((17, 17, 17), BOX, jitter=True)
    vel = np.random.default_rng(sc.VEL_SEED).normal(0, 100, pos.shape).astype(F)
    order = np.argsort(np.abs(pos - np.array(sc.PADDLE["pivot"], F)).max(axis=1), kind="stable")[:n]
    pos, vel = pos[order].copy(), vel[order].copy()
    runs = [_guarded_run(False, pos, vel), _guarded_run(True, pos, vel)]
    for (sa, la), (sb, lb) in zip(runs[0], runs[1]):
        for x, y in zip(sa, sb):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for a, b in zip(la, lb):
            assert np.array_equal(_u64(a["J"]), _u64(b["J"])) and np.array_equal(_u64(a["L"]), _u64(b["L"]))
            assert a["steps"] == b["steps"]
            _same(a["about"], b["about"])
    if n >= 63:                                             # (the paddle kicked some of them: 34 of the 63 as uploaded)
        assert np.abs(runs[0][0][1][0]["J"]).max() > 0


# ---- 9: beside the tracked spheres and the mixed-precision pass ---------------------------------------------------------------------------
def test_beside_a_tracked_sphere():
    pos, vel = sc.dam()
    with _ctx() as a, _ctx() as b:
        for c in (a, b):
            c.set_colliders([[-1.75, -1.72, -1.74]], [0.1875], [[300.0, -150.0, 80.0]])
            c.set_collider_bodies([F(50) * MASS], [[0.0, -1000.0, 0.0]])
            c.upload(pos, vel)
        _install_scene(a, sc.SCENE)
        a.step(DT, 1); b.step(DT, 1)
        ja, jb = a.collider_impulses(), b.collider_impulses()
        assert np.array_equal(_u64(ja[0]), _u64(jb[0])) and ja[1] == jb[1] == 1 and np.abs(ja[0]).max() > 0
        _check_pair(a, b, sc.SCENE)


def test_beside_the_mixed_precision_pass():
    st = _one_step(sc.SCENE, _fused, True, configure=lambda c: c.set_precision(True))
    assert all(s["touched"].sum() >= 100 for s in st.values())

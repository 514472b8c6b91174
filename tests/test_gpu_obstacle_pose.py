"""GPU: obstacles that turn and the load the fluid puts on them (include/sph_hip.h: sph_obstacle_set_pose, _get_pose, _set_sensor,
_get_load) against the numpy model of tests/obstacle_pose_model.py, BIT FOR BIT.  The method is tests/test_gpu_obstacles.py's: a
twin context without an obstacle gives the integrate's output, and the model pushed on that (in slot order: the load's sums
depend on it) must equal the obstacle context in position, velocity, by-index row and next keys; the load equals the model's
ordered sums, and the pose the model's float64 quaternion."""
import contextlib
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import obstacle_model as om
import obstacle_pose_model as pm
from collider_body_model import run_length
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
BMIN, BMAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
S = 1.0 / 16.0
EPS, DAMP, MASS = F(1e-5), F(-0.75), F(65.0)
ZERO = (0.0, 0.0, 0.0)
N = 15 * 15 * 15                                   # 3375: the last wave and the last mover tile are partial
BAND = 4096

# A local lattice (10 x 15 x 10 nodes) around the solid, so that the turned grid leaves part of the dam outside.  Both scenes
# were chosen on the CPU (the model on the dam as uploaded, velocities of VEL_SEED): the pillar touches 408 particles, pushed
# 1, 2, 3, 4 times in 29, 25, 24 and 330 cases, 246 particles outside the lattice; the paddle 327 (38, 14, 23, 252), 307 outside.
LOCAL = ((-1.95, -2.1, -1.95), (-1.55, -1.4, -1.55))
SKEW = (0.9, 0.2, -0.3, 0.25)                      # (w, x, y, z), not normalised: a skew axis
VEL_SEED = 41
SCENES = {
    "pillar": dict(shapes=[om.box((-1.75, -1.75, -1.75), (0.07, 0.3, 0.09))], bounds=LOCAL, pivot=(-1.75, -1.75, -1.75), quat=SKEW,
                   omega=ZERO, off=ZERO, u=ZERO),
    "paddle": dict(shapes=[om.box((-1.75, -1.75, -1.75), (0.25, 0.05, 0.12))], bounds=LOCAL, pivot=(-1.7, -1.8, -1.75), quat=SKEW,
                   omega=(300.0, -200.0, 4000.0), off=(0.03, -0.02, 0.04), u=(50.0, 0.0, -20.0)),
}


@functools.lru_cache(maxsize=None)
def _dam_arrays():
    pos, _ = ic.dam_break_lattice((15, 15, 15), BOX, jitter=True)      # fills [-2, -1.53]^3
    vel = np.random.default_rng(VEL_SEED).normal(0, 100, pos.shape).astype(F)
    return pos, vel


def _dam():
    pos, vel = _dam_arrays()
    return pos.copy(), vel.copy()


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


def _keys_of(pos):
    q = (((pos - F(-2.0)) / F(4.0)) * F(64.0)).astype(F)
    c = np.clip(np.floor(q).astype(np.int64), 0, 63)
    return ((c[:, 2] * 64 + c[:, 1]) * 64 + c[:, 0]).astype(np.uint32)


def _install(c, sc, posed=True, sensor=True):
    c.build_obstacle([_shape(s) for s in sc["shapes"]], S, sc["bounds"])
    c.set_obstacle_motion(offset=sc["off"], velocity=sc["u"])
    if posed:
        c.set_obstacle_pose(sc["pivot"], sc["quat"], sc["omega"])
    c.set_obstacle_sensor(sensor)


def _pose_of(sc, posed=True):
    return pm.pose(sc["pivot"], sc["quat"], sc["omega"]) if posed else None


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


def _check_pair(a, b, sc, posed=True, sensor=True, fused=True, steps_before=0):
    """a (with the obstacle of `sc`) and b (without) have just taken ONE step from the same particles.  Every particle, the
    by-index rows, the next keys, the load and the advanced pose against the model on b's output.  Returns the model's stats."""
    pa, va, ia = a.download_owned()
    pb, vb, ib = b.download_owned()
    n = pb.shape[0]
    assert a.n == b.n == n and np.array_equal(ia, ib)
    ob = a.obstacle(read=True)
    grid = {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}
    ps = _pose_of(sc, posed)
    st = {}
    want_p, want_v, touched = pm.push(pb, vb, grid, ob["phi"], sc["off"], sc["u"], ps, BMIN, BMAX, EPS, DAMP, MASS, stats=st)
    st["touched"] = touched
    st["inside"] = pm.sample(grid, ob["phi"], sc["off"], ps, pb)[2]
    print("touched", int(touched.sum()), "iterations", np.bincount(st["iterations"], minlength=5), "outside the lattice",
          int((~st["inside"]).sum()), "kicked", int(st["kicked"].sum()))
    _same(pa, want_p, "pos")
    _same(va, want_v, "vel")
    assert touched.sum() > 0 and not np.array_equal(pa, pb)
    p4 = a.positions4()
    _same(p4[ia, :3], want_p, "positions by index")
    assert (p4[:, 3] == 1.0).all()
    # the advanced state: offset, quaternion (float64) and rot (float32)
    _same(ob["offset"], om.advance(sc["off"], sc["u"], DT, 1))
    got = a.obstacle_pose()
    if posed:
        nxt, _ = pm.advance(ps, sc["off"], sc["u"], DT)
        assert np.array_equal(_u64(got["quat"]), _u64(nxt["q"])), (got["quat"], nxt["q"])
        _same(got["rot"], pm.rot_of(nxt["q"]))
        _same(got["pivot"], ps["pivot"]); _same(got["omega"], ps["omega"])
    else:
        assert got is None
    load = a.obstacle_load()
    if sensor:
        J, L = pm.load_in_order(st["lane"], st["kicked"], n)
        assert np.array_equal(_u64(load["J"]), _u64(J)), (load["J"], J)
        assert np.array_equal(_u64(load["L"]), _u64(L)), (load["L"], L)
        _same(load["about"], pm.world_pivot(ps, sc["off"]))
        assert load["steps"] == steps_before + 1
        assert st["kicked"].sum() > 0 and np.abs(J).max() > 0 and np.abs(L).max() > 0
    else:
        assert load["steps"] == 0 and not load["J"].any() and not load["L"].any()
    a.hash()                                               # the NEXT hash: after a fused step it takes the keys the pass left
    keys = a.keys()
    slot_pos, _, _ = a.download_owned()
    assert np.array_equal(keys, _keys_of(slot_pos)), int((keys != _keys_of(slot_pos)).sum())
    if fused:                                              # (so the key fix is exercised: the push took particles to other cells)
        assert ((_keys_of(want_p) != _keys_of(pb)) & touched).sum() > 0
    return st


def _one_step(sc, stepper, fused, posed=True, sensor=True, pos_vel=None, cap=N, configure=None):
    pos, vel = pos_vel if pos_vel is not None else _dam()
    with _ctx(cap) as a, _ctx(cap) as b:
        for c in (a, b):
            if configure:
                configure(c)
            c.upload(pos, vel)
        stepper(a, lambda: _install(a, sc, posed, sensor))
        stepper(b, lambda: None)
        return _check_pair(a, b, sc, posed, sensor, fused)


def _assert_scene(st):
    assert st["touched"].sum() >= 100, st["touched"].sum()
    assert (np.bincount(st["iterations"], minlength=5)[1:] > 0).all(), np.bincount(st["iterations"])
    assert st["inside"].sum() > 0 and (~st["inside"]).sum() > 0


# ---- the push of a posed context, fused and phased ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["pillar", "paddle"])
@pytest.mark.parametrize("stepper,fused", [(_fused, True), (_phased, False)], ids=["fused", "phased"])
def test_one_step_is_the_model_on_the_twins_output(scene, stepper, fused):
    _assert_scene(_one_step(SCENES[scene], stepper, fused))


def test_set_between_density_and_force_the_integrate_uses_it():
    _assert_scene(_one_step(SCENES["paddle"], _mid_step, False))


def test_the_sensor_on_an_unposed_context():
    """P = off, d = x - off, and the particles are the plain obstacle's"""
    sc = dict(SCENES["paddle"], shapes=[om.box((-1.78, -1.73, -1.77), (0.25, 0.05, 0.12))])
    st = _one_step(sc, _fused, True, posed=False)
    assert st["touched"].sum() >= 100


def test_sensor_on_and_off_give_the_same_particles():
    sc = SCENES["paddle"]
    pos, vel = _dam()
    out = []
    for sensor in (True, False):
        with _ctx() as c:
            _install(c, sc, sensor=sensor)
            c.upload(pos, vel)
            c.step(DT, 3)
            c.step_phased(DT, 2)
            out.append((c.download_owned(), c.positions4(), c.obstacle_load()))
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    _same(out[0][1], out[1][1])
    assert out[0][2]["steps"] == 5 and out[1][2]["steps"] == 0


def test_the_merge_sort_sees_the_marks_of_a_posed_push():
    sc = SCENES["paddle"]
    pos, vel = _dam()
    out = []
    for merge in (True, False):
        with _ctx() as c:
            c.set_sort_mode(merge)
            _install(c, sc)
            c.upload(pos, vel)
            c.step(DT, 20)
            out.append((c.download(), c.sort_stats(), c.positions4(), c.obstacle_load()))
    for k in ("pos", "vel", "density", "pressure"):
        _same(out[0][0][k], out[1][0][k], k)
    _same(out[0][2], out[1][2])
    assert out[0][1]["merges"] >= 10 and out[0][1]["movers_total"] > 0 and out[1][1]["merges"] == 0, (out[0][1], out[1][1])
    assert np.array_equal(_u64(out[0][3]["J"]), _u64(out[1][3]["J"])) and np.array_equal(_u64(out[0][3]["L"]), _u64(out[1][3]["L"]))


# ---- the pose in lockstep with the model ---------------------------------------------------------------------------------------------
def test_fifty_steps_of_a_spinning_paddle_in_lockstep():
    sc = SCENES["paddle"]
    pos, vel = _dam()
    ps, off = _pose_of(sc), np.array(sc["off"], F)
    with _ctx() as c:
        _install(c, sc)
        c.upload(pos, vel)
        got = c.obstacle_pose()
        assert np.array_equal(_u64(got["quat"]), _u64(ps["q"]))
        _same(got["rot"], pm.rot_of(ps["q"]))
        for step in range(50):
            if step % 2:
                c.step_phased(DT, 1)
            else:
                c.step(DT, 1)
            ps, off = pm.advance(ps, off, sc["u"], DT)
            got = c.obstacle_pose()
            assert np.array_equal(_u64(got["quat"]), _u64(ps["q"])), step
            _same(got["rot"], pm.rot_of(ps["q"]), step)
            _same(c.obstacle()["offset"], off, step)
        load = c.obstacle_load()
        assert load["steps"] == 50
        _same(load["about"], pm.world_pivot(pm.advance(_pose_of(sc), sc["off"], sc["u"], DT, 49)[0],
                                            om.advance(sc["off"], sc["u"], DT, 49)))
    assert abs(float(ps["q"] @ ps["q"]) - 1.0) < 1e-12 and not np.array_equal(ps["q"], _pose_of(sc)["q"])


def test_the_pose_only_advances_while_a_grid_is_installed():
    sc = SCENES["paddle"]
    pos, vel = _dam()
    with _ctx() as c:
        c.set_obstacle_pose(sc["pivot"], sc["quat"], sc["omega"])
        c.upload(pos, vel)
        c.step(DT, 3)
        assert np.array_equal(_u64(c.obstacle_pose()["quat"]), _u64(_pose_of(sc)["q"]))
        assert c.obstacle() is None


# ---- sample -----------------------------------------------------------------------------------------------------------------------------
def test_sample_on_a_posed_context():
    sc = SCENES["paddle"]
    rng = np.random.default_rng(17)
    pts = rng.uniform(-2.2, -1.3, (1001, 3)).astype(F)
    pts[:40, 0] = np.nan; pts[40:80, 1] = np.inf; pts[80:120, 2] = -np.inf; pts[120:160] = rng.uniform(-50, 50, (40, 3))
    with _ctx(64) as c:
        _install(c, sc, sensor=False)
        ob = c.obstacle(read=True)
        got_phi, got_n, got_in = c.sample_obstacle(pts)
    grid = {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}
    want_phi, want_n, want_in, _ = pm.sample(grid, ob["phi"], sc["off"], _pose_of(sc), pts)
    assert 200 < want_in.sum() < 900 and not want_in[:160].any()
    assert np.array_equal(got_in, want_in)
    _same(got_phi, want_phi); _same(got_n, want_n)
    assert np.isinf(got_phi[~got_in]).all() and not got_n[~got_in].any()
    # (the rotation is seen: the unposed rule gives other bits)
    assert not np.array_equal(_u32(om.sample(grid, ob["phi"], sc["off"], pts)[0]), _u32(want_phi))


# ---- the sums: one short run, and past 1024 waves ---------------------------------------------------------------------------------------
def test_the_load_of_one_short_run():
    pos, vel = _dam()
    order = np.argsort(np.abs(pos - np.array([-1.75, -1.75, -1.75], F)).max(axis=1))[:100]     # the 100 nearest the solid
    st = _one_step(SCENES["paddle"], _fused, True, pos_vel=(pos[order].copy(), vel[order].copy()), cap=100)
    assert run_length(100) == 4 and st["kicked"].sum() >= 5


BIG_N = 70001
BIG = dict(shapes=[om.halfspace((-1.0, -1.5, -1.4), (0.4, 1.0, -0.3))], bounds=None, pivot=(-1.0, -1.5, -1.4), quat=(0.95, -0.1, 0.15, 0.2),
           omega=(100.0, -2000.0, 300.0), off=(0.01, 0.02, -0.01), u=(20.0, -10.0, 0.0))


def test_the_load_past_1024_waves():
    """70 001 particles of the 64 x 32 x 35 lattice (x in [-2, 0], y in [-2, -1], z in [-2, -0.9]) cut by a large turned
    half-space: 1094 waves, runs of 8, a last wave of 49 lanes"""
    pos, _ = ic.dam_break_lattice((64, 32, 35), BOX, jitter=True, count=BIG_N)
    vel = np.random.default_rng(43).normal(0, 100, pos.shape).astype(F)
    st = _one_step(BIG, _fused, True, pos_vel=(pos, vel), cap=BIG_N)
    assert (BIG_N + 63) // 64 == 1094 and run_length(BIG_N) == 8 and BIG_N % 64 == 49
    waves = np.unique(np.nonzero(st["kicked"])[0] // 64)
    runs = np.unique(waves // 8)
    assert waves.size > 200 and runs.size > 40 and st["kicked"].sum() > 5000, (waves.size, runs.size)
    assert waves.max() == 1093                              # the partial last wave holds a kicked lane


def test_a_step_with_nothing_in_contact_reads_zeros():
    sc = dict(SCENES["pillar"], off=(2.5, 2.5, 2.5))        # carried far from the dam
    pos, vel = _dam()
    with _ctx() as a, _ctx() as b:
        a.upload(pos, vel); b.upload(pos, vel)
        _install(a, sc)
        a.step(DT, 1); b.step(DT, 1)
        for x, y in zip(a.download_owned(), b.download_owned()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        load = a.obstacle_load()
        assert load["steps"] == 1 and not load["J"].any() and not load["L"].any()
        _same(load["about"], pm.world_pivot(_pose_of(sc), sc["off"]))
        a.step_phased(DT, 1)
        assert a.obstacle_load()["steps"] == 2
    with _ctx() as c:                                       # no particles: the sum still runs and writes zeros
        _install(c, SCENES["paddle"])
        c.step(DT, 1)
        load = c.obstacle_load()
        assert load["steps"] == 1 and not load["J"].any() and not load["L"].any()
        _same(load["about"], pm.world_pivot(_pose_of(SCENES["paddle"]), SCENES["paddle"]["off"]))
    with _ctx() as c:                                       # the sensor without an obstacle: legal, zeros
        c.set_obstacle_sensor(True)
        c.upload(pos, vel)
        c.step(DT, 1)
        load = c.obstacle_load()
        assert load["steps"] == 0 and not load["J"].any() and not load["L"].any() and not load["about"].any()


# ---- the life cycle ------------------------------------------------------------------------------------------------------------------
def test_clear_resets_the_pose_and_a_new_grid_keeps_it():
    sc = SCENES["paddle"]
    pos, vel = _dam()
    with _ctx() as c:
        _install(c, sc)
        c.upload(pos, vel)
        c.step(DT, 2)
        q2 = c.obstacle_pose()["quat"]
        assert c.obstacle_load()["steps"] == 2
        c.build_obstacle([_shape(om.sphere((-1.7, -1.7, -1.7), 0.2))], S)          # another grid: the pose stays
        got = c.obstacle_pose()
        assert np.array_equal(_u64(got["quat"]), _u64(q2)) and np.array_equal(_u64(q2), _u64(pm.advance(_pose_of(sc), ZERO, ZERO, DT, 2)[0]["q"]))
        assert c.obstacle_load()["steps"] == 2
        c.clear_obstacle()
        assert c.obstacle_pose() is None
        load = c.obstacle_load()
        assert load["steps"] == 0 and not load["J"].any() and not load["L"].any() and not load["about"].any()
        # the sensor's switch stayed: the next obstacle is sensed without another call
        c.build_obstacle([_shape(s) for s in sc["shapes"]], S, sc["bounds"])
        c.step(DT, 1)
        load = c.obstacle_load()
        assert load["steps"] == 1 and np.abs(load["J"]).max() > 0
        c.set_obstacle_pose(sc["pivot"], sc["quat"], sc["omega"])
        c.set_obstacle_pose(None)                              # dropped by the caller
        assert c.obstacle_pose() is None


def test_refusals_change_nothing_and_allocate_nothing():
    L = capi.load()
    INVALID, STATE = -1, -5
    sc = SCENES["paddle"]

    def pose(pivot=sc["pivot"], quat=sc["quat"], omega=sc["omega"]):
        f = lambda v, k: (C.c_float * k)(*[float(x) for x in v])
        return capi.ObstaclePose(f(pivot, 3), f(quat, 4), f(omega, 3))

    with capi.Context(N, params=capi.default_params(BOX, GRID), slab=(0, GRID[2]), ghost_capacity=256) as s:
        base = capi.memory_stats()
        assert L.sph_obstacle_set_pose(s.h, C.byref(pose())) == STATE
        assert L.sph_obstacle_set_pose(s.h, None) == STATE
        assert L.sph_obstacle_set_sensor(s.h, 1) == STATE
        assert L.sph_obstacle_get_load(s.h, None, None, None, None) == STATE
        assert s.obstacle_pose() is None and capi.memory_stats() == base
    with _ctx() as c:
        _install(c, sc, sensor=False)
        base = capi.memory_stats()
        before = c.obstacle_pose()
        nan, inf = float("nan"), float("inf")
        bad = [pose(pivot=(nan, 0, 0)), pose(omega=(0, inf, 0)), pose(quat=(1, nan, 0, 0)), pose(quat=(0, 0, 0, 0)),
               pose(quat=(-inf, 0, 0, 0)), pose(quat=(3e38, 3e38, 3e38, 3e38)), pose(quat=(1e-30, 0, 0, 0))]
        for k, p in enumerate(bad[:5]):
            assert L.sph_obstacle_set_pose(c.h, C.byref(p)) == INVALID, k
            after = c.obstacle_pose()
            assert all(np.array_equal(before[f].view(np.uint8), after[f].view(np.uint8)) for f in before), k
            assert capi.memory_stats() == base
        # finite in fp32 and in double: the squared norm 3.6e77 / 1e-60 is a double like any other, so these are poses
        for p in bad[5:]:
            assert L.sph_obstacle_set_pose(c.h, C.byref(p)) == 0
        assert abs(float(c.obstacle_pose()["quat"][0]) - 1.0) < 1e-15 and capi.memory_stats() == base


def test_a_life_cycle_with_the_sensor_returns_every_byte():
    base = capi.memory_stats()
    pos, vel = _dam()
    with _ctx() as c:
        created = capi.memory_stats()
        _install(c, SCENES["paddle"], sensor=False)
        built = capi.memory_stats()
        c.set_obstacle_sensor(True)
        waves = (N + 63) // 64
        sensed = capi.memory_stats()
        assert sensed[2] == built[2] + 3
        assert sensed[0] - built[0] == 48 * waves + 4 * (((waves + 3) & ~3) + 4) + 72
        c.set_obstacle_sensor(False); c.set_obstacle_sensor(True)          # allocated once
        assert capi.memory_stats() == sensed
        c.upload(pos, vel); c.step(DT, 2)
        c.clear_obstacle()
        assert capi.memory_stats()[0] == created[0] + (sensed[0] - built[0])     # the sensor's buffers stay until sph_destroy
    assert capi.memory_stats() == base


# ---- guarded allocations -----------------------------------------------------------------------------------------------------------
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


def _guarded_run(fill):
    sc = SCENES["paddle"]
    pos, vel = _dam()
    pts = np.random.default_rng(3).uniform(-2.1, -1.4, (1001, 3)).astype(F)
    with _guard(fill):
        with _ctx() as c:
            _install(c, sc)
            c.upload(pos, vel)
            c.step(DT, 1)
            r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
            fused = (c.download_owned(), c.obstacle_load())
            c.step_phased(DT, 1)
            r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
            phased = (c.download_owned(), c.obstacle_load())
            sample = c.sample_obstacle(pts)
            r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
    return fused, phased, sample


def test_guarded_posed_sensing_steps_write_inside_their_buffers_and_ignore_fresh_memory():
    runs = [_guarded_run(False), _guarded_run(True)]
    for (sa, la), (sb, lb) in zip(runs[0][:2], runs[1][:2]):
        for x, y in zip(sa, sb):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        for k in ("J", "L"):
            assert np.array_equal(_u64(la[k]), _u64(lb[k])) and np.abs(la[k]).max() > 0
        assert la["steps"] == lb["steps"]
        _same(la["about"], lb["about"])
    for x, y in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---- beside the tracked spheres and the mixed-precision pass ---------------------------------------------------------------------------
def _tracked(c):
    c.set_colliders([[-1.75, -1.72, -1.74]], [0.1875], [[300.0, -150.0, 80.0]])
    c.set_collider_bodies([F(50) * MASS], [[0.0, -1000.0, 0.0]])


def test_beside_a_tracked_sphere():
    pos, vel = _dam()
    with _ctx() as a, _ctx() as b:
        for c in (a, b):
            _tracked(c)
            c.upload(pos, vel)
        _install(a, SCENES["paddle"])
        a.step(DT, 1); b.step(DT, 1)
        ja, jb = a.collider_impulses(), b.collider_impulses()
        assert np.array_equal(_u64(ja[0]), _u64(jb[0])) and ja[1] == jb[1] == 1 and np.abs(ja[0]).max() > 0
        _check_pair(a, b, SCENES["paddle"])


def test_beside_the_mixed_precision_pass():
    st = _one_step(SCENES["paddle"], _fused, True, configure=lambda c: c.set_precision(True))
    assert st["touched"].sum() >= 100

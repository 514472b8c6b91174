"""GPU: free obstacle bodies (include/sph_hip.h: THE BODY; sph_obstacle_set_body, _get_body) against the numpy model of
tests/obstacle_body_model.py, BIT FOR BIT.  The scene is tests/test_gpu_obstacle_pose.py's paddle in its 3375-particle dam (a
partial last wave and mover tile, a local lattice).  The particles and the load of a step are checked by that file's method: a
twin context without an obstacle gives the integrate's output, and the pose model pushed on it with the state the body had
BEFORE the step must equal the body context; the state AFTER the step is the body model fed the device's J and L."""
import ctypes as C

import numpy as np
import pytest

import obstacle_body_model as bm
import obstacle_model as om
import obstacle_pose_model as pm
import test_gpu_obstacle_pose as tp
import test_gpu_render_solids as rs
import solid_render_cases as sc
import solid_render_model as so
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu
F = np.float32
DT = tp.DT
PADDLE = tp.SCENES["paddle"]
INVALID, STATE = -1, -5
MASS = tp.MASS

# The bodies of the paddle.  A kick needs `wn < 0`: a particle the solid has kicked leaves its face at 0.75 of the speed it came
# with, and at dt = 5e-7 and 3e4 particles per unit volume fresh ones arrive at less than one per step.  So a LIGHT body the fluid
# carries along is kicked for four or five steps and then hardly at all (measured: 184, 149, 155, 141, 21, 16, 10, 9, 2 for a
# hinge of moment 40).  These bodies are heavy -- the paddle's own volume holds some 400 particles of mass 65 -- and pushed hard
# enough by `accel` / `torque` that their faces gain a few hundred in speed per step and catch the particles lying on them
# again: the fluid's J and L stay in every step (measured, kicks per step: hinge 184, 33, 78, 121, 137, 144, 145, 156, 159;
# spin 184, 51, 74, 100, 113, 120, 129, 134, 141; free 184, 76, 139, 170, 187, 196, 196, 205, 206).
BODIES = {
    "hinge": dict(dof=bm.HINGE, inertia=(2000.0, 0.0, 0.0), axis=(0.2, -0.1, 3.0), torque=(0.0, 0.0, 6.0e12)),
    "spin": dict(dof=bm.SPIN, inertia=(1500.0, 4500.0, 3000.0), torque=(2.0e12, 0.0, 6.0e12)),
    "free": dict(dof=bm.FREE_XYZ, mass=30000.0, accel=(1.0e8, -6.0e8, -1.0e8), lo=(-0.5, -0.5, -0.5), hi=(0.5, 0.5, 0.5)),
}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _install(c, body, slot=0, scene=PADDLE):
    """the posed, sensing paddle in `slot`; body: keywords of ObstacleBody.make, or None for the kinematic slot"""
    c.select_obstacle(slot)
    tp._install(c, scene)
    if body is not None:
        c.set_obstacle_body(**body)
    c.select_obstacle(0)


def _fetch(c, slot=0):
    """the slot's state as the model holds it, and rot as the next launch takes it"""
    ob, ps = c.obstacle(slot=slot), c.obstacle_pose(slot=slot)
    return {"off": ob["offset"], "u": ob["velocity"], "pivot": ps["pivot"], "omega": ps["omega"], "q": ps["quat"]}, ps["rot"]


def _same_state(got, rot, want, what=""):
    for k in ("off", "u", "pivot", "omega"):
        assert np.array_equal(_u32(got[k]), _u32(want[k])), (what, k, got[k], want[k])
    assert np.array_equal(_u64(got["q"]), _u64(want["q"])), (what, "q", got["q"], want["q"])
    assert np.array_equal(_u32(rot), _u32(bm.rot_of(want))), (what, "rot")


def _everything(c, slot=0):
    """what two contexts that did the same must agree on, as arrays of bits"""
    p, v, i = c.download_owned()
    load = c.obstacle_load(slot=slot)
    st, rot = _fetch(c, slot)
    return {"pos": _u32(p), "vel": _u32(v), "index": i, "by_index": _u32(c.positions4()), "J": _u64(load["J"]), "L": _u64(load["L"]),
            "about": _u32(load["about"]), "steps": np.array([load["steps"]]), "rot": _u32(rot), "q": _u64(st["q"]),
            **{k: _u32(st[k]) for k in ("off", "u", "pivot", "omega")}}


def _agree(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


# ---- 1. dof = 0 is the kinematic slot moved to the device --------------------------------------------------------------------------
def _twelve_fused(c, install):
    install()
    c.step(DT, 12)


def _twelve_phased(c, install):
    install()
    c.step_phased(DT, 12)


def _mid_step(c, install):
    c.hash(); c.sort(); c.build_cells(); c.density()
    install()                                              # between sph_density and sph_force: this step's integrate uses it
    c.force(); c.collide(); c.integrate(DT)
    c.step(DT, 3)


STATIC = om.sphere((-1.62, -1.9, -1.6), 0.12)             # a second solid in the dam: slot 0 of the set


@pytest.mark.parametrize("slot", [0, 2], ids=["alone_in_slot_0", "slot_2_of_a_set"])
@pytest.mark.parametrize("stepper", [_twelve_fused, _twelve_phased, _mid_step], ids=["fused", "phased", "mid_step"])
def test_a_body_without_a_freedom_is_the_kinematic_slot(stepper, slot):
    pos, vel = tp._dam()
    out = []
    for body in (dict(dof=0), None):
        with tp._ctx() as c:
            c.upload(pos, vel)

            def install():
                if slot:
                    c.build_obstacle([tp._shape(STATIC)], tp.S)
                _install(c, body, slot)
            stepper(c, install)
            assert (c.obstacle_body(slot=slot) is not None) == (body is not None)
            out.append(_everything(c, slot))
    _agree(out[0], out[1])
    want, off = pm.advance(tp._pose_of(PADDLE), PADDLE["off"], PADDLE["u"], DT, int(out[1]["steps"][0]))
    assert np.array_equal(out[0]["q"], _u64(want["q"])) and np.array_equal(out[0]["off"], _u32(off))
    with tp._ctx() as c:                                   # (the premise: the paddle changed the run)
        c.upload(pos, vel)
        stepper(c, lambda: None)
        assert not np.array_equal(_u32(c.download_owned()[0]), out[0]["pos"])


# ---- 2. bodies the fluid drives, step by step against the models -------------------------------------------------------------------
def _model_step(a, twin, body, grid, phi):
    """One step of `a` (a body slot 0) checked against the twin and both models.  Returns the kicks of the step."""
    prev, _ = _fetch(a)
    pa, va, ia = a.download_owned()
    twin.upload(pa, va, index=ia)                          # the same particles in the same slots
    a.step(DT, 1)
    twin.step(DT, 1)
    pb, vb, ib = twin.download_owned()
    st = {}
    want_p, want_v, _ = pm.push(pb, vb, grid, phi, prev["off"], prev["u"], bm.pose_of(prev), tp.BMIN, tp.BMAX, tp.EPS, tp.DAMP, MASS,
                                stats=st)
    J, L = pm.load_in_order(st["lane"], st["kicked"], pb.shape[0])
    got_p, got_v, got_i = a.download_owned()
    load = a.obstacle_load()
    now, rot = _fetch(a)
    kicks = int(st["kicked"].sum())
    print("kicked", kicks, "J", load["J"], "L", load["L"], "u", now["u"], "omega", now["omega"])
    assert np.array_equal(got_i, ib)
    tp._same(got_p, want_p, "pos"); tp._same(got_v, want_v, "vel")
    tp._same(a.positions4()[got_i, :3], want_p, "positions by index")
    assert np.array_equal(_u64(load["J"]), _u64(J)) and np.array_equal(_u64(load["L"]), _u64(L)), (load, J, L)
    tp._same(load["about"], bm.world_pivot(prev))
    _same_state(now, rot, bm.step(prev, body, load["J"], load["L"], DT, tp.DAMP))
    return kicks


@pytest.mark.parametrize("name", list(BODIES))
def test_a_driven_body_step_by_step(name):
    body = bm.body(**BODIES[name])
    pos, vel = tp._dam()
    with tp._ctx() as a, tp._ctx() as twin, tp._ctx() as b:
        for c in (a, b):
            c.upload(pos, vel)
            _install(c, BODIES[name])
        ob = a.obstacle(read=True)
        grid = {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}
        start, rot = _fetch(a)
        _same_state(start, rot, bm.state(PADDLE["off"], PADDLE["u"], PADDLE["pivot"], PADDLE["quat"], PADDLE["omega"]), "as set")
        kicks = [_model_step(a, twin, body, grid, ob["phi"]) for _ in range(9)]
        assert min(kicks) >= 20, kicks                     # the run's premise: the fluid drives every step
        now, _ = _fetch(a)
        moved = {"hinge": "omega", "spin": "omega", "free": "u"}[name]
        assert not np.array_equal(now[moved], start[moved])
        if name == "hinge":                                # omega = (float)(s e): on the axis but for the roundings to fp32
            e = np.array(bm.unit_axis(body["axis"]))
            s = float(now["omega"][2]) / e[2]
            assert np.abs(now["omega"] - (s * e).astype(F)).max() <= np.abs(now["omega"]).max() * 2.0 ** -22
        b.step(DT, 1)
        b.step(DT, 8)                                      # eight steps in one call: no host in between
        _agree(_everything(a), _everything(b), "8 steps in one call")


# ---- 3. no particles: only the body step runs -- the float64 division and square root -----------------------------------------------
def _alone(body, scene, dt, calls, steps_per_call):
    model = bm.state(scene["off"], scene["u"], scene["pivot"], scene["quat"], scene["omega"])
    zero = np.zeros(3)
    trail = [model]
    with tp._ctx(64) as c:
        _install(c, body, scene=scene)
        for k in range(calls):
            c.step(dt, steps_per_call)
            for _ in range(steps_per_call):
                model = bm.step(model, bm.body(**body), zero, zero, dt, tp.DAMP)
                trail.append(model)
            got, rot = _fetch(c)
            _same_state(got, rot, model, k)
            load = c.obstacle_load()
            assert load["steps"] == (k + 1) * steps_per_call and not load["J"].any() and not load["L"].any()
    return trail


def test_a_body_under_gravity_reaches_its_bound_and_bounces():
    scene = dict(PADDLE, off=(0.0, 0.0, 0.0), u=(0.0, -1000.0, 0.0), omega=(0.0, 0.0, 0.0))
    body = dict(dof=bm.FREE_Y, mass=10.0, accel=(0.0, -107910.0, 0.0), lo=(0.0, -0.004, 0.0), hi=(0.0, 1.0, 0.0))
    trail = _alone(body, scene, DT, 6, 5)
    uy = np.array([s["u"][1] for s in trail])
    oy = np.array([s["off"][1] for s in trail])
    assert uy[0] < 0 and uy[-1] > 0 and (np.diff(np.sign(uy)) != 0).sum() == 1          # one bounce
    assert oy.min() < F(-0.004) and oy[-1] > F(-0.004)                                   # past the bound for one step, then back
    assert all(s["u"][0] == 0 and s["off"][2] == 0 for s in trail)                       # the other axes are not free


def test_a_torque_free_top_with_three_moments_tumbles():
    scene = dict(PADDLE, u=(0.0, 0.0, 0.0), omega=(3.0, 40.0, -5.0))
    body = dict(dof=bm.SPIN, inertia=(1.0, 2.0, 3.0))
    trail = _alone(body, scene, 1e-3, 4, 50)
    w = np.array([s["omega"] for s in trail], np.float64)
    assert len(trail) == 201
    assert np.abs(w - w[0]).max() > 5.0                                                  # omega wanders in the world: a tumble
    assert not np.array_equal(trail[-1]["q"], trail[0]["q"])


# ---- 4. views ----------------------------------------------------------------------------------------------------------------------
def test_the_pictures_and_the_sample_see_the_body_where_it_is():
    cam, solids, light, ambient = sc.SCENES["two_slots"]
    cam = cam()
    body = dict(dof=bm.HINGE | bm.FREE_X, mass=2.0, accel=(3.0e5, 0.0, 0.0), lo=(-1.0, 0.0, 0.0), hi=(1.0, 0.0, 0.0),
                inertia=(5.0, 0.0, 0.0), axis=(0.3, 1.0, 0.2), torque=(0.0, 2.0e7, 0.0))
    with rs._ctx(64) as c:
        c.upload(np.array([[-0.9, -0.9, -0.9], [-0.85, -0.9, -0.9]], F))
        rs._install(c, solids)
        c.set_obstacle_body(slot=1, **body)
        c.set_render_solids(rs._style(solids, light, ambient))
        before = rs._device_slots(c, solids)
        c.step(sc.DT, 5)
        slots = rs._device_slots(c, solids)                # (fetches the block: offset and pose as the next launch takes them)
        assert not np.array_equal(slots[1]["pose"]["q"], before[1]["pose"]["q"])
        assert not np.array_equal(slots[1]["off"], before[1]["off"])
        sol = so.march(cam, slots, light, ambient)
        old = so.march(cam, {**slots, 1: before[1]}, light, ambient)
        assert (sol.slot[sol.hit] == 1).sum() > 100 and not np.array_equal(sol.z, old.z)    # the motion is in the picture
        got, want, _ = rs._sprites(c, cam, sol)
        rs._same(got, want, "a body, sprites")
        got, want, _ = rs._surface(c, cam, sol)
        rs._same(got, want, "a body, surface")
        # the sample rule at world points
        st, _ = _fetch(c, 1)
        ob = c.obstacle(read=True, slot=1)
        lo = ob["origin"] + st["off"]
        pts = np.random.default_rng(5).uniform(lo - 0.2, lo + (np.array(ob["dims"]) - 1) * ob["spacing"] + 0.2, (1001, 3)).astype(F)
        got_phi, got_n, got_in = c.sample_obstacle(pts, slot=1)
        grid = {"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}
        want_phi, want_n, want_in, _ = pm.sample(grid, ob["phi"], st["off"], bm.pose_of(st), pts)
        assert 100 < want_in.sum() < 1001 and np.array_equal(got_in, want_in)
        tp._same(got_phi, want_phi); tp._same(got_n, want_n)


# ---- 5. refusals and lifetimes -----------------------------------------------------------------------------------------------------
def _raw(**kw):
    return capi.ObstacleBody.make(**kw)


def _params(c):
    """(has_body, the 80 bytes of sph_obstacle_get_body)"""
    has, b = C.c_int(), capi.ObstacleBody()
    assert c.L.sph_obstacle_get_body(c.h, C.byref(has), C.byref(b)) == 0
    return has.value, bytes(b)


def test_refusals_change_nothing_and_allocate_nothing():
    L = capi.load()
    nan, inf = float("nan"), float("inf")
    good = dict(dof=bm.FREE_XYZ | bm.SPIN, mass=5.0, inertia=(1.0, 2.0, 3.0), lo=(-1, -1, -1), hi=(1, 1, 1))
    bad = [dict(good, dof=32), dict(good, dof=bm.SPIN | bm.HINGE, axis=(0, 1, 0)), dict(good, mass=0.0), dict(good, mass=-1.0),
           dict(good, mass=nan), dict(good, mass=inf), dict(good, inertia=(1.0, 0.0, 3.0)), dict(good, inertia=(1.0, 2.0, nan)),
           dict(good, accel=(0, inf, 0)), dict(good, torque=(nan, 0, 0)), dict(good, lo=(-1, 2, -1)), dict(good, hi=(1, nan, 1)),
           dict(good, lo=(-inf, -1, -1)), dict(dof=bm.HINGE, inertia=(1.0, 0, 0), axis=(0, 0, 0)),
           dict(dof=bm.HINGE, inertia=(1.0, 0, 0), axis=(0, inf, 0)), dict(dof=bm.HINGE, inertia=(0.0, 1.0, 1.0), axis=(0, 1, 0))]
    with capi.Context(tp.N, params=capi.default_params(tp.BOX, tp.GRID), slab=(0, tp.GRID[2]), ghost_capacity=256) as s:
        base = capi.memory_stats()
        assert L.sph_obstacle_set_body(s.h, C.byref(_raw(**good))) == STATE
        assert L.sph_obstacle_set_body(s.h, None) == STATE
        assert capi.memory_stats() == base and s.obstacle_body() is None
    with tp._ctx() as c:
        tp._install(c, PADDLE, posed=False, sensor=False)
        base = capi.memory_stats()
        assert L.sph_obstacle_set_body(c.h, C.byref(_raw(**good))) == STATE            # no pose
        assert capi.memory_stats() == base and c.obstacle_body() is None
        c.set_obstacle_pose(PADDLE["pivot"], PADDLE["quat"], PADDLE["omega"])
        for k, kw in enumerate(bad):
            assert L.sph_obstacle_set_body(c.h, C.byref(_raw(**kw))) == INVALID, k
            assert capi.memory_stats() == base and c.obstacle_body() is None, k
        # fields the dof does not use are not looked at; 0 is a body
        assert L.sph_obstacle_set_body(c.h, C.byref(_raw(dof=0, mass=nan, inertia=(nan, 0, -1), lo=(1, 1, 1), hi=(0, 0, 0)))) == 0
        with_body = capi.memory_stats()
        waves = (tp.N + 63) // 64
        assert with_body[2] == base[2] + 4                                              # the sensor's three buffers and the block
        assert with_body[0] - base[0] == 48 * waves + 4 * (((waves + 3) & ~3) + 4) + 72 + 128
        before, rot = _fetch(c)
        params = _params(c)
        assert params[0] == 1
        for k, kw in enumerate(bad):                                                    # ... and on a slot that has a body
            assert L.sph_obstacle_set_body(c.h, C.byref(_raw(**kw))) == INVALID, k
            assert _params(c) == params, k
        assert L.sph_obstacle_set_sensor(c.h, 0) == STATE
        assert L.sph_obstacle_set_pose(c.h, None) == STATE
        assert L.sph_obstacle_set_sensor(c.h, 1) == 0
        now, rot2 = _fetch(c)
        _same_state(now, rot2, before); tp._same(rot, rot2)
        assert capi.memory_stats() == with_body


def test_clear_drops_the_body_and_another_grid_keeps_it():
    base = capi.memory_stats()
    pos, vel = tp._dam()
    with tp._ctx() as c:
        c.upload(pos, vel)
        _install(c, BODIES["hinge"])
        with_body = capi.memory_stats()
        c.step(DT, 2)
        st, rot = _fetch(c)
        c.build_obstacle([tp._shape(om.sphere((-1.7, -1.7, -1.7), 0.2))], tp.S)          # another grid: body and state stay
        got = c.obstacle_body()
        assert got is not None and got["dof"] == bm.HINGE and np.array_equal(got["axis"], np.array(BODIES["hinge"]["axis"], F))
        _same_state(*_fetch(c), st)
        c.step(DT, 1)
        assert not np.array_equal(_fetch(c)[0]["q"], st["q"])
        # dropped by the caller: kinematic from where it is, posed and sensing
        st, rot = _fetch(c)
        c.set_obstacle_body(None)
        assert c.obstacle_body() is None
        _same_state(*_fetch(c), st)
        c.step(DT, 1)
        want, off = pm.advance(bm.pose_of(st), st["off"], st["u"], DT)
        got, _ = _fetch(c)
        assert np.array_equal(_u64(got["q"]), _u64(want["q"])) and np.array_equal(_u32(got["off"]), _u32(off))
        tp._same(got["omega"], st["omega"])
        assert c.obstacle_load()["steps"] == 4
        c.set_obstacle_sensor(False)                                                     # (legal again)
        c.set_obstacle_body(**BODIES["spin"])
        c.clear_obstacle()
        assert c.obstacle_body() is None and c.obstacle_pose() is None and c.obstacle() is None
        assert capi.memory_stats()[2] == with_body[2] - 2                                 # the grid's two buffers left, nothing else
    assert capi.memory_stats() == base


def test_set_pose_and_set_motion_on_a_body_slot_reach_the_next_integrate():
    pos, vel = tp._dam()
    other = dict(pivot=(-1.72, -1.78, -1.76), quat=(0.8, -0.1, 0.5, 0.2), omega=(-900.0, 100.0, 2500.0))
    out = []
    for late in (True, False):
        with tp._ctx() as c:
            c.upload(pos, vel)
            scene = PADDLE if late else dict(PADDLE, off=(0.01, -0.03, 0.02), u=(-30.0, 10.0, 5.0), **other)
            _install(c, BODIES["free"], scene=scene)
            if late:                                       # written into the block on the stream
                c.set_obstacle_motion(offset=(0.01, -0.03, 0.02))
                c.set_obstacle_motion(velocity=(-30.0, 10.0, 5.0))
                c.set_obstacle_pose(other["pivot"], other["quat"], other["omega"])
            c.step(DT, 2)
            out.append(_everything(c))
    _agree(out[0], out[1])


# ---- 6. stages ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", range(4), ids=["loaded", "hashed", "sorted", "cells"])
def test_set_body_and_get_body_at_every_stage(stage):
    pos, vel = tp._dam()
    out = []
    for at in (stage, None):
        with tp._ctx() as c:
            c.upload(pos, vel)
            _install(c, BODIES["spin"] if at is None else None)
            phases = [c.hash, c.sort, c.build_cells]
            for k, phase in enumerate(phases + [None]):
                if k == at:
                    assert c.obstacle_body() is None
                    c.set_obstacle_body(**BODIES["spin"])
                    assert c.obstacle_body()["dof"] == bm.SPIN
                if phase:
                    phase()
            c.density(); c.force(); c.collide(); c.integrate(DT)
            c.step(DT, 1)
            out.append(_everything(c))
    _agree(out[0], out[1])
    assert out[0]["J"].any()


# ---- 7. guarded memory ----------------------------------------------------------------------------------------------------------------
def test_guarded_body_steps_and_pictures_write_inside_their_buffers():
    pos, vel = tp._dam()
    cam = capi.look_at(96, 64, eye=(-0.6, -1.2, -0.4), target=(-1.75, -1.75, -1.75))
    runs = []
    for fill in (False, True):
        with tp._guard(fill):
            with tp._ctx() as c:
                c.upload(pos, vel)
                c.build_obstacle([tp._shape(STATIC)], tp.S)
                _install(c, BODIES["spin"], slot=2)
                _install(c, BODIES["free"], slot=3, scene=dict(PADDLE, off=(0.1, 0.0, 0.05)))
                c.set_render_solids(capi.solid_defaults())
                c.step(DT, 2)
                r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
                c.step_phased(DT, 1)
                c.set_obstacle_motion(velocity=(1.0, 2.0, 3.0), slot=3)
                r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
                c.render(cam)
                image = c.read_image()
                c.render_surface(cam)
                surface = c.read_image()
                r = capi.guard_check(); assert r[0] > 0 and r[1] == 0, r
                runs.append((_everything(c, 2), _everything(c, 3), image, surface))
    _agree(runs[0][0], runs[1][0]); _agree(runs[0][1], runs[1][1])
    for x, y in zip(runs[0][2] + runs[0][3], runs[1][2] + runs[1][3]):
        assert np.array_equal(rs._bits(x), rs._bits(y))
    assert (runs[0][2][1] >= so.ID_SOLID).any()                                           # a solid is in the picture

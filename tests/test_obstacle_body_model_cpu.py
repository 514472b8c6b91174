"""CPU: the numpy model of a free obstacle body (tests/obstacle_body_model.py) against the models it stands on and against what
mechanics says of a hinge and of a symmetric top; the struct and the signatures of the two new calls; the premise of the GPU
tests' scene (tests/test_gpu_obstacle_body.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import obstacle_body_model as bm
import obstacle_model as om
import obstacle_pose_model as pm
from gpufluidsimulator_amd import capi, ic

F = np.float32
DT = float(ic.DEFAULT_DT)
SKEW = (0.9, 0.2, -0.3, 0.25)
RNG = np.random.default_rng(7)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_without_a_freedom_the_step_is_the_kinematic_advance():
    st = bm.state((0.03, -0.02, 0.04), (50.0, 0.0, -20.0), (-1.7, -1.8, -1.75), SKEW, (300.0, -200.0, 4000.0))
    # the load, the torque and every parameter a freedom would use are there and must not matter
    body = bm.body(dof=0, mass=3.0, inertia=(1.0, 2.0, 3.0), axis=(0.0, 1.0, 0.0), accel=(0.0, -1e5, 0.0), lo=(1.0, 1.0, 1.0))
    q, off = st["q"], st["off"]
    for k in range(25):
        st = bm.step(st, body, RNG.normal(0, 1e5, 3), RNG.normal(0, 1e4, 3), DT)
        q = pm.quat_step(q, (300.0, -200.0, 4000.0), DT)
        off = om.advance(off, (50.0, 0.0, -20.0), DT, 1)
        assert np.array_equal(_u64(st["q"]), _u64(q)) and np.array_equal(_u32(st["off"]), _u32(off)), k
        assert np.array_equal(st["omega"], np.array((300.0, -200.0, 4000.0), F)) and np.array_equal(st["u"], np.array((50.0, 0.0, -20.0), F))
    want, woff = pm.advance(pm.pose((-1.7, -1.8, -1.75), SKEW, (300.0, -200.0, 4000.0)), (0.03, -0.02, 0.04), (50.0, 0.0, -20.0), DT, 25)
    assert np.array_equal(_u64(st["q"]), _u64(want["q"])) and np.array_equal(_u32(st["off"]), _u32(woff))
    assert np.array_equal(_u32(bm.rot_of(st)), _u32(pm.rot_of(want["q"]))) and np.array_equal(bm.world_pivot(st), pm.world_pivot(want, woff))


def test_a_hinge_keeps_omega_on_its_axis():
    axis = (0.2, -0.1, 3.0)
    e = np.array(bm.unit_axis(axis))
    assert abs(float(e @ e) - 1.0) < 4e-16
    st = bm.state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.1, 0.2, 0.3), SKEW, (300.0, -200.0, 4000.0))
    body = bm.body(dof=bm.HINGE, inertia=(40.0, 0.0, 0.0), axis=axis, torque=(5e8, 0.0, -2e9))
    s_prev = float(np.array(st["omega"], np.float64) @ e)
    for k in range(40):
        L = RNG.normal(0, 1e4, 3)
        st = bm.step(st, body, np.zeros(3), L, DT)
        s = s_prev + float((L + DT * np.array(body["torque"], np.float64)) @ e) / 40.0      # the scalar equation of a hinge
        w = np.array(st["omega"], np.float64)
        assert np.abs(np.cross(w, e)).max() <= np.abs(w).max() * 2.0 ** -23, k                # parallel but for the fp32 roundings
        assert abs(float(w @ e) - s) <= abs(s) * 2.0 ** -22, k
        s_prev = float(w @ e)
        assert not st["u"].any() and not st["off"].any()
    assert abs(float(st["q"] @ st["q"]) - 1.0) < 1e-14


def test_a_torque_free_top_with_equal_moments_keeps_omega():
    omega = (3.0, 40.0, -5.0)
    st = bm.state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), SKEW, omega)
    body = bm.body(dof=bm.SPIN, inertia=(2.5, 2.5, 2.5))
    for k in range(300):
        st = bm.step(st, body, np.zeros(3), np.zeros(3), 1e-3)
        # R (R^T w) in float64 is w to a few parts in 1e16 and g is rounding noise: the fp32 omega does not move
        assert np.array_equal(_u32(st["omega"]), _u32(np.array(omega, F))), k
    assert not np.array_equal(st["q"], pm.quat_set(SKEW))
    # ... and with three different moments it does not keep it: the Euler term is there
    st = bm.state((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), SKEW, omega)
    w2 = lambda s: float(np.sum(np.array(s["omega"], np.float64) ** 2))
    tumble = bm.body(dof=bm.SPIN, inertia=(1.0, 2.0, 3.0))
    trail = [st]
    for k in range(200):
        trail.append(bm.step(trail[-1], tumble, np.zeros(3), np.zeros(3), 1e-3))
    w = np.array([s["omega"] for s in trail], np.float64)
    assert np.abs(w - w[0]).max() > 5.0
    # the angular momentum in the world, R I R^T w, is what a free top keeps: explicit Euler drifts, slowly
    def momentum(s):
        R = np.array(bm.rot_exact(s["q"]))
        return R @ (np.array([1.0, 2.0, 3.0]) * (R.T @ np.array(s["omega"], np.float64)))
    assert np.abs(momentum(trail[-1]) - momentum(trail[0])).max() < 0.05 * np.abs(momentum(trail[0])).max()
    assert w2(trail[-1]) > 0


def test_free_axes_take_the_impulse_gravity_and_the_wall_rule():
    st = bm.state((0.0, 0.0, 0.0), (1.0, -1000.0, 2.0), (0.0, 0.0, 0.0), (1, 0, 0, 0), (0.0, 0.0, 0.0))
    body = bm.body(dof=bm.FREE_Y, mass=10.0, accel=(5.0, -107910.0, 0.0), lo=(0.0, -0.004, 0.0), hi=(0.0, 1.0, 0.0))
    J = np.array([100.0, 30.0, -7.0])
    nxt = bm.step(st, body, J, np.zeros(3), DT)
    assert nxt["u"][0] == F(1.0) and nxt["u"][2] == F(2.0)                                    # not free: J and accel do not reach them
    assert nxt["u"][1] == F((-1000.0 + 30.0 / 10.0) + float(F(DT)) * float(F(-107910.0)))
    assert nxt["off"][1] == F(F(DT) * nxt["u"][1]) and nxt["off"][0] == F(F(DT) * F(1.0))
    for _ in range(30):
        st = bm.step(st, body, np.zeros(3), np.zeros(3), DT)
    assert st["u"][1] > 0 and st["off"][1] > F(-0.004)                                        # it has bounced: u *= wall_damping


def test_struct_and_signatures():
    assert C.sizeof(capi.ObstacleBody) == 80
    assert [f for f, _ in capi.ObstacleBody._fields_] == ["dof", "mass", "inertia", "axis", "accel", "torque", "lo", "hi"]
    assert capi.ObstacleBody.mass.offset == 4 and capi.ObstacleBody.lo.offset == 56 and capi.ObstacleBody.hi.offset == 68
    assert (capi.BODY_FREE_X, capi.BODY_FREE_Y, capi.BODY_FREE_Z, capi.BODY_SPIN, capi.BODY_HINGE) == (1, 2, 4, 8, 16)
    assert (bm.FREE_X, bm.FREE_Y, bm.FREE_Z, bm.SPIN, bm.HINGE) == (1, 2, 4, 8, 16)
    res, args = capi.SIGNATURES["sph_obstacle_set_body"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(capi.ObstacleBody)]
    res, args = capi.SIGNATURES["sph_obstacle_get_body"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(capi.ObstacleBody)]
    lib = capi.load()
    assert hasattr(lib, "sph_obstacle_set_body") and hasattr(lib, "sph_obstacle_get_body")
    b = capi.ObstacleBody.make(dof=capi.BODY_HINGE, inertia=(2.0, 0, 0), axis=(0, 0, 1), hi=(1, 2, 3))
    d = b.as_dict()
    assert d["dof"] == 16 and d["inertia"][0] == 2.0 and tuple(d["hi"]) == (1.0, 2.0, 3.0) and d["mass"] == 0.0


B, BALL, SPIN1 = "-benchmark", "sphere:0,0,0,0.2", "-solidspin=1:0,0,0,0,0,1"
BODY_FORM = "expected <k>:hinge,ax,ay,az,I[,tau] or <k>:float,mass,Ix,Iy,Iz[,gy], k = 0..3"
HEADLESS_CASES = [          # (arguments, exit status, a piece of the one line on stderr -- status 0: of stdout); none reaches a GPU call
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=hinge,0,0,1,5"], 1, "-solidbody=hinge,0,0,1,5: " + BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=4:hinge,0,0,1,5"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:wheel,0,0,1,5"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1,5,2,9"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1,5x"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:float,10,1,2"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:float,10,1,2,3,-9.8,7"], 1, BODY_FORM),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,0,5"], 1, "the axis must not be zero and I must be positive"),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,1,0,-5"], 1, "the axis must not be zero and I must be positive"),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:float,0,1,2,3"], 1, "the mass and the three moments must be positive"),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:float,10,1,-2,3"], 1, "the mass and the three moments must be positive"),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1,5", "-solidbody=1:float,10,1,2,3"], 1, "slot 1 already has a body"),
    ([B, "-solid=1:" + BALL, "-solidbody=1:hinge,0,0,1,5"], 1, "-solidbody=1:... goes with a -solid=1:... and a -solidspin=1:..."),
    ([B, SPIN1, "-solidbody=1:hinge,0,0,1,5"], 1, "goes with a -solid=1:..."),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=2:float,10,1,2,3"], 1, "-solidbody=2:... goes with a -solid=2:..."),
    ([B, "-gpus=2", "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1,5"], 1, "-solid is not supported with -gpus=2"),
    ([B, "-solid=1:" + BALL, SPIN1, "-solidbody=1:hinge,0,0,1,5,-3e4", "-solid=2:" + BALL, "-solidspin=2:0,0,0,0,0,0",
      "-solidbody=2:float,10,1,2,3,-9.8", "-solidhelp"], 0, "[-solidbody=<k>:hinge,<ax>,<ay>,<az>,<I>[,<tau>] | <k>:float,<mass>,<Ix>,<Iy>,<Iz>[,<gy>]]"),
    ([B, "-solidhelp"], 0, "-solidbody: the FLUID drives slot k"),
]


@pytest.fixture(scope="module")
def exe():
    from headless_cli_cases import EXE
    if not os.path.exists(EXE):
        from gpufluidsimulator_amd import build
        build.build()
    return EXE


@pytest.mark.parametrize("i", range(len(HEADLESS_CASES)))
def test_a_solidbody_option_answers_as_written_down(exe, i):
    """in the manner of tests/test_headless_solid_cli_cpu.py: the options are parsed once, before any GPU call"""
    args, status, piece = HEADLESS_CASES[i]
    out = subprocess.run([exe] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=60)
    assert out.returncode == status, (args, out.stderr)
    assert "gfx950" not in out.stderr, args
    if status:
        assert out.stdout == "" and len(out.stderr.splitlines()) == 1 and piece in out.stderr, (args, out.stderr)
    else:
        assert out.stderr == "" and piece in out.stdout, (args, out.stdout)


def test_premise_the_paddle_kicks_the_dam_as_uploaded():
    """tests/test_gpu_obstacle_body.py asserts at least 20 kicks in every step; here the scene as uploaded, by the pose model."""
    box, s = (4.0, 4.0, 4.0), 1.0 / 16.0
    pos, _ = ic.dam_break_lattice((15, 15, 15), box, jitter=True)
    vel = np.random.default_rng(41).normal(0, 100, pos.shape).astype(F)
    lo, hi = (-1.95, -2.1, -1.95), (-1.55, -1.4, -1.55)
    grid = om.lattice(s, lo, hi)
    phi = om.rasterise([om.box((-1.75, -1.75, -1.75), (0.25, 0.05, 0.12))], grid)
    ps = pm.pose((-1.7, -1.8, -1.75), SKEW, (300.0, -200.0, 4000.0))
    st = {}
    pm.push(pos, vel, grid, phi, (0.03, -0.02, 0.04), (50.0, 0.0, -20.0), ps, (-2.0,) * 3, (2.0,) * 3, stats=st)
    assert st["kicked"].sum() >= 20, st["kicked"].sum()

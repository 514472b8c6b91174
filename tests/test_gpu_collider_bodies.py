"""GPU: sphere colliders the fluid pushes back (include/sph_hip.h: sph_set_collider_bodies, sph_get_collider_impulses) -- the
impulse a tracked context reports against the momentum the fluid lost (a context with the sphere against one without) and
against the numpy model of tests/collider_body_model.py, tracking that changes no bit, the body update bit for bit, a ball
falling in an empty box, run-to-run identity, particle edits, the refusals, and the host class through the headless driver."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic
from collider_body_model import body_update, impulses
from collider_model import advance

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)          # cell edge 1/16; the 16^3 dam fills [-2, -1.5]^3
BMIN, BMAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
EPS, DAMP = F(1e-5), F(-0.75)
MASS = F(65.0)                                      # sph_default_params
E_INVALID, E_STATE = -1, -5
# the sphere of tests/test_gpu_colliders.py (three cells radius, inside the dam) and one out in the empty box
C0, R0, U0 = np.array([-1.75, -1.72, -1.74], F), F(0.1875), np.array([300.0, -150.0, 80.0], F)
C1, R1, U1 = np.array([1.0, 1.0, 1.0], F), F(0.25), np.array([0.0, 10.0, 0.0], F)


def _dam():
    return ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)


def _flowing():
    pos, vel = _dam()
    pos[:, 1] += F(0.5)
    vel[:, 0] = 300.0
    return pos, vel


def _ctx(n=4096):
    return capi.Context(n, box=BOX, grid=GRID)


def _ulp(a):
    return np.spacing(np.abs(a).astype(F)).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _code(fn, *args):
    with pytest.raises(capi.SphError) as e:
        fn(*args)
    return int(str(e.value).split("error ")[1].split(":")[0])


def _identity(a, b, centers, radii, vels, min_particles=100, min_waves=3):
    """a (tracked) and b (no sphere) have just taken ONE step from the same particles in the same slot order; centers are
    the ones that step pushed with.  J_0 of a = -m * sum (v_a - v_b) over the particles the model marks as touched and no
    wall moved, within m * sum (ulp(v_b) + ulp(term)): one rounding of the add, one of the product.  Returns what test 2
    needs."""
    J, _ = a.collider_impulses()
    pa, va, ia = a.download_owned()
    pb, vb, ib = b.download_owned()
    assert np.array_equal(ia, ib)
    Jm, terms, kicked, touched, walled = impulses(pb, vb, centers, radii, vels, MASS, BMIN, BMAX, EPS, DAMP)
    d = pb - np.asarray(centers[0], F)
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    rp2 = F(F(radii[0]) + EPS) ** 2
    tie = np.abs(r2.astype(np.float64) - rp2) <= 1e-6 * rp2
    assert tie.sum() <= 3, tie.sum()
    assert not (walled & kicked.any(axis=1)).any()           # (a wall pass behind a kick would change v_a - v_b)
    sel = touched & ~walled & ~tie
    # a tie the device decided its own way: whatever it did to that particle is in J (at most 3, usually none)
    odd = tie & (_bits(va) != _bits(vb)).any(axis=1)
    k = kicked[:, 0] & sel
    m = np.float64(MASS)
    want = -m * (va[sel | odd].astype(np.float64) - vb[sel | odd]).sum(axis=0)
    bound = m * (_ulp(vb[k]) + _ulp(terms[k, 0])).sum(axis=0)
    bound += m * (_ulp(vb[odd]) + _ulp(F(MASS) * (va[odd] - vb[odd]))).sum(axis=0)
    waves = np.unique(np.nonzero(k)[0] // 64)                # download_owned is in slot order: a wave is 64 slots
    print(f"J0 {J[0]} want {want} |diff| {np.abs(J[0] - want)} bound {bound} particles {k.sum()} waves {waves.size} ties {tie.sum()}")
    assert k.sum() >= min_particles and waves.size >= min_waves, (k.sum(), waves.size)
    assert (np.abs(J[0] - want) <= bound).all(), (J[0], want, bound)
    return J, Jm, k, va, vb, terms


def _one_step_pair(stepper, drop=0, small=None):
    pos, vel = _dam()
    if drop:
        pos, vel = pos[:-drop], vel[:-drop]
    with _ctx() as a, _ctx() as b:
        for c in (a, b):
            if small is not None:
                c.set_pair_small_launch(small)
            c.upload(pos, vel)
        a.set_colliders([C0, C1], [R0, R1], [U0, U1])
        a.set_collider_bodies([0.0, 0.0])
        stepper(a); stepper(b)
        out = _identity(a, b, [C0, C1], [R0, R1], [U0, U1])
        J, steps = a.collider_impulses()
        assert steps == 1
        assert np.array_equal(J[1], np.zeros(3)), J[1]      # the sphere in the empty box took exactly nothing
        assert np.abs(J[0]).max() > 0
        cen = a.colliders()
        assert np.array_equal(cen["centers"], np.stack([advance([C0], [U0], DT, 1)[0], advance([C1], [U1], DT, 1)[0]]))
    return out


@pytest.mark.parametrize("case", ["as_is", "blocks_of_256", "partial_last_wave"])
def test_the_impulse_is_the_momentum_taken(case):
    _one_step_pair(lambda c: c.step(DT, 1), drop=37 if case == "partial_last_wave" else 0,
                   small=0 if case == "blocks_of_256" else None)


def test_the_impulse_against_the_model():
    J, Jm, k, va, vb, terms = _one_step_pair(lambda c: c.step(DT, 1))
    vmax = float(np.abs(va).max())
    want_v = vb[k].astype(np.float64) - terms[k, 0].astype(np.float64) / np.float64(MASS)     # the model's new velocity
    bound = np.float64(MASS) * (1e-6 * vmax + _ulp(want_v)).sum(axis=0)
    print(f"J0 {J[0]} model {Jm[0]} |diff| {np.abs(J[0] - Jm[0])} bound {bound}")
    assert (np.abs(J[0] - Jm[0]) <= bound).all(), (J[0], Jm[0], bound)
    assert np.array_equal(Jm[1], np.zeros(3))


def test_the_phased_step_reports_the_same_identity():
    _one_step_pair(lambda c: c.step_phased(DT, 1))


def test_tracking_changes_no_bit_and_set_colliders_ends_it():
    pos, vel = _flowing()
    spheres = ([[-1.75, -1.2, -1.75], [0.0, 0.0, 0.0]], [0.2, 0.3], [[10.0, 0, 0], [0, 0, 0]])
    with _ctx() as a, _ctx() as b:
        a.set_colliders(*spheres); b.set_colliders(*spheres)
        a.set_collider_bodies([0.0, 0.0])
        a.upload(pos, vel); b.upload(pos, vel)
        a.step(DT, 50); b.step(DT, 50)
        J, steps = a.collider_impulses()
        assert steps == 50 and J.shape == (2, 3)
        assert b.collider_impulses()[0].shape == (0, 3) and b.collider_impulses()[1] == 0      # never tracked
        sa, sb = a.download(), b.download()
        for k in ("pos", "vel", "density", "pressure"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        ca, cb = a.colliders(), b.colliders()
        for k in ca:
            assert np.array_equal(_bits(ca[k]), _bits(cb[k])), k
        assert not np.array_equal(sa["pos"], pos)
        # sph_set_colliders drops the bodies: not tracked any more, and the by-value kernels run again
        a.set_colliders(ca["centers"], ca["radii"], ca["velocities"])
        J, steps = a.collider_impulses()
        assert J.shape == (0, 3) and steps == 0
        a.step(DT, 10); b.step(DT, 10)
        sa, sb = a.download(), b.download()
        for k in ("pos", "vel", "density", "pressure"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        assert np.array_equal(_bits(a.colliders()["centers"]), _bits(b.colliders()["centers"]))


def _free_body_step(mass, accel):
    pos, vel = _dam()
    with _ctx() as c:
        c.upload(pos, vel)
        c.set_colliders([C0], [R0], [U0])
        c.set_collider_bodies([mass], [accel])
        c.step(DT, 1)
        J, steps = c.collider_impulses()
        assert steps == 1
        return J[0], c.colliders()


def test_the_body_update_is_the_model_bit_for_bit():
    M = float(50 * MASS)
    g = (0.0, float(capi.default_params(BOX, GRID).gravity_y), 0.0)
    J, col = _free_body_step(M, g)
    assert np.abs(J).min() > 0
    c_want, u_want = body_update(C0, U0, J, M, g, R0, DT, BMIN, BMAX, DAMP)
    assert np.array_equal(_bits(col["velocities"][0]), _bits(u_want)), (col["velocities"][0], u_want)
    assert np.array_equal(_bits(col["centers"][0]), _bits(c_want)), (col["centers"][0], c_want)
    assert not np.array_equal(u_want, U0)
    # twice the mass, the same upload: the same J to the bit, half the velocity change to one fp32 ulp
    zero = (0.0, 0.0, 0.0)
    J1, col1 = _free_body_step(M, zero)
    J2, col2 = _free_body_step(2 * M, zero)
    assert np.array_equal(J1.view(np.uint64), J2.view(np.uint64)) and np.array_equal(J1.view(np.uint64), J.view(np.uint64))
    u1, u2 = col1["velocities"][0], col2["velocities"][0]
    d1, d2 = u1.astype(np.float64) - U0, u2.astype(np.float64) - U0
    assert (np.abs(d1) > 100 * _ulp(u1)).all()
    assert (np.abs(0.5 * d1 - d2) <= np.maximum(_ulp(u1), _ulp(u2))).all(), (d1, d2)


def test_a_free_body_falls_in_a_context_without_particles():
    R, dt, g, M = F(0.25), 1e-3, 8.0, 10.0
    c0, u0 = np.array([0.5, -2.0 + 0.25 + 0.05, -0.5], F), np.array([0.3, 0.0, -0.2], F)
    steps = 200
    with _ctx(64) as c:
        assert c.n == 0
        c.set_colliders([c0], [R], [u0])
        c.set_collider_bodies([M], [(0.0, -g, 0.0)])
        got = []
        for _ in range(steps):
            c.step(dt, 1)
            col = c.colliders()
            got.append((col["centers"][0].copy(), col["velocities"][0].copy()))
        J, n = c.collider_impulses()
        assert n == steps and not J.any()
    cc, uu, hit_step = c0, u0, None
    for s in range(steps):
        before = uu[1]
        cc, uu = body_update(cc, uu, np.zeros(3), M, (0.0, -g, 0.0), R, dt, BMIN, BMAX, DAMP)
        if hit_step is None and uu[1] > 0 > before:
            hit_step = s
            # the wall rule scaled the updated velocity by wall_damping and put the centre on box_min + R before the advance
            fell = F(np.float64(before) + np.float64(F(dt)) * np.float64(F(-g)))
            assert uu[1] == F(fell * DAMP) and cc[1] == F(F(F(-2.0) + R) + F(dt) * uu[1])
        assert np.array_equal(_bits(got[s][0]), _bits(cc)) and np.array_equal(_bits(got[s][1]), _bits(uu)), s
        assert (got[s][0] > -2.0).all() and (got[s][0] < 2.0).all()
    assert hit_step is not None and hit_step < steps - 1, hit_step


def _drop_a_ball():
    pos, vel = _dam()
    R, M = F(0.125), float(50 * MASS)
    c0, u0 = np.array([-1.75, -1.5 + 0.125 + 0.01, -1.75], F), np.array([0.0, -500.0, 0.0], F)
    g = (0.0, float(capi.default_params(BOX, GRID).gravity_y), 0.0)
    Js = []
    with _ctx() as c:
        c.upload(pos, vel)
        c.set_colliders([c0], [R], [u0])
        c.set_collider_bodies([M], [g])
        for chunk in range(10):
            c.step(DT, 19)
            used = c.colliders()["centers"][0].copy()        # the centre the chunk's last step pushes with
            c.step(DT, 1)
            Js.append(c.collider_impulses())
        st = c.download()
        col = c.colliders()
    return c0, R, Js, used, st, col


def test_a_dropped_ball_repeats_run_to_run():
    c0, R, Js, used, st, col = _drop_a_ball()
    _, _, Js2, used2, st2, col2 = _drop_a_ball()
    for (J, n), (J2, n2), want_n in zip(Js, Js2, range(20, 201, 20)):
        assert n == n2 == want_n and np.array_equal(J.view(np.uint64), J2.view(np.uint64))
    assert any(np.abs(J).max() > 0 for J, _ in Js)
    for k in col:
        assert np.array_equal(_bits(col[k]), _bits(col2[k])), k
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(_bits(st[k]), _bits(st2[k])), k
    assert np.isfinite(st["pos"]).all() and np.isfinite(st["vel"]).all()
    assert col["centers"][0][1] < c0[1]
    dist = np.linalg.norm(st["pos"].astype(np.float64) - used, axis=1)
    assert dist.min() >= F(R + EPS) - 1e-5 * 4.0, dist.min()


def test_the_identity_holds_after_remove_and_emit():
    pos, vel = _dam()
    with capi.Context(8192, box=BOX, grid=GRID) as a:
        a.upload(pos, vel)
        a.set_colliders([C0, C1], [R0, R1], [U0, U1])
        a.set_collider_bodies([0.0, 0.0])
        removed = a.remove([capi.Region.sphere((-2.0, -2.0, -2.0), 0.2)])      # the fluid in a corner of the box, away from sphere 0
        assert 0 < len(removed) < 1000
        for emit in (False, True):
            cen = a.colliders()
            if emit:
                # 100 particles into the middle of sphere 0 (which the first step emptied), each moving towards its centre
                # faster than the sphere moves: the sphere kicks every one of them, so the second step has test 1's coverage too
                gx, gy, gz = np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij")
                off = (np.stack([gx, gy, gz], axis=-1).reshape(-1, 3) * F(0.02) - F(0.043)).astype(F)      # none at the centre
                extra = (cen["centers"][0] + off).astype(F)
                a.emit(extra, (U0 - F(500.0) * off / np.linalg.norm(off, axis=1, keepdims=True)).astype(F))
            p, v, idx = a.download_owned()
            with capi.Context(8192, box=BOX, grid=GRID) as twin:            # the same particles in the same order, no sphere
                twin.upload(p, v, idx)
                a.step(DT, 1); twin.step(DT, 1)
                _identity(a, twin, cen["centers"], cen["radii"], cen["velocities"])
        assert a.collider_impulses()[1] == 2 and a.n == 4096 - len(removed) + 100


def test_refusals_change_nothing():
    pos, vel = _dam()
    M = float(50 * MASS)
    with capi.Context(4096, box=BOX, grid=GRID, slab=(0, 32), ghost_capacity=64) as s:
        s.set_colliders([C0], [R0], [U0])
        assert _code(s.set_collider_bodies, [M]) == E_STATE                # slab contexts: out of scope
        assert _code(s.set_collider_bodies, []) == E_STATE
    with _ctx() as c, _ctx() as twin:
        for x in (c, twin):
            x.upload(pos, vel)
            x.set_colliders([C0, C1], [R0, R1], [U0, U1])
        assert _code(c.set_collider_bodies, [M]) == E_INVALID              # on an untracked context: stays untracked
        assert c.collider_impulses() [1] == 0 and c.collider_impulses()[0].shape == (0, 3)
        for x in (c, twin):
            x.set_collider_bodies([M, 0.0], [(0.0, -1e5, 0.0), (0.0, 0.0, 0.0)])
            x.step(DT, 1)
        before, J_before = c.colliders(), c.collider_impulses()
        nan, inf = float("nan"), float("inf")
        zero = (0.0, 0.0, 0.0)
        assert _code(c.set_collider_bodies, [M]) == E_INVALID              # n off by one
        assert _code(c.set_collider_bodies, [M, M, M]) == E_INVALID
        for bad in (-1.0, inf, nan):
            assert _code(c.set_collider_bodies, [M, bad]) == E_INVALID
        assert _code(c.set_collider_bodies, [M, M], [zero, (0.0, nan, 0.0)]) == E_INVALID
        assert _code(c.set_collider_bodies, [M, M], [(inf, 0.0, 0.0), zero]) == E_INVALID
        after, J_after = c.colliders(), c.collider_impulses()
        for k in before:
            assert np.array_equal(_bits(before[k]), _bits(after[k])), k
        assert J_after[1] == J_before[1] == 1 and np.array_equal(J_after[0].view(np.uint64), J_before[0].view(np.uint64))
        c.step(DT, 1); twin.step(DT, 1)
        sa, sb = c.download(), twin.download()
        for k in ("pos", "vel", "density", "pressure"):
            assert np.array_equal(_bits(sa[k]), _bits(sb[k])), k
        ca, cb = c.colliders(), twin.colliders()
        for k in ca:
            assert np.array_equal(_bits(ca[k]), _bits(cb[k])), k
        assert np.array_equal(c.collider_impulses()[0].view(np.uint64), twin.collider_impulses()[0].view(np.uint64))
        # an empty list stops the tracking and leaves the spheres where the device had them
        c.set_collider_bodies([])
        assert c.collider_impulses()[1] == 0
        for k in ca:
            assert np.array_equal(_bits(c.colliders()[k]), _bits(ca[k])), k


@pytest.mark.parametrize("M", [3250.0, 0.0])          # a free body; a kinematic sphere read as a sensor
def test_headless_driver_free_body_equals_c_abi_path(M):
    c0, R, u = (-1.75, -1.4, -1.75), 0.125, (0.0, -400.0, 100.0)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "state.bin")
        arg = "-collider=" + ",".join(repr(float(v)) for v in (*c0, R, *u))
        out = subprocess.run([EXE, "-benchmark", "-n=4096", "-box=4", "-i=5", "-nowarmup", arg, f"-collidermass={M!r}", f"-out={f}"],
                             check=True, capture_output=True, text=True, timeout=300)
        raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("collider: ")]
    assert len(line) == 1, out.stdout
    m = re.fullmatch(r"collider: centre (\S+) (\S+) (\S+) velocity (\S+) (\S+) (\S+) impulse (\S+) (\S+) (\S+)", line[0])
    vals = [float(v) for v in m.groups()]
    pos, vel = _dam()
    with _ctx() as c:
        c.upload(pos, vel)
        c.set_colliders([c0], [R], [u])
        c.set_collider_bodies([M], [(0.0, float(c.params.gravity_y), 0.0)])       # the driver's default acceleration
        c.step(DT, 5)
        st, col, (J, steps) = c.download(), c.colliders(), c.collider_impulses()
    assert np.array_equal(np.array(vals[0:3], F), col["centers"][0]) and np.array_equal(np.array(vals[3:6], F), col["velocities"][0])
    assert np.array_equal(np.array(vals[6:9]), J[0])
    assert steps == 5 and np.abs(J[0]).max() > 0
    assert np.array_equal(col["velocities"][0], np.array(u, F)) == (M == 0.0)      # the fluid moved the body, not the obstacle
    assert np.array_equal(_bits(raw[0, :, :3]), _bits(st["pos"]))
    assert np.array_equal(_bits(raw[1, :, :3]), _bits(st["vel"]))

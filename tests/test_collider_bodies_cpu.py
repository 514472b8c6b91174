"""CPU: the numpy model of the tracked sphere colliders (tests/collider_body_model.py, include/sph_hip.h:
sph_set_collider_bodies) -- the impulse is the momentum the fluid lost, the body update, the sum of the terms in the
device's order (impulse_sum_in_order, run_length), and the headless driver's -collidermass flag in its help text."""
import os
import subprocess

import numpy as np
import pytest

from collider_body_model import body_update, impulse_sum_in_order, impulses, run_length, terms_one, thread_sums
from collider_model import advance, push, push_one

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
BMIN, BMAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
MASS = F(65.0)


def _ulp(a):
    return np.spacing(np.abs(np.asarray(a, F))).astype(np.float64)


def test_the_impulse_is_minus_the_momentum_change_of_the_fluid():
    rng = np.random.default_rng(11)
    pos = rng.uniform(-0.4, 0.4, (4000, 3)).astype(F)
    vel = rng.normal(0, 50, (4000, 3)).astype(F)
    c, R, u = [[0.05, -0.02, 0.1]], [0.3], [[30.0, -10.0, 5.0]]            # one sphere, far from every wall
    J, terms, kicked, touched, walled = impulses(pos, vel, c, R, u, MASS, BMIN, BMAX)
    p2, v2, t2 = push(pos, vel, c, R, u, BMIN, BMAX)
    assert np.array_equal(t2, touched) and not walled.any()
    assert kicked[:, 0].sum() >= 100 and (touched & ~kicked[:, 0]).sum() >= 100       # approaching and leaving particles
    k = kicked[:, 0]
    assert not terms[~k].any()
    dp = -(MASS.astype(np.float64) * (v2[k].astype(np.float64) - vel[k]).sum(axis=0))
    # v + k*nrm is rounded once (half an ulp of the new velocity), the product mass * (k*nrm) once
    bound = (MASS.astype(np.float64) * 0.5 * _ulp(v2[k]) + 0.5 * _ulp(terms[k, 0])).sum(axis=0)
    assert (np.abs(J[0] - dp) <= bound).all(), (J[0], dp, bound)
    assert np.abs(J[0]).max() > 1e3 * bound.max()


def test_terms_one_is_push_one_with_the_terms():
    rng = np.random.default_rng(5)
    centers, radii = np.array([[0.0, -1.9, 0.0], [0.15, -1.9, 0.0]], F), np.array([0.2, 0.2], F)       # overlapping, at the floor
    vels = np.array([[1.0, 0, 0], [0, 3.0, -1.0]], F)
    walled_seen = 0
    for _ in range(300):
        x = (centers[0] + rng.uniform(-0.3, 0.3, 3)).astype(F)
        x[1] = max(x[1], F(-1.999))
        v = rng.normal(0, 10, 3).astype(F)
        xa, va, hit = push_one(x, v, centers, radii, vels, BMIN, BMAX)
        xb, vb, terms, kicked, hit_b, walled = terms_one(x, v, centers, radii, vels, MASS, BMIN, BMAX)
        assert hit == hit_b and np.array_equal(xa, xb) and np.array_equal(va, vb)
        assert not terms[~kicked].any()
        walled_seen += walled
    assert walled_seen > 0


def test_twice_the_mass_takes_half_the_velocity_change():
    J = np.array([1234.5, -987.25, 55.125])
    c, u = np.array([0.1, 0.2, 0.3], F), np.array([3.0, -2.0, 1.0], F)
    zero = (0.0, 0.0, 0.0)
    _, u1 = body_update(c, u, J, 3250.0, zero, 0.1, 5e-7, BMIN, BMAX)
    _, u2 = body_update(c, u, J, 6500.0, zero, 0.1, 5e-7, BMIN, BMAX)
    d1, d2 = u1.astype(np.float64) - u, u2.astype(np.float64) - u
    assert (np.abs(d1 - 2.0 * d2) <= _ulp(u1) + 2.0 * _ulp(u2)).all(), (d1, d2)
    assert (np.abs(d1 - J / 3250.0) <= _ulp(u1)).all()          # one rounding of the new velocity
    # a constant acceleration enters as dt * accel
    _, ug = body_update(c, u, np.zeros(3), 1.0, (0.0, -1000.0, 0.0), 0.1, 1e-3, BMIN, BMAX)
    assert ug[1] == F(np.float64(u[1]) + np.float64(F(1e-3)) * np.float64(-1000.0)) and ug[0] == u[0] and ug[2] == u[2]


def test_the_wall_rule_holds_a_body_in_the_box():
    R, dt, damp = F(0.25), F(1e-3), F(-0.75)
    c, u = np.array([0.0, -1.7, 0.0], F), np.zeros(3, F)
    hits, low = 0, 10.0
    for _ in range(400):
        before = u[1]
        c, u = body_update(c, u, np.zeros(3), 100.0, (0.0, -2000.0, 0.0), R, dt, BMIN, BMAX, damp)
        if u[1] > 0 and before < 0:
            hits += 1
        low = min(low, float(c[1]))
        assert BMIN[1] < c[1] < BMAX[1]
        # the wall rule leaves the centre at box_min + R at the latest one step after it dipped below
        assert c[1] >= F(-2.0) + R - dt * abs(float(u[1])) - 1e-6
    assert hits >= 2 and low < -1.74


def test_mass_zero_reproduces_advance():
    c, u = np.array([0.0, 0.1, 0.2], F), np.array([3.0, 0.0, -7.0], F)
    cur_c, cur_u = c, u
    for _ in range(5):
        cur_c, cur_u = body_update(cur_c, cur_u, np.array([1e6, 1e6, 1e6]), 0.0, (0.0, -9.0, 0.0), 0.1, 5e-7, BMIN, BMAX)
    assert np.array_equal(cur_u, u)
    assert np.array_equal(cur_c, advance([c], [u], 5e-7, 5)[0])


def _synthetic(n, nsph, seed, every=5):
    """Terms that are small integers times 2^-10 on every `every`-th slot and sphere (j + slot) % 3 == 0: any float64 sum
    of them is exact, whatever its order."""
    rng = np.random.default_rng(seed)
    terms = (rng.integers(-1000, 1001, (n, nsph, 3)) * 2.0 ** -10).astype(F)
    kicked = np.zeros((n, nsph), bool)
    for j in range(nsph):
        kicked[(np.arange(n) + j) % every == 0, j] = True
    kicked[:, nsph - 1] = False                              # a sphere that kicks nothing
    terms[~kicked] = 0
    return terms, kicked


@pytest.mark.parametrize("n", [37, 64, 4096 + 37, 65536, 65573, 131100])
def test_the_ordered_sum_of_exact_terms_is_the_plain_sum(n):
    terms, kicked = _synthetic(n, 8, n)
    J = impulse_sum_in_order(terms, kicked, n)
    want = terms.astype(np.float64).sum(axis=0)
    assert J.shape == (8, 3) and J.dtype == np.float64
    assert np.array_equal(J.view(np.uint64), want.view(np.uint64))
    assert np.abs(J[:7]).min() > 0 and not J[7].any() and not np.signbit(J[7]).any()
    assert np.array_equal(impulse_sum_in_order(terms, kicked, n, runs_descending=True), J)
    # a term of a lane that was not kicked is not part of the sum
    terms[~kicked] = 7.0
    assert np.array_equal(impulse_sum_in_order(terms, kicked, n), J)


def test_the_order_of_the_runs_can_be_seen_in_the_bits():
    n = 65573
    rng = np.random.default_rng(3)
    mag = 2.0 ** rng.uniform(-20, 20, (n, 1, 3))             # 2^40 between the smallest and the largest: well past 2^30
    terms = (mag * rng.choice([-1.0, 1.0], (n, 1, 3))).astype(F)
    kicked = np.zeros((n, 1), bool)
    kicked[::7] = True
    up = impulse_sum_in_order(terms, kicked, n)
    down = impulse_sum_in_order(terms, kicked, n, runs_descending=True)
    assert (up.view(np.uint64) != down.view(np.uint64)).any(), (up, down)
    assert np.allclose(up, down, rtol=1e-9, atol=0)          # (the same sum, to rounding)
    plain = np.array([sum(float(x) for x in terms[kicked[:, 0], 0, a]) for a in range(3)])     # one running sum, slot by slot
    assert np.allclose(up[0], plain, rtol=1e-9, atol=0)


def test_run_length():
    assert [run_length(n) for n in (64, 65536, 65537, 131100)] == [4, 4, 8, 12]
    assert [run_length(n) for n in (1, 63, 4096, 65573, 131072, 131073, 196608, 196609)] == [4, 4, 4, 8, 8, 12, 12, 16]


def test_a_run_that_starts_beyond_the_waves_contributes_nothing():
    n = 65573                                                # 1,025 waves, K = 8: threads 0..128 own waves, 129..255 none
    terms, kicked = _synthetic(n, 2, 1, every=1)
    kicked[:, 1] = kicked[:, 0]
    acc, found = thread_sums(terms, kicked, n)
    assert found[:129].all() and not found[129:].any() and not acc[129:].any()
    # thread 128 holds the one short wave of 37 lanes, lane by lane
    last = np.zeros(3)
    for i in range(1024 * 64, n):
        last = last + terms[i, 0].astype(np.float64)
    assert np.array_equal(acc[128, 0], last)
    # the last run short, not empty: 131,100 slots are 2,049 waves, K = 12, thread 170 owns the 9 waves 2040..2048
    n = 131100
    kicked = np.zeros((n, 1), bool)
    kicked[[0, 2039 * 64 + 63, 2040 * 64, n - 1]] = True
    terms = np.zeros((n, 1, 3), F)
    terms[kicked[:, 0]] = [[[1, 2, 3]], [[10, 20, 30]], [[100, 200, 300]], [[1000, 2000, 3000]]]
    acc, found = thread_sums(terms, kicked, n)
    assert list(np.nonzero(found)[0]) == [0, 169, 170]
    assert np.array_equal(acc[170, 0], [1100, 2200, 3300]) and np.array_equal(acc[169, 0], [10, 20, 30])
    assert np.array_equal(impulse_sum_in_order(terms, kicked, n)[0], [1111, 2222, 3333])


def test_headless_help_names_the_collidermass_flag():
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    out = subprocess.run([EXE, "-help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "-collidermass=" in out.stdout


@pytest.mark.parametrize("args", [["-collidermass=5"], ["-collider=0,0,0,0.1", "-collidermass=-1"],
                                  ["-collider=0,0,0,0.1", "-collidermass=1,2"]])
def test_headless_refuses_a_malformed_collidermass(args):
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    out = subprocess.run([EXE, "-benchmark"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "-collidermass" in out.stderr

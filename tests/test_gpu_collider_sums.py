"""GPU: tracked sphere colliders held to their word (include/sph_hip.h: sph_set_colliders, sph_set_collider_bodies) -- every
particle bit for bit against the numpy model of tests/collider_body_model.py, and J bit for bit against the sum in the
device's order (impulse_sum_in_order), with eight spheres (overlapping ones, a free body) at the smallest sizes at which the
summing block (csrc/sph_pairs.hip: k_spheres_step) takes each of its paths:

    n        waves   K
    65,536   1,024   4    all 256 runs full; rows found in all four waves of the summing block
    65,573   1,025   8    the last run is one wave of 37 lanes; threads 129..255 start beyond the waves
    131,100  2,049   12   K no power of two; the last run short; 1,025 workgroups of 128 threads

The pattern: context A is tracked, its twin B has no spheres; both take the same step from the same upload; the model applied
to B's download_owned output is A's, every particle, no tolerance.  Every test prints its wave count and K, the found threads
per 64-thread group of the summing block, the kicked count per sphere and the number of doubly kicked particles."""
import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic
from collider_body_model import body_update, impulse_sum_in_order, push_with_terms, run_length, terms_one
from collider_model import advance

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)          # cell edge 1/16, lattice spacing 1/32: the dam starts in the corner (-2, -2, -2)
BMIN, BMAX = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
EPS, DAMP = F(1e-5), F(-0.75)
MASS = F(65.0)                                      # sph_default_params
# the lattice each size is cut from (index = x + nx (y + ny z), slots are z-major): 65,573 and 131,100 end in a few particles
# of a 33rd z layer, which are alone in their cell layer and so the last slots of all
LATTICE = {65536: (64, 32, 32), 65573: (64, 32, 33), 131100: (64, 64, 33)}
GROUPS = {65536: (0, 1, 2, 3), 65573: (0, 1, 2), 131100: (0, 1, 2)}       # 64-thread groups of the summing block that own a wave
BODY = 4                                            # the sphere that is a free body


def _fluid(n):
    return ic.dam_break_lattice(LATTICE[n], BOX, jitter=True, count=n)


def _spheres(n, stage=0):
    """Eight spheres of about two cells radius whose velocities point into the fluid, spread over the dam's z extent
    [-2, -1]; 0, 1 and 2 overlap each other inside the fluid, within one wave's stretch of cells along x, and 1 drives into
    the particles 0 has just kicked; sphere 4 is a free body; sphere 7 sits on the top z layer over the last slots, and no
    other sphere lifts a particle into that cell layer, whose particles a later sort would put behind them.  Stage 1 and 2
    are the same set moved along x to fluid that the stage before has not touched."""
    top = ([-0.25, -1.06, -1.0], [0.0, -200.0, -300.0]) if n == 65536 else ([-1.8, -1.88, -0.96], [0.0, -100.0, -400.0])
    centers = np.array([[-1.36, -1.60, -1.85], [-1.24, -1.60, -1.85], [-1.30, -1.50, -1.85], [-1.15, -1.50, -1.62],
                        [-1.20, -1.30, -1.40], [-1.70, -1.70, -1.30], [-1.75, -1.40, -1.15], top[0]], F)
    centers[:7, 0] += F(0.5 * stage)
    centers[7, 0] += F(0.4 * stage)
    radii = np.array([0.125, 0.125, 0.12, 0.13, 0.125, 0.12, 0.125, 0.14], F)
    vels = np.array([[300.0, 0.0, 0.0], [-500.0, 0.0, 0.0], [0.0, 400.0, 50.0], [0.0, 200.0, 300.0], [-250.0, 100.0, 0.0],
                     [100.0, 100.0, -300.0], [0.0, -300.0, 100.0], top[1]], F)
    masses = np.zeros(8, F)
    masses[BODY] = F(50) * MASS
    accels = np.zeros((8, 3), F)
    accels[BODY, 1] = capi.default_params(BOX, GRID).gravity_y
    return centers, radii, vels, masses, accels


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _coverage(kicked, n, label):
    """What the inputs reach, from the model's `kicked` (n, nsph) in slot order; printed for the log."""
    n_waves, K = (n + 63) // 64, run_length(n)
    waves = np.nonzero(kicked.any(axis=1))[0] // 64
    per_wave = np.zeros((n_waves, kicked.shape[1]), bool)
    for j in range(kicked.shape[1]):
        per_wave[np.nonzero(kicked[:, j])[0] // 64, j] = True
    found = np.unique(waves // K)
    cov = {"waves": n_waves, "K": K, "found_per_group": [int(((found >> 6) == g).sum()) for g in range(4)],
           "kicked_per_sphere": [int(v) for v in kicked.sum(axis=0)], "doubly_kicked": int((kicked.sum(axis=1) >= 2).sum()),
           "most_spheres_in_a_wave": int(per_wave.sum(axis=1).max()), "last_wave_kicked": bool(per_wave[n_waves - 1].any()),
           "kicked_waves": int(np.unique(waves).size)}
    print(f"{label}: n {n} " + " ".join(f"{k} {v}" for k, v in cov.items()))
    return cov


def _assert_coverage(cov, groups):
    assert min(cov["kicked_per_sphere"]) >= 50, cov                # every mask bit 0..7
    assert cov["most_spheres_in_a_wave"] >= 3, cov
    assert cov["doubly_kicked"] >= 1, cov
    assert all((cov["found_per_group"][g] > 0) == (g in groups) for g in range(4)), cov
    assert cov["last_wave_kicked"], cov                            # the wave that ends the last run that holds any


def _check_step(a, b, spheres, dt, label, premise=None):
    """a (tracked) and b (no spheres) have just taken ONE step of dt from the same particles; `spheres` is what that step
    pushed with (centers, radii, velocities, masses, accels).  Every particle, J, and the spheres after the step, bit for
    bit against the model applied to b's output.  `premise`, if given, is called with the model's terms, kicked and n before
    the device's J is looked at.  Returns the coverage and the model's terms and kicked."""
    centers, radii, vels, masses, accels = spheres
    pa, va, ia = a.download_owned()
    pb, vb, ib = b.download_owned()
    n = pb.shape[0]
    assert a.n == b.n == n and np.array_equal(ia, ib)
    want_p, want_v, terms, kicked, touched = push_with_terms(pb, vb, centers, radii, vels, MASS, BMIN, BMAX, EPS, DAMP)
    cov = _coverage(kicked, n, label)
    bad = np.nonzero((_u32(pa) != _u32(want_p)).any(axis=1) | (_u32(va) != _u32(want_v)).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:4], pb[bad[:4]], vb[bad[:4]], pa[bad[:4]], want_p[bad[:4]], va[bad[:4]], want_v[bad[:4]])
    assert touched.sum() >= kicked.any(axis=1).sum() and not np.array_equal(pa, pb)
    if premise is not None:
        premise(terms, kicked, n)
    J, _ = a.collider_impulses()
    Jm = impulse_sum_in_order(terms, kicked, n)
    assert J.shape == Jm.shape and np.array_equal(_u64(J), _u64(Jm)), (J, Jm, J - Jm)
    col = a.colliders()
    for j in range(centers.shape[0]):
        if masses[j] > 0:
            c_want, u_want = body_update(centers[j], vels[j], Jm[j], masses[j], accels[j], radii[j], dt, BMIN, BMAX, DAMP)
            assert not np.array_equal(u_want, vels[j])
        else:
            c_want, u_want = advance([centers[j]], [vels[j]], dt, 1)[0], vels[j]
        assert np.array_equal(_u32(col["centers"][j]), _u32(c_want)), (j, col["centers"][j], c_want)
        assert np.array_equal(_u32(col["velocities"][j]), _u32(u_want)), (j, col["velocities"][j], u_want)
    assert np.array_equal(_u32(col["radii"]), _u32(radii))
    return cov, terms, kicked


def _track(c, spheres):
    centers, radii, vels, masses, accels = spheres
    c.set_colliders(centers, radii, vels)
    c.set_collider_bodies(masses, accels)


def _one_step(n, stepper, label):
    pos, vel = _fluid(n)
    spheres = _spheres(n)
    with capi.Context(n, box=BOX, grid=GRID) as a, capi.Context(n, box=BOX, grid=GRID) as b:
        a.upload(pos, vel); b.upload(pos, vel)
        _track(a, spheres)
        stepper(a); stepper(b)
        cov, _, _ = _check_step(a, b, spheres, DT, label)
        assert a.collider_impulses()[1] == 1
    assert (cov["waves"], cov["K"]) == {65536: (1024, 4), 65573: (1025, 8), 131100: (2049, 12)}[n]
    _assert_coverage(cov, GROUPS[n])


@pytest.mark.parametrize("n", [65536, 65573, 131100])
def test_fused_step_bits_and_ordered_sum(n):
    _one_step(n, lambda c: c.step(DT, 1), f"fused {n}")


@pytest.mark.parametrize("n", [65573, 131100])
def test_phased_step_bits_and_ordered_sum(n):
    _one_step(n, lambda c: c.step_phased(DT, 1), f"phased {n}")


OBS_DT = 1e-9                # the step of the observable-order case: dt * v stays below a cell up to v = 6e7


def _observable_case():
    """65,573 particles, three resting spheres of three cells radius apart from each other, and in each a shell of
    particles moving towards the centre at speeds log-spread from 1e-2 to 5e7 (dt * v <= 0.05 < 1/16 at OBS_DT)."""
    n = 65573
    pos, vel = _fluid(n)
    centers = np.array([[-1.0, -1.5, -1.5], [-1.5, -1.45, -1.7], [-0.5, -1.5, -1.25]], F)
    radii = np.full(3, 0.1875, F)
    rng = np.random.default_rng(7)
    in_shell = 0
    for c in centers:
        d = pos.astype(np.float64) - c
        r = np.linalg.norm(d, axis=1)
        shell = (r > 0.1) & (r < 0.18)
        speed = 10.0 ** rng.uniform(-2.0, np.log10(5e7), int(shell.sum()))
        vel[shell] = (-speed[:, None] * d[shell] / r[shell, None]).astype(F)
        in_shell += int(shell.sum())
    assert in_shell >= 1200 and float(np.abs(vel).max()) * OBS_DT <= 0.05
    return n, pos, vel, (centers, radii, np.zeros((3, 3), F), np.zeros(3, F), np.zeros((3, 3), F))


def test_the_order_of_the_sum_is_observable():
    """Without this case the float64 sum of the fp32 terms is usually exact and no order could show.  Here the terms spread
    over nine decades: the largest sums reach 2^36, where a float64 keeps nothing below 2^-16, and a 24-bit term below 2^7 --
    a normal speed below about 1 -- has bits there, so nearly every addition of two runs' sums rounds.  The premise -- the
    model's sum with the runs in descending order differs from the documented order in some bit -- is asserted first, on the
    model alone; the device gives the documented order."""
    n, pos, vel, spheres = _observable_case()

    def premise(terms, kicked, n):
        up, down = impulse_sum_in_order(terms, kicked, n), impulse_sum_in_order(terms, kicked, n, runs_descending=True)
        print(f"components whose bits differ between ascending and descending runs: {int((_u64(up) != _u64(down)).sum())} of 9")
        assert (_u64(up) != _u64(down)).any(), (up, down)        # on these terms the order shows

    with capi.Context(n, box=BOX, grid=GRID) as a, capi.Context(n, box=BOX, grid=GRID) as b:
        a.upload(pos, vel); b.upload(pos, vel)
        _track(a, spheres)
        a.step(OBS_DT, 1); b.step(OBS_DT, 1)
        cov, terms, kicked = _check_step(a, b, spheres, OBS_DT, "observable order", premise)
        J, _ = a.collider_impulses()
    mags = np.abs(terms[kicked])
    print(f"found threads {sum(cov['found_per_group'])} |term| {mags[mags > 0].min()} .. {mags.max()}")
    assert min(cov["kicked_per_sphere"]) >= 300 and cov["K"] == 8 and sum(cov["found_per_group"]) >= 16, cov
    up, down = impulse_sum_in_order(terms, kicked, n), impulse_sum_in_order(terms, kicked, n, runs_descending=True)
    assert np.array_equal(_u64(J), _u64(up)) and not np.array_equal(_u64(J), _u64(down)), (J, up, down)


def test_a_particle_at_a_centre_takes_the_y_normal():
    """r2 == 0: the normal is (0, 1, 0).  One particle far from the dam, exactly at the centre of sphere 1, and a step with
    dt = 0, which leaves x += 0 * v exact (the twin shows it): the particle ends at c + (R + eps) * (0, 1, 0)."""
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    c1, R1, u1 = np.array([1.0, 0.5, 1.0], F), F(0.125), np.array([0.0, 5.0, 0.0], F)
    v1 = np.array([3.0, -7.0, 2.0], F)                                  # (v - u) . (0, 1, 0) = -12: kicked
    pos, vel = np.concatenate([pos, c1[None]]), np.concatenate([vel, v1[None]])
    n = pos.shape[0]
    spheres = (np.stack([np.array([-1.75, -1.72, -1.74], F), c1]), np.array([0.1875, R1], F),
               np.stack([np.array([300.0, -150.0, 80.0], F), u1]), np.zeros(2, F), np.zeros((2, 3), F))
    with capi.Context(n, box=BOX, grid=GRID) as a, capi.Context(n, box=BOX, grid=GRID) as b:
        a.upload(pos, vel); b.upload(pos, vel)
        _track(a, spheres)
        a.step(0.0, 1); b.step(0.0, 1)
        cov, terms, kicked = _check_step(a, b, spheres, 0.0, "centre")
        pa, va, ia = a.download_owned()
        pb, vb, _ = b.download_owned()
        J, _ = a.collider_impulses()
    s = int(np.nonzero(ia == n - 1)[0][0])
    assert np.array_equal(_u32(pb[s]), _u32(c1)) and np.array_equal(vb[s], v1)          # the pre-push position IS the centre
    rp = F(R1 + EPS)
    assert np.array_equal(_u32(pa[s]), _u32(np.array([c1[0], F(c1[1] + rp), c1[2]], F))), pa[s]
    x, v, t, k, hit, walled = terms_one(c1, v1, spheres[0], spheres[1], spheres[2], MASS, BMIN, BMAX, EPS, DAMP)
    assert k[1] and not k[0] and hit and not walled and np.array_equal(x, np.array([c1[0], F(c1[1] + rp), c1[2]], F))
    assert np.array_equal(v, np.array([3.0, F(-7.0) + F(F(-1.75) * F(-12.0)), 2.0], F))
    assert np.array_equal(_u32(va[s]), _u32(v))
    assert kicked[:, 1].sum() == 1 and kicked[s, 1] and np.array_equal(_u32(terms[s, 1]), _u32(t[1]))
    assert np.array_equal(_u64(J[1]), _u64(t[1].astype(np.float64) + 0.0))
    assert cov["kicked_per_sphere"][0] >= 50


def _launch_form_run(n, pos, vel, spheres, steps, form):
    with capi.Context(n, box=BOX, grid=GRID) as c:
        form(c)
        c.upload(pos, vel)
        _track(c, spheres)
        Js = []
        for _ in range(steps):
            c.step(DT, 1)
            Js.append(c.collider_impulses()[0])
        p, v, i = c.download_owned()
        return np.stack(Js), p, v, i, c.colliders()


def test_launch_forms_change_no_bit():
    """The order of the sum depends on the wave count alone: workgroups of 128 and of 256 threads, the block orders (at
    1,025 workgroups the strip order engages from the second step on, once a sort has left its key range; 1,025 is no
    multiple of 8) and the direct walk give the same J after every step, the same particles and the same spheres."""
    n, steps = 131100, 4
    pos, vel = _fluid(n)
    spheres = _spheres(n)
    forms = {"default": lambda c: None,
             "blocks of 128": lambda c: c.set_pair_small_launch(0xFFFFFFFF),
             "blocks of 256": lambda c: c.set_pair_small_launch(0),
             "plain block order": lambda c: c.set_block_order(0, 0, 4),
             "xcd and strip order": lambda c: (c.set_pair_small_launch(0xFFFFFFFF), c.set_block_order(1, 1, 4)),
             "direct walk": lambda c: c.set_direct_hull(0)}
    ref = None
    for name, form in forms.items():
        got = _launch_form_run(n, pos, vel, spheres, steps, form)
        if ref is None:
            ref = got
            print(f"launch forms: n {n} waves {(n + 63) // 64} K {run_length(n)} workgroups of 128: {(n + 127) // 128} J after step 1 {got[0][0][0]}")
            print(f"launch forms: spheres with an impulse after steps 1..{steps}: {(np.abs(got[0]).max(axis=2) > 0).sum(axis=1)}")
            assert (np.abs(got[0][0]).max(axis=1) > 0).all()
            continue
        assert np.array_equal(_u64(got[0]), _u64(ref[0])), (name, got[0] - ref[0])
        assert np.array_equal(got[3], ref[3]), name
        assert np.array_equal(_u32(got[1]), _u32(ref[1])) and np.array_equal(_u32(got[2]), _u32(ref[2])), name
        for k in ref[4]:
            assert np.array_equal(_u32(got[4][k]), _u32(ref[4][k])), (name, k)


def test_the_sum_follows_the_population_across_a_run_boundary():
    """65,573 particles (K = 8) take a step that leaves rows and mask words up to wave 1,024; a drain then leaves 1,024 waves
    or fewer (K = 4), and a faucet brings the count back past 65,536 (K = 8).  Rows and mask words of waves that no longer
    exist must not be read -- the first step leaves such a word in the quad of mask words that holds the drained run's last
    wave, which the test asserts --, and the new waves' words are written before they are summed.  The spheres move to
    fresh fluid before each step (a step empties them), which keeps the buffers the first step wrote."""
    n0 = 65573
    pos, vel = _fluid(n0)
    corner = capi.Region.sphere((-2.0, -2.0, -2.0), 0.25)        # away from every sphere
    with capi.Context(n0, box=BOX, grid=GRID) as a:
        a.upload(pos, vel)
        removed, written = None, None
        for k, stage in enumerate(("full", "drained", "refilled")):
            if stage == "drained":
                removed = a.remove([corner])
                assert removed.size >= 100 and a.n == n0 - removed.size
            if stage == "refilled":
                a.emit(pos[removed], vel[removed], removed)       # the drained particles' first positions, at rest
                assert a.n == n0
            spheres = _spheres(n0, k)
            if stage == "full":                                   # sphere 6 on the last rows of the full top layer: the waves
                spheres[0][6], spheres[2][6] = [-0.25, -1.06, -1.0], [0.0, -200.0, -300.0]      # in front of the 37 last slots
            _track(a, spheres)
            p, v, idx = a.download_owned()
            with capi.Context(n0, box=BOX, grid=GRID) as twin:   # the same particles in the same order, no spheres
                twin.upload(p, v, idx)
                a.step(DT, 1); twin.step(DT, 1)
                cov, _, kicked = _check_step(a, twin, spheres, DT, f"population {stage}")
            want = {"full": (1025, 8), "drained": ((a.n + 63) // 64, 4), "refilled": (1025, 8)}[stage]
            assert (cov["waves"], cov["K"]) == want and (stage != "drained" or cov["waves"] <= 1024), cov
            _assert_coverage(cov, (0, 1, 2, 3) if stage == "drained" else (0, 1, 2))
            if stage == "full":
                written = np.unique(np.nonzero(kicked.any(axis=1))[0] // 64)
            if stage == "drained":
                stale = written[(written >= cov["waves"]) & (written < ((cov["waves"] + 3) & ~3))]
                print(f"population drained: stale mask words next to the last wave: {stale}")
                assert stale.size >= 1, (written[-8:], cov)


def _ten_steps(n, pos, vel, spheres, tracked):
    centers, radii, vels, _, _ = spheres
    with capi.Context(n, box=BOX, grid=GRID) as c:
        c.upload(pos, vel)
        c.set_colliders(centers, radii, vels)
        if tracked:
            c.set_collider_bodies(np.zeros(8, F))
        Js, done = [], 0
        for upto in (1, 5, 10):
            c.step(DT, upto - done)
            done = upto
            Js.append(c.collider_impulses())
        return Js, c.download(), c.colliders()


def test_tracking_changes_no_bit_at_size():
    n = 131100
    pos, vel = _fluid(n)
    spheres = _spheres(n)
    Js, st, col = _ten_steps(n, pos, vel, spheres, True)
    Js2, st2, col2 = _ten_steps(n, pos, vel, spheres, True)
    Jn, stn, coln = _ten_steps(n, pos, vel, spheres, False)
    print(f"tracking at size: n {n} waves {(n + 63) // 64} K {run_length(n)} |J| after steps 1, 5, 10: "
          f"{[float(np.abs(J).max()) for J, _ in Js]}")
    for (J, steps), (J2, steps2), want in zip(Js, Js2, (1, 5, 10)):
        assert steps == steps2 == want and J.shape == (8, 3) and np.array_equal(_u64(J), _u64(J2))
    assert (np.abs(Js[0][0]).max(axis=1) > 0).all() and all(J.shape == (0, 3) and s == 0 for J, s in Jn)
    for other, colo in ((st2, col2), (stn, coln)):
        for k in ("pos", "vel", "density", "pressure"):
            assert np.array_equal(_u32(st[k]), _u32(other[k])), k
        for k in col:
            assert np.array_equal(_u32(col[k]), _u32(colo[k])), k
    assert np.array_equal(col["centers"], advance(spheres[0], spheres[2], DT, 10))

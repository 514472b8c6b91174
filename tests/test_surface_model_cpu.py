"""CPU: the numpy model of the surface renderer (tests/surface_model.py, include/sph_hip.h: sph_render_surface) held to facts
worked out by hand -- the sphere depth of one particle, the filter's fixed points and its edge rule, the thickness counts, the
normals of a wall and at the image border, independence of the particle order -- plus sph_surface_defaults (host code: no GPU)
and the headless driver's -surface flags in its help text and its refusals."""
import os
import subprocess

import numpy as np
import pytest

import render_model as rm
import surface_model as sm
from gpufluidsimulator_amd import capi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
AXIS = rm.camera(64, 48, [1, 0, 0, 0, 1, 0, 0, 0, -1], [0, 0, 3], 0.5 * 48 / np.tan(np.pi / 6), 0.1, 100.0)
NO_SMOOTH = dict(smooth_radius_px=0, smooth_iterations=0)


def _eye_cam(w, h, focal, near=0.1, far=100.0):
    """eye space = world space: the camera at the origin looking down +z"""
    return rm.camera(w, h, [1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], focal, near, far)


def _wall(w, h, focal=8.0, d=4.25):
    """one particle behind every pixel centre, at depth d = 4.25 (with R = 0.25 its sphere's front is at 4, a power of two): the
    positions, (k + 0.5) * 17 / 32, and their projections back onto the pixel centres are exact in fp32"""
    jj, ii = np.mgrid[0:h, 0:w]
    x = ((ii + 0.5) - 0.5 * w) * d / focal
    y = (0.5 * h - (jj + 0.5)) * d / focal
    return np.stack([x.ravel(), y.ravel(), np.full(w * h, d)], axis=1).astype(F)


def test_one_particle_has_the_depth_of_its_sphere():
    R = 0.3
    out = sm.render([[0.0, 0.0, 0.0]], AXIS, sm.surface_style(**NO_SMOOTH), radius=R, index=[5], background=(9, 8, 7, 255))
    _, ident, _ = rm.render([[0.0, 0.0, 0.0]], AXIS, radius=R, index=[5])
    covered = out.id != rm.NO_ID
    assert covered.sum() == 52 and np.array_equal(covered, ident != rm.NO_ID)          # sph_render's disc
    assert (out.id[covered] == 5).all() and np.isinf(out.raw[~covered]).all() and (out.rgba[~covered] == (9, 8, 7, 255)).all()
    # the pixel (32, 24): its centre (32.5, 24.5) is one of the four nearest the sprite's centre (32, 24); in double
    rp = 0.3 * float(F(AXIS.focal_px)) / 3.0
    mag = 2 * (0.5 / rp) ** 2
    want = 3.0 - 0.3 * np.sqrt(1.0 - mag)
    assert abs(float(out.raw[24, 32]) - want) <= np.spacing(F(want))                    # one rounding of a number near 2.7
    assert out.raw[24, 32] == out.raw[23, 31] == out.raw[23, 32] == out.raw[24, 31]     # the disc is symmetric
    assert out.raw[covered].min() == out.raw[24, 32] and out.raw[covered].max() <= F(3.0)
    assert np.array_equal(out.depth.view(np.uint32), out.raw.view(np.uint32))           # no smoothing: Z_K = Z_0
    assert (out.normal[~covered] == 0).all()
    assert np.abs(np.linalg.norm(out.normal[covered].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (out.normal[covered][:, 2] < 0).all()                                        # every normal faces the eye


def test_no_iteration_or_no_radius_is_the_identity():
    rng = np.random.default_rng(3)
    z = rng.uniform(1, 2, (9, 11)).astype(F)
    z[2:4, 3:6] = np.inf
    for r, K in ((0, 3), (4, 0), (0, 0)):
        assert np.array_equal(sm.smooth(z, r, K, 0.5).view(np.uint32), z.view(np.uint32))
    a = sm.render(_wall(5, 4), _eye_cam(5, 4, 8.0), sm.surface_style(smooth_radius_px=0, smooth_iterations=2), radius=0.25)
    b = sm.render(_wall(5, 4), _eye_cam(5, 4, 8.0), sm.surface_style(smooth_radius_px=3, smooth_iterations=0), radius=0.25)
    for k in ("rgba", "id", "depth", "raw", "thick", "normal"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.depth, a.raw)


def test_a_plane_is_a_fixed_point_of_the_filter():
    z = np.full((20, 23), F(2.7), F)
    out = sm.smooth(z, 5, 3, 0.25)
    # num / den with num = sum w * z: every term and every partial sum rounds, 121 taps: within a few ulp
    assert np.abs(out.astype(np.float64) - float(F(2.7))).max() <= 121 * np.spacing(F(2.7))
    # the depth a power of two: every product w * 4 and every partial sum of num is 4 x that of den, exactly -- bit-exact
    z = np.full((7, 9), F(4.0), F)
    assert np.array_equal(sm.smooth(z, 1, 2, 0.25).view(np.uint32), z.view(np.uint32))
    assert np.array_equal(sm.smooth(z, 3, 3, 0.25).view(np.uint32), z.view(np.uint32))
    # all weights equal -- a single pixel of surface has one tap, of weight 1 * 1 * 1: num / den = z / 1
    z = np.full((5, 5), np.inf, F)
    z[2, 2] = F(1.2345)
    assert np.array_equal(sm.smooth(z, 2, 4, 0.1).view(np.uint32), z.view(np.uint32))


def test_a_step_deeper_than_tau_is_not_blurred_by_a_bit():
    z = np.full((12, 16), F(2.0), F)
    z[:, 8:] = F(2.5)                         # two sheets, 0.5 apart; tau = 0.4
    out = sm.smooth(z, 4, 3, 0.4)
    # within each sheet the plane is constant and a power-of-two-free value: equal up to the rounding of num / den;
    # across the step the weight is exactly 0, so the near sheet holds no trace of the far one
    assert np.abs(out[:, :8].astype(np.float64) - 2.0).max() <= 81 * np.spacing(F(2.0))
    assert np.abs(out[:, 8:].astype(np.float64) - 2.5).max() <= 81 * np.spacing(F(2.5))
    same = sm.smooth(z[:, :8].copy(), 4, 3, 0.4)                      # the near sheet alone: the image ends where the step was
    assert np.array_equal(out[:, :8].view(np.uint32), same.view(np.uint32))
    blurred = sm.smooth(z, 4, 3, 0.6)                                 # tau beyond the step: now it does blur
    assert (blurred[:, 7] > F(2.001)).all() and (blurred[:, 8] < F(2.499)).all()


def test_the_silhouette_does_not_move():
    rng = np.random.default_rng(5)
    z = rng.uniform(1.0, 1.3, (31, 37)).astype(F)
    hole = rng.uniform(0, 1, z.shape) < 0.4
    z[hole] = np.inf
    out = sm.smooth(z, 6, 4, 0.2)
    assert np.array_equal(np.isinf(out), hole) and not np.isnan(out).any()
    assert out[~hole].min() >= z[~hole].min() and out[~hole].max() <= z[~hole].max()      # an average stays in the range
    assert not np.array_equal(out[~hole], z[~hole])


def test_coincident_particles_add_their_thickness():
    one = sm.splat(np.array([[0.1, -0.05, 0.2]], F), AXIS, 0.3)[1]
    assert one.max() == 16 and 40 < (one > 0).sum() < 80
    for k in (2, 5):
        keys, many = sm.splat(np.repeat(np.array([[0.1, -0.05, 0.2]], F), k, axis=0), AXIS, 0.3)
        assert np.array_equal(many, k * one)
        assert ((keys[keys != rm.EMPTY] & np.uint64(0xFFFFFFFF)) == 0).all()         # equal depth: slot 0 is in front everywhere
    # by hand at the pixel (32, 24) for the particle on the axis: nz = sqrt(1 - mag), q = floor(16 nz + 0.5)
    rp = 0.3 * float(F(AXIS.focal_px)) / 3.0
    q = int(16 * np.sqrt(1 - 2 * (0.5 / rp) ** 2) + 0.5)
    assert sm.splat(np.array([[0, 0, 0]], F), AXIS, 0.3)[1].reshape(48, 64)[24, 32] == q == 16
    out = sm.render(np.zeros((3, 3), F), AXIS, sm.surface_style(absorb=(0, 0, 0)), radius=0.3)
    assert not out.thick.any()                                                        # absorb all zero: no thickness pass


def test_a_wall_seen_head_on_has_normals_towards_the_eye():
    w, h = 9, 7
    cam = _eye_cam(w, h, 8.0)
    out = sm.render(_wall(w, h), cam, sm.surface_style(smooth_radius_px=2, smooth_iterations=2), radius=0.25)
    assert (out.id.ravel() == np.arange(w * h)).all()                 # rp = 0.75 px: every pixel sees its own particle, mag = 0
    assert (out.raw == F(4.0)).all() and (out.depth == F(4.0)).all() and (out.thick == 16).all()
    assert (out.normal == np.array([0, 0, -1], F)).all()              # exactly: also at the border, where one neighbour is missing
    # lit head-on by a light from the eye: ndl = 1, n.V < 1 off the axis only
    lit = sm.render(_wall(w, h), cam, sm.surface_style(light=(0, 0, -1), absorb=(0, 0, 0), specular=0.0, tint=(0.5, 0.5, 0.5)),
                    radius=0.25)
    centre = lit.rgba[h // 2, w // 2]
    assert centre[3] == 255 and 127 <= centre[0] <= 133 and centre[0] == centre[1] == centre[2]      # 0.5 * 0.98 + 0.02 = 0.51


def test_normals_at_the_border_of_tiny_images():
    # 1 x 1: no neighbour at all -> ddx = (z/f, 0, 0), ddy = (0, z/f, 0), n = (0, 0, -1)
    z = np.array([[2.0]], F)
    assert np.array_equal(sm.normals(z, _eye_cam(1, 1, 4.0)), np.array([[[0, 0, -1]]], F))
    # 3 x 1, depths 2, 2, 3: the middle pixel picks the flatter (backward) side; the ends have one neighbour each
    cam = _eye_cam(3, 1, 4.0)
    z = np.array([[2.0, 2.0, 3.0]], F)
    n = sm.normals(z, cam).astype(np.float64)
    P = sm.eye_points(z, cam).astype(np.float64)
    for i, ddx in ((0, P[0, 1] - P[0, 0]), (1, P[0, 1] - P[0, 0]), (2, P[0, 2] - P[0, 1])):
        ddy = np.array([0.0, z[0, i] / 4.0, 0.0])
        want = np.cross(ddy, ddx)
        assert np.abs(n[0, i] - want / np.linalg.norm(want)).max() < 1e-6, i
    assert np.array_equal(n[0, 0], n[0, 1]) or np.abs(n[0, 0] - n[0, 1]).max() < 1e-6
    assert n[0, 2][0] > 0.1 and n[0, 2][2] < 0                        # the slope towards the far pixel tilts the normal to +x
    # a background neighbour is no neighbour
    z = np.array([[np.inf, 2.0, np.inf]], F)
    assert np.array_equal(sm.normals(z, cam)[0], np.array([[0, 0, 0], [0, 0, -1], [0, 0, 0]], F))
    # equal |dz| on both sides: the forward difference
    z = np.array([[1.0, 2.0, 3.0]], F)
    n = sm.normals(z, cam).astype(np.float64)
    P = sm.eye_points(z, cam).astype(np.float64)
    want = np.cross([0.0, 0.5, 0.0], P[0, 2] - P[0, 1])
    assert np.abs(n[0, 1] - want / np.linalg.norm(want)).max() < 1e-6
    other = np.cross([0.0, 0.5, 0.0], P[0, 1] - P[0, 0])
    assert np.abs(n[0, 1] - other / np.linalg.norm(other)).max() > 1e-3         # (the backward difference would show)


def test_the_order_of_the_particles_changes_only_the_ids_of_ties():
    rng = np.random.default_rng(11)
    pos = rng.uniform(-0.8, 0.8, (300, 3)).astype(F)
    pos[100:110] = pos[0:10]                                          # ten exact duplicates: depth ties
    perm = rng.permutation(300)
    a = sm.render(pos, AXIS, radius=0.08)
    b = sm.render(pos[perm], AXIS, radius=0.08, index=perm)
    for k in ("raw", "depth", "thick", "normal", "rgba"):             # flat colour: the picture does not know the ids
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    differ = a.id != b.id
    dup = np.isin(a.id, np.r_[0:10, 100:110])
    assert not (differ & ~dup).any()
    assert 0 < (a.id != rm.NO_ID).mean() < 1 and a.thick.max() > 16


def test_surface_defaults_are_the_documented_ones():
    s = capi.surface_defaults()
    assert (s.smooth_radius_px, s.smooth_iterations, s.depth_falloff, s.flat_color) == (5, 2, 0.0, 1)
    assert [F(v) for v in s.tint] == [F(0.25), F(0.55), F(0.95)] and list(s.absorb) == [6.0, 2.0, 0.5]
    assert list(s.light) == [1.0, 1.0, -1.0] and s.specular == F(0.6)
    m = sm.surface_style()
    assert (m.smooth_radius_px, m.smooth_iterations, m.flat_color, m.tint, m.absorb, m.light, m.specular) == \
        (5, 2, 1, [0.25, 0.55, 0.95], [6.0, 2.0, 0.5], [1.0, 1.0, -1.0], 0.6)
    assert sm.weights(4)[0] == 1 and abs(float(sm.weights(4)[4]) - np.exp(-2.0)) < 1e-7        # sigma = r / 2


def test_headless_help_names_the_surface_flags():
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    out = subprocess.run([EXE, "-help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for name in ("-surface", "-tint=", "-absorb="):
        assert name in out.stdout, name


@pytest.mark.parametrize("arg", ["-surface=17,2", "-surface=5,9", "-surface=5", "-surface=5,2,-1", "-surface=a,b", "-surface=5,2,0.1,7",
                                 "-tint=1,2", "-tint=1,2,-3", "-absorb=1", "-absorb=nan,1,1"])
def test_headless_refuses_a_malformed_surface_flag(arg, tmp_path):
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    args = [EXE, "-benchmark", "-frames=" + str(tmp_path / "f"), arg] + ([] if arg.startswith("-surface") else ["-surface"])
    out = subprocess.run(args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and arg.split("=")[0] in out.stderr
    assert len(out.stderr.strip().splitlines()) == 1 and "gfx950" not in out.stderr      # one line, before any GPU call
    assert not (tmp_path / "f").exists()


def test_headless_refuses_surface_without_frames():
    from gpufluidsimulator_amd import build
    build.build()
    out = subprocess.run([EXE, "-benchmark", "-surface=5,2"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "-surface" in out.stderr and "-frames" in out.stderr

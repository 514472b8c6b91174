"""CPU: the numpy model of the device renderer (tests/render_model.py, include/sph_hip.h: sph_render) -- the disc of one
sprite, the depth test and its tie rule, the colour ramp, the camera helper sph_camera_look_at (host arithmetic: no GPU), and
the headless driver's -frames flags in its help text and its refusals."""
import os
import subprocess

import numpy as np
import pytest

import render_model as rm
from gpufluidsimulator_amd import capi

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
# the reference's view written out: eye (0, 0, 3) looking down -z, 60 degrees on 48 rows
AXIS = rm.camera(64, 48, [1, 0, 0, 0, 1, 0, 0, 0, -1], [0, 0, 3], 0.5 * 48 / np.tan(np.pi / 6), 0.1, 100.0)


def test_one_particle_on_the_axis_is_the_disc_of_the_rule():
    R = 0.3
    rgba, ident, depth = rm.render([[0.0, 0.0, 0.0]], AXIS, radius=R, index=[5], index_count=8, background=(9, 8, 7, 255))
    # the rule by hand, pixel by pixel, in Python floats rounded to fp32 at every step
    focal, d = F(AXIS.focal_px), F(3.0)
    rp = F(F(R) * focal) / d
    assert 4.0 < rp < 4.5
    cx, cy = F(32.0), F(24.0)
    want = np.zeros((48, 64), bool)
    for j in range(48):
        for i in range(64):
            u, v = F(F(F(i) + F(0.5)) - cx) / rp, F(F(F(j) + F(0.5)) - cy) / rp
            want[j, i] = F(F(u * u) + F(v * v)) <= F(1.0)
    assert want.sum() == 52                                   # pixel centres within 4.157 px of the image centre
    assert np.array_equal(ident != rm.NO_ID, want)
    assert (ident[want] == 5).all() and (depth[want] == F(3.0)).all() and np.isinf(depth[~want]).all()
    assert (rgba[~want] == (9, 8, 7, 255)).all() and (rgba[want][:, 3] == 255).all()
    # lit from the upper right, towards the viewer: the brightest pixel lies up and to the right of the centre
    j, i = np.unravel_index(np.argmax(rgba[..., :3].sum(axis=-1) * want), want.shape)
    assert i >= 32 and j <= 23


def test_the_nearer_particle_wins_and_equal_depth_goes_to_the_lower_slot():
    near, far = [0.0, 0.0, 0.5], [0.0, 0.0, 0.0]
    for pos, winner in (([near, far], 0), ([far, near], 1)):
        _, ident, depth = rm.render(pos, AXIS, radius=0.1)
        assert ident[24, 32] == winner and depth[24, 32] == F(2.5)
    # same z under a camera that looks down z: the same d, bit for bit, whatever x and y
    _, ident, depth = rm.render([[0.05, 0.0, 0.0], [0.0, 0.0, 0.0]], AXIS, radius=0.3)
    both = np.zeros((48, 64), bool)
    cx, cy, rp, d, _ = rm.sprites(np.array([[0.05, 0, 0], [0, 0, 0]], F), AXIS, 0.3)
    assert d[0] == d[1]
    jj, ii = np.mgrid[0:48, 0:64]
    in0 = rm.mag_of(cx[0], cy[0], rp[0], ii, jj)[2] <= 1
    in1 = rm.mag_of(cx[1], cy[1], rp[1], ii, jj)[2] <= 1
    both = in0 & in1
    assert both.sum() > 30 and (in1 & ~in0).sum() > 0
    assert (ident[both] == 0).all() and (ident[in1 & ~in0] == 1).all()


@pytest.mark.parametrize("w,h", [(64, 48), (4096, 6), (6, 4096)])
def test_the_walk_bounds_hold_every_covered_pixel(w, h):
    """The splat tests only the pixels of walk_bounds (the device's fp32 expressions): against the whole image, for centres on
    and between pixel centres and edges, radii from the floor to the cap, and magnitudes up to the largest image."""
    rng = np.random.default_rng(7)
    k = 400
    cx = rng.uniform(-70, w + 70, k).astype(F)
    cy = rng.uniform(-70, h + 70, k).astype(F)
    rp = rng.uniform(0.75, 64.0, k).astype(F)
    # adversarial: centres exactly on pixel centres / edges and one ulp beside them, exact radii
    base = np.array([0.0, 0.5, 1.0, 2.5, w / 2, w - 1.0, w - 0.5, w], F)
    adv = np.concatenate([base, np.nextafter(base, F(1e9)), np.nextafter(base, F(-1e9))])
    radii = np.array([0.75, 1.0, 1.5, 2.0, 2.5, 63.5, 64.0], F)
    gx, gr = np.meshgrid(adv, radii)
    cx = np.concatenate([cx, gx.ravel(), np.full(gx.size, 2.5, F)])
    cy = np.concatenate([cy, np.full(gx.size, min(h, 3) - 0.5, F), np.minimum(gx.ravel(), F(h))])
    rp = np.concatenate([rp, gr.ravel(), gr.ravel()])
    i0, i1, j0, j1 = rm.walk_bounds(cx, cy, rp, w, h)
    assert (0 <= i0).all() and (i1 <= w).all() and (0 <= j0).all() and (j1 <= h).all()
    jj, ii = np.mgrid[0:h, 0:w]
    seen = 0
    for q in range(cx.size):
        cov = rm.mag_of(cx[q], cy[q], rp[q], ii, jj)[2] <= F(1.0)
        if not cov.any():
            continue
        seen += 1
        rows, cols = np.nonzero(cov.any(axis=1))[0], np.nonzero(cov.any(axis=0))[0]
        assert i0[q] <= cols[0] and cols[-1] < i1[q] and j0[q] <= rows[0] and rows[-1] < j1[q], (cx[q], cy[q], rp[q])
        # ... and tight where the image does not cut the disc off its widest part: at most three columns / rows to spare
        if 0 <= cx[q] < w and 0 <= cy[q] < h:
            assert cols[0] - i0[q] <= 3 and i1[q] - 1 - cols[-1] <= 3 and rows[0] - j0[q] <= 3 and j1[q] - 1 - rows[-1] <= 3
    assert seen > 100


def test_the_ramp_ends_and_its_clamp():
    c = rm.ramp(np.array([0.0, 1.0, 2.0, -1.0, 0.5, 1.0 / 12.0], F))
    assert np.array_equal(c[0], [1, 0, 0]) and np.array_equal(c[3], [1, 0, 0])             # red, also below 0
    assert np.array_equal(c[1], [1, 0, 1]) and np.array_equal(c[2], [1, 0, 1])             # t = 1: segment 5 with f = 1 -- magenta, no eighth colour
    assert np.array_equal(c[4], [0, 1, 0])                                                 # green in the middle
    assert c[5][0] == 1 and abs(c[5][1] - 0.25) < 1e-6 and c[5][2] == 0                    # half way to orange (1, 0.5, 0)
    assert rm.RAMP.shape == (7, 3)


def test_look_at_of_the_reference_view():
    cam = capi.look_at(640, 480)                      # eye (0, 0, 3), the origin, up +y, 60 degrees, 0.1 .. 100
    assert list(cam.rot) == [1, 0, 0, 0, 1, 0, 0, 0, -1]                 # +z FORWARD: the identity with the sign of z flipped
    assert list(cam.trans) == [0, 0, 3]
    got = np.array(list(cam.rot) + list(cam.trans), F).view(np.uint32)                     # ... and no -0 among the zeros
    assert np.array_equal(got, np.array([1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 3], F).view(np.uint32))
    assert cam.focal_px == F(0.5 * 480 / np.tan(np.deg2rad(30.0)))       # double arithmetic, rounded once
    assert (cam.width, cam.height) == (640, 480) and cam.near_z == F(0.1) and cam.far_z == F(100.0)
    # a general view: rot is orthonormal and takes the view direction to +z, trans takes the eye to the origin
    eye, tgt = np.array([0.7, -0.4, 1.9]), np.array([-0.5, -0.6, -0.55])
    cam = capi.look_at(160, 120, eye=eye, target=tgt, up=(0.2, 1.0, 0.1), fovy_deg=45.0)
    rot, trans = np.array(list(cam.rot), np.float64).reshape(3, 3), np.array(list(cam.trans), np.float64)
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-6 and np.linalg.det(rot) < 0           # (x right, y up, z forward: left-handed)
    fwd = (tgt - eye) / np.linalg.norm(tgt - eye)
    assert np.abs(rot @ fwd - [0, 0, 1]).max() < 1e-6 and np.abs(rot @ eye + trans).max() < 1e-6
    assert (rot @ np.array([0.2, 1.0, 0.1]))[1] > 0


@pytest.mark.parametrize("kw", [dict(eye=(1, 2, 3), target=(1, 2, 3)), dict(eye=(0, 0, 0), target=(0, 2, 0)),
                                dict(eye=(float("nan"), 0, 3)), dict(up=(0, float("inf"), 0)), dict(fovy_deg=float("nan")),
                                dict(near_z=0.0), dict(near_z=2.0, far_z=1.0), dict(width=0), dict(height=4097)])
def test_look_at_refuses(kw):
    args = dict(width=64, height=48)
    args.update(kw)
    with pytest.raises(capi.SphError, match="error -1"):
        capi.look_at(**args)


def test_headless_help_names_the_frames_flags():
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    out = subprocess.run([EXE, "-help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for name in ("-frames=", "-frameevery=", "-framesize=", "-camera=", "-color="):
        assert name in out.stdout, name
    assert "0-based number of the update" in out.stdout        # the numbering of frame_NNNNNN.ppm is stated


@pytest.mark.parametrize("arg", ["-framesize=96", "-framesize=0x64", "-framesize=96x64x3", "-framesize=5000x10", "-camera=0,0,3",
                                 "-camera=0,0,3,0,0,0,200", "-camera=0,3,0,0,0,0", "-camera=a,b,c,d,e,f", "-color=speed",
                                 "-color=speed:2:2", "-color=density:1", "-color=rainbow", "-frameevery=0"])
def test_headless_refuses_a_malformed_frames_flag(arg, tmp_path):
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    out = subprocess.run([EXE, "-benchmark", "-frames=" + str(tmp_path / "f"), arg], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and arg.split("=")[0] in out.stderr
    assert len(out.stderr.strip().splitlines()) == 1 and "gfx950" not in out.stderr      # one line, before any GPU call
    assert not (tmp_path / "f").exists()

"""GPU: the device renderer (sph_render, sph_render_read, sph_render_image_dev) against the numpy model of
tests/render_model.py, fed with exactly the arrays sph_download_owned returns (slot order).  The id and depth images are
compared bit for bit.  The RGBA image too: model and device perform the same IEEE fp32 operations in the same order (no
multiply-add fusion, correctly rounded division and square root), so the 8-bit colours come out equal, not merely within
the one level that the quantisation would excuse."""
import ctypes

import numpy as np
import pytest

import render_model as rm
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)
E_INVALID, E_STATE = -1, -5
F = np.float32
BG = (10, 20, 30, 255)
DT = 2e-5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ctx(capacity, **kw):
    return capi.Context(capacity, box=BOX, grid=GRID, **kw)


def _code(fn, *args, **kw):
    with pytest.raises(capi.SphError) as e:
        fn(*args, **kw)
    return int(str(e.value).split("error ")[1].split(":")[0])


def _want(c, cam, **style):
    """The model's image of the context's particles as sph_download_owned returns them."""
    pos, vel, idx = c.download_owned()
    dens = c.download(want=("density",))["density"][idx] if style.get("color") == "density" else None
    return rm.render(pos, cam, vel=vel, index=idx, density=dens, background=BG, **style)


def _same_images(got, want, what=""):
    assert got[1].shape == want[1].shape, what
    assert np.array_equal(got[1], want[1]), f"{what}: id"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), f"{what}: depth"
    diff = int(np.abs(got[0].astype(np.int32) - want[0].astype(np.int32)).max())
    print(f"{what}: covered {(want[1] != rm.NO_ID).mean():.3f}, max RGBA difference {diff}")
    assert np.array_equal(got[0], want[0]), f"{what}: rgba differs by up to {diff} levels"


def _check(c, cam, what="", **style):
    """Render with the style, compare all three images with the model; returns the model's images."""
    want = _want(c, cam, **dict(style, radius=style.get("radius") or c.params.particle_radius))
    c.render(cam, background=BG, **style)
    _same_images(c.read_image(), want, what)
    return want


@pytest.fixture(scope="module")
def cloud():
    """About 20,000 random particles with velocities, and a rolled, off-axis camera close to them (chosen on the CPU with
    the model): sprites of 1.9 to 4.6 px, some across each of the four image edges, a quarter of the image background."""
    pos, vel = ic.random_box(20000, BOX, speed=40.0, fill=0.45)
    cam = capi.look_at(160, 120, eye=(-0.45, -0.62, 0.62), target=(-0.55, -0.55, -0.55), up=(1.0, 1.0, 0.0), fovy_deg=60.0)
    return pos, vel, cam, 0.03


def test_one_particle_is_the_exact_disc():
    cam = capi.look_at(64, 48)
    with _ctx(16) as c:
        c.upload(np.array([[0.0, 0.0, 0.0]], F), index=[5])
        want = _check(c, cam, "one particle", radius=0.3, index_count=8)
        assert (want[1] != rm.NO_ID).sum() == 52              # counted by hand in tests/test_render_model_cpu.py
        _check(c, cam, "one particle, its own radius")        # 1/64: the 0.75 px floor
        _, ident, _ = c.read_image()
        assert 1 <= (ident == 5).sum() <= 4


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_a_line_of_particles_across_waves_and_blocks(n):
    cam = capi.look_at(64, 48)
    t = np.linspace(-0.9, 0.9, n)
    pos = np.stack([t, 0.5 * np.sin(3.0 * t), 0.5 * t], axis=1).astype(F)
    with _ctx(n) as c:
        c.upload(pos)
        want = _check(c, cam, f"line of {n}", radius=0.1)
        assert np.unique(want[1]).size > min(n, 40) // 2      # many different winners: every part of the launch draws
        last = want[1] == n - 1
        assert last.any()                                     # the last slot (a wave / a block of its own for 65 / 257) is drawn


def test_nearer_wins_and_equal_depth_goes_to_the_lower_slot():
    cam = capi.look_at(64, 48)
    with _ctx(8) as c:
        for pos, winner in (([[0, 0, 0.5], [0, 0, 0]], 0), ([[0, 0, 0], [0, 0, 0.5]], 1)):
            c.upload(np.array(pos, F))
            _check(c, cam, "two over one pixel", radius=0.1)
            _, ident, depth = c.read_image()
            assert ident[24, 32] == winner and depth[24, 32] == F(2.5)
        # identical d: the same z under a camera that looks down z.  Slot 0 holds creation index 7.
        pos = np.array([[0.2, 0.0, 0.0], [0.0, 0.0, 0.0]], F)
        c.upload(pos, index=[7, 3])
        for stage in ("uploaded", "sorted"):
            order = c.order()
            p, _, idx = c.download_owned()
            assert np.array_equal(idx, order)
            cx, cy, rp, d, _ = rm.sprites(p, cam, 0.3)
            assert d[0] == d[1]
            jj, ii = np.mgrid[0:48, 0:64]
            both = (rm.mag_of(cx[0], cy[0], rp[0], ii, jj)[2] <= 1) & (rm.mag_of(cx[1], cy[1], rp[1], ii, jj)[2] <= 1)
            assert both.sum() > 10
            _check(c, cam, f"equal depth, {stage}", radius=0.3)
            _, ident, _ = c.read_image()
            assert (ident[both] == order[0]).all()
            if stage == "uploaded":
                assert list(order) == [7, 3]
                c.hash()
                c.sort()                                      # x = 0.2 lies in a later cell: the sort swaps the two
        assert list(order) == [3, 7]


def test_random_cloud_through_a_perspective_camera(cloud):
    pos, vel, cam, radius = cloud
    with _ctx(pos.shape[0]) as c:
        c.upload(pos, vel)
        want = _check(c, cam, "cloud", radius=radius)
        covered = (want[1] != rm.NO_ID).mean()
        assert 0.2 <= covered <= 0.8                          # neither an empty nor a full image
        cx, cy, rp, d, vis = rm.sprites(pos, cam, radius)
        on = vis & (cx + rp > 0) & (cx - rp < 160) & (cy + rp > 0) & (cy - rp < 120)
        assert rp[on].min() >= 1.0 and rp[on].max() <= 10.0
        for edge in ((cx - rp < 0), (cx + rp > 160), (cy - rp < 0), (cy + rp > 120)):
            assert (edge & on).sum() >= 5                     # sprites across each of the four edges
        assert np.unique(want[1]).size > 500
        _check(c, cam, "cloud by speed", radius=radius, color="speed", lo=5.0, hi=35.0)


def test_culling_the_cap_and_the_floor():
    cam = capi.look_at(160, 120, eye=(0.0, 0.0, 0.5), target=(0.0, 0.0, -1.0), near_z=0.2, far_z=1.0)
    with _ctx(16) as c:
        # in front of near_z, behind the camera, beyond far_z, off to the side (x / d = 1.1 against tan = 0.77)
        c.upload(np.array([[0, 0, 0.4], [0, 0, 0.9], [0, 0, -0.8], [0.9, 0, -0.3], [0, -0.9, -0.3]], F))
        want = _check(c, cam, "culled")
        assert (want[1] == rm.NO_ID).all() and np.isinf(want[2]).all() and (want[0] == BG).all()
        # just above near_z: the 64 px cap
        pos = np.array([[0.1, 0.05, 0.5 - 0.2001]], F)
        c.upload(pos)
        assert rm.sprites(pos, cam, 0.2)[2][0] == F(64.0) and (F(0.2) * F(cam.focal_px)) / rm.sprites(pos, cam, 0.2)[3][0] > 100
        want = _check(c, cam, "cap", radius=0.2)
        assert 0.3 < (want[1] == 0).mean() < 0.8
        # far away and tiny: the 0.75 px floor still owns a pixel
        pos = np.array([[0.3, -0.2, -0.45]], F)
        c.upload(pos)
        assert rm.sprites(pos, cam, 1e-4)[2][0] == F(0.75)
        want = _check(c, cam, "floor", radius=1e-4)
        assert (want[1] == 0).sum() >= 1


def _dam():
    cfg = ic.CONFIGS["C1"]
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True)
    c = capi.Context(pos.shape[0], box=cfg["box"], grid=cfg["grid"])
    c.upload(pos, vel)
    cam = capi.look_at(160, 120, eye=(-1.2, -1.5, -0.6), target=(-1.75, -1.75, -1.75), fovy_deg=50.0)
    return c, cam


def test_after_motion_the_image_is_that_of_the_owned_range():
    c, cam = _dam()
    with c:
        c.step(float(ic.DEFAULT_DT), 3)
        want = _check(c, cam, "dam after 3 steps", radius=0.03)
        assert 0.05 < (want[1] != rm.NO_ID).mean() < 0.95
        c.step_phased(float(ic.DEFAULT_DT), 1)
        _check(c, cam, "dam after a phased step", radius=0.03)


def test_colour_modes():
    c, cam = _dam()
    with c:
        want = _check(c, cam, "density before any step", radius=0.03, color="density", lo=0.0, hi=2000.0)
        covered = want[1] != rm.NO_ID
        assert covered.any() and not want[0][covered][:, 1:3].any()          # t = 0 everywhere: shades of red
        c.step(float(ic.DEFAULT_DT), 2)
        pos, vel, idx = c.download_owned()
        rho = c.download(want=("density",))["density"][idx]
        speed = np.linalg.norm(vel, axis=1)
        assert rho.min() > 0 and speed.max() > 0
        want = _check(c, cam, "density", radius=0.03, color="density", lo=float(rho.min()), hi=float(rho.max()))
        assert len(np.unique(want[0][want[1] != rm.NO_ID][:, :3], axis=0)) > 20
        _check(c, cam, "speed", radius=0.03, color="speed", lo=0.0, hi=float(speed.max()))
        _check(c, cam, "speed, range upside down", radius=0.03, color="speed", lo=float(speed.max()), hi=0.0)


def test_after_emit_and_remove_and_with_no_particle(cloud):
    pos, vel, cam, radius = cloud
    n = 4000
    with _ctx(2 * n) as c:
        c.upload(pos[:n], vel[:n])
        c.step(DT, 1)
        c.emit(pos[n:n + 1000], vel[n:n + 1000])
        want = _check(c, cam, "after emit", radius=radius)
        assert (want[1] >= n).any() and (want[1][want[1] != rm.NO_ID] < n + 1000).all()
        gone = c.remove(capi.Region.halfspace((-0.55, 0.0, 0.0), (1.0, 0.0, 0.0)))
        assert 1000 < len(gone) < n
        want = _check(c, cam, "after remove", radius=radius)
        assert not np.isin(want[1], gone).any()
        _check(c, cam, "after remove, by density", radius=radius, color="density", lo=0.0, hi=1.0)
        c.remove(capi.Region.box((-1, -1, -1), (1, 1, 1)))
        assert c.n == 0
        c.render(cam, background=BG)
        rgba, ident, depth = c.read_image()
        assert (ident == rm.NO_ID).all() and np.isinf(depth).all() and (depth > 0).all() and (rgba == BG).all()
    with _ctx(64) as c:                                        # a context that never held a particle
        c.render(cam, background=BG)
        rgba, ident, depth = c.read_image()
        assert (ident == rm.NO_ID).all() and np.isinf(depth).all() and (rgba == BG).all()


def test_rendering_is_invisible_to_the_simulation(cloud):
    pos, vel, cam, radius = cloud
    n = 6000
    small = capi.look_at(64, 48, eye=(-0.45, -0.62, 0.62), target=(-0.55, -0.55, -0.55))
    runs = []
    for render in (True, False):
        with _ctx(n) as c:
            c.upload(pos[:n], vel[:n])
            for k in range(5):
                c.step(DT, 1)
                if render:
                    c.render(cam if k % 2 else small, radius=radius, color=("index", "speed", "density")[k % 3], lo=0.0, hi=50.0)
                    c.read_image()
            runs.append((c.download_owned(), c.order(), c.sort_stats(), c.download(want=("density", "pressure"))))
    (a, oa, sa, da), (b, ob, sb, db) = runs
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.array_equal(oa, ob) and sa == sb
    assert np.array_equal(_bits(da["density"]), _bits(db["density"])) and np.array_equal(_bits(da["pressure"]), _bits(db["pressure"]))
    with _ctx(n) as c:
        c.upload(pos[:n], vel[:n])
        c.step(DT, 2)
        c.render(cam, radius=radius, background=BG)
        first = c.read_image()
        c.render(cam, radius=radius, background=BG)             # the keys are cleared per call: the same bits again
        again = c.read_image()
        for x, y in zip(first, again):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        for size_cam, what in ((small, "64x48"), (cam, "160x120"), (small, "64x48 again")):
            _check(c, size_cam, what, radius=radius)


def test_refusals_leave_the_previous_image():
    cam = capi.look_at(64, 48)
    with _ctx(64) as c:
        c.upload(np.array([[0.0, 0.0, 0.0], [0.3, 0.2, -0.4]], F))
        assert _code(c.read_image) == E_STATE                   # nothing rendered yet
        assert c.L.sph_render_read(c.h, None, None, None) == E_STATE
        c.render(cam, radius=0.2, background=BG)
        before = c.read_image()
        assert (before[1] != rm.NO_ID).any()

        def cam_with(**kw):
            bad = capi.Camera.from_buffer_copy(cam)
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(bad, k)[v[0]] = v[1]
                else:
                    setattr(bad, k, v)
            return bad
        nan, inf = float("nan"), float("inf")
        bad_cams = [cam_with(width=0), cam_with(width=4097), cam_with(height=0), cam_with(height=4097), cam_with(rot=(4, nan)),
                    cam_with(trans=(2, inf)), cam_with(focal_px=0.0), cam_with(focal_px=-1.0), cam_with(focal_px=nan),
                    cam_with(near_z=0.0), cam_with(near_z=-0.1), cam_with(near_z=nan), cam_with(far_z=0.1), cam_with(far_z=0.05),
                    cam_with(far_z=inf)]
        for bad in bad_cams:
            assert _code(c.render, bad, radius=0.2) == E_INVALID
        for kw in (dict(color="speed", lo=1.0, hi=1.0), dict(color="density", lo=0.0, hi=0.0), dict(color="speed", lo=nan, hi=1.0),
                   dict(radius=-0.1), dict(radius=nan), dict(radius=inf)):
            assert _code(c.render, cam, **kw) == E_INVALID, kw
        style = capi.RenderStyle(3, 0.0, 1.0, 0.0, 0, (ctypes.c_uint8 * 4)(0, 0, 0, 255))       # an unknown mode
        assert c.L.sph_render(c.h, ctypes.byref(cam), ctypes.byref(style)) == E_INVALID
        style.color_mode = -1
        assert c.L.sph_render(c.h, ctypes.byref(cam), ctypes.byref(style)) == E_INVALID
        assert c.L.sph_render(c.h, None, ctypes.byref(style)) == E_INVALID
        for x, y in zip(before, c.read_image()):                  # the previous image: readable and unchanged
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        c.render(cam, color="index", lo=1.0, hi=1.0, radius=0.2, background=BG)      # index mode does not use lo / hi
        assert c.image_dev()[1:] == (64, 48)
    with capi.Context(64, box=BOX, grid=GRID, slab=(0, 16), ghost_capacity=64) as s:
        assert _code(s.render, cam) == E_STATE                  # the ranks would have to composite
        assert _code(s.read_image) == E_STATE


def test_image_dev_follows_the_last_render():
    with _ctx(8) as c:
        c.upload(np.array([[0.0, 0.0, 0.0]], F))
        assert _code(c.image_dev) == E_STATE
        c.render(capi.look_at(64, 48))
        p, w, h = c.image_dev()
        assert p and (w, h) == (64, 48)
        c.render(capi.look_at(160, 120))
        p, w, h = c.image_dev()
        assert p and (w, h) == (160, 120)
        c.sync()

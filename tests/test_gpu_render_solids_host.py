"""GPU: the solids in the picture through the host class and the headless driver (sph_headless -frames=DIR -drawsolids
[-solidlook=k:r,g,b[,open]]: ParticleSystem::setRenderSolids / renderFrame / writeFrame on top of sph_render_set_solids) -- the PPM
files against the image of the C ABI, against the frames of a run without -drawsolids and the numpy model's id plane
(tests/solid_render_model.py), and the command-line refusals."""
import os
import subprocess

import numpy as np
import pytest

import render_model as rm
import solid_render_model as so
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
W, H = 160, 120
EYE, TARGET, FOVY = (-1.2, -1.3, -0.9), (-1.75, -1.75, -1.75), 50.0
CELL = 0.125                                       # 35 nodes per axis over the box of edge 4
BALL = ((-1.45, -1.8, -1.45), 0.2)                 # -obstacle=sphere: slot 0
PADDLE = ((-1.7, -1.45, -1.7), (0.3, 0.1, 0.15))   # -solid=1:box, turning about its centre
OMEGA = (0.0, 0.0, 4000.0)
LOOK = (0.9, 0.4, 0.1)
ARGS = ["-benchmark", "-n=4096", "-box=4", "-i=2", "-nowarmup", f"-framesize={W}x{H}",
        "-camera=" + ",".join(str(v) for v in EYE + TARGET + (FOVY,)),
        "-obstacle=sphere:" + ",".join(str(v) for v in BALL[0] + (BALL[1],)), f"-obstaclecell={CELL}",
        "-solid=1:box:" + ",".join(str(v) for v in PADDLE[0] + PADDLE[1]), f"-solidcell=1:{CELL}",
        "-solidspin=1:" + ",".join(str(v) for v in PADDLE[0] + OMEGA)]
DRAW = ["-drawsolids", "-solidlook=1:" + ",".join(str(v) for v in LOOK)]


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=120)      # a fresh child process


def _ppm(path):
    data = path.read_bytes()
    header = b"P6\n%d %d\n255\n" % (W, H)
    assert data.startswith(header) and len(data) == len(header) + W * H * 3
    return np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)


def _frames(d, extra):
    out = _run(ARGS + ["-frames=" + str(d)] + extra)
    assert out.returncode == 0, out.stderr
    assert sorted(os.listdir(d)) == ["frame_000000.ppm", "frame_000001.ppm"]
    return [_ppm(d / "frame_000000.ppm"), _ppm(d / "frame_000001.ppm")]


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """the driver's two frames (after the updates 0 and 1) with -drawsolids and without, written once for the tests below"""
    d = tmp_path_factory.mktemp("solids")
    return _frames(d / "with", DRAW), _frames(d / "without", [])


def _context():
    """what the driver runs: ParticleSystem(4096, box 4) + reset(CONFIG_GRID), the ball in slot 0 and the turning paddle in slot 1"""
    pos, vel = ic.dam_break_lattice((16, 16, 16), (4.0, 4.0, 4.0), jitter=True)
    c = capi.Context(4096, box=(4.0,) * 3, grid=(64,) * 3)
    c.upload(pos, vel)
    c.build_obstacle([capi.Shape.sphere(*BALL)], CELL, slot=0)
    c.build_obstacle([capi.Shape.box(*PADDLE)], CELL, slot=1)
    c.set_obstacle_pose(PADDLE[0], (1.0, 0.0, 0.0, 0.0), OMEGA, slot=1)
    c.set_obstacle_sensor(True, slot=1)
    c.set_render_solids(capi.solid_defaults(looks={1: dict(color=LOOK)}))
    return c


def test_the_host_class_writes_the_image_of_the_c_abi(frames):
    """ParticleSystem::setRenderSolids + renderFrame + writeFrame == sph_render_set_solids + sph_render + sph_render_read"""
    cam = capi.look_at(W, H, eye=EYE, target=TARGET, fovy_deg=FOVY)
    with _context() as c:
        for k in range(2):
            c.step(float(ic.DEFAULT_DT), 1)
            c.render(cam)
            rgba, ident, _ = c.read_image()
            assert np.array_equal(frames[0][k], rgba[..., :3]), f"frame {k}"
            for slot in (0, 1):
                assert (ident == so.ID_SOLID + slot).sum() > 50, (k, slot)


def test_drawsolids_changes_the_frames_exactly_where_the_model_says_solid(frames):
    cam = capi.look_at(W, H, eye=EYE, target=TARGET, fovy_deg=FOVY)
    looks = {0: so.DEFAULT_COLOR, 1: LOOK}
    with _context() as c:
        for k in range(2):
            c.step(float(ic.DEFAULT_DT), 1)
            pos, vel, idx = c.download_owned()
            slots = {}
            for s in (0, 1):
                ob, ps = c.obstacle(read=True, slot=s), c.obstacle_pose(slot=s)
                pose = None if ps is None else {"pivot": ps["pivot"], "q": ps["quat"], "omega": ps["omega"]}
                slots[s] = so.slot({"dims": ob["dims"], "origin": ob["origin"], "spacing": ob["spacing"]}, ob["phi"], ob["offset"], pose,
                                   color=looks[s])
            assert slots[0]["pose"] is None and slots[1]["pose"] is not None
            sol = so.march(cam, slots)
            rgba, ident, _, win = so.compose_render(rm.render(pos, cam, index=idx, radius=c.params.particle_radius), sol)
            differ = (frames[0][k] != frames[1][k]).any(axis=2)
            print("frame", k, "solid pixels", int(win.sum()), "of them with the colour they had", int((win & ~differ).sum()))
            assert win.sum() > 200 and np.array_equal((ident >= so.ID_SOLID) & (ident != rm.NO_ID), win)
            assert not differ[~win].any()
            assert np.array_equal(frames[0][k], rgba[..., :3])
            assert np.array_equal(frames[1][k][~win], rgba[..., :3][~win])
            assert (win & ~differ).sum() <= win.sum() // 100          # (a solid pixel may by chance have the colour of what it hides)


@pytest.mark.parametrize("args, word", [
    (["-drawsolids"], "-drawsolids / -solidlook: expected -frames=<directory>"),
    (["-frames=DIR", "-solidlook=1:0.5,0.5,0.5"], "-drawsolids / -solidlook: expected -frames=<directory>"),
    (["-frames=DIR", "-drawsolids", "-solidlook=4:0.5,0.5,0.5"], "-solidlook=4:0.5,0.5,0.5: expected <k>:<r>,<g>,<b>[,<open>]"),
    (["-frames=DIR", "-drawsolids", "-solidlook=1:0.5,1.5,0.5"], "each colour in [0, 1]"),
    (["-frames=DIR", "-drawsolids", "-solidlook=1:0.5,0.5"], "-solidlook=1:0.5,0.5: expected"),
    (["-frames=DIR", "-drawsolids", "-solidlook=1:0.5,0.5,0.5,2"], "open 0 or 1"),
    (["-frames=DIR", "-drawsolids", "-gpus=2", "-onegpu"], "-drawsolids is not supported with -gpus=2"),
    (["-frames=DIR", "-drawsolids", "-gpus=1", "-slab"], "-drawsolids is not supported with -gpus=1 -slab"),
])
def test_headless_refusals(tmp_path, args, word):
    d = tmp_path / "frames"
    out = _run(ARGS + [a.replace("DIR", str(d)) for a in args])
    assert out.returncode != 0 and word in out.stderr, out.stderr
    assert not d.exists()


def test_solidhelp_names_the_options():
    out = _run(["-benchmark", "-solidhelp"])
    assert out.returncode == 0 and "-drawsolids" in out.stdout and "[-solidlook=<k>:<r>,<g>,<b>[,<open>]]" in out.stdout

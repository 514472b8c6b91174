"""GPU: mesh obstacles through the OBJ reader, the host class and the headless driver (sph_headless -obstaclemesh=FILE.obj:
ParticleSystem::setObstacleMeshOBJ on top of sph_obstacle_build_obj) -- the state the driver writes equals the C-ABI path bit for
bit, a saved mesh comes back with the same bits, the forms of an OBJ file, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import mesh_obstacle_cases as mc
from gpufluidsimulator_amd import capi, ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)
F = np.float32


def _run(args):
    return subprocess.run([EXE, "-benchmark", "-n=4096", "-box=4", "-nowarmup"] + args, capture_output=True, text=True, timeout=300)


def _write_obj(path, v, t):
    with open(path, "w") as f:
        for p in v:
            f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        for a, b, c in t:
            f.write(f"f {a + 1} {b + 1} {c + 1}\n")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


PILLAR = mc.box_mesh((-1.71, -2.2, -1.93), (-1.43, -1.33, -1.62))      # stands in the dam; its foot is below the floor


def test_headless_mesh_obstacle_equals_the_c_abi_path(tmp_path):
    v, t = PILLAR
    obj, f = tmp_path / "pillar.obj", tmp_path / "state.bin"
    _write_obj(obj, v, t)
    out = _run(["-i=5", f"-obstaclemesh={obj}", "-obstaclecell=0.0625", "-obstaclevel=150,0,0", f"-out={f}"])
    assert out.returncode == 0, out.stderr
    assert "obstacle mesh: 12 triangles used, 0 skipped, 0 lost crossings, 0 odd columns" in out.stdout
    raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    with capi.Context(4096, box=BOX, grid=GRID) as c, capi.Context(4096, box=BOX, grid=GRID) as b:
        c.build_obstacle_mesh(v, t, 0.0625)
        assert c.obstacle_mesh_stats() == (12, 0, 0, 0)
        c.set_obstacle_motion(velocity=(150.0, 0.0, 0.0))
        c.upload(pos, vel); b.upload(pos, vel)
        c.step(DT, 5); b.step(DT, 5)
        st = c.download()
        assert (st["pos"] != b.download()["pos"]).any(axis=1).sum() > 300          # (the solid did move particles)
    assert np.array_equal(_bits(raw[0, :, :3]), _bits(st["pos"]))
    assert np.array_equal(_bits(raw[1, :, :3]), _bits(st["vel"]))


def test_a_saved_mesh_comes_back_with_the_same_bits(tmp_path):
    pos = mc.blob_particles()
    obj = tmp_path / "blob.obj"
    bounds = (mc.BMIN, mc.BMAX)
    with capi.Context(512, box=mc.BOX, grid=mc.GRID) as c:
        c.upload(pos, np.zeros_like(pos))
        c.extract_mesh(capi.mesh_defaults(spacing=float(mc.S)))
        c.save_obj(obj)
        v, _, t = c.read_mesh()
        c.build_obstacle_mesh(v, t, float(mc.S), bounds=bounds)
        want, stats = c.obstacle(read=True)["phi"], c.obstacle_mesh_stats()
        c.clear_obstacle()
        c.build_obstacle_obj(obj, float(mc.S), bounds=bounds)
        assert np.array_equal(_bits(c.obstacle(read=True)["phi"]), _bits(want))
        assert c.obstacle_mesh_stats() == stats and stats[0] == len(t) and stats[1:] == (0, 0, 0)


def test_the_forms_of_an_obj_file(tmp_path):
    """quads fanned from their first vertex, a, a/b, a//c and a/b/c entries, negative (relative) indices, and the
    lines the reader ignores"""
    v, _ = mc.box_mesh((-0.53, -0.41, -0.27), (0.29, 0.47, 0.36))
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    obj = tmp_path / "forms.obj"
    with open(obj, "w") as f:
        f.write("# a box\nmtllib none.mtl\no box\n")
        for p in v[:4]:
            f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        f.write("vt 0 0\nvn 0 0 1\n")
        a, b, c, d = quads[4]                              # only the first four vertices: written before the others exist
        f.write(f"f {a - 4} {b - 4} {c - 4} {d - 4}\n")    # relative to the four vertices read so far
        for p in v[4:]:
            f.write("  v %.9g %.9g %.9g\r\n" % tuple(float(x) for x in p))
        f.write("s off\nusemtl stone\n")
        a, b, c, d = quads[0]
        f.write(f"f {a + 1}/1/1 {b + 1}/1/1 {c + 1}/1/1 {d + 1}/1/1\n")
        a, b, c, d = quads[1]
        f.write(f"f {a + 1}//1 {b + 1}//1 {c + 1}//1 {d + 1}//1\r\n")
        a, b, c, d = quads[2]
        f.write(f"f {a + 1}/1 {b + 1}/1 {c + 1}/1 {d + 1}/1\n")
        a, b, c, d = quads[3]
        f.write(f"f {a - 8} {b - 8}/1/1 {c + 1} {d - 8}//1\n")
        a, b, c, d = quads[5]
        f.write(f"f\t{a + 1} {b + 1} {c + 1}\nf {a + 1} {c + 1} {d + 1}\n")
        f.write("l 1 2\n")
    order = [4, 0, 1, 2, 3]
    stated = [tri for q in order for tri in ((quads[q][0], quads[q][1], quads[q][2]), (quads[q][0], quads[q][2], quads[q][3]))]
    stated += [(quads[5][0], quads[5][1], quads[5][2]), (quads[5][0], quads[5][2], quads[5][3])]
    bounds = (mc.BMIN, mc.BMAX)
    with capi.Context(64, box=mc.BOX, grid=mc.GRID) as c:
        c.build_obstacle_obj(obj, float(mc.S), bounds=bounds)
        got, stats = c.obstacle(read=True)["phi"], c.obstacle_mesh_stats()
        c.build_obstacle_mesh(v, np.array(stated, np.uint32), float(mc.S), bounds=bounds)
        assert np.array_equal(_bits(got), _bits(c.obstacle(read=True)["phi"]))
        assert stats == (12, 0, 0, 0) == c.obstacle_mesh_stats()
    assert np.array_equal(_bits(got), _bits(mc.model("free_box")[0]))
    # files the reader refuses: no face, an index that names no vertex, a face of two vertices
    L = capi.load()
    with capi.Context(64, box=mc.BOX, grid=mc.GRID) as c:
        for k, text in enumerate(("v 0 0 0\nv 1 0 0\nv 0 1 0\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "v 0 0 0\nv 1 0 0\nf 1 2\n",
                                  "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", "v 0 0\nf 1 1 1\n")):
            bad = tmp_path / f"bad{k}.obj"
            bad.write_text(text)
            before = capi.memory_stats()
            assert L.sph_obstacle_build_obj(c.h, None, None, None, os.fsencode(bad)) == -1, text
            assert c.obstacle() is None and capi.memory_stats() == before


def test_headless_refusals(tmp_path):
    obj = tmp_path / "pillar.obj"
    _write_obj(obj, *PILLAR)
    out = _run(["-i=1", "-gpus=2", "-onegpu", f"-obstaclemesh={obj}"])
    assert out.returncode != 0 and "-obstaclemesh" in out.stderr
    out = _run(["-i=1", f"-obstaclemesh={obj}", "-obstacle=sphere:0,0,0,0.1"])
    assert out.returncode != 0 and "-obstaclemesh" in out.stderr
    for bad in ("-obstacleband=17", "-obstacleband=0", "-obstacleband=x"):
        out = _run(["-i=1", f"-obstaclemesh={obj}", bad])
        assert out.returncode != 0 and "-obstacleband" in out.stderr, bad
    out = _run(["-i=1", "-obstacleband=2"])
    assert out.returncode != 0 and "-obstaclemesh" in out.stderr
    out = _run(["-i=1", "-obstacleinvert"])
    assert out.returncode != 0 and "-obstaclemesh" in out.stderr
    out = _run(["-i=1", "-obstaclemesh="])
    assert out.returncode != 0 and "-obstaclemesh" in out.stderr
    out = _run(["-i=1", f"-obstaclemesh={tmp_path / 'missing.obj'}"])            # the library refuses the file, and the class aborts
    assert out.returncode != 0 and "missing.obj" in out.stderr
    out = _run(["-help"])
    assert out.returncode == 0 and "-obstaclemesh" in out.stdout and "-obstacleband" in out.stdout and "-obstacleinvert" in out.stdout

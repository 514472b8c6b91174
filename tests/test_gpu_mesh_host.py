"""GPU: the headless driver writes geometry (sph_headless -mesh=DIR: ParticleSystem::setMeshParams / writeMeshOBJ / extractMesh on
top of sph_mesh_extract) -- which files, that an OBJ read back is the mesh of the C ABI bit for bit, that the host class's
extractMesh gives the same bytes, that the surface of a stepped dam is closed, and the refusal next to -gpus=N."""
import os
import re
import subprocess

import numpy as np
import pytest

import mesh_model as mm
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
ARGS = ["-benchmark", "-n=4096", "-i=4", "-meshevery=3", "-meshcell=0.04"]
F = np.float32


def _run(args):
    from gpufluidsimulator_amd import build
    build.build()            # (does nothing when the driver is newer than its sources)
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=120)


def _parse_obj(path):
    v, vn, f = [], [], []
    for line in open(path):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([F(x) for x in w[1:4]])
        elif w[0] == "vn":
            vn.append([F(x) for x in w[1:4]])
        elif w[0] == "f":
            corners = [c.split("/") for c in w[1:4]]
            assert all(len(c) == 3 and c[1] == "" and c[0] == c[2] for c in corners), line      # a//a
            f.append([int(c[0]) - 1 for c in corners])
    return np.array(v, F).reshape(-1, 3), np.array(vn, F).reshape(-1, 3), np.array(f, np.uint32).reshape(-1, 3)


def _fnv1a64(*arrays):
    h = 1469598103934665603
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_headless_writes_meshes_that_are_the_c_abis(tmp_path):
    meshes, snap = tmp_path / "meshes", tmp_path / "state.snap"
    out = _run(ARGS + ["-mesh=" + str(meshes), "-save=" + str(snap)])
    assert out.returncode == 0, out.stderr
    # numbered by the 0-based update the mesh follows (stated in -help): updates 0 and 3 of 0..3
    assert sorted(os.listdir(meshes)) == ["mesh_00000.obj", "mesh_00003.obj"]
    # the state after update 3, the last one, is the saved one: its mesh through the C ABI
    n, params = capi.Context.snapshot_info(str(snap))
    with capi.Context(n, params=params) as c:
        c.load_snapshot(str(snap))
        nv, nt = c.extract_mesh(capi.mesh_defaults(spacing=0.04))
        pos, nrm, tri = c.read_mesh()
        c.save_obj(str(tmp_path / "again.obj"))
    assert nv > 100 and nt > 200
    for path in (meshes / "mesh_00003.obj", tmp_path / "again.obj"):     # %.9g round-trips fp32: the same bits
        v, vn, f = _parse_obj(path)
        assert np.array_equal(v.view(np.uint32), pos.view(np.uint32)) and np.array_equal(vn.view(np.uint32), nrm.view(np.uint32))
        assert np.array_equal(f, tri)
    # ParticleSystem::extractMesh of the final state: the driver's last line
    m = re.search(r"^mesh: (\d+) vertices, (\d+) triangles, fnv1a64 ([0-9a-f]{16})$", out.stdout, re.M)
    assert m, out.stdout
    assert (int(m.group(1)), int(m.group(2))) == (nv, nt) and int(m.group(3), 16) == _fnv1a64(pos, nrm, tri)
    # an OBJ of a stepped dam opens as a closed surface, wound outwards
    for name in sorted(os.listdir(meshes)):
        v, vn, f = _parse_obj(meshes / name)
        mm.check_closed_oriented(f)
        assert mm.signed_volume(v, f) > 0
        assert np.allclose(np.linalg.norm(vn.astype(np.float64), axis=1), 1.0, atol=1e-5)


def test_headless_writes_frames_and_meshes_side_by_side(tmp_path):
    out = _run(["-benchmark", "-n=4096", "-i=2", "-meshcell=0.05", "-meshradius=0.1", "-iso=0.8", "-mesh=" + str(tmp_path / "m"),
                "-frames=" + str(tmp_path / "f"), "-framesize=32x24"])
    assert out.returncode == 0, out.stderr
    assert sorted(os.listdir(tmp_path / "m")) == ["mesh_00000.obj", "mesh_00001.obj"]
    assert sorted(os.listdir(tmp_path / "f")) == ["frame_000000.ppm", "frame_000001.ppm"]


def test_headless_refuses_meshes_with_slabs_and_bad_values(tmp_path):
    meshes = tmp_path / "meshes"
    out = _run(ARGS + ["-mesh=" + str(meshes), "-gpus=2", "-onegpu"])
    assert out.returncode != 0 and "-mesh" in out.stderr
    assert not meshes.exists()
    for bad in (["-mesh"], ["-mesh=" + str(meshes), "-meshradius=1"], ["-mesh=" + str(meshes), "-iso=-1"], ["-meshevery=2"],
                ["-mesh=" + str(meshes), "-meshcell=0.0001"]):
        out = _run(["-benchmark", "-n=4096", "-i=1"] + bad)
        assert out.returncode != 0 and "mesh" in out.stderr + out.stdout, bad
        assert not meshes.exists()

"""CPU: libsph_hip.so builds for gfx950, loads, and exports every symbol include/sph_hip.h
declares (no compute calls: there is no GPU here)."""
import json
import os
import re

import pytest

from gpufluidsimulator_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sph_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_the_header():
    lib_path = build.build()
    assert os.path.exists(lib_path)
    lib = capi.load()
    names = _declared("sph_hip.h")
    assert len(names) >= 40
    assert "sph_test_guard" in names and "sph_test_guard_check" in names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sph_hip.h but not exported"
        assert n in capi.SIGNATURES, f"{n} has no ctypes signature in capi.py"
    assert lib.sph_abi_version() == 2


def test_reference_seam_symbols_are_exported():
    """include/sph_compat_seam.h: the reference's own 19 extern "C" names (SPH/particleSystem.cuh:3-30)
    plus the two helpers, and the two IC twins of include/particleSystem.h."""
    import ctypes as C
    lib = C.CDLL(build.build())
    seam = ["iceildiv", "cudaInit", "allocateArray", "freeArray", "registerGLBufferObject", "unregisterGLBufferObject",
            "mapGLBufferObject", "unmapGLBufferObject", "threadSync", "copyArrayFromDevice", "copyArrayToDevice",
            "cudaComputeDensities", "cudaComputeForces", "cudaParticleCollisions", "cudaMapZIndex", "cudaSortParticles",
            "cudaConstructBGrid", "cudaConstructGridArray", "cudaIntegrate"]
    src = open(os.path.join(ROOT, "include", "sph_compat_seam.h")).read()
    # the names the reference's particleSystem.cuh declares, recorded from its source (a list of names)
    with open(os.path.join(ROOT, "tests", "golden", "reference_seam_names.json")) as f:
        ref = set(json.load(f)["names"])
    for n in seam + ["sph_compat_context", "sph_compat_release", "sph_compat_vbo_dev", "sph_ic_dam_break", "sph_ic_random_box"]:
        assert hasattr(lib, n), f"{n} not exported"
        if n in seam:
            assert re.search(r"\b%s\s*\(" % n, src), f"{n} not declared in sph_compat_seam.h"
            assert n in ref, f"{n} is not a name of the reference seam"
    lib.iceildiv.restype = C.c_uint
    assert lib.iceildiv(10, 32) == 1 and lib.iceildiv(64, 32) == 2 and lib.iceildiv(65, 32) == 3   # .cu:423-425
    assert ref == set(seam), ref ^ set(seam)     # the reference declares exactly these 19 functions


def test_default_params_are_the_reference_constants():
    p = capi.default_params((4.0, 4.0, 4.0), (64, 64, 64))
    assert tuple(p.box_min) == (-2.0, -2.0, -2.0) and tuple(p.box_max) == (2.0, 2.0, 2.0)
    assert abs(p.h - 0.1) < 1e-8 and p.mass == 65.0 and p.rest_density == 1000.0 and p.gas_constant == 2000.0
    assert p.viscosity == 250.0 and abs(p.gravity_y - (-9.81 * 11000)) < 1e-1 and p.wall_damping == -0.75
    assert p.particle_radius == 1.0 / 64.0
    lib = capi.load()
    # nextPow2((uint)(edge / (0.66666f * h))), particleSystem.cpp:46
    assert [lib.sph_grid_dim_for_edge(e, 0.1) for e in (2.0, 4.0, 8.0, 32.0, 64.0)] == [32, 64, 128, 512, 1024]


def test_no_cpu_fallback():
    """Without a gfx950 device the product path must fail loudly, not compute on the CPU."""
    n, is950 = capi.device_count()
    if n > 0 and is950:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(capi.SphError):
        capi.Context(64, box=(2, 2, 2), grid=(32, 32, 32))


def test_cpp_initial_conditions_match_numpy_bit_for_bit():
    """ParticleSystem::reset() (C++) and gpufluidsimulator_amd.ic (numpy) must hand the same arrays to
    the device and to the oracle."""
    import ctypes as C

    import numpy as np

    from gpufluidsimulator_amd import ic
    lib = capi.load()
    for lattice, box, jitter in (((16, 16, 16), (4.0, 4.0, 4.0), True), ((7, 5, 9), (2.0, 4.0, 8.0), True),
                                 ((12, 12, 12), (2.0, 2.0, 2.0), False)):
        n = lattice[0] * lattice[1] * lattice[2]
        pos = np.empty((n, 3), np.float32); vel = np.empty((n, 3), np.float32)
        lib.sph_ic_dam_break((C.c_uint32 * 3)(*lattice), (C.c_float * 3)(*box), int(jitter), 0, n,
                             pos.ctypes.data, vel.ctypes.data)
        want, _ = ic.dam_break_lattice(lattice, box, jitter=jitter)
        assert np.array_equal(pos.view(np.uint32), want.view(np.uint32))
        assert not vel.any()
    # a window of a bigger lattice (start/count), as the slab ranks generate it
    lat, box = (64, 64, 64), (8.0, 8.0, 8.0)
    pos = np.empty((1000, 3), np.float32)
    lib.sph_ic_dam_break((C.c_uint32 * 3)(*lat), (C.c_float * 3)(*box), 1, 123456, 1000, pos.ctypes.data, None)
    want, _ = ic.dam_break_lattice(lat, box, jitter=True, start=123456, count=1000)
    assert np.array_equal(pos.view(np.uint32), want.view(np.uint32))
    pos = np.empty((500, 3), np.float32); vel = np.empty((500, 3), np.float32)
    lib.sph_ic_random_box(500, (C.c_float * 3)(2.0, 2.0, 2.0), 7.5, 1973, 0.45, pos.ctypes.data, vel.ctypes.data)
    wp, wv = ic.random_box(500, (2.0, 2.0, 2.0), speed=7.5, fill=0.45)
    assert np.array_equal(pos.view(np.uint32), wp.view(np.uint32)) and np.array_equal(vel.view(np.uint32), wv.view(np.uint32))

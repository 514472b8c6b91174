"""GPU: every walk of the mixed-precision density pass (`k_density_h`, csrc/sph_pairs.hip) against the float64 model of
tests/sph_model.py, on the cases of tests/mixed_cases.py.

The kernel has four walks: the pass loop (at most three reference points per wave), the staged walk (two parity copies per
piece, groups of 4 pairs and a masked tail), the packed direct walk of long hulls, and the fp32 gather of the lanes three
passes did not serve.  tests/test_gpu_mixed_precision.py holds it to 2e-2 max / 4e-3 rms, which one dropped or doubled
candidate out of ~30 does not reach.  Here:
  * DYADIC cases, on which packed fp16 arithmetic is exact (mixed_cases.py says why, tests/test_mixed_cases_cpu.py shows it):
    EVERY particle within the fp32 bar 1e-5 of the model, under the staged walk (direct hull 0xFFFFFFFF), the default (512) and
    the direct walk (0).  A wrong copy, a piece edge off by one or a tail that lets a candidate through twice is an error of
    1e-3 or more there;
  * GENERIC cases at the documented mixed bar: droplets that reach passes 2, 3 and the gather with real neighbours (the gather
    is fp32 arithmetic: those particles at 1e-5), cells up to the 12 h include/sph_hip.h admits, 600 particles in one cell
    (row sums of a few hundred in fp16);
  * the device's order is the stable cell-key order over which the CPU tests state which lane takes which walk.
"""
import numpy as np
import pytest

import mixed_cases as mc
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5                                   # tests/test_gpu_parity.py: the fp32 bar
RHO_MAX, RHO_RMS = 2e-2, 4e-3                    # tests/test_gpu_mixed_precision.py: the mixed bar
STAGED, DEFAULT, DIRECT = 0xFFFFFFFF, 512, 0     # sph_set_direct_hull
FIELDS = ("h", "mass", "rest_density", "gas_constant", "viscosity", "gravity_y", "wall_eps", "wall_damping", "restitution",
          "collision_param", "particle_radius")


def _params(case):
    p = capi.default_params((1, 1, 1), case.params.grid)
    for a in range(3):
        p.box_min[a], p.box_max[a], p.grid[a] = float(case.params.box_min[a]), float(case.params.box_max[a]), int(case.params.grid[a])
    for k in FIELDS:
        setattr(p, k, float(getattr(case.params, k)))
    return p


def _densities(case, hulls, fp32=True):
    """{hull: mixed density} (and {"fp32": density}) of one context, by creation index, plus the order after the sort."""
    out = {}
    with capi.Context(case.pos.shape[0], params=_params(case)) as c:
        for mixed, hull in ([(False, DEFAULT)] if fp32 else []) + [(True, h) for h in hulls]:
            c.set_precision(mixed)
            c.set_direct_hull(hull)
            c.upload(case.pos, np.zeros_like(case.pos))
            c.hash(); c.sort(); c.build_cells(); c.density()
            out[hull if mixed else "fp32"] = c.download(want=("density",))["density"]
        out["order"] = c.order()
    return out


def _rel(case, rho):
    assert np.isfinite(rho).all()
    return rho.astype(np.float64) / mc.model_density(case) - 1


def _worst(case, rel, k=6):
    """The worst particles with what decides their walk: slot, pass, and the nine (start parity, length) of their rows."""
    L, slot = mc.layout(case), np.empty(rel.size, np.int64)
    slot[L.order] = np.arange(rel.size)
    pass_no = mc.passes(case)[0]
    rows = []
    for i in np.argsort(-np.abs(rel))[:k]:
        s = slot[i]
        rows.append((int(i), f"{rel[i]:+.2e}", "slot", int(s), "pass", int(pass_no[s]),
                     [(int(a) & 1, int(b - a)) for a, b in zip(L.lo[s], L.hi[s]) if b > a]))
    return rows


@pytest.mark.parametrize("name", list(mc.DYADIC))
def test_dyadic_case_is_exact_under_every_walk(name):
    case = mc.DYADIC[name]()
    got = _densities(case, (STAGED, DEFAULT, DIRECT))
    fp32 = np.abs(_rel(case, got["fp32"])).max()
    print(f"{name}: fp32 {fp32:.2e}")
    assert fp32 <= REL_TOL, "the case itself: fp32 density against the model"
    errs = {}
    for hull in (STAGED, DEFAULT, DIRECT):
        rel = _rel(case, got[hull])
        errs[hull] = np.abs(rel).max()
        print(f"{name}: direct hull {hull:#x}: max {errs[hull]:.3e}, particles beyond 1e-5: {np.count_nonzero(np.abs(rel) > REL_TOL)}")
    for hull in (STAGED, DEFAULT, DIRECT):
        assert errs[hull] <= REL_TOL, (hex(hull), errs[hull], _worst(case, _rel(case, got[hull])))
    assert np.abs(got[STAGED].astype(np.float64) / got[DIRECT] - 1).max() <= 2 * REL_TOL


def test_the_device_order_is_the_order_the_cpu_tests_walk():
    """The coverage statements of tests/test_mixed_cases_cpu.py are about the stable cell-key order: the device's, slot by
    slot, for a case whose cells hold up to 8 particles and one whose waves cross far-apart droplets."""
    for case in (mc.d_block(), mc.g_droplets()):
        with capi.Context(case.pos.shape[0], params=_params(case)) as c:
            c.set_precision(True)
            c.upload(case.pos, np.zeros_like(case.pos))
            c.hash(); c.sort()
            order, keys = c.order(), c.keys()
        L = mc.layout(case)
        assert np.array_equal(order, L.order), case.name
        assert np.array_equal(keys, L.keys), case.name


def _bar(case, rho, what):
    rel = _rel(case, rho)
    mx, rms = np.abs(rel).max(), np.sqrt(np.mean(rel ** 2))
    print(f"{case.name} {what}: max {mx:.3e} rms {rms:.3e}")
    assert mx <= RHO_MAX and rms <= RHO_RMS, (case.name, what, mx, rms, _worst(case, rel))
    return rel


def test_generic_droplets_in_every_pass_and_the_fp32_gather():
    case = mc.g_droplets()
    got = _densities(case, (DEFAULT,))
    assert np.array_equal(got["order"], mc.layout(case).order)
    assert np.abs(_rel(case, got["fp32"])).max() <= REL_TOL
    rel = _bar(case, got[DEFAULT], "default")
    pass_no = mc.by_creation_index(case, mc.passes(case)[0])
    for k in (1, 2, 3):
        print(f"pass {k}: {np.count_nonzero(pass_no == k)} particles, max {np.abs(rel[pass_no == k]).max():.3e}")
    gather = pass_no == mc.GATHER
    print(f"gather: {np.count_nonzero(gather)} particles, max {np.abs(rel[gather]).max():.3e}")
    assert np.count_nonzero(gather) >= 200
    assert np.abs(rel[gather]).max() <= REL_TOL, "the lanes left after three passes sum in fp32"


@pytest.mark.parametrize("edge", [1.25, 4, 12])
def test_generic_lattice_in_wide_cells(edge):
    """include/sph_hip.h: the mixed pass takes cells up to 12 h wide.  What a wide cell changes is how far the staged y and z
    of a row's candidates lie from the reference point (two cell edges and more, fp16 ulp 2^-6 h) -- but only a candidate
    within h of a target contributes, the target lies within 6 h of the reference, and up to 8 h the ulp is 2^-8 h."""
    case = mc.g_wide(edge)
    got = _densities(case, (STAGED, DIRECT))
    assert np.abs(_rel(case, got["fp32"])).max() <= REL_TOL
    for hull, what in ((STAGED, "staged"), (DIRECT, "direct")):
        _bar(case, got[hull], what)


def test_generic_heavy_cell():
    """600 particles in one cell: the direct walk sums a whole row of ~600 candidates, nearly all within h, in ONE pair of
    fp16 accumulators (ulp 0.125 above 128); the staged walk hands its pair to fp32 after every piece of 128."""
    case = mc.g_heavy()
    got = _densities(case, (STAGED, DIRECT))
    assert np.abs(_rel(case, got["fp32"])).max() <= 4 * REL_TOL          # test_everything_in_one_cell's bar for this input
    for hull, what in ((STAGED, "staged"), (DIRECT, "direct")):
        _bar(case, got[hull], what)

"""CPU: the float64 model of tests/sph_model.py against the bit-exact float32 oracle at the reference's constants, phase by
phase on the committed fixtures.  The model is what tests/test_gpu_physics_params.py holds the GPU to at OTHER parameters;
this keeps it honest where the oracle can speak.  Each phase is fed the oracle's own inputs for that phase."""
import numpy as np
import pytest

import sph_model
from conftest import load_golden
from oracle import oracle


def _rel(a, b, scale=None):
    scale = float(np.abs(b).max()) if scale is None else scale
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) / max(scale, 1e-30)


@pytest.mark.parametrize("name", ["c1_jitter", "random_clump", "c1_flow"])
def test_model_matches_the_oracle_at_default_parameters(name):
    g = load_golden(name)
    dt = float(g["dt"])
    m = sph_model.Model(sph_model.reference_params(g["box"], g["grid"]))
    o = oracle.Oracle(g["pos"], g["vel"], g["box"], g["grid"], oracle.CELL_LINEAR)
    try:
        for step in range(2):
            s0 = o.state()
            pairs = m.pairs(s0["pos"])
            o.map_zindex(); o.sort(); o.construct_bgrid()
            o.compute_densities()
            rho, p = m.density(s0["pos"], pairs)
            assert _rel(rho, o.by_index("density")) <= 1e-5
            assert _rel(p, o.by_index("pressure")) <= 1e-5
            o.compute_forces(); o.particle_collisions()
            fp, fv = m.forces(s0["pos"], s0["vel"], o.by_index("density"), o.by_index("pressure"), pairs)
            fscale = float(max(np.abs(o.by_index("force_press")).max(), np.abs(o.by_index("force_visc")).max()))
            assert _rel(fp, o.by_index("force_press"), fscale) <= 2e-5
            assert _rel(fv, o.by_index("force_visc"), fscale) <= 2e-5
            dv, count = m.collide(s0["pos"], s0["vel"], pairs)
            assert np.array_equal(count, o.by_index("collision_count"))
            assert count.sum() > 0 or name == "c1_jitter"
            dvs = max(float(np.abs(o.by_index("delta_velocity")).max()), 1e-12)
            assert _rel(dv, o.by_index("delta_velocity"), dvs) <= 2e-5
            f = o.by_index("force_press").astype(np.float64) + o.by_index("force_visc")
            out = m.integrate(s0["pos"], s0["vel"], o.by_index("density"), f, o.by_index("delta_velocity"), dt)
            o.integrate(dt)
            s1 = o.state()
            bad = sph_model.integrate_mismatch(out, s1["pos"], s1["vel"], 1e-6 * float(np.max(g["box"])),
                                               1e-5 * float(np.abs(s1["vel"]).max()))
            assert bad.size == 0, (step, bad[:8])
    finally:
        o.close()


def test_model_stencil_misses_what_the_reference_misses():
    """Cells smaller than h: a neighbour two cells away is within h but outside the 27-cell stencil, so it adds nothing
    (the reference's truncation, kept by the model)."""
    p = sph_model.reference_params((2, 2, 2), (64, 64, 64))          # cell edge 1/32 < h = 0.1
    m = sph_model.Model(p)
    pos = np.array([[0.001, 0.001, 0.001], [0.07, 0.001, 0.001]], np.float32)
    rho, _ = m.density(pos)
    self_only = 65 * 315 / (65 * np.pi * 0.1 ** 9) * (0.1 ** 2) ** 3
    assert rho == pytest.approx([self_only, self_only], rel=1e-6)
    p.grid = [16, 16, 16]                                             # cell edge 1/8 >= h: the pair is seen
    assert sph_model.Model(p).density(pos)[0][0] > 1.001 * self_only


def test_model_viscosity_zero_is_well_defined():
    """The reference's formulas at VISC = 0: no viscous force, the pressure force unchanged."""
    g = load_golden("random_clump")
    p = sph_model.reference_params(g["box"], g["grid"])
    m = sph_model.Model(p)
    rho, pr = m.density(g["pos"])
    fp, fv = m.forces(g["pos"], g["vel"], rho, pr)
    p.viscosity = np.float32(0)
    fp0, fv0 = sph_model.Model(p).forces(g["pos"], g["vel"], rho, pr)
    assert np.array_equal(fp0, fp) and not fv0.any() and np.abs(fv).max() > 0

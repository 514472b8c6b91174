"""One step of a context, phase by phase, against the float64 model of tests/sph_model.py -- TEST INFRASTRUCTURE shared by
tests/test_gpu_physics_params.py (non-default parameters) and tests/test_gpu_context_walk.py (the physics anchor of the state
walk).  Each phase is fed the GPU's own inputs for that phase, so errors do not compound.  Bars are those of
tests/test_gpu_parity.py (fp32); collision counts are exact."""
import numpy as np

import sph_model

REL_TOL, FORCE_REL_TOL, POS_TOL_PER_BOX = 1e-5, 2e-5, 1e-6          # tests/test_gpu_parity.py

# where the first step may begin: the phases in front of it have already run on the context
STARTS = ("hash", "sort", "cells", "density", "force", "integrate")


def close(name, a, b, rel, scale=None):
    scale = float(np.abs(b).max()) if scale is None else scale
    err = float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    assert np.isfinite(a).all(), f"{name}: not finite"
    assert err <= rel * max(scale, 1e-30), f"{name}: max abs err {err:.3e} > {rel:g} * {scale:.3e}"


def phases_vs_model(c, p, coll, dt, steps=2, start="hash", p_keys=None):
    """`steps` phased steps of context c, each phase against the model fed the GPU's inputs.

    start: the phase the FIRST step begins with (a context that is between two phases goes on where it is; the phases that
    have already run are not checked).  p_keys: the parameters the cell keys in use were computed with, where they are not p
    (sph_set_params with another box between two phases of the first step): the pair kernels walk the 27 cells around a
    particle's KEY, so the model's stencil is that of those cells, and everything else -- kernels, walls -- is p's."""
    box = float(np.max(np.array(p.box_max[:]) - np.array(p.box_min[:])))
    for k in range(steps):
        at = STARTS.index(start) if k == 0 else 0
        s0 = c.download(want=("pos", "vel"))
        m = sph_model.Model(p, None if coll is None else (c.colliders()["centers"], coll[1], coll[2]))
        pairs = (sph_model.Model(p_keys) if (k == 0 and at > 0 and p_keys is not None) else m).pairs(s0["pos"])
        if at <= 0: c.hash()
        if at <= 1: c.sort()
        if at <= 2: c.build_cells()
        if at <= 3: c.density()
        st = c.download(want=("density", "pressure"))
        if at <= 3:
            rho, pr = m.density(s0["pos"], pairs)
            close("density", st["density"], rho, REL_TOL)
            close("pressure", st["pressure"], pr, REL_TOL)
        if at <= 4:
            c.force(); c.collide()
        f = c.download_forces()
        count = f["count"]
        if at <= 4:
            fp, fv = m.forces(s0["pos"], s0["vel"], st["density"], st["pressure"], pairs)
            fscale = float(max(np.abs(fp).max(), np.abs(fv).max()))
            close("f_press", f["fpress"], fp, FORCE_REL_TOL, fscale)
            close("f_visc", f["fvisc"], fv, FORCE_REL_TOL, fscale)
            dv, count = m.collide(s0["pos"], s0["vel"], pairs)
            assert np.array_equal(f["count"], count), "collision counts"
            close("delta_v", f["dv"], dv, FORCE_REL_TOL, max(float(np.abs(dv).max()), 1e-12))
        out = m.integrate(s0["pos"], s0["vel"], st["density"], f["fpress"].astype(np.float64) + f["fvisc"], f["dv"], dt)
        c.integrate(dt)
        s1 = c.download(want=("pos", "vel"))
        assert np.isfinite(s1["pos"]).all() and np.isfinite(s1["vel"]).all()
        bad = sph_model.integrate_mismatch(out, s1["pos"], s1["vel"], POS_TOL_PER_BOX * box,
                                           REL_TOL * float(np.abs(out[1]).max()))
        assert bad.size == 0, ("integrate", bad.size, bad[:8], s1["pos"][bad[:2]], out[0][bad[:2]], s1["vel"][bad[:2]], out[1][bad[:2]])
        yield count

"""CPU: the oracle against the REFERENCE's own code (oracle/_ref/sph_ref = SPH/particleSystem.cpp compiled where it
lies).  What the binary produced for these inputs is stored in tests/golden/oracle_vs_ref.npz (oracle/make_golden.py
vs_ref), so the pin holds wherever the tests run; where oracle/_ref was built, the binary is also run live and must
reproduce the stored records bit for bit."""
import numpy as np
import pytest

from conftest import bits, load_golden
from gpufluidsimulator_amd import ic
from oracle import oracle, refio


def _live_matches(recs, stored):
    """Where the reference binary exists: its records for the same inputs are the stored ones."""
    for key, want in stored.items():
        assert np.array_equal(recs[key].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), key


@pytest.mark.parametrize("n_side,box,grid,jitter", [(8, 2.0, 32, True), (12, 4.0, 64, False), (20, 4.0, 64, True)])
def test_fresh_inputs_bit_exact_per_phase(n_side, box, grid, jitter):
    g, tag = load_golden("oracle_vs_ref"), f"n{n_side}"
    pos, vel = ic.dam_break_lattice((n_side,) * 3, (box,) * 3, jitter=jitter)
    assert np.array_equal(bits(pos), bits(g[f"{tag}_pos"])) and np.array_equal(bits(vel), bits(g[f"{tag}_vel"]))
    recs = {(k, s): g[f"{tag}_s{s}_{k}"] for s in (1, 2, 3) for k in ("order", "state")}
    if refio.available():
        live, _ = refio.run_ref(pos, vel, box, grid, ic.DEFAULT_DT, 3, phases=True)
        _live_matches(live, recs)
    o = oracle.Oracle(pos, vel, box, grid)
    for s in (1, 2, 3):
        o.map_zindex(); o.sort(); o.apply_order(recs[("order", s)])
        o.construct_bgrid(); o.construct_grid_array()
        o.compute_densities(); o.compute_forces(); o.particle_collisions(); o.integrate(ic.DEFAULT_DT)
        st = recs[("state", s)]
        assert np.array_equal(bits(o.by_index("position")), bits(st[:, 0:3]))
        assert np.array_equal(bits(o.by_index("velocity")), bits(st[:, 3:6]))
        assert np.array_equal(bits(o.by_index("density")), bits(st[:, 6]))
        assert np.array_equal(bits(o.by_index("pressure")), bits(st[:, 7]))
    o.close()


def test_reference_is_thread_count_invariant():
    g = load_golden("oracle_vs_ref")
    r1, r8 = g["threads1_s5_state"], g["threads4_s5_state"]
    if refio.available():
        pos, vel = ic.dam_break_lattice((10,) * 3, (2.0,) * 3, jitter=True)
        live1, _ = refio.run_ref(pos, vel, 2.0, 32, ic.DEFAULT_DT, 5, threads=1)
        live8, _ = refio.run_ref(pos, vel, 2.0, 32, ic.DEFAULT_DT, 5, threads=4)
        _live_matches(live1, {("state", 5): r1})
        _live_matches(live8, {("state", 5): r8})
    assert np.array_equal(bits(r1), bits(r8))

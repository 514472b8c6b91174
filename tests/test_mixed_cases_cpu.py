"""CPU: the cases of tests/mixed_cases.py reach the bars and the walks that tests/test_gpu_mixed_walks.py relies on.

(a) On the dyadic cases the packed fp16 arithmetic of `k_density_h`, restated in numpy float16, gives the float64 model's
    density exactly -- so holding the kernel to the fp32 bar there is fair, and a miss means a dropped, doubled or misplaced
    candidate.
(b) The pass rule of the kernel, restated over the waves of the stable cell-key order, sends enough particles WITH neighbours
    through passes 2 and 3 and the fp32 gather, and the staged walk meets both copies, odd and even lengths, short rows and
    many piece edges.  The GPU test asserts that the device's order is this order, so (b) holds for what the GPU runs.
(c) The tower (mc.d_tower) is a dyadic case at every one of its shifts, one model step takes it from a shift to the next with
    no force at all, and its density does not depend on the shift: what tests/test_gpu_slabs_mixed.py holds a moving fluid
    in slabs to."""
import numpy as np
import pytest

import mixed_cases as mc


TOWER = list(range(mc.TOWER_SHIFTS + 1))


def _dyadic_site_properties(case, n_max=3000, sites_max=72):
    assert case.pos.dtype == np.float32 and case.pos.shape[0] <= n_max
    k = (case.pos.astype(np.float64) - mc.DY_MIN) / (mc.DY_H / 2) - 0.5
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0, "every particle on a site, exactly"
    assert np.unique(k, axis=0).shape[0] == k.shape[0], "one particle per site"
    hi = (np.array(case.params.box_max, np.float64) - mc.DY_MIN) / (mc.DY_H / 2)
    assert (k < hi).all() and hi.max() <= sites_max               # a box of at most 36 h: (p - ref) / h below 64
    total, row_max, coord_max, fine_max = mc.packed_f16_sums(case)
    assert fine_max == 0.0, "the fine x part is 0"
    assert coord_max < 64 and row_max < 32
    assert np.array_equal(total * 64, np.rint(total * 64)), "every term a multiple of 1/64"
    return k


@pytest.mark.parametrize("name", list(mc.DYADIC))
def test_dyadic_sites_have_the_properties_the_bar_rests_on(name):
    _dyadic_site_properties(mc.DYADIC[name]())


@pytest.mark.parametrize("shift", TOWER)
def test_tower_sites_have_the_properties_the_bar_rests_on(shift):
    """The tower has 11,167 particles in a box 48 h tall (96 sites); what the exactness needs -- staged coordinates below 64,
    row sums below 32 -- is asserted as for every other dyadic case."""
    case = mc.d_tower(shift)
    k = _dyadic_site_properties(case, n_max=12000, sites_max=96)
    assert case.pos.shape[0] == mc.d_tower(0).pos.shape[0] == 11167
    assert k[:, 2].min() == 8 + shift and k[:, 2].max() == 79 + shift and k[:, 2].max() + 2 < 96, "2 sites below the top wall"
    per_layer = np.bincount(mc.layout(case).cells[:, 2], minlength=48)
    assert per_layer[per_layer > 0].min() >= 100, "every occupied cell layer is a real boundary layer"


@pytest.mark.parametrize("shift", TOWER)
def test_packed_fp16_arithmetic_is_exact_on_the_tower(shift):
    case = mc.d_tower(shift)
    got = mc.by_creation_index(case, mc.scale64(case) * mc.packed_f16_sums(case)[0])
    want = mc.model_density(case)
    assert want.min() > 0 and want.max() < float(case.params.rest_density), "rest density above every density: pressure 0"
    assert np.abs(got / want - 1).max() <= 1e-6


def test_tower_density_is_the_same_for_every_shift():
    """Cells of edge h: the 27-cell stencil holds every candidate within h wherever the block stands, and every term of the
    float64 sum is a dyadic number that adds exactly.  So the model density by creation index does not depend on the shift,
    and the GPU tests compare every step with ONE array."""
    want = mc.model_density(mc.d_tower(0))
    for shift in TOWER[1:]:
        assert np.array_equal(mc.model_density(mc.d_tower(shift)), want), shift


@pytest.mark.parametrize("shift", TOWER[:-1])
def test_one_model_step_moves_the_tower_one_site(shift):
    """tests/sph_model.py in float64, one step of TOWER_DT at TOWER_VEL: no pressure, no force, no collision, and the next
    shift's sites exactly."""
    import sph_model
    case, nxt = mc.d_tower(shift), mc.d_tower(shift + 1)
    m = sph_model.Model(case.params)
    vel = mc.tower_velocity(case.pos.shape[0])
    pairs = m.pairs(case.pos)
    rho, prs = m.density(case.pos, pairs)
    fp, fv = m.forces(case.pos, vel, rho, prs, pairs)
    dv, count = m.collide(case.pos, vel, pairs)
    x, v, alts = m.integrate(case.pos, vel, rho, fp + fv, dv, mc.TOWER_DT)
    assert not prs.any() and not fp.any() and not fv.any() and not count.any() and not dv.any()
    assert not alts, "no particle near a wall"
    assert np.array_equal(v, vel.astype(np.float64))
    assert np.array_equal(x, nxt.pos.astype(np.float64))
    assert np.array_equal(x.astype(np.float32), nxt.pos)
    # a particle crosses a cell layer every second step: about half of them in every step
    assert np.count_nonzero(m.cells(case.pos)[:, 2] != m.cells(nxt.pos)[:, 2]) > 4000


def test_the_tower_is_sharp():
    """One dropped or doubled candidate changes a normalised sum by at least 1/64: relative to the largest sum of the case
    that is far above the 1e-5 bar."""
    total = mc.packed_f16_sums(mc.d_tower(0))[0]
    assert (1 / 64) / total.max() > 1e-4


@pytest.mark.parametrize("name", list(mc.DYADIC))
def test_packed_fp16_arithmetic_is_exact_on_the_dyadic_cases(name):
    case = mc.DYADIC[name]()
    total = mc.packed_f16_sums(case)[0]
    got = mc.by_creation_index(case, mc.scale64(case) * total)
    want = mc.model_density(case)
    assert want.min() > 0
    assert np.abs(got / want - 1).max() <= 1e-6


def test_the_fp16_restatement_notices_one_candidate():
    """The restatement is sharp: a generic case is NOT exact in it (so (a) is a property of the dyadic sites, not of the
    restatement), and stays within the mixed bar."""
    case = mc.g_droplets()
    rel = mc.by_creation_index(case, mc.scale64(case) * mc.packed_f16_sums(case)[0]) / mc.model_density(case) - 1
    assert 1e-5 < np.abs(rel).max() <= 2e-2


@pytest.mark.parametrize("make", [mc.d_droplets, mc.g_droplets], ids=["D-droplets", "G-droplets"])
def test_droplets_reach_every_pass_and_the_gather_with_real_neighbours(make):
    case = make()
    pass_no = mc.by_creation_index(case, mc.passes(case)[0])
    nb = mc.neighbours_within_h(case)
    assert nb.min() >= 1, "every particle has a real neighbour"
    crowd = nb >= 3
    assert np.count_nonzero(crowd & (pass_no == mc.GATHER)) >= 200
    assert np.count_nonzero(crowd & (pass_no == 2)) >= 100
    assert np.count_nonzero(crowd & (pass_no == 3)) >= 100
    # five or more far-apart groups in most waves: a wave that reaches the gather has used its three references
    L = mc.layout(case)
    slots_pass = mc.passes(case)[0]
    waves = [slots_pass[w:w + mc.WAVE] for w in range(0, L.order.size, mc.WAVE)]
    assert sum(1 for w in waves if (w == mc.GATHER).any()) >= len(waves) // 2


def test_g_droplets_keep_the_order_of_d_droplets():
    a, b = mc.layout(mc.d_droplets()), mc.layout(mc.g_droplets())
    assert np.array_equal(a.order, b.order) and np.array_equal(a.keys, b.keys)
    assert np.array_equal(mc.passes(mc.d_droplets())[0], mc.passes(mc.g_droplets())[0])


def test_d_block_meets_both_copies_and_every_tail():
    case = mc.d_block()
    rel, length, _, _ = mc.staged_segments(case)
    for start in (0, 1):
        for odd in (0, 1):
            assert np.count_nonzero((rel % 2 == start) & (length % 2 == odd)) >= 100, (start, odd)
    assert np.count_nonzero(length < 8) >= 100                        # shorter than one unrolled group of 4 pairs
    assert np.count_nonzero((length % 8 == 0) & (length > 0)) >= 100  # no tail at all
    assert np.count_nonzero(length % 8 == 1) >= 50                    # the tail is the odd candidate alone
    cells = np.unique(mc.layout(case).keys, return_counts=True)[1]
    assert cells.min() == 1 and cells.max() == 8
    assert mc.layout(case).order.size % mc.WAVE != 0                  # the last wave is partly idle


@pytest.mark.parametrize("edge", [4, 12])
def test_d_wide_rows_are_long(edge):
    case = mc.d_wide(edge)
    L = mc.layout(case)
    longest = int((L.hi - L.lo).max())
    rel, length, _, edges = mc.staged_segments(case)
    assert 2300 <= case.pos.shape[0] <= 2700
    if edge == 12:
        assert longest > 1500
        assert edges.max() >= 8 and np.count_nonzero(edges >= 8) >= 1000      # rows across at least 8 piece edges
        assert np.count_nonzero((rel == 0) & (length < mc.PIECE)) >= 1000     # ranges that end inside a piece
        assert np.count_nonzero((rel > 0) & (length < mc.PIECE)) >= 100       # and some that begin inside one as well
        assert np.unique(L.keys).size == 8                                    # the block straddles a cell corner
    else:
        assert longest > 512 and (L.hi - L.lo)[(L.hi - L.lo) > 0].min() <= 512  # both sides of the default direct-walk threshold
        assert np.unique(L.keys).size == 27
    assert (rel % 2 == 1).any() and (rel % 2 == 0).any() and (length % 2 == 1).any()


@pytest.mark.parametrize("edge", mc.WIDE_EDGES)
def test_g_wide_straddles_a_cell_corner(edge):
    case = mc.g_wide(edge)
    p = case.params
    assert case.pos.shape[0] == 2000
    width = (np.array(p.box_max, np.float64) - np.array(p.box_min, np.float64)) / np.array(p.grid) / float(p.h)
    assert np.allclose(width, edge, rtol=1e-6)
    c = mc.layout(case).cells
    for a in range(3):
        assert np.unique(c[:, a]).size >= 2, "cells on either side of the corner on every axis"
    assert (case.pos > np.array(p.box_min)).all() and (case.pos < np.array(p.box_max)).all()


def test_g_heavy_is_one_cell():
    case = mc.g_heavy()
    assert case.pos.shape[0] == 600 and np.unique(mc.layout(case).keys).size == 1
    assert mc.neighbours_within_h(case).min() >= 300

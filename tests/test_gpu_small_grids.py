"""GPU: tiny and degenerate grids (tests/small_grids.py) -- 1, 2 and 3 cells per axis, a cell edge below h, key widths of 1,
8 and 9 bits, slabs without an interior, the reference's seam at gridDim 1, 2 and 4.

Everywhere else the suite runs on grids of 18 or more cells per axis with a cell edge of about h.  There a candidate that
lane_rows wrongly keeps from across a face is more than h away and adds exactly zero; here it is a particle counted twice (1 or
2 cells per axis) or a neighbour the stencil must not have (3 cells of 0.09).  The one-pass radix plans (1 x 8 and 1 x 9 bits:
the first pass is also the last one), the key decode on axes of 1, 2 and 3 cells and the clamp of cell_coord run nowhere else.

  A  hash against the float32 numpy statement, array_equal, on faces, walls and beyond them; the keys the fused step's
     integrate epilogue leaves against the numpy keys of the positions it leaves;
  B  the full sort and the merge path against numpy (tests/sort_reference.py) at the one-pass plans;
  C  the pair kernels against the float64 model (tests/sph_model.py) at the bars of tests/phase_checks.py; fused against
     phased; the direct walk against the staged one, bit for bit;
  D  slabs of two owned layers and slabs with one-row layers against the one-context run, bit for bit;
  E  the reference's own entry points (include/sph_compat_seam.h) against the oracle's integers and a native context's bits.

The bars of C are the project's, not new ones.  On the CPU the same ordered float32 sums of these cases (up to 1,536 same-cell
candidates per particle on g111) stay within 1.1e-6 of the float64 density and within 6.2e-7 of the force scale, so neither the
1e-5 density bar nor the 2e-5 force bar had to be measured anew.  The file's 189 tests take 9.7 s on an MI355X.
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsph_hip.so is loaded: one HIP runtime per process (capi.load)

import small_grids as sg
import sort_reference as sr
import test_gpu_slabs as tgs
import test_gpu_sort_reference as tsr
from conftest import bits
from gpufluidsimulator_amd import capi, slab
from oracle import oracle
from phase_checks import close, phases_vs_model

pytestmark = pytest.mark.gpu

DT = 5e-7
FUSED_POS, FUSED_VEL = 1e-7, 2e-6                                     # tests/test_gpu_physics_params.py: fused vs phased
F = np.float32


def _params(gid):
    grid, box, _ = sg.GRIDS[gid]
    return sg.set_bounds(capi.default_params(box, grid), gid)


# ---- A: the hash, exactly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", list(sg.GRIDS))
def test_hash_equals_numpy_on_faces_walls_and_beyond(gid):
    """k_hash against floor(((p - bmin) / bdim) * g) clipped to the grid, in float32: cell centres, every interior face with its
    float32 neighbours on either side, box_min and box_max themselves, up to one cell edge outside the box, random points."""
    grid = sg.GRIDS[gid][0]
    lo, hi = sg.bounds(gid)
    pos = sg.hash_positions(gid)
    with capi.Context(pos.shape[0], params=_params(gid)) as c:
        c.upload(pos, np.zeros_like(pos))
        c.hash()
        got = c.keys()
    want = sg.np_keys(pos, lo, hi, grid)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, pos[bad[:4]], got[bad[:4]], want[bad[:4]])


@pytest.mark.parametrize("gid", list(sg.GRIDS))
def test_keys_of_the_integrate_epilogue_equal_numpy(gid):
    """One fused step of a fast cloud: the force pass's integrate epilogue writes the keys of the NEXT sort.  After the step
    sph_hash finds them fresh and launches no k_hash (launch_hash: keys_fresh), so c.keys() shows the epilogue's keys, slot by
    slot beside the positions of download_owned."""
    grid = sg.GRIDS[gid][0]
    lo, hi = sg.bounds(gid)
    pos, vel = sg.moving_cloud(gid)
    with capi.Context(pos.shape[0], params=_params(gid)) as c:
        c.upload(pos, vel)
        c.step(DT, 1)
        c.hash()
        got = c.keys()
        p1, _, idx = c.download_owned()
    assert np.array_equal(np.sort(idx), np.arange(pos.shape[0])) and np.isfinite(p1).all()
    assert np.all(p1 >= lo) and np.all(p1 <= hi)
    want = sg.np_keys(p1, lo, hi, grid)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, p1[bad[:4]], got[bad[:4]], want[bad[:4]])
    before = np.empty_like(want)
    before[np.arange(pos.shape[0])] = sg.np_keys(pos, lo, hi, grid)
    assert np.count_nonzero(want != before[idx]) > 0 or np.any(p1 != pos[idx]), "nothing moved"


# ---- B: sort and cell table at the one-pass plans ------------------------------------------------------------------------------
def _sorted_state_mismatches(c, grid, want_keys, want_order):
    """keys, order and the cell table against the reference, and EVERY cell of these small grids through sph_get_cell_range
    (an empty one reads (0, 0)).  A list of differences, empty = exact."""
    out = []
    for what, got, want in (("keys", c.keys(), want_keys), ("order", c.order(), want_order)):
        if not np.array_equal(got, want):
            out.append(tsr._diff(what, got, want))
    wk, ws, wc = sr.cells_expected(want_keys)
    for what, got, want in zip(("cell keys", "cell starts", "cell counts"), c.cells(), (wk, ws, wc)):
        if not np.array_equal(got, want):
            out.append(tsr._diff(what, got, want))
    ranges = {int(k): (int(s), int(s) + int(n)) for k, s, n in zip(wk, ws, wc)}
    for cell in range(int(np.prod(grid))):
        if c.cell_range(cell) != ranges.get(cell, (0, 0)):
            out.append(f"cell {cell} reads {c.cell_range(cell)}, want {ranges.get(cell, (0, 0))}")
    return out


SORT_DISTS = dict(sr.DISTRIBUTIONS, every_cell=sg.every_cell, only_first=sg.only_first, only_last=sg.only_last)
SMALL_N, LARGE_N = (1, 63, 4096, 4097), (262144, 262145, 300001)      # 64 tiles is the last one-group size; then grouped passes
FULL_CASES = ([(g, n, d) for g in sg.SORT_GRIDS for n in SMALL_N for d in ("uniform", "one_cell", "two_extremes", "descending", "skewed")]
              + [(g, n, d) for g in sg.SORT_GRIDS for n in LARGE_N for d in ("uniform", "one_cell")]
              + [(g, n, d) for g in sg.SORT_GRIDS for n in (4097, 300001) for d in ("every_cell", "only_first", "only_last")])


@pytest.mark.parametrize("gid,n,dist", FULL_CASES, ids=[f"{g}-{n}-{d}" for g, n, d in FULL_CASES])
def test_full_sort_against_numpy_at_one_pass_plans(gid, n, dist):
    """The first sort after an upload with one radix pass: that pass is the first one (it reads the upload order) and the last
    one (it leaves the result in the buffers the sort hands on)."""
    grid, box = sg.SORT_GRIDS[gid]
    assert sg.radix_plan(sg.key_bits(grid))[1] == 1
    ncells = int(np.prod(grid))
    cells = SORT_DISTS[dist](n, grid, n)
    keys = sr.keys_of(cells, grid)
    index = np.random.default_rng(n + 1).permutation(n).astype(np.uint32)
    want_keys, want_order = sr.full_sort_expected(keys, index)
    occupied = np.unique(keys)
    if dist == "every_cell":
        assert occupied.size == ncells
    if dist == "only_first":
        assert occupied.tolist() == [0]
    if dist == "only_last":
        assert occupied.tolist() == [ncells - 1]
    with capi.Context(n, box=box, grid=grid) as c:
        c.upload(sr.cell_centres(cells, box, grid), None, index)
        c.hash()
        assert np.array_equal(c.keys(), keys), "hash"
        c.sort()
        c.sync()
        c.build_cells()
        assert _sorted_state_mismatches(c, grid, want_keys, want_order) == []
        st = c.sort_stats()
        assert st["sorts"] == 1 and st["merges"] == 0


class _SmallMergeRun:
    """One context in set_sort_mode(2) on a one-pass grid, taken through rounds of movers (shaped like _MergeRun of
    tests/test_gpu_sort_reference.py).  `cells` (by creation index) and `order` (creation index per slot) are the reference's
    state, advanced in numpy alone; nothing expected comes from the library."""

    def __init__(self, gid, n, seed):
        self.grid, self.box = sg.SORT_GRIDS[gid]
        self.n, self.rng = n, np.random.default_rng(seed)
        self.records, self.forms_seen, self.c = {}, set(), None

    def start(self):
        n, grid, box = self.n, self.grid, self.box
        by_upload = sr.uniform(n, grid, 77)
        index = self.rng.permutation(n).astype(np.uint32)
        self.cells = np.empty_like(by_upload)
        self.cells[index] = by_upload
        want_keys, self.order = sr.full_sort_expected(sr.keys_of(by_upload, grid), index)
        self.c = c = tsr._ctx(n, box, grid, True)
        c.set_sort_mode(2)
        c.upload(sr.cell_centres(by_upload, box, grid), None, index)
        c.hash(); c.sort(); c.sync(); c.build_cells()
        self.hint = 0
        self.records["first sort"] = _sorted_state_mismatches(c, grid, want_keys, self.order)

    def elsewhere(self, old):
        """A random cell of the grid for each row of `old`, never the cell it is in (on two cells: the other one)."""
        nc = int(np.prod(self.grid))
        k = sr.keys_of(old, self.grid).astype(np.int64)
        return sr.cells_of((k + self.rng.integers(1, nc, k.size)) % nc, self.grid)

    def round(self, m, trust):
        c, grid = self.c, self.grid
        name = f"{len(self.records)}: {m} movers behind {self.hint}, {'trusted' if trust else 'both forms'}"
        movers = self.rng.choice(self.n, size=m, replace=False)
        old_keys = sr.keys_of(self.cells, grid)
        self.cells[movers] = self.elsewhere(self.cells[movers])
        new_keys = sr.keys_of(self.cells, grid)
        assert int(np.count_nonzero(new_keys != old_keys)) == m
        forms = tsr._documented_form(self.hint, trust)
        want_keys, self.order = sr.resort_expected(self.order, new_keys)
        c.set_by_index(0, pos=sr.cell_centres(self.cells, self.box, grid))
        if trust:
            c.trust_mover_hint()
        f0, st0 = c.sort_forms(), c.sort_stats()
        c.hash(); c.sort(); c.sync(); c.build_cells()
        out = _sorted_state_mismatches(c, grid, want_keys, self.order)
        st, f1 = c.sort_stats(), c.sort_forms()
        if st["last_movers"] != m:
            out.append(f"last_movers {st['last_movers']}, want {m}")
        if (st["sorts"] - st0["sorts"], st["merges"] - st0["merges"], st["skips"] - st0["skips"]) != (1, 1, 0):
            out.append(f"not one merge: {st0} -> {st}")
        launched = tuple(b - a for a, b in zip(f0, f1))
        if launched != forms:
            out.append(f"forms launched {launched}, want {forms} (hint {self.hint}, trusted {trust})")
        self.forms_seen.add(launched)
        self.hint = m
        self.records[name] = out

    def merge_equals_full(self):
        """The state as the merge context holds it, uploaded in slot order into a context that always runs the full sort."""
        c, grid = self.c, self.grid
        pos, vel, idx = c.download_owned()
        want_keys = sr.keys_of(self.cells, grid)[self.order]
        d = tsr._ctx(self.n, self.box, grid, False)
        try:
            d.upload(pos, vel, idx)
            d.hash(); d.sort(); d.sync(); d.build_cells()
            out = _sorted_state_mismatches(d, grid, want_keys, self.order)
            for what, a, b in (("keys", d.keys(), c.keys()), ("order", d.order(), c.order())):
                if not np.array_equal(a, b):
                    out.append(tsr._diff("full against merge, " + what, a, b))
            for what, a, b in zip(("cell keys", "cell starts", "cell counts"), d.cells(), c.cells()):
                if not np.array_equal(a, b):
                    out.append(tsr._diff("full against merge, " + what, a, b))
            st = d.sort_stats()
            if (st["sorts"], st["merges"]) != (1, 0):
                out.append(f"the second context did not run the full sort: {st}")
        finally:
            d.close()
        self.records["merge equals full"] = out

    def close(self):
        if self.c is not None:
            self.c.close()


# (movers, trusted): behind a count of 0, 5 and 3000 the one-block sort runs alone (also on 12000 and 150000 movers, beyond
# its 8192: `alone`), behind 12000 and more the multi-block passes, and without the hook both forms
MERGE_ROUNDS = [(5, True), (3000, True), (12000, True), (150000, True), (5, True), (3000, False), (12000, True), (12000, False)]


@pytest.mark.parametrize("gid,n", [("g888", 20000), ("g888", 300001), ("g1644", 20000), ("g1644", 300001)])
def test_merge_rounds_against_numpy_at_one_pass_plans(gid, n):
    """The movers' sort with one radix pass, in each of its three forms, round by round against numpy; last_movers exact; the
    last round equals the full sort of the same state element for element."""
    run = _SmallMergeRun(gid, n, seed=n + len(gid))
    try:
        run.start()
        rounds = [(m, t) for m, t in MERGE_ROUNDS if m <= n]
        for m, trust in rounds:
            run.round(m, trust)
        run.merge_equals_full()
    finally:
        run.close()
    assert len(run.records) == len(rounds) + 2
    assert {k: v for k, v in run.records.items() if v} == {}
    assert run.forms_seen == {tsr.BOTH, tsr.SMALL, tsr.PASSES}


def test_merge_rounds_where_every_mover_swaps_between_two_cells():
    """(2, 1, 1): a key of one bit with both keys in use; every mover goes to the only other cell, in the last round all of them."""
    n = 5000
    run = _SmallMergeRun("g211", n, seed=3)
    try:
        run.start()
        for m, trust in [(5, True), (3000, True), (5, True), (3000, False), (n, True)]:
            run.round(m, trust)
        run.merge_equals_full()
    finally:
        run.close()
    assert len(run.records) == 7 and {k: v for k, v in run.records.items() if v} == {}
    assert run.forms_seen == {tsr.BOTH, tsr.SMALL}          # (the passes alone need a count beyond 10240)


# ---- C: the pair kernels against the float64 model -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["block", "clump"])
@pytest.mark.parametrize("gid", list(sg.GRIDS))
def test_pair_kernels_against_the_model(gid, kind):
    """Two phased steps, every phase against the float64 model fed the GPU's own inputs, at the bars of tests/phase_checks.py
    (density and pressure 1e-5, forces 2e-5 of the force scale, collision counts exact).  A candidate kept from across a face
    is here a double count or a neighbour within h, far beyond those bars.  Then three fused steps against three phased ones
    and the direct walk against the staged one.  (float32 ordered sums of these cases against the model, on the CPU: density
    within 1.1e-6, forces within 6.2e-7 of the force scale -- the bars have room at 1,536 same-cell candidates.)"""
    p = _params(gid)
    pos, vel = sg.pair_case(gid, kind)
    n = pos.shape[0]
    with capi.Context(n, params=p) as c:
        c.upload(pos, vel)
        counts = sum(int(k.sum()) for k in phases_vs_model(c, p, None, DT))
    if kind == "clump":
        assert counts > 0, "the clump collides"
    res = {}
    for mode in ("fused", "phased", "direct"):
        with capi.Context(n, params=p) as c:
            if mode == "direct":
                c.set_direct_hull(0)
            c.upload(pos, vel)
            (c.step_phased if mode == "phased" else c.step)(DT, 3)
            res[mode] = c.download()
    a, b = res["fused"], res["phased"]
    box = float(np.max(np.array(p.box_max[:]) - np.array(p.box_min[:])))
    assert np.isfinite(a["vel"]).all() and np.isfinite(a["density"]).all()
    assert np.abs(a["pos"] - b["pos"]).max() <= FUSED_POS * box
    close("fused vs phased velocity", a["vel"], b["vel"], FUSED_VEL)
    assert np.array_equal(a["density"], b["density"])
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(bits(res["direct"][k]), bits(a[k])), f"direct rows: {k}"


# ---- D: thin slabs -------------------------------------------------------------------------------------------------------------
def _one_message_geometry(grid, world):
    """The one-message step needs slabs of four cell layers (include/sph_hip.h: sph_slab_set_protocol): the smallest grid of
    the same layers that it accepts."""
    return grid if grid[2] // world >= 4 else (grid[0], grid[1], 4 * world)


@pytest.mark.parametrize("protocol", [3, 1])
@pytest.mark.parametrize("name", list(sg.SLAB_CASES))
def test_thin_slabs_equal_the_one_context_run(name, protocol):
    """Slabs of two owned layers have no interior: every owned particle is in a boundary layer, every arrival lands beside a
    ghost layer.  Layers of one row (gx = 1 or gy = 1) make the hole arithmetic of the boundary launches run on rows.  Under the
    one-message protocol a case whose slabs are thinner than four layers runs on the smallest grid that protocol accepts; the
    refusal of the thin one is test_one_message_step_refuses_thin_slabs_without_taking_a_step."""
    grid, world = sg.SLAB_CASES[name]
    if protocol == 1:
        grid = _one_message_geometry(grid, world)
    box = sg.slab_box(grid)
    pos, vel = sg.slab_particles(grid)
    steps = 12
    res = tgs._run_slabs(world, box, grid, steps, particles=(pos, vel), transport="local", protocol=protocol)
    ref = tgs._whole_domain(pos, vel, box, grid, steps)
    assert res[0][2] == [r * grid[2] // world for r in range(world + 1)], "even cuts"
    assert sum(r[1]["migrants"] for r in res) > 0
    assert sum(r[3] for r in res) == pos.shape[0]
    assert all(r[1]["protocol"] == protocol for r in res)
    tgs._same_bits(res[0][0], ref)


THIN = [name for name, (grid, world) in sg.SLAB_CASES.items() if grid[2] // world < 4]


@pytest.mark.parametrize("name", THIN)
def test_one_message_step_refuses_thin_slabs_without_taking_a_step(name):
    """sph_slab_set_protocol(s, 1) on a slab of two or three owned layers: SPH_E_STATE with the limit in words, the slab stays
    on the three-group protocol, no step is counted and the particles are the uploaded ones.  A one-layer slab between two
    neighbours is refused by sph_slab_create."""
    assert len(THIN) == 3
    grid, world = sg.SLAB_CASES[name]
    box = sg.slab_box(grid)
    pos, vel = sg.slab_particles(grid)
    cuts = [r * grid[2] // world for r in range(world + 1)]
    layers = slab.cell_layer_of(pos[:, 2], box[2], grid[2])
    L = capi.load()
    hub = capi.LocalHub(world)
    tr = hub.transport(1)
    try:
        mine = np.nonzero((layers >= cuts[1]) & (layers < cuts[2]))[0]
        with capi.Context(mine.size + 1024, params=capi.default_params(box, grid), slab=(cuts[1], cuts[2]), ghost_capacity=4096,
                          ghost_layers=2) as c:
            c.upload(pos[mine], vel[mine], mine.astype(np.uint32))
            h = C.c_void_p()
            capi._check(L.sph_slab_create(C.byref(h), c.h, 1, world, tr, 0))
            try:
                with pytest.raises(capi.SphError, match="at least four cell layers"):
                    capi._check(L.sph_slab_set_protocol(h, 1))
                pr, cnt = (C.c_uint64 * 3)(), (C.c_uint64 * 8)()
                capi._check(L.sph_slab_protocol(h, pr))
                capi._check(L.sph_slab_counters(h, cnt))
                assert (int(pr[0]), int(pr[1])) == (3, 0) and int(cnt[0]) == 0 and not L.sph_slab_failed(h)
                assert int(L.sph_slab_exchanges(h)) == 0
            finally:
                L.sph_slab_destroy(h)
            p1, v1, idx = c.download_owned()
            assert np.array_equal(idx, mine) and np.array_equal(bits(p1), bits(pos[mine])) and np.array_equal(bits(v1), bits(vel[mine]))
        one = np.nonzero(layers == cuts[1])[0]
        with capi.Context(one.size + 1024, params=capi.default_params(box, grid), slab=(cuts[1], cuts[1] + 1),
                          ghost_capacity=4096) as c:
            c.upload(pos[one], vel[one], one.astype(np.uint32))
            h = C.c_void_p()
            with pytest.raises(capi.SphError, match="at least two cell layers"):
                capi._check(L.sph_slab_create(C.byref(h), c.h, 1, world, tr, 0))
            assert not h.value
    finally:
        L.sph_local_transport_destroy(tr)
        hub.close()


# ---- E: the reference's seam at gridDim 1, 2 and 4 -----------------------------------------------------------------------------
# words of the 88-byte Particle (include/sph_compat_seam.h)
W_INDEX, W_POS, W_VEL, W_DV, W_FP, W_FV, W_RHO, W_P, W_COUNT, W_Z = 0, slice(1, 4), slice(4, 7), slice(7, 10), slice(10, 13), \
    slice(13, 16), 17, 18, 20, 21


def _seam(L):
    vp = C.c_void_p
    six = [vp, C.c_uint, vp, C.c_uint, vp, C.c_uint, vp]
    L.cudaMapZIndex.argtypes = [vp, C.c_uint, vp]
    L.cudaSortParticles.argtypes = [vp, C.c_uint]
    L.cudaConstructBGrid.argtypes = [vp, C.c_uint, vp, C.c_uint, vp]
    L.cudaConstructGridArray.argtypes = [vp, C.c_uint, vp, C.c_uint, C.POINTER(vp), C.POINTER(C.c_uint), vp]
    L.cudaComputeDensities.argtypes = L.cudaComputeForces.argtypes = L.cudaParticleCollisions.argtypes = six
    L.cudaIntegrate.argtypes = [vp, C.c_float, vp, C.c_uint, vp]
    L.registerGLBufferObject.argtypes = [C.c_uint, C.POINTER(vp)]
    L.unregisterGLBufferObject.argtypes = [vp]
    L.mapGLBufferObject.argtypes = [C.POINTER(vp)]; L.mapGLBufferObject.restype = vp
    L.sph_compat_vbo_dev.argtypes = [vp, C.POINTER(C.c_size_t)]; L.sph_compat_vbo_dev.restype = vp
    L.copyArrayFromDevice.argtypes = [vp, vp, C.c_size_t]
    L.sph_compat_release.argtypes = [vp]
    for f in ("cudaMapZIndex", "cudaSortParticles", "cudaConstructBGrid", "cudaConstructGridArray", "cudaComputeDensities",
              "cudaComputeForces", "cudaParticleCollisions", "cudaIntegrate", "registerGLBufferObject", "unregisterGLBufferObject",
              "copyArrayFromDevice", "sph_compat_release", "threadSync"):
        getattr(L, f).restype = None
    return L


def _by_index(aos, words):
    """A field of the caller's array, gathered by Particle::index."""
    out = np.empty_like(aos[:, words])
    out[aos[:, W_INDEX]] = aos[:, words]
    return out


def _same(what, seam_words, native):
    a, b = np.ascontiguousarray(seam_words), bits(native) if native.dtype == np.float32 else native.view(np.uint32)
    assert np.array_equal(a.reshape(b.shape), b), what


@pytest.mark.parametrize("g", [1, 2, 4])
def test_seam_at_tiny_grids_against_the_oracle_and_a_native_context(g):
    """cudaMapZIndex .. cudaIntegrate called directly on 700 particles in a 0.3 cube of a 0.5 box, twice over.  The integers --
    Particle::zindex, the sorted order, all of dev_B, dev_B_prime and its size -- against the oracle's Morton-mode phases: 1, 8 and
    56 occupied cells, the fullest with 700, 92 and 64 particles, i.e. 22, 24 and 64 chunks with partial last ones.  The fields
    every later call writes back through m2n, gathered by Particle::index, against what a native context holds after the same
    phase of the same particles, bit for bit; the second round starts from the sorted array, where m2n is no identity."""
    pos, vel = sg.seam_particles()
    n, box = pos.shape[0], (sg.SEAM_BOX,) * 3
    L = _seam(capi.load())
    aos = np.zeros((n, 22), np.uint32)
    aos[:, W_INDEX] = np.arange(n)
    aos[:, W_POS] = pos.view(np.uint32); aos[:, W_VEL] = vel.view(np.uint32)
    aos[:, 16] = F(65.0).view(np.uint32); aos[:, 19] = F(1.0 / 64.0).view(np.uint32)
    prm = np.zeros(18, F)
    prm[7] = 1.0 / 64.0
    prm[8:11] = [-b / 2 for b in box]; prm[11:14] = [b / 2 for b in box]; prm[14:17] = box
    prm.view(np.uint32)[17] = g
    dev = torch.device("cuda", 0)
    d_aos, d_prm = torch.from_numpy(aos.view(np.int32)).to(dev), torch.from_numpy(prm).to(dev)
    b_size = g ** 3
    d_B = torch.full((b_size, 2), -1, dtype=torch.int32, device=dev)
    d_Bp = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
    P, PRM, B, BP = d_aos.data_ptr(), d_prm.data_ptr(), d_B.data_ptr(), d_Bp.data_ptr()
    read = lambda: d_aos.cpu().numpy().view(np.uint32).copy()
    lo, hi = np.full(3, -sg.SEAM_BOX / 2, F), np.full(3, sg.SEAM_BOX / 2, F)
    vbo = C.c_void_p()
    L.registerGLBufferObject(7, C.byref(vbo))
    native = capi.Context(n, box=box, grid=(g,) * 3)
    try:
        native.upload(pos, vel)
        entry = aos                                              # the caller's array as a round finds it
        for rnd in (1, 2):
            e_pos, e_vel = entry[:, W_POS].copy().view(F), entry[:, W_VEL].copy().view(F)
            o = oracle.Oracle(e_pos, e_vel, box, (g,) * 3, oracle.CELL_MORTON)      # array slot = the oracle's index
            o.map_zindex()
            want_z = o.by_index("zindex").copy()
            o.sort(); o.construct_bgrid(); o.construct_grid_array()
            want_sorted = o.particles["zindex"].copy()
            want_B = np.stack([o.B["nParticles"], o.B["start"]], axis=1).astype(np.uint32)
            want_Bp = np.stack([o.Bprime["nParticles"], o.Bprime["start"]], axis=1).astype(np.uint32)
            o.close()
            if rnd == 1:
                assert (int((want_B[:, 0] > 0).sum()), int(want_B[:, 0].max()), want_Bp.shape[0]) == \
                    tuple(sg.SEAM_EXPECT[g][k] for k in ("cells", "fullest", "bprime"))
            # -- the integers
            L.cudaMapZIndex(P, n, PRM)
            L.threadSync()
            got = read()
            assert np.array_equal(got[:, W_Z], want_z), (rnd, "zindex")
            assert np.array_equal(got[:, :W_Z], entry[:, :W_Z]), (rnd, "cudaMapZIndex wrote more than zindex")
            L.cudaSortParticles(P, n)
            L.cudaConstructBGrid(P, n, B, b_size, PRM)
            bp, bp_size = C.c_void_p(BP), C.c_uint(0)
            L.cudaConstructGridArray(P, n, B, b_size, C.byref(bp), C.byref(bp_size), PRM)
            L.threadSync()
            srt = read()
            perm = np.argsort(want_z, kind="stable")             # equal z-indices keep the order of the array (stable)
            assert np.array_equal(srt[:, W_Z], want_sorted), (rnd, "sorted z-indices")
            assert np.array_equal(srt[:, W_INDEX], entry[perm, W_INDEX]), (rnd, "sorted order")
            assert np.array_equal(srt[:, :W_Z], entry[perm, :W_Z]), (rnd, "every struct moved whole")
            assert np.array_equal(d_B.cpu().numpy().view(np.uint32), want_B), (rnd, "dev_B")
            assert bp_size.value == want_Bp.shape[0], (rnd, "dev_B_prime size")
            assert np.array_equal(d_Bp.cpu().numpy().view(np.uint32)[:bp_size.value], want_Bp), (rnd, "dev_B_prime")
            if rnd == 2 and g > 1:       # (one cell: the stable sort leaves the array as it is)
                assert not np.array_equal(srt[:, W_INDEX], np.arange(n)), "the second round's permutation is not the identity"
            # -- the native context: the same particles in creation order, the same phases
            native.hash(); native.sort(); native.build_cells()
            # both contexts hold every cell in the same order when no arrival's source cell ranks differently in the row-major
            # and the Morton numbering; this fixed case has none (the check is numpy's, nothing is taken from the seam)
            rm = np.argsort(sg.np_keys(e_pos, lo, hi, (g,) * 3), kind="stable")
            assert np.array_equal(native.order(), entry[rm, W_INDEX]), (rnd, "the two contexts do not hold the cells in the same order")
            L.cudaComputeDensities(P, n, B, b_size, BP, bp_size.value, PRM)
            L.threadSync()
            a = read()
            native.density()
            st = native.download(want=("density", "pressure"))
            _same((rnd, "density"), _by_index(a, W_RHO), st["density"])
            _same((rnd, "pressure"), _by_index(a, W_P), st["pressure"])
            assert np.array_equal(a[:, :W_RHO], srt[:, :W_RHO]) and np.array_equal(a[:, 19:], srt[:, 19:])
            L.cudaComputeForces(P, n, B, b_size, BP, bp_size.value, PRM)
            L.threadSync()
            a = read()
            native.force()
            f = native.download_forces(collision=False)
            _same((rnd, "force_press"), _by_index(a, W_FP), f["fpress"])
            _same((rnd, "force_visc"), _by_index(a, W_FV), f["fvisc"])
            L.cudaParticleCollisions(P, n, B, b_size, BP, bp_size.value, PRM)
            L.threadSync()
            a = read()
            native.collide()
            f = native.download_forces(force=False)
            _same((rnd, "delta_velocity"), _by_index(a, W_DV), f["dv"])
            assert np.array_equal(_by_index(a, W_COUNT).view(np.int32), f["count"]), (rnd, "collision_count")
            handle = L.mapGLBufferObject(C.byref(vbo))
            L.cudaIntegrate(handle, DT, P, n, PRM)
            L.threadSync()
            a = read()
            native.integrate(DT)
            st = native.download(want=("pos", "vel"))
            _same((rnd, "position"), _by_index(a, W_POS), st["pos"])
            _same((rnd, "velocity"), _by_index(a, W_VEL), st["vel"])
            assert np.array_equal(a[:, W_INDEX], srt[:, W_INDEX]) and np.array_equal(a[:, W_Z], srt[:, W_Z])
            nbytes = C.c_size_t(0)
            vdev = L.sph_compat_vbo_dev(vbo, C.byref(nbytes))
            assert vdev and nbytes.value == n * 16
            pos4 = np.empty((n, 4), F)
            L.copyArrayFromDevice(pos4.ctypes.data, vdev, n * 16)
            want4 = native.positions4()
            assert np.array_equal(bits(pos4), bits(want4)), (rnd, "the VBO")
            assert np.array_equal(bits(pos4[:, :3]), bits(st["pos"])) and np.all(pos4[:, 3] == 1.0)
            entry = a
    finally:
        native.close()
        L.sph_compat_release(P)
        L.unregisterGLBufferObject(vbo)

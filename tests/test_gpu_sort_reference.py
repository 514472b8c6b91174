"""GPU: the radix sort and the merge path of csrc/sph_sort.hip against numpy (tests/sort_reference.py), on both sides of the
switch from the one-group form of the passes (up to 64 tiles of 4096 keys) to the grouped one.

Every bit-for-bit claim of DESIGN.md rests on the sort being the stable sort by cell key.  A wrong rank permutes particles inside
or across cells, and most other tests would see a slightly different fp32 sum order, or nothing.  So here:
  * particles sit at cell centres (the expected key is (z gy + y) gx + x, no rounding question) and carry a random permutation as
    creation indices (a slot number can never pass for an index);
  * only hash(), sort() and build_cells() run (one cell with 3e5 particles would be an O(n^2) pair pass in the neighbour kernels);
  * after every sort c.sync() runs: it raises on the look-back time-out word;
  * keys(), order() and cells() are compared with numpy by np.array_equal, plus a handful of empty cells that must read (0, 0).
Nothing expected is derived from what the library returns: the order the merge rounds start from is the reference's, never
c.order()."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsph_hip.so is loaded: one HIP runtime per process (capi.load)

import sort_reference as sr
from gpufluidsimulator_amd import capi

pytestmark = pytest.mark.gpu


def _box(grid):
    return tuple(g / 16.0 for g in grid)        # cell edge 1/16: centres and faces are exact in float32


def _diff(what, got, want):
    if got.shape != want.shape:
        return f"{what}: {got.shape[0]} entries, want {want.shape[0]}"
    bad = np.flatnonzero(got != want)
    return f"{what}: {bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _mismatches(c, grid, want_keys, want_order, must_be_empty=()):
    """Everything the context shows of its sorted state against the reference: a list of differences (empty = exact)."""
    out = []
    for what, got, want in (("keys", c.keys(), want_keys), ("order", c.order(), want_order)):
        if not np.array_equal(got, want):
            out.append(_diff(what, got, want))
    wk, ws, wc = sr.cells_expected(want_keys)
    for what, got, want in zip(("cell keys", "cell starts", "cell counts"), c.cells(), (wk, ws, wc)):
        if not np.array_equal(got, want):
            out.append(_diff(what, got, want))
    ncells = int(np.prod(grid))
    rng = np.random.default_rng(want_keys.size)
    cand = np.unique(np.concatenate([[0, 1, ncells - 2, ncells - 1], rng.integers(0, ncells, 64)]))
    named = np.asarray(must_be_empty, np.int64)
    assert not np.isin(named, wk).any(), "the test names a cell as empty that the reference has occupied"
    for cell in list(named[:8]) + list(rng.permutation(np.setdiff1d(cand, wk))[:8]):
        if c.cell_range(int(cell)) != (0, 0):
            out.append(f"empty cell {cell} reads {c.cell_range(int(cell))}")
    for j in rng.integers(0, wk.size, 4):         # and a few occupied ones through the same call
        if c.cell_range(int(wk[j])) != (int(ws[j]), int(ws[j]) + int(wc[j])):
            out.append(f"cell {wk[j]} reads {c.cell_range(int(wk[j]))}, want start {ws[j]} count {wc[j]}")
    return out


# ---- (a) the full sort, sizes across the switch ----------------------------------------------------------------------------------
P2x8, P2x9, P3x9, P4x8 = (64, 64, 16), (128, 64, 32), (512, 512, 512), (1024, 1024, 512)      # the radix plans (key bits 16, 18, 27, 29)

FULL_CASES = [
    # one group (chained look-back): the tile edges, and the last one-group size
    (4095, "uniform", P2x8),
    (4096, "one_cell", P2x9),
    (4097, "two_extremes", P2x8),
    (8191, "low_digit_only", P2x9),
    (8192, "high_digit_only", P2x8),
    (8193, "ascending", P2x9),
    (12289, "descending", P2x8),
    (262144, "skewed", P2x9),
    (262144, "one_cell", P2x8),             # 64 full tiles of one digit: the longest chain the one-group form of a full sort sees
    # grouped (groups of 16 tiles, {epoch:19, count:13} words, grid rounded up to a multiple of 8)
    (262145, "uniform", P2x8),              # 65 tiles: the last group holds one tile with one key
    (262145, "one_cell", P2x9),             # ... behind 64 tiles whose 4096 keys share every digit (count = 4096 needs bit 12)
    (300001, "uniform", P2x9),              # 74 tiles: partial tile, partial group, 5 groups (fewer than 8)
    (300001, "skewed", P2x8),
    (300001, "two_extremes", P2x8),
    (528383, "uniform", P3x9),              # 129 tiles: 9 groups, a second ticket round for one XCD only; 1 GiB cell table
    (528383, "one_cell", P3x9),
    (528383, "low_digit_only", P2x9),
    (528383, "high_digit_only", P2x8),
    (1000003, "uniform", P4x8),             # 245 tiles: 16 groups; 4 GiB cell table
    (1000003, "skewed", P4x8),
    (1000003, "ascending", P2x9),
    (1000003, "descending", P2x8),
]


@pytest.mark.parametrize("n,dist,grid", FULL_CASES, ids=[f"{n}-{d}-{'x'.join(map(str, g))}" for n, d, g in FULL_CASES])
def test_full_sort_against_numpy(n, dist, grid):
    """The first sort after an upload is always the full radix sort: hash, stable order and cell table against numpy."""
    box = _box(grid)
    cells = sr.DISTRIBUTIONS[dist](n, grid, n)
    keys = sr.keys_of(cells, grid)
    index = np.random.default_rng(n + 1).permutation(n).astype(np.uint32)
    want_keys, want_order = sr.full_sort_expected(keys, index)
    with capi.Context(n, box=box, grid=grid) as c:
        c.upload(sr.cell_centres(cells, box, grid), None, index)
        c.hash()
        assert np.array_equal(c.keys(), keys), "hash"
        c.sort()
        c.sync()
        c.build_cells()
        assert _mismatches(c, grid, want_keys, want_order) == []
        st = c.sort_stats()
        assert st["sorts"] == 1 and st["merges"] == 0


def test_the_cases_cover_what_they_must():
    """Every size of the table, every distribution on both sides of the switch, every radix plan at a grouped size with
    `uniform` and with a one-digit-heavy distribution; the two big-table grids twice each."""
    one_group = lambda n: -(-n // 4096) <= 64
    assert {n for n, _, _ in FULL_CASES} == {4095, 4096, 4097, 8191, 8192, 8193, 12289, 262144, 262145, 300001, 528383, 1000003}
    for d in sr.DISTRIBUTIONS:
        assert any(dd == d and one_group(n) for n, dd, _ in FULL_CASES), d
        assert any(dd == d and not one_group(n) for n, dd, _ in FULL_CASES), d
    for plan in (P2x8, P2x9, P3x9, P4x8):
        grouped = {d for n, d, g in FULL_CASES if g == plan and not one_group(n)}
        assert "uniform" in grouped and grouped & {"one_cell", "skewed"}, plan
    assert sum(g == P3x9 for _, _, g in FULL_CASES) == 2 and sum(g == P4x8 for _, _, g in FULL_CASES) == 2


# ---- (b) the merge path against numpy at grouped sizes, (c) merge equals full -------------------------------------------------
N_MERGE = 524_325                              # 129 tiles, 8193 chunks of 64 slots: the last chunk holds 37
GRID_M = (128, 128, 64)                        # 20 key bits: three 8-bit passes
BOX_M = _box(GRID_M)
REGION = np.array([[32, 96], [32, 96], [16, 48]])       # the fluid: 131072 cells, four particles per cell -- ties everywhere
CELL_T = (40, 50, 30)                          # gets 100 particles in round 5b (the tie round's destination, one cell on by then)
CELL_E = (5, 40, 31)                           # outside the fluid and never a destination: empty until its round

# the forms sph_sort_forms counts: (both, the one-block sort alone, the multi-block passes alone)
BOTH, SMALL, PASSES = (1, 0, 0), (0, 1, 0), (0, 0, 1)


def _documented_form(hint, trusted):
    """include/sph_hip.h under sph_sort_forms, whole-domain context: new particle data from the caller (set_by_index) means both
    forms for five sorts unless the test hook takes that back; then the count the device last reported decides, with a quarter
    of the one-block sort's capacity (8192) as margin."""
    if not trusted:
        return BOTH
    return SMALL if hint <= 8192 - 2048 else (PASSES if hint > 8192 + 2048 else BOTH)


def _ctx(n, box, grid, merge):
    old = os.environ.get("SPH_SORT_MERGE")
    os.environ["SPH_SORT_MERGE"] = "1" if merge else "0"        # read once, by sph_create
    try:
        return capi.Context(n, box=box, grid=grid)
    finally:
        if old is None:
            del os.environ["SPH_SORT_MERGE"]
        else:
            os.environ["SPH_SORT_MERGE"] = old


def _in_region(rng, m):
    return np.stack([rng.integers(lo, hi, m) for lo, hi in REGION], axis=1).astype(np.int64)


def _elsewhere(rng, old):
    """A random cell of the fluid region for each row of `old`, never the cell it is in."""
    new = _in_region(rng, old.shape[0])
    same = np.all(new == old, axis=1)
    new[same, 0] = REGION[0, 0] + (new[same, 0] - REGION[0, 0] + 1) % (REGION[0, 1] - REGION[0, 0])
    return new


class _MergeRun:
    """One context in set_sort_mode(2) taken through the rounds below; `cells` (by creation index) and `order` (creation index
    per slot) are the reference's state, advanced in numpy alone.  records[name] = the differences of that round ([] = exact)."""

    def __init__(self):
        self.records, self.raised = {}, None
        self.rng = np.random.default_rng(2024)
        n = N_MERGE
        self.cells = _in_region(self.rng, n)
        self.c = None

    def key(self, cell):
        return int(sr.keys_of([cell], GRID_M)[0])

    def start(self):
        n = N_MERGE
        index = self.rng.permutation(n).astype(np.uint32)
        by_upload = self.cells.copy()                   # row i = upload position i
        self.cells = np.empty_like(by_upload)
        self.cells[index] = by_upload                   # row j = creation index j from here on
        want_keys, self.order = sr.full_sort_expected(sr.keys_of(by_upload, GRID_M), index)
        self.c = c = _ctx(n, BOX_M, GRID_M, True)
        c.set_sort_mode(2)                              # the merge path whatever the mover count
        c.upload(sr.cell_centres(by_upload, BOX_M, GRID_M), None, index)
        c.hash(); c.sort(); c.sync(); c.build_cells()
        self.hint = 0                                   # what the device has reported so far: nothing
        self.records["first sort"] = _mismatches(c, GRID_M, want_keys, self.order, [self.key(CELL_E)])

    def round(self, name, movers, new_cells, trust, forms, must_be_empty=()):
        """`movers`: creation indices; they go to `new_cells`.  `trust`: the sort is launched on the count the previous round left
        (the test hook), else with both forms.  `forms`: the sort_forms delta expected."""
        c = self.c
        old_keys = sr.keys_of(self.cells, GRID_M)
        self.cells[movers] = new_cells
        new_keys = sr.keys_of(self.cells, GRID_M)
        want_movers = int(np.count_nonzero(new_keys != old_keys))
        assert want_movers == len(movers), "the round moves a particle into the cell it is in"
        assert forms == _documented_form(self.hint, trust), (name, self.hint, trust)
        want_keys, self.order = sr.resort_expected(self.order, new_keys)
        c.set_by_index(0, pos=sr.cell_centres(self.cells, BOX_M, GRID_M))
        if trust:
            c.trust_mover_hint()
        f0, st0 = c.sort_forms(), c.sort_stats()
        c.hash(); c.sort(); c.sync(); c.build_cells()
        out = _mismatches(c, GRID_M, want_keys, self.order, must_be_empty)
        st, f1 = c.sort_stats(), c.sort_forms()
        if st["last_movers"] != want_movers:
            out.append(f"last_movers {st['last_movers']}, want {want_movers}")
        if (st["sorts"] - st0["sorts"], st["merges"] - st0["merges"], st["skips"] - st0["skips"]) != (1, 1, 0):
            out.append(f"not one merge: {st0} -> {st}")
        if tuple(b - a for a, b in zip(f0, f1)) != forms:
            out.append(f"forms launched {tuple(b - a for a, b in zip(f0, f1))}, want {forms} (hint {self.hint}, trusted {trust})")
        self.hint = want_movers
        self.records[name] = out

    def random_round(self, name, m, trust, forms, into=None):
        movers = self.rng.choice(N_MERGE, size=m, replace=False)
        new = _elsewhere(self.rng, self.cells[movers])
        if into is not None:
            new[: into[1]] = into[0]
        self.round(name, movers, new, trust, forms)

    def slots_round(self, name, slots, dest, trust, forms, must_be_empty=()):
        """The movers are the particles the REFERENCE has in `slots`; dest: one cell for all, or None = anywhere else."""
        movers = self.order[np.asarray(slots, np.int64)].astype(np.int64)
        if dest is not None:
            movers = movers[np.any(self.cells[movers] != np.asarray(dest), axis=1)]
        new = _elsewhere(self.rng, self.cells[movers]) if dest is None else np.tile(np.asarray(dest, np.int64), (len(movers), 1))
        self.round(name, movers, new, trust, forms, must_be_empty)

    def merge_equals_full(self, name):
        """(c): the state as the merge context holds it, uploaded in slot order into a context that always runs the full sort."""
        c = self.c
        pos, vel, idx = c.download_owned()
        want_keys = sr.keys_of(self.cells, GRID_M)[self.order]
        d = _ctx(N_MERGE, BOX_M, GRID_M, False)
        try:
            d.upload(pos, vel, idx)
            d.hash(); d.sort(); d.sync(); d.build_cells()
            out = _mismatches(d, GRID_M, want_keys, self.order)
            for what, a, b in (("keys", d.keys(), c.keys()), ("order", d.order(), c.order())):
                if not np.array_equal(a, b):
                    out.append(_diff("full against merge, " + what, a, b))
            for what, a, b in zip(("cell keys", "cell starts", "cell counts"), d.cells(), c.cells()):
                if not np.array_equal(a, b):
                    out.append(_diff("full against merge, " + what, a, b))
            st = d.sort_stats()
            if (st["sorts"], st["merges"]) != (1, 0):
                out.append(f"the second context did not run the full sort: {st}")
        finally:
            d.close()
        self.records[name] = out

    def run(self):
        n, rng = N_MERGE, self.rng
        self.start()
        # -- stale counts: each round meets the mover count the previous one left (merge_grid_for sizes the passes' grid from it) --
        self.random_round("1: 300000 movers behind a count of 0", 300_000, True, SMALL)     # the one-block sort alone, 37 x its 8192
        self.random_round("2: 300000 movers behind 300000", 300_000, True, PASSES)          # grid 129: grouped, count on the device
        self.random_round("3: 5 movers behind 300000", 5, True, PASSES)                     # grouped grid, one partial tile
        # behind a count of 5 the documented rule launches the one-block sort ALONE when the count is trusted (round 1 is that
        # case); the one-group form of the passes with tens of tiles is what a sort WITHOUT the hook gets: both forms, grid 64
        self.random_round("4: 150000 movers behind 5, both forms", 150_000, False, BOTH)
        self.random_round("5a: 150000 movers behind 150000", 150_000, True, PASSES)         # grid 89 (grouped, 96 blocks), 37 tiles
        self.random_round("5b: 500000 movers behind 150000", 500_000, True, PASSES, into=(CELL_T, 100))   # grid 89, 123 tiles arrive
        # everyone one cell along x, towards the middle of the region: m = n
        step = np.where(self.cells[:, 0] < 64, 1, -1)
        new = self.cells.copy()
        new[:, 0] += step
        self.round("6: all n movers behind 500000", np.arange(n), new, True, PASSES)
        self.merge_equals_full("merge equals full after round 6")
        # -- ties: 20000 movers from slots all over the range into one cell with ~100 residents --
        keys, counts = np.unique(sr.keys_of(self.cells, GRID_M), return_counts=True)
        tie_cell = sr.cells_of(keys[[np.argmax(counts)]], GRID_M)[0]
        assert 90 <= counts.max() <= 130 and abs(int(tie_cell[0]) - CELL_T[0]) == 1, "the tie cell is CELL_T's neighbour"
        self.slots_round("ties: 20000 movers into a cell with 100 residents", np.linspace(0, n - 1, 20_000).astype(np.int64),
                         tuple(tie_cell), True, PASSES)
        # -- the same into a cell that was empty (both forms, grid 64: the one-group passes take the 20000) --
        assert not np.any(np.all(self.cells == np.asarray(CELL_E), axis=1))
        self.slots_round("empty destination: 20000 movers into an empty cell", np.linspace(7, n - 8, 20_000).astype(np.int64),
                         CELL_E, False, BOTH)
        # -- whole source cells are emptied: every particle of ~3000 cells leaves for cells that stay occupied --
        by_index = sr.keys_of(self.cells, GRID_M)
        keys, counts = np.unique(by_index, return_counts=True)
        small = rng.permutation(np.flatnonzero(counts <= 8))
        sources = keys[small[: np.searchsorted(np.cumsum(counts[small]), 12_000) + 1]]
        movers = np.flatnonzero(np.isin(by_index, sources))
        stay = keys[~np.isin(keys, sources)]
        dest = sr.cells_of(rng.choice(stay, size=movers.size), GRID_M)
        self.round("emptied source cells", movers, dest, True, PASSES, must_be_empty=sources[:8])
        # -- one aligned slot run: whole 64-slot chunks and whole tiles of set mask bits --
        self.slots_round("aligned run of three tiles", np.arange(4096 * 50, 4096 * 53), None, False, BOTH)
        # -- slot 0, slot n - 1 and the last partial chunk (the one-block sort takes the 38 of them beside the passes) --
        self.slots_round("ends: slot 0 and the last partial chunk", np.concatenate([[0], np.arange(n - n % 64, n)]), None, False, BOTH)

    def close(self):
        if self.c is not None:
            self.c.close()


ROUNDS = ["first sort", "1: 300000 movers behind a count of 0", "2: 300000 movers behind 300000", "3: 5 movers behind 300000",
          "4: 150000 movers behind 5, both forms", "5a: 150000 movers behind 150000", "5b: 500000 movers behind 150000",
          "6: all n movers behind 500000", "merge equals full after round 6", "ties: 20000 movers into a cell with 100 residents",
          "empty destination: 20000 movers into an empty cell", "emptied source cells", "aligned run of three tiles",
          "ends: slot 0 and the last partial chunk"]


@pytest.fixture(scope="module")
def merge_run():
    """All rounds run once, in order (each meets the mover count and the order the previous one left).  A library error -- the
    look-back time-out c.sync() reports, a device fault -- ends the run there: the rounds behind it are reported as not run."""
    run = _MergeRun()
    try:
        run.run()
    except capi.SphError as e:
        run.raised = repr(e)
    finally:
        run.close()
    return run


@pytest.mark.parametrize("name", ROUNDS)
def test_merge_rounds_against_numpy(merge_run, name):
    assert name in merge_run.records, f"not run: an earlier round raised {merge_run.raised}"
    assert merge_run.records[name] == []


def test_every_round_ran(merge_run):
    assert merge_run.raised is None
    assert list(merge_run.records) == ROUNDS

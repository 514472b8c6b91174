"""GPU: particles enter and leave a running whole-domain context (sph_emit, sph_remove, sph_count_in_regions).  Everything
is compared bit for bit (float arrays as uint32 views): the selection against the numpy model of tests/region_model.py, the
compacted arrays against the rows deleted on the host, and a context that was edited while it ran against one that uploads
the same particles in the same order."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic
from region_model import selected, to_capi

pytestmark = pytest.mark.gpu
BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)
DT = 2e-5                                   # with speed 40 a good share of the particles changes cell in a few steps
E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5
f32 = np.float32
C_F3 = ctypes.c_float * 3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ctx(capacity, **kw):
    return capi.Context(capacity, box=BOX, grid=GRID, **kw)


def _fluid(n, seed=ic.SEED):
    return ic.random_box(n, BOX, speed=40.0, fill=0.45, seed=seed)        # random fp32 positions in [-1, -0.1)^3


def _state(c):
    """Everything a step leaves behind, in slot order: position, velocity, creation index, density, pressure."""
    pos, vel, idx = c.download_owned()
    st = c.download(want=("density", "pressure"))
    return {"pos": pos, "vel": vel, "idx": idx, "density": st["density"][idx], "pressure": st["pressure"][idx]}


def _assert_same_state(a, b, what=""):
    assert np.array_equal(a["idx"], b["idx"]), f"{what}: slot order"
    for k in ("pos", "vel", "density", "pressure"):
        assert _same(a[k], b[k]), f"{what}: {k}"


def _code(fn, *args):
    with pytest.raises(capi.SphError) as e:
        fn(*args)
    return int(str(e.value).split("error ")[1].split(":")[0])


SPHERE = ("sphere", (-0.55, -0.55, -0.55), 0.5)
CASES = {
    "sphere": [("sphere", (-0.5, -0.6, -0.45), 0.37)],
    "box": [("box", (-0.8125, -1.0, -0.7), (-0.3, -0.4375, 0.5))],
    "halfspace": [("halfspace", (-0.5, -0.55, -0.6), (0.6, -0.8, 0.25))],
    "union": [("sphere", (-0.8, -0.8, -0.8), 0.25), ("box", (-0.5, -0.5, -0.5), (-0.25, -0.125, 0.0)),
              ("halfspace", (0.0, -0.9, 0.0), (0.0, 1.0, 0.0))],
}


def _remove_against_model(n, regions):
    pos, vel = _fluid(n)
    with _ctx(n) as c:
        c.upload(pos, vel)
        c.step(DT, 2)                                      # sorted, a live cell table, marks of the integrate epilogue
        p0, v0, i0 = c.download_owned()
        want = selected(p0, regions)
        regs = to_capi(regions)
        assert c.count_in(regs) == int(want.sum())
        assert c.n == n                                    # counting changes nothing
        got = c.remove(regs)
        assert c.last_removed == int(want.sum()) and c.n == n - int(want.sum())
        assert np.array_equal(got, i0[want])               # the removed set, in slot order
        p1, v1, i1 = c.download_owned()
        assert np.array_equal(i1, i0[~want]) and _same(p1, p0[~want]) and _same(v1, v0[~want])
        p4 = c.positions4()
        assert not p4[i0[want]].any()                      # (0, 0, 0, 0): an index without a particle
        assert _same(p4[i1, :3], p1) and np.all(p4[i1, 3] == 1.0)
        st = c.download(want=("density", "pressure"))      # not compacted: 0 until the next step, never a neighbour's value
        assert not st["density"][i1].any() and not st["pressure"][i1].any()
        assert c.count_in(regs) == 0
        few = c.remove(to_capi([("box", (-1, -1, -1), (1, 1, 1))]), max_out=3)      # the rest; only three indices wanted
        assert c.last_removed == n - int(want.sum()) and np.array_equal(few, i1[:3]) and c.n == 0
    return int(want.sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_remove_against_the_model_over_many_tiles(name):
    """70,001 particles: 35 compaction tiles with a ragged tail, each region kind alone and a union of three."""
    k = _remove_against_model(70001, CASES[name])
    assert 0 < k < 70001


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_remove_against_the_model_at_small_sizes(n):
    """Below, at and above one wave, and just past two tiles; a sphere of radius 0.5 in the middle of the fluid."""
    k = _remove_against_model(n, [SPHERE])
    assert n == 1 or 0 < k < n


def test_remove_against_the_model_past_one_chunk_of_the_tile_scan():
    """1025 selection tiles of 2048 slots -- one more than the one-block scan of the tile counts takes at a time, so the last
    tile's offset is the carry of the first 1024: a 128^3 lattice, one particle per cell of a 128^3 grid, and 64 more in the
    last cell.  A slice of x selects particles in every tile but the last, a box in the last cell 33 of its 65; the sort
    needs no step (nothing has moved).  The count, the removed indices and the survivors' order against numpy."""
    m, n = 128, 128 ** 3 + 64
    edge = f32(8.0 / m)
    g = (np.arange(m, dtype=f32) + f32(0.5)) * edge - f32(4.0)                   # cell centres: exact in fp32
    pos = np.empty((n, 3), f32)
    pos[:m ** 3] = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]
    pos[m ** 3:] = g[-1] + (np.arange(64, dtype=f32)[:, None] - f32(32.0)) * f32(2.0 ** -12)     # +- 2^-7 around the last centre
    regions = [("box", (g[5] - edge, -4.0, -4.0), (g[6], 4.0, 4.0)), ("box", (g[-1],) * 3, (4.0, 4.0, 4.0))]
    with capi.Context(n, box=(8.0, 8.0, 8.0), grid=(m, m, m)) as c:
        c.upload(pos, np.zeros_like(pos))
        c.hash(); c.sort(); c.build_cells()
        p0, v0, i0 = c.download_owned()
        want = selected(p0, regions)
        tiles = -(-n // 2048)
        assert tiles == 1025 and want[:2048].any() and want[1024 * 2048:].any() and not want[1024 * 2048:].all()
        regs = to_capi(regions)
        assert c.count_in(regs) == int(want.sum()) == 2 * m * m + 33
        got = c.remove(regs)
        assert c.last_removed == int(want.sum()) and c.n == n - int(want.sum())
        assert np.array_equal(got, i0[want])
        p1, v1, i1 = c.download_owned()
        assert np.array_equal(i1, i0[~want]) and _same(p1, p0[~want]) and _same(v1, v0[~want])
        assert c.count_in(regs) == 0


# ---- patterns: regions that cover exact cells ----------------------------------------------------------------------------
EDGE = f32(2.0 / 32)


def _cell_box(lo, hi):
    """The cells lo <= (cx, cy, cz) < hi as a box region: cell faces are multiples of 1/16, exact in fp32."""
    return ("box", tuple(f32(-1.0) + EDGE * f32(v) for v in lo), tuple(f32(-1.0) + EDGE * f32(v) for v in hi))


def _pattern_particles():
    """6000 particles on multiples of 2^-10 (so that x - box_min is exact and cell faces decide as the box test does): 64 in
    cell (0,0,0), 64 in cell (1,0,0) -- the two lowest keys -- and the rest at random in the cell layers z < 16, x >= 2."""
    rng = np.random.default_rng(11)
    q = 1024
    a = rng.integers(0, 64, (64, 3)) / q - 1.0
    b = rng.integers(0, 64, (64, 3)) / q - 1.0 + np.array([EDGE, 0, 0])
    rest = np.stack([rng.integers(128, 2048, 5872), rng.integers(0, 2048, 5872), rng.integers(0, 1024, 5872)], 1) / q - 1.0
    pos = np.concatenate([rest[:3000], a, rest[3000:], b]).astype(f32)
    return pos, np.zeros_like(pos)


def _sorted_ctx(pos, vel):
    c = _ctx(pos.shape[0])
    c.upload(pos, vel)
    c.hash(); c.sort(); c.build_cells()                    # positions and keys agree: nothing has moved yet
    return c


def test_remove_patterns():
    pos, vel = _pattern_particles()
    n = pos.shape[0]
    one = lambda p: ("box", tuple(p), tuple(np.nextafter(p, f32(9), dtype=f32)))       # exactly this position
    with _sorted_ctx(pos, vel) as c:
        keys = c.keys()
        p0, _, i0 = c.download_owned()
        assert np.all(keys[:64] == 0) and np.all(keys[64:128] == 1) and keys[128] > 1
    patterns = {
        "everything": ([("halfspace", (0, 1.5, 0), (0, 1, 0))], np.ones(n, bool)),
        "first and last slot": ([one(p0[0]), one(p0[-1])], np.isin(np.arange(n), [0, n - 1])),
        "one whole wave": ([_cell_box((1, 0, 0), (2, 1, 1))], (np.arange(n) >= 64) & (np.arange(n) < 128)),
        "every other cell layer": ([_cell_box((0, 0, z), (32, 32, z + 1)) for z in range(0, 16, 2)],
                                   (keys // (32 * 32)) % 2 == 0),
    }
    for name, (regions, want) in patterns.items():
        assert np.array_equal(selected(p0, regions), want), name          # the pattern is what it claims to be
        with _sorted_ctx(pos, vel) as c:
            got = c.remove(to_capi(regions))
            assert np.array_equal(got, i0[want]), name
            p1, _, i1 = c.download_owned()
            assert np.array_equal(i1, i0[~want]) and _same(p1, p0[~want]), name
            c.step(5e-7, 2)                                               # and the run goes on -- with no particle at all, too
            assert c.n == n - int(want.sum())
            c.sync()
            if name == "everything":
                assert c.n == 0 and c.count_in(to_capi(regions)) == 0
                assert c.emit(pos[:5], None, [4, 3, 2, 1, 0]) == 4 and c.n == 5      # an emptied context takes particles again
                c.step(5e-7, 1)
                assert np.isfinite(c.download_owned()[0]).all()


@pytest.mark.parametrize("what", ["at rest", "flowing"])
def test_removing_nothing_changes_nothing(what):
    """A twin that never calls sph_remove stays bit-identical through 3 steps -- state, skipped sorts and sort statistics: the
    marks of the integrate epilogue, the fresh keys and the cell table all survive a call that selects nothing."""
    if what == "at rest":
        pos, vel = ic.dam_break_lattice((8, 8, 8), BOX, jitter=False)     # no particle changes cell: the sorts are skipped
        dt = 5e-7
    else:
        (pos, vel), dt = _fluid(6000), DT
    nothing = to_capi([("box", (0.5, 0.5, 0.5), (0.75, 0.75, 0.75)), ("sphere", (0.5, 0.5, -0.5), 0.2)])
    with _ctx(pos.shape[0]) as a, _ctx(pos.shape[0]) as b:
        for c in (a, b):
            c.upload(pos, vel)
            c.step(dt, 2)
            c.sync()
        skipped = []
        for _ in range(3):
            assert a.remove(nothing).size == 0 and a.last_removed == 0 and a.count_in(nothing) == 0
            b.sync()                                       # (the calls above synchronise: keep the twin in lockstep as well)
            a.step(dt, 1); b.step(dt, 1)
            assert a.sort_skipped() == b.sort_skipped()
            skipped.append(a.sort_skipped())
            a.sync(); b.sync()
        assert a.sort_stats() == b.sort_stats()
        assert np.array_equal(a.keys(), b.keys())
        _assert_same_state(_state(a), _state(b), what)
        if what == "at rest":
            assert any(skipped)
        else:
            assert a.sort_stats()["merges"] >= 3 and a.sort_stats()["movers_total"] > 0


# ---- an edited run equals a re-upload ---------------------------------------------------------------------------------------
def test_remove_then_step_equals_reupload():
    """A steps 3, removes, steps 3; B uploads A's survivors (slot order, indices) and steps 3.  With the merge forced
    (mode 2) the sort after the removal takes the merge path -- the compaction kept the order -- and gives the bits of the
    full sort (mode 0) and of the re-upload."""
    n = 20000
    pos, vel = _fluid(n)
    regs = to_capi([SPHERE])
    out = {}
    for mode in (2, 0):
        with _ctx(n) as a:
            a.set_sort_mode(mode)
            a.upload(pos, vel)
            a.step(DT, 3)
            removed = a.remove(regs)
            assert 0 < removed.size < n
            survivors = a.download_owned()
            merges = a.sort_stats()["merges"]
            a.step(DT, 1)
            if mode == 2:
                assert a.sort_stats()["merges"] == merges + 1
            else:
                assert a.sort_stats()["merges"] == 0
            a.step(DT, 2)
            out[mode] = _state(a)
        with _ctx(n) as b:
            b.upload(*survivors)
            b.step(DT, 3)
            _assert_same_state(out[mode], _state(b), f"mode {mode} against the re-upload")
    _assert_same_state(out[2], out[0], "merge against full sort")


def _emitted(p_now, rng):
    """500 particles: 200 next to residents (occupied cells), 279 in the empty upper part of the box, 20 in ONE cell there,
    and one in the last cell of the grid."""
    near = (p_now[rng.choice(p_now.shape[0], 200, replace=False)] + rng.uniform(-0.004, 0.004, (200, 3))).astype(f32)
    near = np.clip(near, -1.0, 1.0).astype(f32)
    empty = rng.uniform(0.2, 0.9, (279, 3)).astype(f32)
    clump = (np.float32([0.5, 0.5, -0.5]) + rng.uniform(0.001, 0.06, (20, 3))).astype(f32)
    last = np.float32([[0.99, 0.99, 0.99]])
    pos = np.concatenate([near[:100], empty, clump, near[100:], last])
    vel = rng.uniform(-40, 40, pos.shape).astype(f32)
    return pos, vel


def _emit_equals_reupload(stepper, prepare=lambda c: None):
    n, m = 20000, 500
    pos, vel = _fluid(n)
    with _ctx(n + m + 1) as a, _ctx(n + m + 1) as b:
        prepare(a)
        a.upload(pos, vel)
        getattr(a, stepper)(DT, 3)
        p, v, i = a.download_owned()
        e_pos, e_vel = _emitted(p, np.random.default_rng(3))
        first = a.emit(e_pos[:300], e_vel[:300])
        assert first == n and a.n == n + 300
        assert a.emit(e_pos[300:], e_vel[300:]) == n + 300 and a.n == n + m      # two calls: call order is slot order
        p4 = a.positions4()
        assert _same(p4[n:n + m, :3], e_pos) and np.all(p4[n:n + m, 3] == 1.0)  # shown before any step
        pa, va, ia = a.download_owned()
        assert np.array_equal(ia, np.concatenate([i, np.arange(n, n + m, dtype=np.uint32)]))
        assert _same(pa, np.concatenate([p, e_pos])) and _same(va, np.concatenate([v, e_vel]))
        prepare(b)
        if a.colliders()["radii"].size:                                          # the centres A's steps advanced them to
            col = a.colliders()
            b.set_colliders(col["centers"], col["radii"], col["velocities"])
        b.upload(pa, va, ia)
        getattr(a, stepper)(DT, 3)
        getattr(b, stepper)(DT, 3)
        sa, sb = _state(a), _state(b)
        _assert_same_state(sa, sb, stepper)
        ka = a.keys()
        assert np.all(np.diff(ka.astype(np.int64)) >= 0) and ka[-1] == 32 ** 3 - 1     # the last cell of the grid is in use
        assert a.emit(e_pos[:1]) == n + m                                        # the next unused index moved on
    return sa


def test_emit_equals_reupload():
    """A steps 3, emits 500 (occupied cells, empty cells, 20 into one cell, one into the last cell of the grid), steps 3; B
    uploads A's particles at the moment of the emission plus the 500 behind them and steps 3: the same bits.  The same holds
    phase by phase (sph_step_phased on both sides).  The fused and the phased step agree with each other only to fp32
    rounding (include/sph_hip.h), so each is compared bit for bit with its own kind here, and with the other kind within
    that rounding in test_phased_step_after_an_emit_agrees_with_the_fused_step."""
    fused = _emit_equals_reupload("step")
    phased = _emit_equals_reupload("step_phased")
    assert np.array_equal(np.sort(fused["idx"]), np.sort(phased["idx"]))


def test_phased_step_after_an_emit_agrees_with_the_fused_step():
    """Two contexts with the same history (3 fused steps, the same 500 particles emitted) take the step after the emission
    one fused, one phase by phase.  Same sort, same density pass: slot order, density and pressure are the same bits.  The
    force is summed in another order, so velocity and position agree to fp32 rounding -- the bounds are those the suite
    already holds one fused step against one phased step to (test_gpu_fullsize): 1e-7 of the box edge (an ulp of a
    coordinate at the wall is 6e-8 of it) and 2e-6 of the largest speed."""
    n, m = 20000, 500
    pos, vel = _fluid(n)
    with _ctx(n + m) as a, _ctx(n + m) as b:
        for c in (a, b):
            c.upload(pos, vel)
            c.step(DT, 3)
        e_pos, e_vel = _emitted(a.download_owned()[0], np.random.default_rng(3))
        for c in (a, b):
            assert c.emit(e_pos, e_vel) == n
        a.step(DT, 1)
        b.step_phased(DT, 1)
        sa, sb = _state(a), _state(b)
    assert np.array_equal(sa["idx"], sb["idx"]) and np.isin(np.arange(n, n + m), sa["idx"]).all()
    assert _same(sa["density"], sb["density"]) and _same(sa["pressure"], sb["pressure"])
    d_pos = float(np.abs(sa["pos"] - sb["pos"]).max())
    d_vel = float(np.abs(sa["vel"] - sb["vel"]).max() / np.abs(sb["vel"]).max())
    print(f"fused against phased after an emit: |dpos| {d_pos:.3e}, dvel/|v|max {d_vel:.3e}")
    assert d_pos <= 1e-7 * BOX[0] and d_vel <= 2e-6


def test_emit_with_a_collider_and_in_mixed_precision():
    """Both sides take identical paths, so the equality holds with a sphere collider set and with the fp16 density pass."""
    _emit_equals_reupload("step", lambda c: c.set_colliders([[-0.6, -0.6, -0.6]], [0.2], [[50.0, 0.0, 25.0]]))
    _emit_equals_reupload("step", lambda c: c.set_precision(mixed_f16=True))


# ---- faucet and drain -----------------------------------------------------------------------------------------------------
def _faucet_run(c, first_step, last_step, free, counts, snap_at=None, snap_path=None):
    r = float(ic.PARTICLE_RADIUS)
    g = (np.arange(4, dtype=f32) - f32(1.5)) * f32(2 * r)
    jet = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32([0.3, 0.7, 0.3])).astype(f32)
    jet_vel = np.tile(np.float32([0.0, -600.0, 0.0]), (64, 1))
    nozzle = capi.Region.sphere((0.3, 0.7, 0.3), 0.1)
    drain = capi.Region.box((-1.0, -1.0, -1.0), (-0.8, -0.9, -0.8))
    saved = None
    for s in range(first_step, last_step):
        if s == snap_at:
            c.save(snap_path)
            saved = (list(free), dict(counts))
        if s % 4 == 0:
            if c.count_in(nozzle) == 0:                    # the nozzle is clear
                if len(free) >= 64:
                    index, free[:] = np.uint32(free[:64]), free[64:]
                    assert c.emit(jet, jet_vel, index) == int(index[0])
                else:
                    c.emit(jet, jet_vel)
                counts["emitted"] += 64
            gone = c.remove(drain)
            counts["removed"] += gone.size
            free.extend(int(v) for v in gone)
        c.step(DT, 1)
    return saved


def test_faucet_and_drain_with_a_snapshot_resume():
    """200 steps over a pool of 4096: 64 particles from a nozzle near the top every 4 steps when its sphere is clear, a box at
    the floor drained every 4 steps, the freed creation indices used again.  A snapshot taken at step 100 and resumed in a
    fresh context reproduces the rest of the run bit for bit, the next auto-assigned index included."""
    pos, vel = ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)
    n0, cap = pos.shape[0], 4096 + 2048
    with tempfile.TemporaryDirectory() as d, _ctx(cap) as a, _ctx(cap) as b:
        snap = os.path.join(d, "mid.sph")
        a.upload(pos, vel)
        free, counts = [], {"emitted": 0, "removed": 0}
        free_mid, counts_mid = _faucet_run(a, 0, 200, free, counts, snap_at=100, snap_path=snap)
        assert counts["emitted"] >= 3 * 64 and counts["removed"] > 0
        assert counts_mid["emitted"] > 0 and counts_mid["removed"] > 0          # the snapshot sits inside the edited run
        pa, va, ia = a.download_owned()
        assert a.n == n0 + counts["emitted"] - counts["removed"] == ia.size
        assert np.unique(ia).size == ia.size and ia.max() < cap
        assert np.isfinite(pa).all() and np.isfinite(va).all() and np.abs(pa).max() <= 1.0
        b.load_snapshot(snap)
        _faucet_run(b, 100, 200, free_mid, counts_mid)
        assert counts_mid == counts and free_mid == free
        _assert_same_state(_state(a), _state(b), "resumed run")
        assert _same(a.positions4(), b.positions4())
        one = np.float32([[0.0, 0.5, 0.0]])
        assert a.emit(one) == b.emit(one) >= n0                                  # the next auto-assigned index


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    n, cap = 1000, 1100
    pos, vel = _fluid(n)
    inside = np.float32([[0.1, 0.2, 0.3]])
    ok = capi.Region.sphere((-0.5, -0.5, -0.5), 0.3)
    with _ctx(cap) as c:
        c.upload(pos, vel, index=np.arange(n, dtype=np.uint32) + 50)             # next unused index: 1050
        c.step(DT, 2)
        before = c.download_owned()
        p4 = c.positions4()

        def unchanged():
            now = c.download_owned()
            return c.n == n and all(_same(x, y) for x, y in zip(now, before)) and _same(c.positions4(), p4)

        many = np.tile(inside, (101, 1))
        assert _code(c.emit, many) == E_CAPACITY and unchanged()                             # n + 101 > capacity
        assert _code(c.emit, np.tile(inside, (51, 1))) == E_CAPACITY and unchanged()         # indices 1050 .. 1100 reach the capacity
        assert _code(c.emit, np.float32([[0.1, np.nan, 0.3]])) == E_INVALID and unchanged()
        assert _code(c.emit, np.float32([[0.1, np.inf, 0.3]])) == E_INVALID and unchanged()
        assert _code(c.emit, inside, np.float32([[0.0, np.nan, 0.0]])) == E_INVALID and unchanged()
        assert _code(c.emit, np.float32([[0.1, 1.0001, 0.3]])) == E_INVALID and unchanged()  # outside the box
        assert _code(c.emit, np.concatenate([inside, np.float32([[-1.5, 0, 0]])])) == E_INVALID and unchanged()
        assert _code(c.emit, inside, None, [cap]) == E_INVALID and unchanged()               # explicit index >= capacity
        assert _code(c.remove, []) == E_INVALID and _code(c.count_in, []) == E_INVALID and unchanged()
        assert _code(c.remove, [ok] * 9) == E_INVALID and _code(c.count_in, [ok] * 9) == E_INVALID and unchanged()
        bad_kind = capi.Region(3, (C_F3)(-0.5, -0.5, -0.5), (C_F3)(), 0.3)
        assert _code(c.remove, [ok, bad_kind]) == E_INVALID and _code(c.count_in, bad_kind) == E_INVALID and unchanged()
        for bad in (capi.Region.sphere((-0.5, np.nan, -0.5), 0.3), capi.Region.sphere((-0.5, -0.5, -0.5), np.inf),
                    capi.Region.box((-1, -1, -1), (0, np.inf, 0)), capi.Region.halfspace((0, 0, 0), (0, np.nan, 0))):
            assert _code(c.remove, [ok, bad]) == E_INVALID and _code(c.count_in, bad) == E_INVALID and unchanged()
        # the edge of the box is inside; the refused calls used no index: the first one handed out is 1050
        assert c.emit(np.float32([[1.0, -1.0, 1.0]]), None, None) == 1050 and c.n == n + 1
        c.step(DT, 1)
        assert np.isfinite(c.download_owned()[0]).all()
    with _ctx(cap, slab=(8, 16), ghost_capacity=256) as s:                       # a z-slab context: not supported
        own = pos[(pos[:, 2] >= -0.5) & (pos[:, 2] < 0.0)]
        s.upload(own)
        before = s.download_owned()
        assert _code(s.emit, np.float32([[0.1, 0.2, -0.3]])) == E_STATE
        assert _code(s.remove, ok) == E_STATE and _code(s.count_in, ok) == E_STATE
        assert s.n == own.shape[0] and all(_same(x, y) for x, y in zip(s.download_owned(), before))


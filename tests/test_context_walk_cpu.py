"""CPU: the walk of the context's state table is complete and agrees with the document -- a condition, checked before any GPU
run: the matrix of tests/test_gpu_context_walk.py and the seeds of tests/test_gpu_context_fuzz.py, walked through the mirror of
tests/context_walk.py alone."""
import hashlib
import os
import re

import numpy as np
import pytest

import context_walk as cw
import obstacle_model as om
import small_grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _design_rows():
    """first cell -> {column: first word} of the table under "What is stale after X" in DESIGN.md"""
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    body = text.split("### What is stale after X", 1)[1]
    lines = []
    for ln in body.splitlines():            # the first table under the heading, and nothing behind it
        if ln.startswith("|"):
            lines.append(ln)
        elif lines:
            break
    head = [c.strip().strip("`") for c in lines[0].strip("|").split("|")]
    rows = {}
    for ln in lines[2:]:
        cells = [c.strip() for c in ln.strip("|").split("|")]
        assert len(cells) == len(head), ln
        rows[cells[0]] = {h: re.sub(r"\(\d+\)", "", c).split()[0] for h, c in zip(head[1:], cells[1:])}
    return rows


def _histories():
    return [(s, False) for s in cw.FUZZ_SEEDS] + [(s, True) for s in cw.FUZZ_SEEDS_OBSTACLE]


@pytest.fixture(scope="module")
def walked():
    """(rows reached, (stage, call) pairs reached) of the matrix and the fuzz seeds together"""
    reached, calls = set(), set()
    for prefix in cw.PREFIXES:
        for call in cw.calls_for(prefix):
            for cont in cw.CONTINUATIONS:
                m = cw.dry_case(prefix, call, cont)
                if m is not None:
                    reached |= m.reached
                    calls |= m.calls
    for seed, extended in _histories():
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        for op in cw.fuzz_ops(seed, extended=extended):
            m.apply(op)
            for ph in m.refused_phases():
                m.calls.add((m.stage, ph))
        reached |= m.reached
        calls |= m.calls
    return reached, calls


def test_the_generator_is_deterministic_per_seed():
    for seed, extended in _histories():
        a, b = cw.fuzz_ops(seed, extended=extended), cw.fuzz_ops(seed, extended=extended)
        assert a == b and len(a) == 42
    assert len({tuple(cw.fuzz_ops(s)) for s in cw.FUZZ_SEEDS}) == len(cw.FUZZ_SEEDS) == 8
    assert len({tuple(cw.fuzz_ops(s, extended=True)) for s in cw.FUZZ_SEEDS_OBSTACLE}) == len(cw.FUZZ_SEEDS_OBSTACLE) == 6


# sha256 of repr(fuzz_ops(seed)), first 16 hex digits, taken before the generator learnt the obstacle calls
PLAIN_HISTORIES = {101: "a04b747eb9e8c6fb", 102: "35ebd8b5ff533462", 103: "3e6cffc884ad03eb", 104: "47be6fa7a95964cf",
                   106: "bbaffccd09fc5970", 107: "9577e926d03a6ffe", 108: "c01a06c2a5cb8798", 109: "70b8b4e6e4524557"}


def test_the_plain_histories_are_what_they_always_were():
    assert tuple(PLAIN_HISTORIES) == cw.FUZZ_SEEDS
    for seed, digest in PLAIN_HISTORIES.items():
        assert hashlib.sha256(repr(cw.fuzz_ops(seed)).encode()).hexdigest()[:16] == digest, seed
        assert not any(op[0] in cw.OBSTACLE_OPS + ("render_surface", "extract_mesh") for op in cw.fuzz_ops(seed))


def test_the_obstacle_histories_hold_what_they_are_for():
    for seed in cw.FUZZ_SEEDS_OBSTACLE:
        ops = cw.fuzz_ops(seed, extended=True)
        count = lambda *names: sum(op[0] in names for op in ops)
        assert count("obstacle_build", "obstacle_set_grid") >= 2 and count("obstacle_clear") >= 1, seed
        assert count("obstacle_motion") >= 1 and count(*cw.VIEWS) >= 1, seed
        assert all(op[1] == 1 for op in ops if op[0] in ("step", "step_phased")), seed      # single steps: each one is anchored
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        for op in ops:
            m.apply(op)
        assert m.ob_steps >= 2, seed                       # integrates with an obstacle installed


def test_every_call_is_legal_or_refused_by_the_mirror():
    """a history never holds a call whose outcome the table leaves open (a phase call on positions newer than its keys)"""
    for seed, extended in _histories():
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        illegal = 0
        for op in cw.fuzz_ops(seed, extended=extended):
            assert cw.usable(m, [op]), (seed, op)
            illegal += m.apply(op) != 0
            assert op[0] == "set_sort_mode" or 0 < m.n <= m.capacity and m.next_index <= m.capacity
        assert illegal >= 1, seed


def test_the_mirror_is_the_table_of_the_document():
    rows = _design_rows()
    assert len(rows) == 15, sorted(rows)
    cols = {"stage": "stage", "order_valid": "order_valid", "have_*": "have_*", "sort_form_both_until": "sort_form_both_until"}
    used = set()
    for name, words in cw.TABLE.items():
        first = [r for r in rows if f"`{name}`" in r]
        assert len(first) == 1, (name, first)
        used.add(first[0])
        for col, word in zip(cw.COLUMNS, words):
            assert rows[first[0]][cols[col]] == word.split()[0], (name, col, rows[first[0]][cols[col]], word)
    skipped = set()
    for name in cw.SKIPPED_ROWS:
        first = [r for r in rows if f"`{name}`" in r and r not in used]
        assert len(first) == 1, (name, first)
        skipped.add(first[0])
    assert used | skipped == set(rows), set(rows) - used - skipped      # every row is walked, or skipped by name


def test_every_stage_meets_every_call(walked):
    _, calls = walked
    ids = set()
    for _, ops, _ in cw.CALLS.values():
        for k, op in enumerate(ops):        # reachable at every stage: nothing in front of it in its call moves the stage
            if all(o[0] not in cw.EDITS for o in ops[:k]):
                ids.add(cw.call_id(op))
    ids |= set(cw.PHASES) | {"step", "step_phased"}
    missing = sorted((s, i) for s in (cw.LOADED, cw.HASHED, cw.SORTED, cw.CELLS) for i in ids if (s, i) not in calls)
    assert not missing, missing


def test_every_entry_of_the_four_columns_is_reached_where_it_shows(walked):
    """kept / cleared where there was something to lose, set where the field held something else"""
    reached, _ = walked
    missing = sorted((name, col) for name in cw.TABLE for col in cw.COLUMNS if (name, col, True) not in reached)
    assert not missing, missing


# ---- what makes the bare-twin anchor bite: the model alone, on the particles as installed ------------------------------------------
def _generators():
    from gpufluidsimulator_amd import ic
    out = {f"flow {n}": cw._particles(n, "flow") for n in (6000, 3000, 5000, 20000)}
    out["snapshot"] = ic.random_box(cw.SNAP_N, cw.BOX, speed=40.0, fill=0.45, seed=cw.SNAP_SEED)
    out["rest"] = cw._particles(512, "rest")
    for jitter in (False, True):
        out[f"lattice 12, jitter {jitter}"] = ic.dam_break_lattice((12, 12, 12), cw.BOX, jitter=jitter)
    seeds = {op[2] for _, ops, _ in cw.CALLS.values() for op in ops if op[0] in ("set_by_index", "emit")}
    seeds |= {op[2] for P in cw.PREFIXES.values() for op in P["before"] + P["after"] if op[0] in ("set_by_index", "emit")}
    for seed in sorted(seeds):
        out[f"points {seed}"] = cw._points(cw.SBI_COUNT, seed)
    return out


def test_the_walks_obstacles_touch_every_particle_set():
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    grid = om.lattice(cw.OBSTACLE_SPACING, lo, hi)
    both = om.rasterise(cw.OBSTACLES["both"], grid)
    caller = om.clamp(cw.caller_field(52), cw.CALLER_GRID)
    off, u = cw.MOTION["on"]
    touched = {}
    for name, (pos, vel) in _generators().items():
        after, _, t = om.push(pos, vel, grid, both, (0, 0, 0), (0, 0, 0), lo, hi)
        touched[name] = int(t.sum())
        assert t.sum() >= 20, name
        # ... also where the motion has carried the solid four steps on, and with the caller's field
        assert om.push(pos, vel, grid, both, om.advance(off, u, cw.DT_FLOW, 4), u, lo, hi)[2].sum() >= 20, name
        assert om.push(pos, vel, cw.CALLER_GRID, caller, off, u, lo, hi)[2].sum() >= 20, name
        if name == "rest":       # the push alone takes particles of the lattice at rest to other cells: the sort behind it cannot be skipped
            keys = lambda p: small_grids.np_keys(p, np.array(lo, np.float32), np.array(hi, np.float32), cw.GRID)
            assert (keys(after) != keys(pos)).sum() == 112
    assert [touched[k] for k in ("flow 6000", "flow 3000", "flow 20000", "snapshot", "rest", "lattice 12, jitter False", "points 33")] == \
        [1802, 905, 5943, 892, 160, 504, 112]


def test_every_prefix_runs_the_obstacle_on_calls():
    for prefix in cw.PREFIXES:
        calls = cw.calls_for(prefix)
        assert {"obstacle_on", "obstacle_off", "obstacle_moving"} <= set(calls), prefix
        for call in calls:
            if cw.CALLS[call][2] == "bare":
                assert all(cw.dry_case(prefix, call, cont) is not None for cont in cw.CONTINUATIONS), (prefix, call)
    assert any(op[0] == "obstacle_build" for op in cw.PREFIXES["stepped_obstacle"]["before"])
    assert any(op[0] == "obstacle_build" for k, P in cw.PREFIXES.items() if P.get("calls") == "few" for op in P["before"])

"""CPU: the walk of the context's state table is complete and agrees with the document -- a condition, checked before any GPU
run: the matrix of tests/test_gpu_context_walk.py and the seeds of tests/test_gpu_context_fuzz.py, walked through the mirror of
tests/context_walk.py alone."""
import os
import re

import pytest

import context_walk as cw

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
    for seed in cw.FUZZ_SEEDS:
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        for op in cw.fuzz_ops(seed):
            m.apply(op)
            for ph in m.refused_phases():
                m.calls.add((m.stage, ph))
        reached |= m.reached
        calls |= m.calls
    return reached, calls


def test_the_generator_is_deterministic_per_seed():
    for seed in cw.FUZZ_SEEDS:
        a, b = cw.fuzz_ops(seed), cw.fuzz_ops(seed)
        assert a == b and len(a) == 42
    assert len({tuple(cw.fuzz_ops(s)) for s in cw.FUZZ_SEEDS}) == len(cw.FUZZ_SEEDS) == 8


def test_every_call_is_legal_or_refused_by_the_mirror():
    """a history never holds a call whose outcome the table leaves open (a phase call on positions newer than its keys)"""
    for seed in cw.FUZZ_SEEDS:
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        illegal = 0
        for op in cw.fuzz_ops(seed):
            assert cw.usable(m, [op]), (seed, op)
            illegal += m.apply(op) != 0
            assert op[0] == "set_sort_mode" or 0 < m.n <= m.capacity and m.next_index <= m.capacity
        assert illegal >= 1, seed


def test_the_mirror_is_the_table_of_the_document():
    rows = _design_rows()
    assert len(rows) == 13, sorted(rows)
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

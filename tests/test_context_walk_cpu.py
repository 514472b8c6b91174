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
import obstacle_pose_model as pm
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
    return [(s, False) for s in cw.FUZZ_SEEDS] + [(s, True) for s in cw.FUZZ_SEEDS_OBSTACLE] + [(s, "pose") for s in cw.FUZZ_SEEDS_POSE]


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
    assert len({tuple(cw.fuzz_ops(s, extended="pose")) for s in cw.FUZZ_SEEDS_POSE}) == len(cw.FUZZ_SEEDS_POSE) == 6


# sha256 of repr(fuzz_ops(seed)), first 16 hex digits, taken before the generator learnt the obstacle calls
PLAIN_HISTORIES = {101: "a04b747eb9e8c6fb", 102: "35ebd8b5ff533462", 103: "3e6cffc884ad03eb", 104: "47be6fa7a95964cf",
                   106: "bbaffccd09fc5970", 107: "9577e926d03a6ffe", 108: "c01a06c2a5cb8798", 109: "70b8b4e6e4524557"}


def test_the_plain_histories_are_what_they_always_were():
    assert tuple(PLAIN_HISTORIES) == cw.FUZZ_SEEDS
    for seed, digest in PLAIN_HISTORIES.items():
        assert hashlib.sha256(repr(cw.fuzz_ops(seed)).encode()).hexdigest()[:16] == digest, seed
        assert not any(op[0] in cw.OBSTACLE_OPS + ("render_surface", "extract_mesh") for op in cw.fuzz_ops(seed))


# the same of repr(fuzz_ops(seed, extended=True)), taken before the generator learnt the pose, the sensor and the mesh doors
OBSTACLE_HISTORIES = {201: "4d1659e226b33f97", 202: "5338cb260d88584e", 203: "500e231910156dcc", 204: "9539ebb9442a2fba",
                      206: "d077a890f4ebdc40", 211: "8a41c5b53c841123"}
_POSE_OPS = ("obstacle_pose", "obstacle_get_pose", "obstacle_sensor", "obstacle_load", "obstacle_build_mesh", "obstacle_mesh_stats",
             "obstacle_build_mesh_dev")


def test_the_obstacle_histories_are_what_they_always_were():
    assert tuple(OBSTACLE_HISTORIES) == cw.FUZZ_SEEDS_OBSTACLE
    for seed, digest in OBSTACLE_HISTORIES.items():
        ops = cw.fuzz_ops(seed, extended=True)
        assert hashlib.sha256(repr(ops).encode()).hexdigest()[:16] == digest, seed
        assert not any(op[0] in _POSE_OPS for op in ops)


def test_the_pose_histories_hold_what_they_are_for():
    for seed in cw.FUZZ_SEEDS_POSE:
        ops = cw.fuzz_ops(seed, extended="pose")
        m = cw.Mirror(cw.FUZZ_CAPACITY)
        poses = turning = drops = sensor_on = meshes = edits_posed = refused = 0
        for op in ops:
            posed = m.pose is not None
            rc = m.apply(op)
            refused += rc != 0
            if rc:
                continue
            poses += op[0] == "obstacle_pose"
            turning += op == ("obstacle_pose", "turning")
            drops += op in (("obstacle_pose", "none"), ("obstacle_clear",))
            sensor_on += op == ("obstacle_sensor", 1)
            meshes += op[0] in ("obstacle_build_mesh", "obstacle_build_mesh_dev")
            edits_posed += posed and op[0] in cw.EDITS and not (op[0] == "remove" and op[1] == "none")
        assert poses >= 2 and turning >= 1 and drops >= 1 and sensor_on >= 1 and meshes >= 1, seed
        assert edits_posed >= 1 and refused >= 1, seed
        assert all(op[1] == 1 for op in ops if op[0] in ("step", "step_phased")), seed      # single steps: each one is anchored
        assert m.ob_steps >= 3 and m.posed_sense_steps >= 2, seed                            # ... posed and sensing, two of them


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


# entry point of row (7) -> the call id that executes it
ROW_7 = {"sph_obstacle_build": "obstacle_build:both", "sph_obstacle_set_grid": "obstacle_set_grid", "sph_obstacle_clear": "obstacle_clear",
         "sph_obstacle_set_motion": "obstacle_motion:on", "sph_obstacle_sample": "obstacle_sample",
         "sph_obstacle_build_mesh": "obstacle_build_mesh:ico", "sph_obstacle_build_mesh_dev": "obstacle_build_mesh_dev",
         "sph_obstacle_mesh_stats": "obstacle_mesh_stats", "sph_obstacle_set_pose": "obstacle_pose:turning",
         "sph_obstacle_get_pose": "obstacle_get_pose", "sph_obstacle_set_sensor": "obstacle_sensor:1", "sph_obstacle_get_load": "obstacle_load"}


def test_every_name_of_the_obstacle_row_is_walked_at_every_stage_or_skipped_by_name(walked):
    """the names are the document's: a call added to row (7) of DESIGN.md fails here until it is walked or skipped with a reason"""
    _, calls = walked
    row = [r for r in _design_rows() if "`sph_obstacle_build`" in r]
    assert len(row) == 1
    names = re.findall(r"`(sph_\w+)`", row[0])
    assert len(names) == len(set(names)) == 13, names
    assert set(names) == set(ROW_7) | set(cw.SKIPPED_CALLS) and not set(ROW_7) & set(cw.SKIPPED_CALLS)
    assert all(len(reason) > 20 for reason in cw.SKIPPED_CALLS.values())
    missing = sorted((s, n) for s in (cw.LOADED, cw.HASHED, cw.SORTED, cw.CELLS) for n, i in ROW_7.items() if (s, i) not in calls)
    assert not missing, missing
    # ... the accepted form of the two that can be refused, too: a mesh-built grid for the stats, an extracted mesh for the device door
    for prefix in cw.HEAVY_PREFIXES:
        assert set(cw.HEAVY) <= set(cw.calls_for(prefix)) and cw.PREFIXES[prefix].get("calls", "all") == "all"
    for call in ("mesh_stats",) + cw.HEAVY:
        m = cw.Mirror(8192)
        for op in cw.PREFIXES["cells"]["before"] + cw.PREFIXES["cells"]["after"] + cw.CALLS[call][1]:
            assert m.apply(op) == 0, (call, op)


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
    for prefix in ("stepped_posed", "hashed_20k_posed"):
        before = cw.PREFIXES[prefix]["before"]
        assert {("obstacle_build", "both"), ("obstacle_pose", "turning"), ("obstacle_sensor", 1)} <= set(before), prefix
        assert {"sensor_posed", "posed_remove", "posed_emit", "mesh_on"} <= set(cw.calls_for(prefix)), prefix
    assert cw.PREFIXES["hashed_20k_posed"]["before"][3] == ("upload", 20000, "flow") and -(-20000 // 64) == 313


# ---- the same for the pose, the sensor and the mesh door -----------------------------------------------------------------------------
def _walk_solids():
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    grid = om.lattice(cw.OBSTACLE_SPACING, lo, hi)
    ico, stats = cw.mesh_field(*cw.walk_mesh("ico"), grid)
    assert stats == (320, 0, 0, 0)
    return {"both": (grid, om.rasterise(cw.OBSTACLES["both"], grid)), "caller": (cw.CALLER_GRID, om.clamp(cw.caller_field(52), cw.CALLER_GRID)),
            "mesh": (grid, ico)}, lo, hi


def test_the_walks_posed_and_mesh_solids_touch_every_particle_set():
    """the mesh solid as installed, and every solid under both poses -- as installed and where four steps of motion and pose
    have carried it -- touches at least 20 particles of every set; the turning pose kicks some of every set (the sensing anchor
    needs one) as installed and under MOTION["in"], the motion of the prefix "stepped_posed", and under MOTION["on"] wherever the
    particles have velocities"""
    solids, lo, hi = _walk_solids()
    zero = np.zeros(3, np.float32)
    # the pivot sits inside the solid of OBSTACLES["both"]
    assert om.sample(*solids["both"], zero, np.array([cw.POSE_PIVOT], np.float32))[0][0] < 0
    pinned = {}
    for name, (pos, vel) in _generators().items():
        unposed = int(om.push(pos, vel, *solids["mesh"], zero, zero, lo, hi)[2].sum())
        assert unposed >= 20, name
        pinned[name] = [unposed]
        for what, (grid, phi) in solids.items():
            for tag in ("turning", "still"):
                for (o0, u0), steps in (((zero, zero), 0), (cw.MOTION["on"], 4), (cw.MOTION["in"], 2), (cw.MOTION["in"], 4)):
                    ps, o = pm.advance(pm.pose(*cw.POSES[tag]), o0, u0, cw.DT_FLOW, steps)
                    st = {}
                    touched = pm.push(pos, vel, grid, phi, o, u0, ps, lo, hi, stats=st)[2]
                    assert touched.sum() >= 20, (name, what, tag, steps)
                    # MOTION["on"] carries the ramp away from the fluid: particles at rest are pushed by it and not kicked
                    if tag == "turning" and (u0 is not cw.MOTION["on"][1] or vel.any()):
                        assert st["kicked"].sum() >= 1, (name, what, steps)
                    if tag == "turning" and steps == 0:
                        pinned[name] += [int(touched.sum()), int(st["kicked"].sum())]
    # [the mesh unposed; touched, kicked under the turning pose as installed: both, caller, mesh]
    assert pinned["flow 6000"][0] == 1244 and pinned["flow 3000"][0] == 624
    assert pinned["flow 20000"] == [4053, 7364, 5111, 4273, 2270, 4185, 2200]
    assert pinned["snapshot"] == [659, 1098, 742, 670, 343, 662, 319]
    assert pinned["rest"] == [98, 205, 171, 98, 26, 87, 21]
    assert pinned["lattice 12, jitter False"] == [831, 667, 632, 850, 301, 823, 309]
    assert pinned["points 36"] == [103, 143, 86, 80, 29, 81, 28]


def test_an_advanced_pose_has_no_exact_way_back_in():
    """why Walker.rebase re-seats: sph_obstacle_set_pose normalises a float32 quaternion, sph_obstacle_get_pose shows the float64
    one a Cayley step has normalised already.  For the walk's turning pose, normalising again changes bits at some of the first
    ten steps and the trip through float32 at every one; with omega = 0 a step changes nothing, so a pose that stands still
    could be handed over as it was set"""
    ps = pm.pose(*cw.POSES["turning"])
    q, again, through_f32 = ps["q"], 0, 0
    for _ in range(10):
        q = pm.quat_step(q, ps["omega"], cw.DT_FLOW)
        again += not np.array_equal(pm._unit(q), q)
        through_f32 += not np.array_equal(pm.quat_set(q.astype(np.float32)), q)
    assert again >= 1 and through_f32 == 10, (again, through_f32)
    ps = pm.pose(*cw.POSES["still"])
    q = ps["q"]
    for _ in range(200):
        q = pm.quat_step(q, ps["omega"], cw.DT_FLOW)
        assert np.array_equal(q.view(np.uint64), ps["q"].view(np.uint64))


def test_the_posed_anchor_can_fail():
    """what Walker._check_against_model compares: for a posed record the unposed obstacle_model.push is another function of the
    same particles, and a sum in another order other bits"""
    solids, lo, hi = _walk_solids()
    pos, vel = cw._particles(6000, "flow")
    zero = np.zeros(3, np.float32)
    ps = pm.pose(*cw.POSES["turning"])
    st = {}
    posed_p, posed_v, posed_t = pm.push(pos, vel, *solids["both"], zero, zero, ps, lo, hi, stats=st)
    plain_p, plain_v, plain_t = om.push(pos, vel, *solids["both"], zero, zero, lo, hi)
    differ = (posed_p.view(np.uint32) != plain_p.view(np.uint32)).any(axis=1) | (posed_v.view(np.uint32) != plain_v.view(np.uint32)).any(axis=1)
    assert differ.sum() >= 1000 and (posed_t != plain_t).sum() >= 100, (differ.sum(), (posed_t != plain_t).sum())
    # ... the still pose too (the rotation alone), and the unposed model under the sensor is obstacle_model.push to the bit
    still_p = pm.push(pos, vel, *solids["both"], zero, zero, pm.pose(*cw.POSES["still"]), lo, hi)[0]
    assert (still_p.view(np.uint32) != plain_p.view(np.uint32)).any()
    none_p, none_v, _ = pm.push(pos, vel, *solids["both"], zero, zero, None, lo, hi)
    assert np.array_equal(none_p.view(np.uint32), plain_p.view(np.uint32)) and np.array_equal(none_v.view(np.uint32), plain_v.view(np.uint32))
    J, L = pm.load_in_order(st["lane"], st["kicked"], len(pos))
    J2, L2 = pm.load_in_order(st["lane"], st["kicked"], len(pos), runs_descending=True)
    assert st["kicked"].sum() > 100 and np.abs(J).max() > 0 and np.abs(L).max() > 0
    assert not (np.array_equal(J.view(np.uint64), J2.view(np.uint64)) and np.array_equal(L.view(np.uint64), L2.view(np.uint64)))

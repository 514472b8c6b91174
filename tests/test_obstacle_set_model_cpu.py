"""CPU: the model of several obstacles (tests/obstacle_set_model.py) and the scenes of tests/test_gpu_obstacle_set.py
(tests/obstacle_set_cases.py), on the dam as uploaded with its seeded velocities.  These are CONDITIONS: a scene that stops
meeting them no longer tests what the GPU test says it tests."""
import numpy as np

import obstacle_model as om
import obstacle_pose_model as pm
import obstacle_set_cases as sc
import obstacle_set_model as sm

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_a_set_of_one_slot_is_the_single_model():
    pos, vel = sc.dam()
    for k, solid in ((0, sc.RAMP), (2, sc.BAR), (3, sc.PADDLE)):
        sl = sc.model_slot(solid)
        p, v, touched, st = sc.push(pos, vel, {k: sl})
        one = {}
        wp, wv, wt = pm.push(pos, vel, sl["grid"], sl["phi"], sl["off"], sl["u"], sl["pose"], sc.BMIN, sc.BMAX, sc.EPS, sc.DAMP, sc.MASS,
                             stats=one)
        assert np.array_equal(_u32(p), _u32(wp)) and np.array_equal(_u32(v), _u32(wv)) and np.array_equal(touched, wt)
        assert touched.sum() > 100
        J, L = sm.load(st[k], pos.shape[0])
        wJ, wL = pm.load_in_order(one["lane"], one["kicked"], pos.shape[0])
        assert np.array_equal(J.view(np.uint64), wJ.view(np.uint64)) and np.array_equal(L.view(np.uint64), wL.view(np.uint64))
        if sl["pose"] is None:                              # ... and an unposed slot is tests/obstacle_model.py
            op, ov, ot = om.push(pos, vel, sl["grid"], sl["phi"], sl["off"], sl["u"], sc.BMIN, sc.BMAX, sc.EPS, sc.DAMP)
            assert np.array_equal(_u32(p), _u32(op)) and np.array_equal(_u32(v), _u32(ov)) and np.array_equal(touched, ot)


def test_the_scene_has_particles_of_every_class():
    pos, vel = sc.dam()
    slots = sc.model_slots(sc.SCENE)
    assert sorted(slots) == [0, 1, 3] and slots[1]["pose"] is not None and slots[0]["pose"] is None and slots[3]["pose"] is None
    p, v, touched, st = sc.push(pos, vel, slots)
    cls = sm.classes(pos, slots, st, 0, 1)
    counts = {k: int(m.sum()) for k, m in cls.items()}
    print(counts)
    assert all(c > 0 for c in counts.values()), counts
    assert counts["stale"] >= 10 and counts["none"] > 1000
    assert all(st[k]["touched"].sum() >= 100 for k in slots)
    assert st[1]["kicked"].sum() > 0 and st[3]["kicked"].sum() > 0          # both sensing slots have a load
    # the stale particles are really outside slot 1's guard where they start and inside solid 1 after slot 0
    stale = cls["stale"]
    assert not sm.may_touch(slots[1], pos)[stale].any() and sm.may_touch(slots[1], st[1]["before"])[stale].all()
    # a pass that kept the first look-up would leave them where slot 0 put them: other bits
    assert (_u32(p[stale]) != _u32(st[1]["before"][stale])).any(axis=1).all()
    # the untouched keep their bits
    assert np.array_equal(_u32(p[~touched]), _u32(pos[~touched])) and np.array_equal(_u32(v[~touched]), _u32(vel[~touched]))


def test_swapping_two_overlapping_solids_changes_bits():
    pos, vel = sc.dam()
    ab = sc.push(pos, vel, sc.model_slots({0: sc.OVERLAP_A, 1: sc.OVERLAP_B}))
    ba = sc.push(pos, vel, sc.model_slots({0: sc.OVERLAP_B, 1: sc.OVERLAP_A}))
    assert ab[3][0]["touched"].sum() > 100 and ab[3][1]["touched"].sum() > 100
    assert (ab[3][0]["touched"] & ab[3][1]["touched"]).sum() > 0
    assert (_u32(ab[0]) != _u32(ba[0])).any() and (_u32(ab[1]) != _u32(ba[1])).any()


def test_the_identity_pose_about_a_far_pivot_is_not_the_unposed_rule():
    pos, vel = sc.dam()
    posed = sc.push(pos, vel, {2: sc.model_slot(sc.IDENTITY_POSED)})
    plain = sc.push(pos, vel, {2: sc.model_slot(dict(sc.IDENTITY_POSED, pivot=None))})
    assert posed[2].sum() > 100 and (_u32(posed[0]) != _u32(plain[0])).any(axis=1).sum() > 50


def test_the_advance_is_per_slot():
    slots = sc.model_slots(sc.SCENE)
    nxt = sm.advance(slots, 1e-4, 3)
    assert np.array_equal(nxt[0]["off"], np.zeros(3, F)) and nxt[0]["pose"] is None
    assert np.array_equal(_u32(nxt[3]["off"]), _u32(om.advance(sc.BAR["off"], sc.BAR["u"], 1e-4, 3)))
    ps, off = pm.advance(sc.pose_of(sc.PADDLE), sc.PADDLE["off"], sc.PADDLE["u"], 1e-4, 3)
    assert np.array_equal(nxt[1]["pose"]["q"].view(np.uint64), ps["q"].view(np.uint64)) and np.array_equal(_u32(nxt[1]["off"]), _u32(off))
    assert not np.array_equal(nxt[1]["pose"]["q"], slots[1]["pose"]["q"])

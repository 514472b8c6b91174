"""GPU: the context's state table walked entry point by entry point, at every stage.

Every state of context_walk.PREFIXES is crossed with every call of context_walk.CALLS and finished in three ways (phase by
phase, with sph_force_collide_integrate, or restarted with sph_step).  Per case: the return code of the call and of every phase
call the table now refuses; order_valid and sort_form_both_until through the sort statistics of the next sort; and the TWIN
identity -- a fresh context that uploads what the public API showed at the last moment particles changed and repeats the
calls since then has the same keys, order, cell table, densities, forces and particles bit for bit, at every stage of the step
that follows and after two more steps (stale marks or stale fresh keys only bite at the next sort).  One call per class and
prefix also runs the step that follows against the float64 model (tests/phase_checks.py), in case both are wrong together.

The obstacle calls, the surface and the mesh are calls of the matrix like any other, and one prefix has a moving obstacle from
the start.  What the library shows of the obstacle is held to a numpy record of it after every call (field, lattice, the offset
advanced once per integrate); every view is compared with its numpy model; and wherever an obstacle is installed when the step
is finished, the first integrate is obstacle_model.push applied to the output of a BARE twin -- a context without the obstacle
that made the same calls -- for every particle, under all three continuations.

So are the pose, the load sensor and the mesh doors (sph_obstacle_set_pose, _get_pose, _set_sensor, _get_load, _build_mesh,
_build_mesh_dev, _mesh_stats): set, switched, read and built at every stage, alone and together, on a caller's grid and on a
mesh-built one, in front of every edit, and on two prefixes that are posed and sensing from the start.  The pose and the load
the library shows are held to a numpy record after every call (the quaternion as uint64 bits, `steps` by the header's words);
behind a posed or sensing obstacle the first integrate is obstacle_pose_model.push of the bare twin's output in slot order, with
J and L summed in the header's order, and at least one particle kicked.  The twin is handed the sensor's switch and the pose;
a pose that has advanced is re-seated on the context under test first (context_walk.Walker.rebase says why).  The device door
voxelises the context's own last mesh; its numpy model takes seconds, so its calls -- one of them with a mesh that is an edit old -- run under context_walk.HEAVY_PREFIXES."""
import pytest

import context_walk as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("walk") / "walk.snap")
    cw.make_snapshot(path)
    return path


def run_case(prefix, call, cont, snapshot):
    P = cw.PREFIXES[prefix]
    _, ops, anchor = cw.CALLS[call]
    with cw.Walker(P.get("capacity", 8192), P.get("dt", cw.DT_FLOW), snapshot) as w:
        # the bare twin (no obstacle): for the calls that install one, and for every call of a prefix that has one already
        w.bare = anchor == "bare" or any(op[0] == "obstacle_build" for op in P["before"])
        w.reach(prefix)
        if not cw.usable(w.m, ops):
            return False
        w.probe_refusals()
        for op in ops:
            w.do(op)
            w.probe_refusals()
            w.compare("the call")
        pushes = w.bare and w.m.obstacle is not None       # the first integrate from here: the model's push of the bare twin's output
        if anchor is True and cont == "phases" and w.m.precision == 0 and w.m.obstacle is None:     # (the model's bars are the fp32
            w.anchor_step()                                                                          # ones, and it knows no obstacle)
            w.compare("the anchored step")
        else:
            for op in cw.continuation(cont, w.m):
                w.do(op)
                w.probe_refusals()
                w.compare("the continuation")
        if pushes:
            assert w.anchored == 1 and w.anchor_touched > 0, (w.anchored, w.anchor_touched)
            assert w.anchor_sensed == int(w.m.sense), (w.anchor_sensed, w.m.sense)
            if w.m.sense:                                  # a load of zero would prove nothing
                assert w.anchor_kicked > 0, "no particle was kicked under the sensor"
            if w.m.obstacle == ("mesh_dev",) and w.m.pose is None:     # the mould of the fluid's own mesh: some particles, not all
                assert 20 <= w.anchor_last[0] < w.anchor_last[1], w.anchor_last
            w.do(("hash",))                                # the keys the pass left (fused) or a hash computes: numpy's, of the slots' positions
            w.compare("the hash behind the push")
        elif w.bare:
            assert w.anchored == 0
        w.do(("step", 2))
        w.compare("two more steps")
    return True


@pytest.mark.parametrize("cont", cw.CONTINUATIONS)
@pytest.mark.parametrize("prefix", list(cw.PREFIXES))
def test_walk(prefix, cont, snapshot):
    ran = 0
    for call in cw.calls_for(prefix):
        try:
            ran += run_case(prefix, call, cont, snapshot)
        except AssertionError as e:
            raise AssertionError(f"{prefix} x {call} x {cont}: {e}") from e
    # (a repeated phase call has no meaning right after a step: context_walk.usable leaves it out, here as in the CPU walk)
    assert ran == sum(cw.dry_case(prefix, call, cont) is not None for call in cw.calls_for(prefix))

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
that made the same calls -- for every particle, under all three continuations."""
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

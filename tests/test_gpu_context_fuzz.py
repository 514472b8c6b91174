"""GPU: long histories through the context's state table.  Eight fixed seeds, forty calls each, drawn from every entry point
of context_walk.CALLS plus whole fused and phased steps, each legal or deliberately illegal by the mirror.  At every boundary
(an integrate or an edit) the twin is rebuilt from what the public API shows; at every completed step the state, order, keys
and cell table are compared with it bit for bit, and after every call the particle set tracked by creation index on the host
must be what sph_download_owned, sph_download and sph_download_positions4 report.

Six more seeds also draw the obstacle calls and the views.  There every view is compared with its numpy model, the obstacle the
library shows with numpy's record of it, and every completed step that has an obstacle is obstacle_model.push applied to the
output of a bare twin (a context without the obstacle, rebuilt at the same boundaries).

Six more again (context_walk.FUZZ_SEEDS_POSE) also draw the pose, the load sensor and the mesh doors: every completed step behind a
posed or sensing obstacle is obstacle_pose_model.push of the bare twin's output with the load's J and L in the header's order, and
the pose and the load are held to the numpy record after every call.  Every completed step is a boundary, so an advanced pose is
re-seated there (context_walk.Walker.rebase); long uninterrupted advances are tests/test_gpu_obstacle_pose.py's."""
import pytest

import context_walk as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fuzz") / "fuzz.snap")
    cw.make_snapshot(path)
    return path


def _history(seed, snapshot, extended):
    ops = cw.fuzz_ops(seed, extended=extended)
    with cw.Walker(cw.FUZZ_CAPACITY, cw.DT_FLOW, snapshot) as w:
        w.twinning = True
        w.bare = extended
        done = []
        try:
            for op in ops:
                done.append(op)
                w.do(op)
                w.probe_refusals()
                w.compare()
                if w.m.integrated and op[0] in ("integrate", "fci", "step", "step_phased"):
                    w.rebase()                    # a completed step is a boundary
        except AssertionError as e:
            raise AssertionError(f"seed {seed}, call {len(done)} of {ops}: {e}") from e
        if extended:         # every integrate with an obstacle installed was the first behind a boundary, and was held to the model
            assert w.anchored == w.m.ob_steps >= 2 and w.anchor_touched > 0, (w.anchored, w.m.ob_steps, w.anchor_touched)
        if extended == "pose":
            assert w.anchored >= 3 and w.anchor_sensed >= w.m.posed_sense_steps >= 2 and w.anchor_kicked > 0, \
                (w.anchored, w.anchor_sensed, w.m.posed_sense_steps, w.anchor_kicked)


@pytest.mark.parametrize("seed", cw.FUZZ_SEEDS)
def test_history(seed, snapshot):
    _history(seed, snapshot, False)


@pytest.mark.parametrize("seed", cw.FUZZ_SEEDS_OBSTACLE)
def test_history_with_obstacles_and_views(seed, snapshot):
    _history(seed, snapshot, True)


@pytest.mark.parametrize("seed", cw.FUZZ_SEEDS_POSE)
def test_history_with_pose_sensor_and_mesh(seed, snapshot):
    _history(seed, snapshot, "pose")

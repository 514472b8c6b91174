"""GPU: long histories through the context's state table.  Eight fixed seeds, forty calls each, drawn from every entry point
of context_walk.CALLS plus whole fused and phased steps, each legal or deliberately illegal by the mirror.  At every boundary
(an integrate or an edit) the twin is rebuilt from what the public API shows; at every completed step the state, order, keys
and cell table are compared with it bit for bit, and after every call the particle set tracked by creation index on the host
must be what sph_download_owned, sph_download and sph_download_positions4 report."""
import pytest

import context_walk as cw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fuzz") / "fuzz.snap")
    cw.make_snapshot(path)
    return path


@pytest.mark.parametrize("seed", cw.FUZZ_SEEDS)
def test_history(seed, snapshot):
    ops = cw.fuzz_ops(seed)
    with cw.Walker(cw.FUZZ_CAPACITY, cw.DT_FLOW, snapshot) as w:
        w.twinning = True
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

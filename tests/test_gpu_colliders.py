"""GPU: sphere colliders (include/sph_hip.h: sph_set_colliders) -- the fused and the phased integrate against the numpy
model of tests/collider_model.py, an empty set against a context that never had one, a sphere moving through the dam,
z-slab runs against the one-context run bit for bit, the host class through the headless driver, and the refusals."""
import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

from gpufluidsimulator_amd import capi, ic, slab
from collider_model import advance, push
from slab_oracle_engine import make_case
from test_gpu_slabs import _comm, _same_bits

pytestmark = pytest.mark.gpu
F = np.float32
DT = float(ic.DEFAULT_DT)
BOX, GRID = (4.0, 4.0, 4.0), (64, 64, 64)          # cell edge 1/16; the 16^3 dam fills [-2, -1.5]^3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gpufluidsimulator_amd", "sph_headless")
EPS = F(1e-5)


def _dam():
    return ic.dam_break_lattice((16, 16, 16), BOX, jitter=True)


def _check_one_step(stepper):
    """One step of a context with a sphere (A) against one without (B), from the same upload: the particles the sphere
    does not touch keep every bit, the touched ones are the model applied to B's output, bit for bit (the rule is + - * /
    and sqrt on fp32, unfused: tests/test_gpu_collider_sums.py holds eight spheres to the same)."""
    pos, vel = _dam()
    c0, R, u = np.array([-1.75, -1.72, -1.74], F), F(0.1875), np.array([300.0, -150.0, 80.0], F)   # R = 3 cells, inside
    with capi.Context(pos.shape[0], box=BOX, grid=GRID) as a, capi.Context(pos.shape[0], box=BOX, grid=GRID) as b:
        a.set_colliders([c0], [R], [u])
        a.upload(pos, vel); b.upload(pos, vel)
        stepper(a); stepper(b)
        sa, sb = a.download(), b.download()
        assert np.array_equal(a.colliders()["centers"][0], (c0 + F(DT) * u).astype(F))
    want_p, want_v, touched = push(sb["pos"], sb["vel"], [c0], [R], [u], (-2, -2, -2), (2, 2, 2))
    assert touched.sum() >= 100, touched.sum()
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(sa[k][~touched].view(np.uint32), sb[k][~touched].view(np.uint32)), k
    assert np.array_equal(sa["pos"].view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(sa["vel"].view(np.uint32), want_v.view(np.uint32))
    return sa, sb, (c0, R)


def test_fused_step_against_the_model():
    _check_one_step(lambda c: c.step(DT, 1))


def _at_the_shell(sb, c0, R):
    """Particles whose distance from c0 is within 1e-6 of R + eps before the push (at most 3, usually none): the two step
    forms agree to a tolerance there, so one of them may push such a particle and the other not."""
    d = sb["pos"].astype(F) - c0
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    rp2 = F(R + EPS) ** 2
    tie = np.abs(r2.astype(np.float64) - rp2) <= 1e-6 * rp2
    assert tie.sum() <= 3, tie.sum()
    return tie


def test_phased_step_against_the_model_and_the_fused_step():
    sp, bp, (c0, R) = _check_one_step(lambda c: c.step_phased(DT, 1))
    sf, bf, _ = _check_one_step(lambda c: c.step(DT, 1))
    ok = ~(_at_the_shell(bp, c0, R) | _at_the_shell(bf, c0, R))
    # the tolerances of test_gpu_parity.py::test_fused_step_equals_phased_step
    assert np.abs(sf["pos"][ok] - sp["pos"][ok]).max() <= 1e-7 * 4
    assert np.abs(sf["vel"][ok].astype(np.float64) - sp["vel"][ok]).max() <= 2e-6 * np.abs(sp["vel"]).max()
    assert np.array_equal(sf["density"], sp["density"])


def _flowing():
    pos, vel = _dam()
    pos[:, 1] += F(0.5)
    vel[:, 0] = 300.0
    return pos, vel


def test_an_emptied_set_changes_no_bit():
    pos, vel = _flowing()
    with capi.Context(pos.shape[0], box=BOX, grid=GRID) as a, capi.Context(pos.shape[0], box=BOX, grid=GRID) as b:
        a.set_colliders([[-1.75, -1.2, -1.75], [0.0, 0.0, 0.0]], [0.2, 0.3], [[10.0, 0, 0], [0, 0, 0]])
        assert a.colliders()["radii"].size == 2
        a.set_colliders(np.zeros((0, 3)), np.zeros(0))
        assert a.colliders()["radii"].size == 0
        a.upload(pos, vel); b.upload(pos, vel)
        a.step(DT, 50); b.step(DT, 50)
        sa, sb = a.download(), b.download()
    for k in ("pos", "vel", "density", "pressure"):
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k


def test_a_moving_sphere_pushes_the_dam():
    pos, vel = _dam()
    n = pos.shape[0]
    c0, R = np.array([-1.80, -1.78, -1.75], F), F(0.125)
    u = np.array([833.0, 0.0, 0.0], F)                   # 300 steps of 5e-7: 0.125 = two cells along x
    uh = u / np.linalg.norm(u)
    rp = F(R + EPS)
    runs = {}
    for name, sphere in (("with", True), ("without", False)):
        with capi.Context(n, box=BOX, grid=GRID) as c:
            if sphere:
                c.set_colliders([c0], [R], [u])
            c.upload(pos, vel)
            done = 0
            for chunk in (50,) * 6:
                c.step(DT, chunk)
                done += chunk
                st = c.download()
                assert np.isfinite(st["pos"]).all() and np.isfinite(st["vel"]).all()
                assert (np.abs(st["pos"]) <= 2.0).all() and c.n == n
                if sphere:
                    cur = c.colliders()["centers"][0]
                    assert np.array_equal(cur, advance([c0], [u], DT, done)[0])
                    used = advance([c0], [u], DT, done - 1)[0]        # the centre the last step pushed with
                    dist = np.linalg.norm(st["pos"].astype(np.float64) - used, axis=1)
                    assert dist.min() >= rp - 1e-5 * 4.0, dist.min()
            runs[name] = (st, advance([c0], [u], DT, done - 1)[0])
    st, cen = runs["with"]
    d = st["pos"].astype(np.float64) - cen
    r = np.linalg.norm(d, axis=1)
    ahead = (r < rp + 0.1) & (d @ uh > 0.5 * r)           # within h of the shell, in front of the sphere
    assert ahead.sum() >= 20, ahead.sum()
    along = float((st["vel"][ahead] @ uh).mean())
    base = runs["without"][0]
    along0 = float((base["vel"][ahead] @ uh).mean())
    assert along > 0.2 * float(np.linalg.norm(u)), (along, along0)
    assert abs(along0) < 0.05 * float(np.linalg.norm(u)), (along, along0)


def _run_slabs_with_sphere(world, pos, vel, box, grid, steps, sphere, protocol, early_force):
    hub = slab.LocalComm.Hub(world)
    dev_hub = capi.LocalHub(world, timeout_s=60)
    results, errors = [None] * world, []

    def rank_main(r):
        try:
            sim = slab.NativeSlabSimulation(_comm(hub, dev_hub, r), box, grid, device_index=0, transport="local",
                                            particles=(pos, vel), early_force=early_force, protocol=protocol, colliders=sphere)
            cuts = list(sim.cuts)
            sim.run(DT, steps)
            sim.sync()
            results[r] = (sim.gather_state(), dict(sim.stats), cuts, sim.colliders(), sim.engine.n)
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=600)
    dev_hub.close()
    assert not errors, errors
    return results


@pytest.mark.parametrize("case,world,protocol,early", [("up", 3, 3, False), ("up", 3, 1, False), ("tall_up", 2, 3, True),
                                                       ("tall_up", 2, 1, True)])
def test_slab_runs_with_a_sphere_across_a_cut_match_one_context(case, world, protocol, early):
    pos, vel, box, grid = make_case(case)
    cell = box[2] / grid[2]
    min_layers = 4 if protocol == 1 else slab.MIN_SLAB_LAYERS
    hist = np.bincount(slab.cell_layer_of(pos[:, 2], box[2], grid[2]), minlength=grid[2])
    cut = slab.choose_cuts(hist, world, min_layers)[1]
    z_cut = -box[2] / 2 + cut * cell
    steps = 24
    R = F(0.05)                                           # below a cell edge: a push never moves a particle a whole layer
    u = np.array([0.0, 0.0, 2000.0], F)                   # 24 steps: 0.024 in z, from 0.02 below the cut to above it
    c0 = np.array([-1.8125, -1.8125, z_cut - 0.02], F)
    sphere = ([c0], [R], [u])
    res = _run_slabs_with_sphere(world, pos, vel, box, grid, steps, sphere, protocol, early)
    assert res[0][2][1] == cut
    with capi.Context(pos.shape[0], box=box, grid=grid) as c:
        c.set_colliders(*sphere)
        c.upload(pos, vel)
        c.step(DT, steps)
        ref, ref_col = c.download(), c.colliders()
        # the sphere touched the fluid, and ends on the other side of the cut
        d = ref["pos"] - ref_col["centers"][0]
        assert (np.linalg.norm(d, axis=1) < R + 0.02).sum() > 0
    assert ref_col["centers"][0][2] > z_cut
    assert sum(r[4] for r in res) == pos.shape[0]
    for r in res:
        assert np.array_equal(r[3]["centers"].view(np.uint32), ref_col["centers"].view(np.uint32))
    if early:
        assert all(r[1]["early_force_used"] == steps for r in res), [r[1] for r in res]
    if protocol == 1:
        assert all(r[1]["one_message_steps"] == steps - 1 for r in res), [r[1] for r in res]
    _same_bits(res[0][0], ref)


def test_headless_driver_collider_equals_c_abi_path():
    c0, R, u = (-1.75, -1.75, -1.75), 0.125, (500.0, 0.0, -250.0)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "state.bin")
        arg = "-collider=" + ",".join(repr(float(v)) for v in (*c0, R, *u))
        out = subprocess.run([EXE, "-benchmark", "-n=4096", "-box=4", "-i=5", "-nowarmup", arg, f"-out={f}"], check=True,
                             capture_output=True, text=True, timeout=300)
        assert "Throughput = " in out.stdout
        raw = np.fromfile(f, dtype=np.float32).reshape(2, 4096, 4)
    pos, vel = _dam()
    with capi.Context(4096, box=BOX, grid=GRID) as c:
        c.set_colliders([c0], [R], [u])
        c.upload(pos, vel)
        c.step(DT, 5)
        st = c.download()
    with capi.Context(4096, box=BOX, grid=GRID) as b:   # (and the sphere did move particles)
        b.upload(pos, vel)
        b.step(DT, 5)
        assert not np.array_equal(b.download()["pos"], st["pos"])
    assert np.array_equal(raw[0, :, :3].view(np.uint32), st["pos"].view(np.uint32))
    assert np.array_equal(raw[1, :, :3].view(np.uint32), st["vel"].view(np.uint32))


def test_headless_driver_refuses_a_collider_on_several_gpus():
    out = subprocess.run([EXE, "-benchmark", "-n=4096", "-box=4", "-i=1", "-gpus=2", "-onegpu", "-collider=0,0,0,0.1"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "-collider" in out.stderr


def test_invalid_sets_are_refused_and_change_nothing():
    L = capi.load()
    with capi.Context(64, box=BOX, grid=GRID) as c:
        c.set_colliders([[0.1, 0.2, 0.3]], [0.25], [[1.0, 2.0, 3.0]])
        before = c.colliders()

        def raw(rows):
            arr = (capi.Collider * max(len(rows), 1))()
            for j, (cen, r, vel) in enumerate(rows):
                arr[j].center[:] = cen
                arr[j].radius = r
                arr[j].velocity[:] = vel
            return arr

        ok = ([0.0, 0.0, 0.0], 0.1, [0.0, 0.0, 0.0])
        assert L.sph_set_colliders(c.h, 9, raw([ok] * 9)) == -1
        assert L.sph_set_colliders(c.h, 1, raw([([0.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0])])) == -1
        assert L.sph_set_colliders(c.h, 1, raw([([0.0, 0.0, 0.0], -1.0, [0.0, 0.0, 0.0])])) == -1
        assert L.sph_set_colliders(c.h, 1, raw([([float("nan"), 0.0, 0.0], 0.1, [0.0, 0.0, 0.0])])) == -1
        assert L.sph_set_colliders(c.h, 1, raw([([0.0, 0.0, 0.0], float("inf"), [0.0, 0.0, 0.0])])) == -1
        assert L.sph_set_colliders(c.h, 1, raw([([0.0, 0.0, 0.0], 0.1, [0.0, float("inf"), 0.0])])) == -1
        assert L.sph_set_colliders(c.h, 2, raw([ok, ([0.0, 0.0, 0.0], 0.0, [0.0, 0.0, 0.0])])) == -1   # all or nothing
        assert L.sph_set_colliders(None, 1, raw([ok])) == -1
        n = C.c_uint32()
        assert L.sph_get_colliders(None, C.byref(n), None) == -1
        after = c.colliders()
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        with pytest.raises(capi.SphError):
            c.set_colliders(np.zeros((9, 3)), np.full(9, 0.1))

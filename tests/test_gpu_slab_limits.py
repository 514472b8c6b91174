"""GPU: the slab step where it fails and at its limits -- a re-cut that overflows one rank, the one-message step with message
buffers smaller than its size rule asks for, and the write / wait-value sequence numbers just under the point where the slab
gives them up.  Ranks are threads of one process on one GPU over the device-to-device transport, as in tests/test_gpu_slabs.py;
the systems are tests/slab_oracle_engine.py's."""
import ctypes as C
import gc
import os
import time

import pytest

from gpufluidsimulator_amd import capi
from slab_oracle_engine import CLAMP_CASE, make_case, one_cap, slab_buffers
from test_gpu_slabs import DT, _exchanges_ok, _same_bits, _whole_domain, _with_ranks

pytestmark = pytest.mark.gpu
E_CAPACITY, E_PEER = -4, -6
HOP_SEQ_LIMIT = 0x7FFFFFF0           # csrc/sph_slab.hip: a slab with an edge at this number orders its streams by events from then on


def _last_error():
    return capi.load().sph_last_error().decode()


@pytest.mark.parametrize("protocol", [3, 1])
def test_a_recut_that_overflows_one_rank_reaches_every_rank_within_steps_not_timeouts(protocol):
    """Three ranks own 8 cell layers of 288 particles each (24 layers; under the one-message protocol a slab keeps four); the top
    rank has room for exactly the 2304 particles it starts with.  After two steps (nobody has crossed a cut yet; the one-message
    protocol has learnt its sizes) every rank calls sph_slab_recut with the top cut one layer lower: rank 2 is owed a layer it
    cannot hold.  It takes part in every round, returns SPH_E_CAPACITY and is failed as a failed step is: its abort header is the
    first message of the step its neighbour takes next.  So ranks 0 and 1 get SPH_OK from the re-cut, rank 1 SPH_E_PEER from its
    first step after it, rank 0 from its second (slab_fail: one rank per step), and rank 2 the same SPH_E_CAPACITY from every
    later call.  Time-outs are 60 s; everybody is done in under 30, every slab closes and the library holds what it held before.
    (Before the fix rank 2 sent nothing and rank 1 sat out the time-out.)"""
    gc.collect()
    base = capi.memory_stats()
    pos, vel, box, grid = make_case("tall_up")
    L = capi.load()
    t0 = time.perf_counter()

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), protocol=protocol, capacity_factor=1.0 if r == 2 else 1.5,
                   capacity_slack=0 if r == 2 else 4096)
        try:
            capi._check(L.sph_slab_set_wait_timeout(sim._slab, 60.0))
            cuts, owned = list(sim.cuts), sim.engine.n
            sim.run(DT, 2)
            sim.sync()
            one_ready = sim.stats["one_message_steps"]
            new = [cuts[0], cuts[1], cuts[2] - 1, cuts[3]]
            sim.comm.barrier()
            rc = L.sph_slab_recut(sim._slab, new[r], new[r + 1])
            calls = [(rc, _last_error() if rc else "", L.sph_slab_failed(sim._slab))]
            for _ in range(4):
                rc = L.sph_slab_step(sim._slab, DT, 1)
                calls.append((rc, _last_error() if rc else "", L.sph_slab_failed(sim._slab)))
            rc = L.sph_slab_recut(sim._slab, cuts[r], cuts[r + 1])                  # (a failed slab refuses before it sends)
            calls.append((rc, _last_error() if rc else "", L.sph_slab_failed(sim._slab)))
            return cuts, owned, sim.capacity, one_ready, calls, time.perf_counter() - t0
        finally:
            sim.close()

    out, errors = _with_ranks(3, body, timeout_s=200)
    took = time.perf_counter() - t0
    assert errors == [None] * 3, errors
    print("re-cut overflow, protocol", protocol, ": ranks done after", [round(o[5], 2) for o in out], "s; all closed after", round(took, 2), "s")
    assert all(o[0] == [0, 8, 16, 64] for o in out) and [o[1] for o in out] == [2304] * 3 and out[2][2] == 2304, [o[:3] for o in out]
    assert all(o[3] == (1 if protocol == 1 else 0) for o in out), "the step before the re-cut was a one-message step"
    top, mid, low = out[2][4], out[1][4], out[0][4]
    assert top[0][0] == E_CAPACITY and "hold 2592 particles, the capacity is 2304" in top[0][1], top
    assert all(c[0] == E_CAPACITY and c[2] == E_CAPACITY and c[1] == top[0][1] for c in top), top      # the same code, the same cause
    assert mid[0] == (0, "", 0) and low[0] == (0, "", 0), (mid, low)
    assert mid[1][0] == E_PEER and "upper neighbour reported a failure" in mid[1][1] and mid[1][2] == E_PEER, mid
    assert low[1] == (0, "", 0), low
    assert low[2][0] == E_PEER and "upper neighbour reported a failure" in low[2][1] and low[2][2] == E_PEER, low
    assert all(c[0] == E_PEER for c in mid[1:] + low[2:]), (mid, low)
    assert max(o[5] for o in out) < 30.0 and took < 30.0, ([o[5] for o in out], took)        # nobody sat out a 60 s time-out
    assert capi.memory_stats() == base


def test_one_message_step_with_sizes_cut_down_to_the_buffers_matches_whole_domain():
    """slab_oracle_engine.CLAMP_CASE: three slabs under the one-message protocol with a ghost capacity of 1024 and a migrant
    capacity of 512, so that the message buffers hold 1600 records where the size rule asks for 1664 (a link's usual 576 records)
    and 1792 / 1536 (the two directions on the step after a lattice plane crossed).  Every message fits -- the CPU ranks of
    tests/test_slab_cpu.py::test_clamp_case_premises count at most 720 records, 576 ghosts and 144 leavers -- so the run goes
    through with the sizes cut down to the buffers (it used to be refused with SPH_E_CAPACITY at its second step) and has the
    bits of the one-context run.  On every one-message step of every rank one direction of a link carried at least 576 the step
    before, so each of them is counted as cut down; a message cut down to 1600 still holds its 720 at most, so none needs a
    second message."""
    cc = CLAMP_CASE
    pos, vel, box, grid = make_case(cc["case"])
    steps, world = cc["steps"], cc["world"]
    gcap, mcap, msg_cap = slab_buffers(288, cc["ghost_factor"], cc["migrant_capacity"])
    assert one_cap(432) < msg_cap < one_cap(576) < one_cap(720)
    t0 = time.perf_counter()

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), protocol=1, ghost_factor=cc["ghost_factor"],
                   migrant_capacity=cc["migrant_capacity"])
        try:
            sizes = (sim.per_layer, sim.ghost_capacity, list(sim.cuts))
            sim.run(DT, steps)
            sim.sync()
            return sim.gather_state(), dict(sim.stats), sizes
        finally:
            sim.close()

    out, errors = _with_ranks(world, body, timeout_s=200)
    assert errors == [None] * world, errors                             # no rank returned an error
    stats = [o[1] for o in out]
    print("sizes cut down to the buffers:", [s["one_message_clamped"] for s in stats], "of", [s["one_message_steps"] for s in stats],
          "one-message steps; migrants", [s["migrants"] for s in stats], "; ran", round(time.perf_counter() - t0, 2), "s")
    assert all(o[2] == (288, gcap, [0, 8, 16, 64]) for o in out), [o[2] for o in out]
    assert all(s["protocol"] == 1 and s["one_message_steps"] == steps - 1 for s in stats), stats
    assert all(s["one_message_clamped"] >= 1 for s in stats), stats
    assert all(s["one_message_clamped"] == s["one_message_steps"] for s in stats), stats
    assert all(_exchanges_ok(s) and s["one_message_rests"] == 0 and s["rest_messages"] == 0 for s in stats), stats
    assert sum(s["migrants"] for s in stats) > 0 and all(s["host_waits"] == steps for s in stats), stats
    _same_bits(out[0][0], _whole_domain(pos, vel, box, grid, steps))


@pytest.mark.parametrize("protocol", [3, 1])
@pytest.mark.parametrize("below", [3, 1])
def test_hop_sequence_numbers_at_their_limit_switch_the_slab_to_events(below, protocol):
    """The step's cross-stream edges are 32-bit sequence numbers waited for with "word >= number": they must not wrap.  Two slabs
    of 12 layers with the early force launch on (four of the five edges are taken every step -- main to comm 1 mark, comm to main
    2, the early launch's fork and join 1 each, as the run prints; the fifth, the deep-density edge, is for sparse slabs), two
    steps, then the test hook puts every edge's counter and word `below` marks under HOP_SEQ_LIMIT -- 3: the busiest edge crosses
    the limit in the middle of the second step; 1: at its first mark -- and ten more steps follow.  The step that crosses the
    limit still runs by value (the slab looks only on entry to a call); from its next call on the slab orders by events, for
    good, with the counters left where they stood.  Same bits as the one-context run after twelve steps."""
    if os.environ.get("SPH_SLAB_HOPS", "")[:1] == "e":
        pytest.skip("SPH_SLAB_HOPS=event: the slabs order their streams by events from the start, there is no sequence number")
    pos, vel, box, grid = make_case("tall_up")
    L = capi.load()
    preset = HOP_SEQ_LIMIT - below
    t0 = time.perf_counter()

    def hops(sim):
        out = (C.c_uint32 * 6)()
        capi._check(L.sph_slab_test_hop_state(sim._slab, out))
        return int(out[0]), [int(v) for v in out[1:]]

    def body(make, r):
        sim = make(box=box, grid=grid, particles=(pos, vel), early_force=True, protocol=protocol)
        try:
            first = hops(sim)
            sim.run(DT, 2)
            sim.sync()
            used = hops(sim)
            sim.comm.barrier()
            capi._check(L.sph_slab_test_set_hop_seq(sim._slab, preset))
            seen = [hops(sim)]
            sim.comm.barrier()
            for _ in range(10):
                sim.run(DT, 1)
                seen.append(hops(sim))
            sim.sync()
            refused = L.sph_slab_test_set_hop_seq(sim._slab, 0)           # (a slab that orders by events has nothing to set)
            return sim.gather_state(), first, used, seen, refused, dict(sim.stats)
        finally:
            sim.close()

    out, errors = _with_ranks(2, body, timeout_s=200)
    assert errors == [None] * 2, errors
    print("hops", below, "under the limit, protocol", protocol, ": by value after each step", [[s[0] for s in o[3]] for o in out],
          "; marks per edge in the step after the preset", [[b - a for a, b in zip(o[3][0][1], o[3][1][1])] for o in out],
          "; ran", round(time.perf_counter() - t0, 2), "s")
    for state, first, used, seen, refused, stats in out:
        assert first[0] == 1, "this device serves write / wait value: the slab starts by value"
        assert used[0] == 1 and used[1][0] > first[1][0] and used[1][1] > first[1][1], (first, used)
        assert seen[0] == (1, [preset] * 5), seen[0]
        assert seen[1][0] == 1 and max(seen[1][1]) > preset, "the step after the preset still ran by value"
        assert max(seen[1][1]) >= HOP_SEQ_LIMIT or below > 1, seen[1]
        by_value = [s[0] for s in seen]
        assert by_value == sorted(by_value, reverse=True) and by_value[3:] == [0] * 8, by_value       # switched once, within three steps
        gone = by_value.index(0)
        assert max(seen[gone - 1][1]) >= HOP_SEQ_LIMIT and all(s[1] == seen[gone - 1][1] for s in seen[gone:]), seen
        assert max(seen[-1][1]) < HOP_SEQ_LIMIT + 64, seen[-1]
        assert refused == -5                                               # SPH_E_STATE
        assert stats["steps"] == 12 and stats["early_force_used"] == 12, stats
    _same_bits(out[0][0], _whole_domain(pos, vel, box, grid, 12))

"""The kernels a few small scenarios launch, in order -- to show that a host-only change launches what its parent launched.
    rocprofv3 --kernel-trace --output-format csv -d OUT -o a -- python profiles/scripts/launch_sequence.py      (GPU box, repo root;
        SPH_HIP_LIB picks another build of the library)
    python profiles/scripts/launch_sequence.py compare A_kernel_trace.csv B_kernel_trace.csv [more.csv ...]
Every scenario synchronises after every step, so that no decision of the host (merge or full sort, a skipped sort) hangs
on how far it runs ahead of the device.  `compare` lists the kernels of the one process a trace file holds in dispatch order
as (name, grid, workgroup) -- per hardware queue, per stream and per host thread (a slab rank is a thread) -- and compares
the first trace with the third and later ones; the first two are runs of the same library, and what differs between them (the
runtime deals the streams of several threads onto a few hardware queues as they come) is left out and named."""
import csv, os, sys, threading
from collections import defaultdict

DT = 5e-7


def sequences(path, key):
    per = defaultdict(list)
    for r in csv.DictReader(open(path)):
        per[tuple(r[k] for k in key)].append((int(r["Dispatch_Id"]), r["Kernel_Name"],
                                               (r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]),
                                               (r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"])))
    # (queue and thread ids differ from run to run: a sequence is known by its content, the longest first)
    return sorted(([d[1:] for d in sorted(v)] for v in per.values()), key=lambda s: (-len(s), s))


def compare(paths):
    """paths[0] and paths[1]: two runs of the same library; what differs between them is noise and is left out below"""
    bad = 0
    for what, key in (("hardware queue", ("Agent_Id", "Queue_Id")), ("stream", ("Stream_Id",)), ("host thread", ("Thread_Id",))):
        seqs = [sequences(p, key) for p in paths]
        print(f"per {what}:")
        for p, q in zip(paths, seqs):
            print(f"  {p}: launches {[len(s) for s in q]}")
        noisy = [k for k, (a, b) in enumerate(zip(seqs[0], seqs[1])) if a != b] if len(seqs[0]) == len(seqs[1]) else list(range(len(seqs[0])))
        print(f"  {paths[0]} vs {paths[1]} (same library twice): " + (f"sequences {noisy} differ: left out" if noisy else "all equal"))
        for p, q in zip(paths[2:], seqs[2:]):
            diff = [k for k in range(max(len(q), len(seqs[0]))) if k not in noisy and (k >= len(q) or k >= len(seqs[0]) or q[k] != seqs[0][k])]
            print(f"  {paths[0]} vs {p}: " + (f"sequences {diff} DIFFERENT" if diff else f"EQUAL in all {len(seqs[0]) - len(noisy)} sequences compared"))
            bad += len(diff)
            for k in diff:
                if k < len(q) and k < len(seqs[0]):
                    a, b = seqs[0][k], q[k]
                    d = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                    print(f"    sequence {k}: first difference at launch {d} of {len(a)} / {len(b)}: {a[d:d + 1]} / {b[d:d + 1]}")
    return bad


def whole_domain():
    import numpy as np
    from gpufluidsimulator_amd import capi, ic
    cfg = ic.CONFIGS["C1"]
    pos, vel = ic.dam_break_lattice(cfg["lattice"], cfg["box"], jitter=True)
    # every particle its own velocity, a cell in ~30 steps: a few per cent of movers in EVERY step (a lattice that moves as
    # one crosses a cell face layer by layer: bursts with nothing in between)
    flow = np.random.default_rng(1).uniform(-4000.0, 4000.0, vel.shape).astype(np.float32)
    with capi.Context(pos.shape[0] + 512, box=cfg["box"], grid=cfg["grid"]) as c:
        def steps(k):
            for _ in range(k):
                c.step(DT)
                c.sync()
        c.upload(pos, flow); steps(40)     # the merge path
        print("flow", c.sort_stats())
        c.upload(pos, vel); steps(10)      # at rest: skipped sorts
        print("rest", c.sort_stats())
        c.set_sort_mode(0); steps(10)      # the full sort
        c.set_sort_mode(1)
        for _ in range(5):                 # phase by phase
            c.hash(); c.sort(); c.build_cells(); c.density(); c.force(); c.collide(); c.integrate(DT)
            c.sync()
        c.emit(pos[:100] + np.float32(0.01), flow[:100]); c.sync()
        gone = c.remove(capi.Region.sphere(pos.mean(axis=0), 0.2)); c.sync()
        steps(1)
        print("edit", len(gone), c.sort_stats())


def slabs(protocol):
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    from gpufluidsimulator_amd import capi, slab
    from slab_oracle_engine import make_case
    pos, vel, box, grid = make_case("shear")
    world = 3
    hub, dev_hub = slab.LocalComm.Hub(world), capi.LocalHub(world, timeout_s=60)
    errors = []

    def rank_main(r):
        try:
            comm = slab.LocalComm(hub, r)
            comm.local_hub = dev_hub
            sim = slab.NativeSlabSimulation(comm, box, grid, device_index=0, transport="local", particles=(pos, vel), protocol=protocol,
                                            capacity_factor=3.2)
            for k in range(24):
                sim.run(DT, 1)
                sim.sync()
                if k == 11:                # one rebalance, to cuts given by hand (slabs of >= 4 layers: the one-message step)
                    sim.rebalance(cuts=[0, 6, 10, grid[2]])
            print("slabs, protocol", protocol, "rank", r, {k: sim.stats[k] for k in ("migrants", "resorts", "in_place_merges", "rebalances")})
            sim.close()
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
            hub.bar.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads: t.start()
    for t in threads: t.join(timeout=300)
    dev_hub.close()
    if errors:
        raise errors[0]


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "compare":
        sys.exit(1 if compare(sys.argv[2:]) else 0)
    sys.path.insert(0, os.getcwd())
    import torch  # noqa
    whole_domain()
    slabs(3)
    slabs(1)

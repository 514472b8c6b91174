"""Price of the push over a SET of obstacle slots (sph_obstacle_select; k_obstacle_push_set) next to the push of one obstacle
(k_obstacle_push), at BASELINE config 3 (16,777,216 particles): the flowing dam with the box pillar of
profiles/scripts/obstacle_time.py on its local grid, stepped in windows that go round the variants three times --

    one     the pillar in slot 0 alone: the kernels of a library of one obstacle
    two     the pillar in slot 0 and a second, smaller block in slot 1: one k_obstacle_push_set
    four    the pillar and three small blocks, all four slots
    one_in_slot_1  (reference) the pillar alone, but installed in slot 1: k_obstacle_push_set with one slot

-- small solids, so nearly every wave leaves at the guard's ballot.  Prints the windows' wall clock per step and, as "plan", the
variant and the number of integrates of every window in order: every integrate launches exactly one push kernel, so the n-th
k_obstacle_push* dispatch of a kernel trace belongs to a known window.  Run from the repo root under the kernel trace

    rocprofv3 --kernel-trace --output-format csv -d OUT -o p -- python profiles/scripts/obstacle_set_time.py [warm steps] > OUT/run.json
    python profiles/scripts/obstacle_set_time.py --trace OUT/run.json OUT/<...>/p_kernel_trace.csv

The second form prints per variant the median, minimum and maximum of the push kernel's duration over the timed windows, and
the launches per step of the first timed `one` window by kernel name.  With a
library of before the slots (SPH_HIP_LIB=..., SPH_HIP_LIB_ALLOW_MISSING=1) only `one` runs: the parent's figure."""
import csv
import json
import statistics
import sys
import time

WINDOW, SETTLE, ROUNDS = 50, 5, 3


def trace(run_json, trace_csv):
    plan = json.load(open(run_json))["plan"]
    rows, every = [], []
    with open(trace_csv, newline="") as f:
        for r in csv.DictReader(f):
            every.append((int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0]))
            if "k_obstacle_push" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    assert len(rows) == sum(p["integrates"] for p in plan), (len(rows), sum(p["integrates"] for p in plan))
    at, per = 0, {}
    for p in plan:
        mine = rows[at:at + p["integrates"]]
        at += p["integrates"]
        if p["timed"] and p["variant"] == "one" and "one" not in per:      # the launches of this window's steps, by name
            names = {}
            for t, name in every:
                if mine[0][0] < t <= mine[-1][0]:
                    names[name] = names.get(name, 0) + 1
            steps_of_one = {k: round(v / (len(mine) - 1), 3) for k, v in sorted(names.items())}
        if p["timed"]:
            d = per.setdefault(p["variant"], {"us": [], "kernels": set()})
            d["us"] += [(e - s) / 1e3 for s, e, _ in mine]
            d["kernels"] |= {name.split("(")[0] for _, _, name in mine}
    print(json.dumps({v: {"kernel": sorted(d["kernels"]), "dispatches": len(d["us"]), "median_us": round(statistics.median(d["us"]), 2),
                          "min_us": round(min(d["us"]), 2), "max_us": round(max(d["us"]), 2),
                          "p10_us": round(sorted(d["us"])[len(d["us"]) // 10], 2), "p90_us": round(sorted(d["us"])[len(d["us"]) * 9 // 10], 2)}
                      for v, d in per.items()} | {"launches_per_step_of_one": steps_of_one}, indent=1))


def main():
    import torch  # noqa: F401  (first: the HIP runtime torch bundles must be the one that gets loaded, see capi.load)

    sys.path.insert(0, ".")
    from gpufluidsimulator_amd import capi, ic

    warm = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
    cfg = ic.CONFIGS["C3"]
    n = cfg["lattice"][0] * cfg["lattice"][1] * cfg["lattice"][2]
    dt = float(ic.DEFAULT_DT)
    cell = cfg["box"][0] / cfg["grid"][0]

    def block(centre, half):
        return ([capi.Shape.box(centre, half)], cell,
                (tuple(c - h - 4.0 * cell for c, h in zip(centre, half)), tuple(c + h + 4.0 * cell for c, h in zip(centre, half))))

    pillar = block((-11.0, -13.0, -12.0), (4.0 * cell, 3.0, 4.0 * cell))
    small = [block((-9.0, -14.0, -10.0), (3.0 * cell, 1.0, 3.0 * cell)), block((-13.0, -14.5, -9.0), (2.0 * cell, 0.5, 6.0 * cell)),
             block((-10.0, -15.0, -14.0), (6.0 * cell, 0.4, 2.0 * cell))]
    has_slots = hasattr(capi.load(), "sph_obstacle_select")
    variants = ("one", "two", "four", "one_in_slot_1") if has_slots else ("one",)
    layout = {"one": {0: pillar}, "two": {0: pillar, 1: small[0]}, "four": {0: pillar, 1: small[0], 2: small[1], 3: small[2]},
              "one_in_slot_1": {1: pillar}}
    windows = {v: [] for v in variants}
    plan = []
    with capi.Context(n, box=cfg["box"], grid=cfg["grid"]) as c:
        c.reset_lattice(cfg["lattice"], jitter=True)
        c.step(dt, warm)
        if has_slots:                                      # every solid clears its place before anything is timed
            for k, b in layout["four"].items():
                c.build_obstacle(*b, slot=k)
        else:
            c.build_obstacle(*pillar)
        c.step(dt, 100); c.sync()
        plan.append({"variant": "settle", "integrates": 100, "timed": False})
        for w in range(ROUNDS * len(variants)):
            name = variants[w % len(variants)]
            if has_slots:
                c.clear_obstacles_all()
                for k, b in layout[name].items():
                    c.build_obstacle(*b, slot=k)
            c.step(dt, SETTLE); c.sync()
            plan.append({"variant": name, "integrates": SETTLE, "timed": False})
            t0 = time.perf_counter()
            c.step(dt, WINDOW); c.sync()
            windows[name].append(round((time.perf_counter() - t0) / WINDOW * 1e3, 4))
            plan.append({"variant": name, "integrates": WINDOW, "timed": True})
    print(json.dumps({"particles": n, "warm_steps": warm, "slots": has_slots, "ms_per_step": windows,
                      "median_ms": {k: statistics.median(v) for k, v in windows.items()}, "plan": plan}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        trace(sys.argv[2], sys.argv[3])
    else:
        main()

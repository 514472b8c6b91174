"""The context's state table ("What is stale after X") as something a test can execute -- TEST
INFRASTRUCTURE, in the style of sph_model.py and region_model.py.

Three things live here, all of them plain data or plain Python:

  Mirror   the OBSERVABLE columns of the table (stage, order_valid, have_dens / have_force / have_coll, sort_form_both_until,
           n, next_index) in a few dozen lines.  apply(op) follows TABLE -- the four columns of DESIGN's table, word for word;
           tests/test_context_walk_cpu.py parses the document and compares -- and the SPH_REQUIRE conditions of the phase
           calls, and says "accepted" (0) or SPH_E_STATE for any call, and which phase calls must now be refused.

  Walker   a context under test, its Mirror, its TWIN and, where an obstacle is about, a BARE twin (the twin without the obstacle:
           the first integrate behind a boundary must be obstacle_model.push of ITS output) and a numpy record of the obstacle.  The twin is the expected value of everything that is NOT
           observable (keys_fresh, the mover marks, the cell table, the scan bookkeeping): a FRESH context that is given what
           the public API showed at the last BOUNDARY -- the last moment particles changed: an integrate or an edit -- by
           sph_upload in slot order, with the same parameters, colliders, bodies and settings, and that then makes the calls
           the context under test has made since.  The two have different histories (merge sort against full sort, deferred
           table clear against none, fresh keys against a hash) and the same inputs call for call, so they agree bit for bit.

  PREFIXES, CALLS, continuation(), fuzz_ops()   the states, the calls that cross them and the long histories, as data: the
           GPU tests run them, the CPU test walks them through a Mirror alone and proves the coverage.

An op is a tuple (name, args...); call_id() names it.  Nothing here peeks into the struct."""
import numpy as np

import obstacle_model as om
import region_model

LOADED, HASHED, SORTED, CELLS = 0, 1, 2, 3
STAGES = {"LOADED": LOADED, "HASHED": HASHED, "SORTED": SORTED, "CELLS": CELLS}
E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5

# ---- entry point -> (stage, order_valid, have_*, sort_form_both_until) ------------------------------------
COLUMNS = ("stage", "order_valid", "have_*", "sort_form_both_until")
_INSTALL = ("set LOADED", "cleared", "cleared", "set")
_NONE = ("kept", "kept", "kept", "kept")
TABLE = {
    "sph_upload": _INSTALL, "sph_snapshot_load": _INSTALL, "sph_reset_lattice": _INSTALL,
    "sph_set_by_index": ("set LOADED", "kept", "cleared", "set"),
    "sph_set_params": ("kept", "cleared", "kept", "set"),
    "sph_remove": ("set LOADED", "kept", "cleared", "set"),
    "sph_emit": ("set LOADED", "cleared", "cleared", "set"),
    "sph_set_collider_bodies": _NONE, "sph_set_colliders": _NONE,
    "sph_sort": ("set SORTED", "set", "cleared", "kept"),
    "force_finish": _NONE,
    "sph_obstacle_build": _NONE,         # ... and _set_grid, _clear, _set_motion, _sample: one row of the document
    "sph_mesh_extract": _NONE,           # the views: sph_render, sph_render_surface, sph_mesh_extract, one row as well
}
# rows of the document that a whole-domain context under the native API cannot execute (named by an identifier of their
# first cell): not walked, and said so
SKIPPED_ROWS = {
    "sph_migrants_append": "slab contexts only",
    "step_settle": "sph_slab_step only",
    "set_slab_range": "sph_slab_recut only",
    "cudaMapZIndex": "the compat seam's own entry point",
    "launch_merge_arrivals": "sph_slab_step only",
}

PHASES = ("hash", "sort", "build_cells", "density", "force", "collide", "integrate", "fci")
EDITS = ("upload", "load_snapshot", "reset_lattice", "set_by_index", "emit", "remove")

BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)
DT_FLOW, DT_REST = 2e-5, 5e-7
SNAP_N, SNAP_SEED = 3000, 7
SBI_FIRST, SBI_COUNT = 100, 300                 # creation indices every installed set of this module holds
# regions of sph_remove: z-slabs of 0.05 (every set of this module has particles in each of 0 .. 4: the lattices have a layer
# every 0.03125 from -0.984 up to -0.766 at least, the random boxes fill z in [-1, -0.1); slab 5 is for the histories, which hold
# the random boxes when they get there); no box variant below moves a z wall
REGIONS = {k: [("box", (-4.0, -4.0, -1.0 + 0.05 * k), (4.0, 4.0, -1.0 + 0.05 * (k + 1)))] for k in range(6)}
REGIONS["none"] = [("box", (0.5, 0.5, 0.5), (0.75, 0.75, 0.75)), ("sphere", (0.5, 0.5, -0.5), 0.2)]
PARAM_VARIANTS = ("P0", "visc", "shift", "wall")
COLLIDER = (np.array([[-0.5, -0.6, -0.55]], np.float32), np.array([0.12], np.float32), np.array([[300.0, 0.0, -200.0]], np.float32))
BODY = (np.array([2.0e4], np.float32), np.array([[0.0, -9.81 * 11000, 0.0]], np.float32))
# the solid of ("obstacle_build", "both"): a ramp under the fluid and a pillar in it (it touches particles of EVERY set this
# module installs: tests/test_context_walk_cpu.py), and the motion of ("obstacle_motion", "on")
OBSTACLE_SPACING = 1.0 / 16.0
OBSTACLES = {"both": [om.halfspace((-0.9, -0.93, 0.0), (-0.5, 1.0, 0.0)), om.box((-0.55, -0.6, -0.5), (0.1, 0.4, 0.1))]}
MOTION = {"on": (np.array([0.013, -0.007, 0.004], np.float32), np.array([300.0, 0.0, -200.0], np.float32)),
          "off": (np.zeros(3, np.float32), np.zeros(3, np.float32))}
CALLER_GRID = {"dims": (23, 21, 19), "origin": np.array([-1.13, -1.11, -1.07], np.float32), "spacing": np.float32(0.1)}
OBSTACLE_OPS = ("obstacle_build", "obstacle_set_grid", "obstacle_motion", "obstacle_clear", "obstacle_sample")
VIEWS = ("render", "render_surface", "extract_mesh")
MESH = dict(spacing=1.0 / 16.0, radius=1.0 / 8.0)


def caller_field(seed):
    """the field of ("obstacle_set_grid", seed): a ball in the fluid, roughened -- no distance"""
    x, y, z = (a.astype(np.float64) for a in om.node_positions(CALLER_GRID))
    d = np.sqrt((x[None, None, :] + 0.6) ** 2 + (y[None, :, None] + 0.8) ** 2 + (z[:, None, None] + 0.6) ** 2) - 0.35
    return (d + np.random.default_rng(seed).normal(0.0, 0.02, d.shape)).astype(np.float32)


def sample_points():
    return np.random.default_rng(77).uniform(-1.2, 1.2, (500, 3)).astype(np.float32)


def params_variant(name):
    """P0: the defaults; visc: a physics field only; shift: the box moved by a non-dyadic amount in x and y; wall: the lower x
    wall moved inward past particles (cells of another width)."""
    from gpufluidsimulator_amd import capi
    p = capi.default_params(BOX, GRID)
    if name == "visc":
        p.viscosity = 400.0
    elif name == "shift":
        for a in (0, 1):
            p.box_min[a] = float(np.float32(p.box_min[a]) + np.float32(0.0123))
            p.box_max[a] = float(np.float32(p.box_max[a]) + np.float32(0.0123))
    elif name == "wall":
        p.box_min[0] = -0.8
    elif name != "P0":
        raise KeyError(name)
    return p


def call_id(op):
    name = op[0]
    if name == "set_by_index": return f"set_by_index:{op[1]}"
    if name == "emit": return "emit:explicit" if op[3] else "emit:auto"
    if name == "remove": return "remove:nothing" if op[1] == "none" else "remove:something"
    if name in ("set_params", "set_colliders", "set_collider_bodies", "set_precision", "set_sort_mode", "obstacle_build",
                "obstacle_motion"): return f"{name}:{op[1]}"
    return name


# ---- the mirror --------------------------------------------------------------------------------------------------------------
class Mirror:
    """The observable state of one whole-domain context, advanced by the table -- never by the library."""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.stage, self.order_valid = LOADED, False
        self.have_dens = self.have_force = self.have_coll = False
        self.n = self.next_index = 0
        self.sort_calls = self.both_until = 0
        # not columns of the table, but what a prediction or a twin needs
        self.integrated = False          # an integrate ran since the last hash: keys, table and results are the step's, not the positions'
        self.sort_mode, self.precision = 1, 0
        self.direct_hull, self.small_launch, self.block_order = None, None, None
        self.params = self.params_at_hash = "P0"
        self.n_colliders, self.tracked = 0, False
        self.obstacle, self.motion = None, None     # the installed grid (None, or a tag that names the field) and the last motion set
        self.ob_steps = 0                # integrates that advanced the obstacle's offset (those with a grid installed)
        self.sorts = []                  # what apply() predicted for the sorts of the last op: (merge: True/False/None, both forms: True/False/None)
        self.reached, self.calls = set(), set()     # coverage: (row, column, observable), (stage, call id)

    # -- the table ------------------------------------------------------------------------------------------------------------
    def _window(self):
        return self.both_until > self.sort_calls          # the next sort still launches both forms

    def _row(self, name):
        stage, order, have, forms = TABLE[name]
        had = self.have_dens or self.have_force or self.have_coll
        prior = {"stage": self.stage, "order_valid": self.order_valid, "have_*": had, "sort_form_both_until": self._window()}
        if stage.startswith("set"):
            self.stage = STAGES[stage.split()[1]]
            if self.stage == LOADED:
                self.integrated = False
        if order != "kept":
            self.order_valid = order == "set"
        if have == "cleared":
            self.have_dens = self.have_force = self.have_coll = False
        if forms == "set":
            self.both_until = self.sort_calls + 5
        for col, word in zip(COLUMNS, (stage, order, have, forms)):
            w = word.split()[0]
            if w == "set":       # shows where the field was something else
                seen = prior[col] != (self.stage if col == "stage" else True)
            else:                # kept / cleared: shows where there was something to lose
                seen = prior[col] != LOADED if col == "stage" else bool(prior[col])
            self.reached.add((name, col, bool(seen)))

    # -- the phase calls (SPH_REQUIRE of each) -----------------------------------------------------------------------------------
    def accepts(self, name):
        s = self.stage
        if name == "sort": return s == HASHED
        if name == "build_cells": return s >= SORTED
        if name in ("density", "collide"): return s >= CELLS
        if name in ("force", "fci"): return s >= CELLS and self.have_dens
        if name == "integrate": return self.have_dens and self.have_force and self.have_coll
        if name == "download_forces": return self.have_force and self.have_coll
        return True

    def refused_phases(self):
        return [p for p in PHASES if not self.accepts(p)]

    def mid_step(self):
        """the keys, the table and the results in place are those of the particles as they are now"""
        return self.stage >= HASHED and not self.integrated

    def _hash(self):
        self.stage, self.integrated, self.params_at_hash = HASHED, False, self.params

    def _sort(self):
        if self.n:
            self.sort_calls += 1
            merge = False if (self.sort_mode == 0 or not self.order_valid) else (True if self.sort_mode == 2 else None)
            self.sorts.append((merge, None if merge is None else (merge and self.sort_calls <= self.both_until)))
        self._row("sph_sort")

    def _fused(self):
        self._row("force_finish")
        self.have_force = self.have_coll = False
        self.integrated = True
        self.ob_steps += self.obstacle is not None

    def _phase(self, name):
        if name == "hash": self._hash()
        elif name == "sort": self._sort()
        elif name == "build_cells": self.stage = CELLS
        elif name == "density": self.have_dens = True
        elif name == "force": self.have_force = True
        elif name == "collide": self.have_coll = True
        elif name == "integrate":
            self.have_force = self.have_coll = False; self.integrated = True
            self.ob_steps += self.obstacle is not None
        elif name == "fci": self._fused()

    # -- every entry point -------------------------------------------------------------------------------------------------------
    def apply(self, op, selected=None):
        """The return code the library must give, after advancing the mirror.  selected: what sph_remove selects (a dry walk
        does not know the particles: a region other than "none" then counts as one particle)."""
        name = op[0]
        self.sorts = []
        self.calls.add((self.stage, call_id(op)))
        if name in PHASES:
            if not self.accepts(name): return E_STATE
            self._phase(name)
        elif name in ("step", "step_phased", "step_until_skipped"):
            tail = ("fci",) if name != "step_phased" else ("force", "collide", "integrate")
            for _ in range(int(op[1])):
                for ph in ("hash", "sort", "build_cells", "density") + tail:
                    self._phase(ph)
        elif name == "upload":
            self.n = self.next_index = int(op[1]); self._row("sph_upload")
        elif name == "load_snapshot":
            # (the library calls sph_set_params first; the rows commute, and in this order the load's own row shows)
            self.n = self.next_index = SNAP_N; self._row("sph_snapshot_load")
            self._row("sph_set_params"); self.params = "P0"
        elif name == "reset_lattice":
            self.n = self.next_index = int(np.prod(op[1])); self._row("sph_reset_lattice")
        elif name == "set_by_index":
            self._row("sph_set_by_index")
        elif name == "emit":
            if self.n + op[1] > self.capacity or self.next_index + op[1] > self.capacity: return E_CAPACITY
            self.n += op[1]; self.next_index += op[1]; self._row("sph_emit")
        elif name == "remove":
            k = (0 if op[1] == "none" else 1) if selected is None else int(selected)
            if k:
                self.n -= min(k, self.n); self._row("sph_remove")
        elif name == "set_params":
            self.params = op[1]; self._row("sph_set_params")
        elif name == "set_colliders":
            self.n_colliders, self.tracked = (1 if op[1] == "one" else 0), False; self._row("sph_set_colliders")
        elif name == "set_collider_bodies":
            self.tracked = op[1] == "on" and self.n_colliders > 0; self._row("sph_set_collider_bodies")
        elif name == "download_forces":
            if not self.accepts(name): return E_STATE
        elif name == "set_precision": self.precision = int(op[1])
        elif name == "set_sort_mode": self.sort_mode = int(op[1])
        elif name == "set_direct_hull": self.direct_hull = int(op[1])
        elif name == "set_pair_small_launch": self.small_launch = int(op[1])
        elif name == "set_block_order": self.block_order = (int(op[1]), int(op[2]))
        elif name == "trust_mover_hint": self.both_until = 0
        elif name == "obstacle_build": self.obstacle = ("build", op[1]); self._row("sph_obstacle_build")
        elif name == "obstacle_set_grid": self.obstacle = ("grid", int(op[1])); self._row("sph_obstacle_build")
        elif name == "obstacle_motion": self.motion = op[1]; self._row("sph_obstacle_build")
        elif name == "obstacle_clear": self.obstacle = self.motion = None; self._row("sph_obstacle_build")     # (the motion goes with it)
        elif name == "obstacle_sample":
            if self.obstacle is None: return E_STATE
            self._row("sph_obstacle_build")
        elif name in VIEWS: self._row("sph_mesh_extract")
        elif name not in ("count_in", "download", "sync"):
            raise KeyError(name)
        return 0

    def next_phase(self, fused=False):
        """the phase call that goes on with the step where it is"""
        if not self.mid_step(): return "hash"
        if self.stage == HASHED: return "sort"
        if self.stage == SORTED: return "build_cells"
        if not self.have_dens: return "density"
        if fused and not (self.have_force or self.have_coll): return "fci"
        if not self.have_force: return "force"
        if not self.have_coll: return "collide"
        return "integrate"


def continuation(kind, m):
    """The ops that finish (or restart) the step of a context whose mirror is m -- phases: phase by phase; fci: with
    sph_force_collide_integrate where the stage allows it; step: sph_step from wherever the context is."""
    if kind == "step":
        return [("step", 1)]
    d = Mirror(m.capacity)
    d.__dict__.update({k: v for k, v in m.__dict__.items() if k not in ("reached", "calls", "sorts")})
    ops = []
    while True:
        ph = d.next_phase(fused=kind == "fci")
        ops.append((ph,))
        d.apply((ph,))
        if ph in ("integrate", "fci"):
            return ops


# ---- states and calls as data ------------------------------------------------------------------------------------------------
_STEPPED = [("step", 2), ("trust_mover_hint",)]
_UP = ("upload", 6000, "flow")
PREFIXES = {     # name -> dict(before: ops in front of the boundary, after: ops behind it, dt, capacity, calls: "all" / "few")
    "stepped": dict(before=[_UP] + _STEPPED, after=[]),
    "stepped_phased": dict(before=[_UP, ("step_phased", 2), ("trust_mover_hint",)], after=[]),
    "hashed": dict(before=[_UP] + _STEPPED, after=[("hash",)]),
    "sorted": dict(before=[_UP] + _STEPPED, after=[("hash",), ("sort",)]),
    "cells": dict(before=[_UP] + _STEPPED, after=[("hash",), ("sort",), ("build_cells",)]),
    "density": dict(before=[_UP] + _STEPPED, after=[("hash",), ("sort",), ("build_cells",), ("density",)]),
    "forces": dict(before=[_UP] + _STEPPED, after=[("hash",), ("sort",), ("build_cells",), ("density",), ("force",), ("collide",)]),
    "skipped": dict(before=[("upload", 512, "rest"), ("step_until_skipped", 3), ("trust_mover_hint",)], after=[], dt=DT_REST, capacity=4096),
    "uploaded": dict(before=[_UP], after=[]),
    "edited": dict(before=[_UP] + _STEPPED, after=[("set_by_index", "both", 21)]),
    # more than one sort tile (4096 keys) and more than one 16384-slot mover tile; the merge path behind a deferred table clear
    "hashed_20k": dict(before=[("upload", 20000, "flow")] + _STEPPED, after=[("hash",)], capacity=24576, calls="few"),
    # a collider with a free body (tracked: the spheres live on the device), and the mixed-precision density pass
    "density_body": dict(before=[("set_colliders", "one"), ("set_collider_bodies", "on"), _UP] + _STEPPED,
                         after=[("hash",), ("sort",), ("build_cells",), ("density",)], calls="few"),
    "sorted_mixed": dict(before=[("set_precision", 1), _UP] + _STEPPED, after=[("hash",), ("sort",)], calls="few"),
    # a moving obstacle installed before anything else: every call of CALLS meets a context that already has one
    "stepped_obstacle": dict(before=[("obstacle_build", "both"), ("obstacle_motion", "on"), _UP] + _STEPPED, after=[]),
    # ... and with two tiles of the movers' marks (16384 slots each) under the obstacle's pass
    "hashed_20k_obstacle": dict(before=[("obstacle_build", "both"), ("upload", 20000, "flow")] + _STEPPED, after=[("hash",)],
                                capacity=24576, calls="few"),
}
CONTINUATIONS = ("phases", "fci", "step")

# name -> (class, ops, anchor): anchor True = the step that follows also runs against the float64 model; "bare" = the first
# integrate that follows is tests/obstacle_model.py's push applied to the output of a BARE twin (Walker.bare), a context without
# the obstacle.  (A prefix that installs an obstacle runs every call it has with the bare twin, and none against the float64
# model, which knows no obstacle.)
_OB = ("obstacle_build", "both")
CALLS = {
    "upload_smaller": ("edit", [("upload", 3000, "flow")], False),
    "load_snapshot": ("edit", [("load_snapshot",)], False),
    "reset_lattice": ("edit", [("reset_lattice", (12, 12, 12), 1)], False),
    "set_by_index_pos": ("edit", [("set_by_index", "pos", 31)], False),
    "set_by_index_vel": ("edit", [("set_by_index", "vel", 32)], False),
    "set_by_index_both": ("edit", [("set_by_index", "both", 33)], False),
    "emit_explicit": ("edit", [("emit", 100, 41, True)], False),
    "emit_auto": ("edit", [("emit", 77, 42, False)], False),
    "remove_something": ("edit", [("remove", 2)], False),
    "remove_nothing": ("edit", [("remove", "none")], False),
    "remove_emit": ("edit", [("remove", 3), ("emit", 90, 43, False)], True),
    "emit_remove": ("edit", [("emit", 90, 44, True), ("remove", 4)], False),
    "set_by_index_remove": ("edit", [("set_by_index", "both", 34), ("remove", 1)], False),
    "emit_set_params": ("edit", [("emit", 64, 45, False), ("set_params", "visc")], False),
    "params_physics": ("keep", [("set_params", "visc")], False),
    "params_box_moved": ("keep", [("set_params", "shift")], True),
    "params_wall_inward": ("keep", [("set_params", "wall")], False),
    "colliders_on": ("keep", [("set_colliders", "one")], False),
    "colliders_off": ("keep", [("set_colliders", "one"), ("set_colliders", "none")], False),
    "bodies_on": ("keep", [("set_colliders", "one"), ("set_collider_bodies", "on")], False),
    "bodies_off": ("keep", [("set_colliders", "one"), ("set_collider_bodies", "on"), ("set_collider_bodies", "off")], False),
    "render": ("keep", [("render",)], False),
    "count_in": ("keep", [("count_in", 0)], False),
    "download": ("keep", [("download",)], False),
    "download_forces": ("keep", [("download_forces",)], False),
    "precision_mixed": ("keep", [("set_precision", 1)], False),
    "precision_back": ("keep", [("set_precision", 1), ("set_precision", 0)], False),
    "sort_mode_0": ("keep", [("set_sort_mode", 0)], False),
    "sort_mode_1": ("keep", [("set_sort_mode", 1)], False),
    "sort_mode_2": ("keep", [("set_sort_mode", 2)], False),
    "direct_hull_0": ("keep", [("set_direct_hull", 0)], False),
    "pair_small_launch": ("keep", [("set_pair_small_launch", 0)], False),
    "block_order_plain": ("keep", [("set_block_order", 0, 0)], False),
    "hash_again": ("keep", [("hash",)], False),
    "cells_again": ("keep", [("build_cells",)], False),
    "density_again": ("keep", [("density",)], False),
    "refused_phase": ("keep", [], False),          # the walker probes every refused phase call after every call: here nothing else happens
    "obstacle_on": ("keep", [_OB], "bare"),
    "obstacle_off": ("keep", [_OB, ("obstacle_clear",)], "bare"),
    "obstacle_moving": ("keep", [_OB, ("obstacle_motion", "on")], "bare"),
    "obstacle_replaced": ("keep", [("obstacle_set_grid", 51), _OB], "bare"),
    "obstacle_caller_grid": ("keep", [_OB, ("obstacle_set_grid", 52), ("obstacle_motion", "on")], "bare"),
    "obstacle_motion_alone": ("keep", [("obstacle_motion", "on")], "bare"),       # no grid: nothing pushes, the offset stays
    "obstacle_sample": ("keep", [_OB, ("obstacle_motion", "on"), ("obstacle_sample",)], "bare"),
    "obstacle_sample_none": ("keep", [("obstacle_sample",)], False),               # refused without a grid
    "render_surface": ("keep", [("render_surface",)], False),
    "extract_mesh": ("keep", [("extract_mesh",)], False),
    "obstacle_remove": ("edit", [_OB, ("remove", 0)], "bare"),
    "obstacle_emit": ("edit", [_OB, ("emit", 120, 46, False)], "bare"),
    "obstacle_set_by_index": ("edit", [_OB, ("set_by_index", "both", 35)], "bare"),
    "obstacle_load_snapshot": ("edit", [_OB, ("load_snapshot",)], "bare"),
    "obstacle_box_moved": ("keep", [_OB, ("set_params", "shift")], "bare"),        # the walls are the new box's; the solid stays
}
FEW = ("upload_smaller", "reset_lattice", "set_by_index_both", "emit_auto", "remove_something", "remove_nothing", "remove_emit",
       "emit_remove", "params_box_moved", "precision_mixed", "sort_mode_0", "hash_again", "refused_phase",
       "obstacle_on", "obstacle_off", "obstacle_moving", "obstacle_remove", "obstacle_emit")


def calls_for(prefix):
    return list(CALLS) if PREFIXES[prefix].get("calls", "all") == "all" else list(FEW)


def usable(m, ops):
    """a phase call that the table accepts on positions newer than its keys (sph_density right after a step) computes on a
    stale table: accepted, but not a use with a meaning a twin could share.  Such calls are left out, not walked."""
    return not (ops and ops[0][0] in PHASES[1:] and m.integrated and m.accepts(ops[0][0]))


# ---- long histories ----------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = (101, 102, 103, 104, 106, 107, 108, 109)       # each holds at least one refused call
# histories that also draw the obstacle calls and the views (extended=True): each holds at least two installations, a clear, a
# change of motion, a view and a refused call (tests/test_context_walk_cpu.py); their steps are single ones, so that the bare
# twin anchors every completed step that has an obstacle
FUZZ_SEEDS_OBSTACLE = (201, 202, 203, 204, 206, 211)
FUZZ_CAPACITY = 16384


def fuzz_ops(seed, n_ops=40, extended=False):
    """The operation list of one seed: an upload and n_ops calls, each legal or deliberately illegal by the mirror.  extended: a
    quarter of the calls are the obstacle's or a view (drawn first, so the lists of the plain seeds are what they always were)."""
    rng = np.random.default_rng(seed)
    m = Mirror(FUZZ_CAPACITY)
    ops = []
    removes = [0]

    def push(op):
        ops.append(op)
        m.apply(op)
        if op[0] in ("upload", "load_snapshot", "reset_lattice"): removes[0] = 0
        if op[0] == "remove" and op[1] != "none": removes[0] += 1

    push(("set_sort_mode", (1, 2)[seed % 2]))
    push(("upload", 6000, "flow"))
    head = len(ops)
    while len(ops) < head + n_ops:
        if extended and rng.random() < 0.25:
            k = int(rng.integers(12))
            s = int(rng.integers(1 << 20))
            if k in (0, 1, 2): push(("obstacle_build", "both"))
            elif k in (3, 4): push(("obstacle_set_grid", s))
            elif k == 5: push(("obstacle_clear",))
            elif k in (6, 7): push(("obstacle_motion", ("on", "off")[s % 2]))
            elif k == 8: push(("obstacle_sample",))           # refused while no grid is installed
            elif k == 9: push(("render",))
            elif k == 10: push(("render_surface",))
            else: push(("extract_mesh",))
            continue
        r = rng.random()
        if r < 0.20:
            push([("step", 1), ("step", 2), ("step_phased", 1)][rng.integers(3)] if not extended else
                 [("step", 1), ("step_phased", 1)][rng.integers(2)])
        elif r < 0.50:
            push((m.next_phase(fused=rng.random() < 0.4),))
        elif r < 0.72:
            k = int(rng.integers(10))
            s = int(rng.integers(1 << 20))
            if k == 0: push(("upload", (3000, 5000)[s % 2], "flow"))
            elif k == 1: push(("load_snapshot",))
            elif k == 2: push(("reset_lattice", (12, 12, 12), s % 2))
            elif k in (3, 4): push(("set_by_index", ("pos", "vel", "both")[s % 3], s))
            elif k in (5, 6): push(("emit", 1 + s % 128, s, k == 5))
            elif k in (7, 8) and removes[0] < 6: push(("remove", removes[0]))
            else: push(("remove", "none"))
        elif r < 0.94:
            k = int(rng.integers(14))
            s = int(rng.integers(1 << 20))
            if k == 0: push(("set_params", PARAM_VARIANTS[s % 4]))
            elif k == 1: push(("set_colliders", ("one", "none")[s % 2]))
            elif k == 2: push(("set_collider_bodies", "on" if (m.n_colliders and s % 2) else "off"))
            elif k == 3: push(("render",))
            elif k == 4: push(("count_in", s % 6))
            elif k == 5: push(("download",))
            elif k == 6: push(("download_forces",))          # refused unless sph_force and sph_collide have both run
            elif k == 7: push(("set_precision", s % 2))
            elif k == 8: push(("set_sort_mode", s % 3))
            elif k == 9: push(("set_direct_hull", (0, 512)[s % 2]))
            elif k == 10: push(("set_pair_small_launch", (0, 524288)[s % 2]))
            elif k == 11: push(("set_block_order", s % 2, s % 2))
            elif k == 12: push(("hash",))
            elif m.mid_step() and m.have_dens: push(("density",))
            else: push(("sync",))
        else:
            bad = m.refused_phases()
            push((bad[int(rng.integers(len(bad)))],) if bad else ("sync",))
    return ops


# ---- what the CPU test needs: the same walks through a mirror alone ---------------------------------------------------------------
def dry_case(prefix, call, cont):
    """the ops of one matrix case through a Mirror; returns it (None where the case is left out, see usable())"""
    P = PREFIXES[prefix]
    m = Mirror(P.get("capacity", 8192))
    m.apply(("set_sort_mode", 2))
    for op in P["before"] + P["after"]:
        assert m.apply(op) == 0, (prefix, op)
    ops = CALLS[call][1]
    if not usable(m, ops):
        return None
    for op in ops:
        m.apply(op)
        for ph in m.refused_phases():
            m.calls.add((m.stage, ph))
    for op in continuation(cont, m) + [("step", 2)]:
        assert m.apply(op) == 0, (prefix, call, cont, op)
    return m


# ---- the walker (GPU) ----------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _rc(fn, *a, **kw):
    """(return code, result) of a capi.Context method"""
    from gpufluidsimulator_amd import capi
    try:
        return 0, fn(*a, **kw)
    except capi.SphError as e:
        return int(str(e).split("error ")[1].split(":")[0]), None


def make_snapshot(path):
    """the file of ("load_snapshot",): SNAP_N random particles, never stepped, default parameters"""
    from gpufluidsimulator_amd import capi, ic
    pos, vel = ic.random_box(SNAP_N, BOX, speed=40.0, fill=0.45, seed=SNAP_SEED)
    with capi.Context(SNAP_N, box=BOX, grid=GRID) as c:
        c.upload(pos, vel)
        c.save(path)


def _particles(n, kind):
    from gpufluidsimulator_amd import ic
    if kind == "rest":
        return ic.dam_break_lattice((8, 8, 8), BOX, jitter=False)
    return ic.random_box(n, BOX, speed=40.0, fill=0.45)


def _points(count, seed):
    """positions inside every box variant, and velocities"""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-0.75, -0.2, count), rng.uniform(-0.95, -0.2, count), rng.uniform(-0.95, -0.2, count)], 1)
    return pos.astype(np.float32), rng.uniform(-40.0, 40.0, (count, 3)).astype(np.float32)


class Compact:
    """a context seen through the rows of its live creation indices (phase_checks.phases_vs_model wants arrays without holes)"""

    def __init__(self, c):
        self._c, self._idx = c, np.sort(c.download_owned()[2])

    def __getattr__(self, name):
        return getattr(self._c, name)

    def download(self, **kw):
        return {k: v[self._idx] for k, v in self._c.download(**kw).items()}

    def download_forces(self, **kw):
        return {k: v[self._idx] for k, v in self._c.download_forces(**kw).items()}


class Walker:
    def __init__(self, capacity, dt, snapshot):
        from gpufluidsimulator_amd import capi
        self.capi, self.capacity, self.dt, self.snapshot = capi, int(capacity), float(dt), snapshot
        self.c = capi.Context(self.capacity, box=BOX, grid=GRID)
        self.m = Mirror(self.capacity)
        self.t = self.tm = None
        self.twinning = False
        self.live = np.zeros(0, np.uint32)
        self.trace = []
        self.cam = capi.look_at(32, 24, eye=(0.0, 0.0, 3.0))
        # the obstacle as numpy knows it (never read from the library): the grid and the field of the last installation, and the
        # offset advanced by obstacle_model.advance once per integrate with a grid installed
        self.ob, self.off, self.u = None, np.zeros(3, np.float32), np.zeros(3, np.float32)
        # the bare twin: like the twin, but without the obstacle and its calls; good for ONE integrate behind its boundary
        self.bare = False
        self.b = self.bm = None
        self.b_fresh = False
        self.anchored = self.anchor_touched = 0

    def close(self):
        for c in (self.c, self.t, self.b):
            if c is not None:
                c.close()
        self.c = self.t = self.b = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reach(self, prefix):
        """the state of PREFIXES[prefix]; the twin starts at its boundary"""
        P = PREFIXES[prefix]
        self.do(("set_sort_mode", 2))
        for op in P["before"]:
            self.do(op)
        self.twinning = True
        self.rebase()
        for op in P["after"]:
            self.do(op)
        if self.m.order_valid:       # the context is on the merge path: a hash leaves the clearing of the table to the sort
            assert self.c.sort_stats()["merges"] >= 1, prefix

    # -- one call on one context -----------------------------------------------------------------------------------------------
    def _perform(self, c, op):
        name, L, h = op[0], c.L, c.h
        if name == "hash": return L.sph_hash(h), None
        if name == "sort": return L.sph_sort(h), None
        if name == "build_cells": return L.sph_build_cells(h), None
        if name == "density": return L.sph_density(h), None
        if name == "force": return L.sph_force(h), None
        if name == "collide": return L.sph_collide(h), None
        if name == "integrate": return L.sph_integrate(h, self.dt), None
        if name == "fci": return L.sph_force_collide_integrate(h, self.dt), None
        if name == "step": return L.sph_step(h, self.dt, int(op[1])), None
        if name == "step_phased": return L.sph_step_phased(h, self.dt, int(op[1])), None
        if name == "step_until_skipped":           # in lockstep with the device, until a sort found nothing to do
            for _ in range(8):
                c.step(self.dt, 1); c.sync()
                if c.sort_skipped(): return 0, None
            raise AssertionError("the fluid at rest never skipped a sort")
        if name == "sync": return _rc(c.sync)
        if name == "upload":
            pos, vel = _particles(op[1], op[2])
            return _rc(c.upload, pos, vel)
        if name == "load_snapshot": return _rc(c.load_snapshot, self.snapshot)
        if name == "reset_lattice": return _rc(c.reset_lattice, op[1], jitter=bool(op[2]))
        if name == "set_by_index":
            pos, vel = _points(SBI_COUNT, op[2])
            return _rc(c.set_by_index, SBI_FIRST, pos if op[1] != "vel" else None, vel if op[1] != "pos" else None)
        if name == "emit":
            pos, vel = _points(op[1], op[2])
            idx = (self._next + np.arange(op[1])[::-1]).astype(np.uint32) if op[3] else None
            return _rc(c.emit, pos, vel, idx)
        if name == "remove": return _rc(c.remove, region_model.to_capi(REGIONS[op[1]]))
        if name == "count_in": return _rc(c.count_in, region_model.to_capi(REGIONS[op[1]]))
        if name == "set_params": return _rc(c.set_params, params_variant(op[1]))
        if name == "set_colliders":
            return _rc(c.set_colliders, *COLLIDER) if op[1] == "one" else _rc(c.set_colliders, np.zeros((0, 3), np.float32), [])
        if name == "set_collider_bodies":
            on = op[1] == "on" and self.m.n_colliders > 0
            return _rc(c.set_collider_bodies, *BODY) if on else _rc(c.set_collider_bodies, [])
        if name == "render":
            rc, _ = _rc(c.render, self.cam, color="speed", lo=0.0, hi=80.0)
            return (rc, None) if rc else _rc(c.read_image)
        if name == "render_surface":               # the defaults: absorption (the thickness pass) on
            rc, _ = _rc(c.render_surface, self.cam)
            return (rc, None) if rc else _rc(lambda: c.read_image() + c.read_surface())
        if name == "extract_mesh":
            mp = self.capi.mesh_defaults(**MESH)
            rc, counts = _rc(c.extract_mesh, mp)
            return (rc, None) if rc else _rc(lambda: (c.mesh_lattice(mp), counts, c.mesh_field()) + c.read_mesh())
        if name == "obstacle_build":
            shapes = [self.capi.Shape(int(sh["kind"]), int(sh["invert"]), self.capi._f3(sh["a"]), self.capi._f3(sh["b"]), float(sh["r"]))
                      for sh in OBSTACLES[op[1]]]
            return _rc(c.build_obstacle, shapes, OBSTACLE_SPACING)
        if name == "obstacle_set_grid": return _rc(c.set_obstacle_grid, caller_field(op[1]), CALLER_GRID["origin"], CALLER_GRID["spacing"])
        if name == "obstacle_motion": return _rc(c.set_obstacle_motion, offset=MOTION[op[1]][0], velocity=MOTION[op[1]][1])
        if name == "obstacle_clear": return _rc(c.clear_obstacle)
        if name == "obstacle_sample": return _rc(c.sample_obstacle, sample_points())
        if name == "download": return _rc(c.download)
        if name == "download_forces": return _rc(c.download_forces)
        if name == "set_precision": return _rc(c.set_precision, bool(op[1]))
        if name == "set_sort_mode": return _rc(c.set_sort_mode, int(op[1]))
        if name == "set_direct_hull": return _rc(c.set_direct_hull, op[1])
        if name == "set_pair_small_launch": return _rc(c.set_pair_small_launch, op[1])
        if name == "set_block_order": return _rc(c.set_block_order, op[1], op[2])
        if name == "trust_mover_hint": return _rc(c.trust_mover_hint)
        raise KeyError(name)

    # -- one call of the walk -------------------------------------------------------------------------------------------------
    def do(self, op):
        c, m = self.c, self.m
        name = op[0]
        self.trace.append(op)
        self._next = m.next_index
        sel, before = None, None
        if name == "remove":
            p0, _, i0 = c.download_owned()
            want = region_model.selected(p0, REGIONS[op[1]])
            sel = int(want.sum())
            assert (sel > 0) == (op[1] != "none"), ("the region of this walk selects", sel)
        if name in ("sort", "step", "step_phased"):
            before = (c.sort_stats(), c.sort_forms())
        ob_steps, off_before = m.ob_steps, self.off
        want_rc = m.apply(op, sel)
        rc, out = self._perform(c, op)
        assert rc == want_rc, f"{op}: returned {rc}, the table says {want_rc}"
        assert c.n == m.n, f"{op}: n = {c.n}, the table says {m.n}"
        if rc:
            return rc
        # what the call itself reports
        if name == "remove":
            assert c.last_removed == sel and np.array_equal(out, i0[want]), f"{op}: removed indices"
            self.live = np.setdiff1d(self.live, out).astype(np.uint32)
        elif name == "emit":
            first = self._next + (op[1] - 1 if op[3] else 0)
            assert out == first, f"{op}: first index {out}, next_index was {self._next}"
            self.live = np.union1d(self.live, self._next + np.arange(op[1])).astype(np.uint32)
        elif name == "count_in":
            assert out == int(region_model.selected(c.download_owned()[0], REGIONS[op[1]]).sum()), f"{op}: count"
        elif name in ("upload", "load_snapshot", "reset_lattice"):
            self.live = np.arange(m.n, dtype=np.uint32)
        elif name in OBSTACLE_OPS:
            self._obstacle_call(op, out)
        elif name in VIEWS:
            self._check_view(op, out)
        self.off = om.advance(self.off, self.u, self.dt, m.ob_steps - ob_steps)
        if before is not None and m.sorts and all(s[0] is not None for s in m.sorts):
            stats, forms = c.sort_stats(), c.sort_forms()
            assert stats["sorts"] - before[0]["sorts"] == len(m.sorts), f"{op}: sorts"
            merges = sum(1 for s in m.sorts if s[0])
            assert stats["merges"] - before[0]["merges"] == merges, \
                f"{op}: {stats['merges'] - before[0]['merges']} merging sorts, the table's order_valid says {merges}"
            both = sum(1 for s in m.sorts if s[1])
            grew = forms[0] - before[1][0]
            skipped = stats["skips"] - before[0]["skips"]           # a skipped sort launches no form at all
            assert grew >= both - skipped and (grew <= both or m.n > 6144), \
                f"{op}: {grew} movers' sorts in both forms, the table's sort_form_both_until says {both}"
        # the twin
        edited = name in EDITS and not (name == "remove" and sel == 0)
        if edited:
            if self.twinning:
                self.rebase()
        elif self.t is not None and self.tm.apply(op) == 0:
            rc2, _ = self._perform(self.t, op)
            assert rc2 == 0, f"{op}: the twin returned {rc2}"
            c.sync(); self.t.sync()               # lockstep: a sort may look at a count the device has produced
            self._bare_follows(op, m.ob_steps - ob_steps, off_before)
        return 0

    # -- the obstacle, by numpy -------------------------------------------------------------------------------------------------
    def _params(self):
        p = self.capi.Params()
        self.capi._check(self.c.L.sph_get_params(self.c.h, p))
        return p

    def _obstacle_call(self, op, out):
        name = op[0]
        if name == "obstacle_build":               # the lattice is that of the box AS IT IS NOW; a later sph_set_params leaves it
            p = self._params()
            grid = om.lattice(OBSTACLE_SPACING, tuple(p.box_min), tuple(p.box_max), p.particle_radius)
            self.ob = {"grid": grid, "phi": om.rasterise(OBSTACLES[op[1]], grid)}
        elif name == "obstacle_set_grid":
            self.ob = {"grid": CALLER_GRID, "phi": om.clamp(caller_field(op[1]), CALLER_GRID)}
        elif name == "obstacle_motion":
            self.off, self.u = MOTION[op[1]]
        elif name == "obstacle_clear":
            self.ob, self.off, self.u = None, np.zeros(3, np.float32), np.zeros(3, np.float32)
        elif name == "obstacle_sample":
            want = om.sample(self.ob["grid"], self.ob["phi"], self.off, sample_points())
            assert 100 < want[2].sum() < 500
            assert np.array_equal(out[2], want[2]), f"{op}: inside the grid"
            assert np.array_equal(_bits(out[0]), _bits(want[0])) and np.array_equal(_bits(out[1]), _bits(want[1])), f"{op}: phi, normal"

    def obstacle_state(self, c):
        """(grid dims, origin, spacing, offset, velocity, field) as sph_obstacle_get / _read show them; dims (0, 0, 0): none"""
        capi = self.capi
        import ctypes as C
        g, off, vel = capi.ObstacleGrid(), (C.c_float * 3)(), (C.c_float * 3)()
        capi._check(c.L.sph_obstacle_get(c.h, C.byref(g), off, vel))
        ob = c.obstacle(read=True)
        assert (ob is None) == (not any(g.dims))
        return (tuple(int(v) for v in g.dims), np.array(list(g.origin), np.float32), np.float32(g.spacing),
                np.array(list(off), np.float32), np.array(list(vel), np.float32), None if ob is None else ob["phi"])

    def _check_obstacle(self, tag):
        """what the library shows of the obstacle against numpy's record, and the twin's against the context's"""
        m = self.m
        got = self.obstacle_state(self.c)
        assert (m.obstacle is None) == (self.ob is None) == (got[5] is None), f"obstacle installed {tag}"
        assert np.array_equal(_bits(got[3]), _bits(self.off)), f"obstacle offset {got[3]}, by numpy {self.off} {tag}"
        assert np.array_equal(_bits(got[4]), _bits(self.u)), f"obstacle velocity {tag}"
        if self.ob is not None:
            grid = self.ob["grid"]
            assert got[0] == tuple(grid["dims"]) and got[2] == grid["spacing"], f"obstacle lattice {tag}"
            assert np.array_equal(_bits(got[1]), _bits(grid["origin"])), f"obstacle origin {tag}"
            assert np.array_equal(_bits(got[5]), _bits(self.ob["phi"])), f"obstacle field {tag}"
        twin = self.obstacle_state(self.t)
        assert twin[0] == got[0] and twin[2] == got[2] and (twin[5] is None) == (got[5] is None), f"the twin's obstacle {tag}"
        for x, y in zip(got[1:], twin[1:]):
            assert x is None or np.array_equal(_bits(x), _bits(y)), f"the twin's obstacle {tag}"

    # -- the views, by numpy ------------------------------------------------------------------------------------------------------
    def _check_view(self, op, out):
        import mesh_model, render_model, surface_model
        c, p = self.c, self._params()
        pos, vel, idx = c.download_owned()
        R = p.particle_radius
        if op[0] == "render":
            want = render_model.render(pos, self.cam, vel=vel, index=idx, color="speed", lo=0.0, hi=80.0, radius=R)
            assert np.array_equal(out[1], want[1]), f"{op}: id"
            assert np.array_equal(_bits(out[2]), _bits(want[2])) and np.array_equal(out[0], want[0]), f"{op}: depth, rgba"
            assert (want[1] != render_model.NO_ID).any()
        elif op[0] == "render_surface":
            w = surface_model.render(pos, self.cam, surface_model.surface_style(), vel=vel, index=idx, radius=R)
            assert (w.id != render_model.NO_ID).any()
            for got, want, what in zip(out, (w.rgba, w.id, w.depth, w.raw, w.thick, w.normal), ("rgba", "id", "depth", "raw", "thick", "normal")):
                assert got.shape == want.shape and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), f"{op}: {what}"
        else:
            counts, origin, _, mpos, mnrm, mtri = mesh_model.mesh_of(pos, tuple(p.box_min), tuple(p.box_max), R, **MESH)
            (dims, got_origin), (nv, nt), got_counts, gpos, gnrm, gtri = out
            assert dims == counts.shape[::-1] and np.array_equal(_bits(got_origin), _bits(origin)), f"{op}: lattice"
            assert nt == len(mtri) > 100 and nv == len(mpos), f"{op}: {nv} vertices, {nt} triangles; the model {len(mpos)}, {len(mtri)}"
            assert np.array_equal(got_counts, counts), f"{op}: counts"
            assert np.array_equal(_bits(gpos), _bits(mpos)) and np.array_equal(_bits(gnrm), _bits(mnrm)), f"{op}: vertices"
            assert np.array_equal(gtri, mtri), f"{op}: triangles"

    # -- the bare twin --------------------------------------------------------------------------------------------------------
    def _bare_follows(self, op, integrates, off_before):
        """the bare twin makes the call too, unless it is the obstacle's; behind the first integrate since its boundary the context
        must hold the model's push of the bare twin's output"""
        if self.b is None or op[0] in OBSTACLE_OPS:
            return
        if self.bm.apply(op) == 0:
            assert self._perform(self.b, op)[0] == 0, f"{op}: the bare twin"
            self.b.sync()
        if op[0] in ("integrate", "fci", "step", "step_phased"):
            if self.b_fresh and integrates == 1:
                self._check_against_model(off_before)
            self.b_fresh = False

    def _check_against_model(self, off_before):
        c, p, live = self.c, self._params(), self.live
        tag = f"behind {self.trace[-3:]}"
        got, bare = c.download(), self.b.download()
        want_p, want_v, touched = om.push(bare["pos"][live], bare["vel"][live], self.ob["grid"], self.ob["phi"], off_before, self.u,
                                          tuple(p.box_min), tuple(p.box_max), p.wall_eps, p.wall_damping)
        assert np.array_equal(_bits(got["pos"][live]), _bits(want_p)), \
            f"positions against obstacle_model.push of the bare twin's: {int((_bits(got['pos'][live]) != _bits(want_p)).any(axis=1).sum())} of {touched.sum()} touched differ {tag}"
        assert np.array_equal(_bits(got["vel"][live]), _bits(want_v)), f"velocities against obstacle_model.push of the bare twin's {tag}"
        for k in ("density", "pressure"):
            assert np.array_equal(_bits(got[k][live]), _bits(bare[k][live])), f"{k} against the bare twin's {tag}"
        self.anchored += 1
        self.anchor_touched += int(touched.sum())

    def probe_refusals(self):
        """every phase call the table says is illegal now returns SPH_E_STATE (and changes nothing: the twin never makes it)"""
        for ph in self.m.refused_phases():
            self.m.calls.add((self.m.stage, ph))
            rc, _ = self._perform(self.c, (ph,))
            assert rc == E_STATE, f"{ph} at stage {self.m.stage} after {self.trace[-3:]}: returned {rc}, the table says refused"

    def _fresh(self, pos, vel, idx, p, obstacle):
        """a new context that holds what the public API shows of this one: parameters, settings, spheres, particles in slot order
        -- and, `obstacle`, the obstacle THROUGH ANOTHER DOOR: the clamped field sph_obstacle_read gives goes in by
        sph_obstacle_set_grid (never by the rasteriser), the ADVANCED offset sph_obstacle_get shows by sph_obstacle_set_motion"""
        capi, c, m = self.capi, self.c, self.m
        t = capi.Context(self.capacity, params=p)
        tm = Mirror(self.capacity)
        for op in (("set_precision", m.precision), ("set_sort_mode", m.sort_mode)) + \
                  ((("set_direct_hull", m.direct_hull),) if m.direct_hull is not None else ()) + \
                  ((("set_pair_small_launch", m.small_launch),) if m.small_launch is not None else ()) + \
                  ((("set_block_order",) + m.block_order,) if m.block_order is not None else ()):
            tm.apply(op)
            assert self._perform(t, op)[0] == 0
        if m.n_colliders:
            col = c.colliders()
            t.set_colliders(col["centers"], col["radii"], col["velocities"])
            if m.tracked:
                t.set_collider_bodies(*BODY)
        tm.n_colliders, tm.tracked, tm.params = m.n_colliders, m.tracked, m.params
        if obstacle:
            dims, origin, spacing, off, vel3, phi = self.obstacle_state(c)
            if phi is not None:
                t.set_obstacle_grid(phi, origin, spacing)
            t.set_obstacle_motion(offset=off, velocity=vel3)
            tm.obstacle, tm.motion = m.obstacle, m.motion
        t.upload(pos, vel, idx)
        tm.n, tm.next_index = m.n, m.next_index
        tm._row("sph_upload")
        return t, tm

    def rebase(self):
        """a boundary: the twin becomes a fresh context that holds what the public API shows now (and so does the bare twin, but
        for the obstacle)"""
        capi, c, m = self.capi, self.c, self.m
        for old in (self.t, self.b):
            if old is not None:
                old.close()
        self.t = self.b = None
        pos, vel, idx = c.download_owned()
        p = self._params()
        assert c.L.sph_get_precision(c.h) == m.precision
        self.t, self.tm = self._fresh(pos, vel, idx, p, True)
        if self.bare:
            self.b, self.bm = self._fresh(pos, vel, idx, p, False)
            self.b_fresh = True
        c.sync(); self.t.sync()

    # -- the identities -------------------------------------------------------------------------------------------------------
    def check_set(self):
        """the particle set, tracked by creation index on the host, against everything the context reports"""
        c = self.c
        pos, vel, idx = c.download_owned()
        assert np.array_equal(np.sort(idx), self.live), "the set of creation indices"
        p4 = c.positions4()
        assert np.array_equal(_bits(p4[idx, :3]), _bits(pos)) and np.all(p4[idx, 3] == 1.0), "positions4 of the particles"
        dead = np.ones(self.capacity, bool)
        dead[idx] = False
        assert not p4[dead].any(), "positions4 of an index without a particle is (0, 0, 0, 0)"
        d = c.download(want=("pos", "vel"))
        assert np.array_equal(_bits(d["pos"][idx]), _bits(pos)) and np.array_equal(_bits(d["vel"][idx]), _bits(vel)), "download by index"
        assert np.isnan(d["pos"][dead]).all(), "download leaves the rows of absent indices alone"

    def compare(self, what=""):
        """the context and its twin, bit for bit, in everything their stages make readable"""
        c, t, m, tm = self.c, self.t, self.m, self.tm
        if t is None:                # (nothing installed yet: the by-index buffer of a new context holds nothing defined)
            return
        self.check_set()
        tag = f"{what} after {self.trace[-4:]}"
        assert c.n == t.n, tag
        a, b = c.download_owned(), t.download_owned()
        assert np.array_equal(a[2], b[2]), f"slot order {tag}"
        assert np.array_equal(_bits(a[0]), _bits(b[0])), f"positions {tag}"
        assert np.array_equal(_bits(a[1]), _bits(b[1])), f"velocities {tag}"
        assert np.array_equal(_bits(c.positions4()), _bits(t.positions4())), f"positions4 {tag}"
        self._check_obstacle(tag)
        if m.stage >= HASHED and tm.stage == m.stage:
            assert np.array_equal(c.keys(), t.keys()), f"keys {tag}"
        if m.stage == HASHED and m.mid_step() and m.params_at_hash == m.params:
            import small_grids           # the keys of a hash: those of the slots' positions in the box as it is now
            p = self._params()
            lo, hi = np.array(list(p.box_min), np.float32), np.array(list(p.box_max), np.float32)
            assert np.array_equal(c.keys(), small_grids.np_keys(a[0], lo, hi, tuple(p.grid))), f"keys against numpy {tag}"
        if m.stage >= SORTED and tm.stage >= SORTED:
            for x, y, k in zip(c.cells(), t.cells(), ("keys", "starts", "counts")):
                assert np.array_equal(x, y), f"cell table: {k} {tag}"
        if m.have_dens and tm.have_dens:
            x, y = c.download(want=("density", "pressure")), t.download(want=("density", "pressure"))
            for k in x:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), f"{k} {tag}"
        if m.accepts("download_forces") and tm.accepts("download_forces"):
            x, y = c.download_forces(), t.download_forces()
            for k in x:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), f"{k} {tag}"
        if m.n_colliders:
            x, y = c.colliders(), t.colliders()
            for k in x:
                assert np.array_equal(_bits(x[k]), _bits(y[k])), f"collider {k} {tag}"
            if m.tracked and m.integrated and tm.integrated:
                assert np.array_equal(c.collider_impulses()[0].view(np.uint64), t.collider_impulses()[0].view(np.uint64)), f"impulses {tag}"

    # -- the physics anchor ------------------------------------------------------------------------------------------------------
    def anchor_step(self):
        """the step that follows, phase by phase against the float64 model fed the GPU's own inputs (the context and its twin
        could be wrong together); the twin makes the same calls afterwards"""
        import phase_checks
        capi, c, m = self.capi, self.c, self.m
        ops = continuation("phases", m)
        start = {"build_cells": "cells"}.get(ops[0][0], ops[0][0])
        p = capi.Params()
        capi._check(c.L.sph_get_params(c.h, p))
        p_keys = params_variant(m.params_at_hash) if (m.mid_step() and m.params_at_hash != m.params) else None
        coll = None
        if m.n_colliders:
            col = c.colliders()
            coll = (None, col["radii"], col["velocities"])
        for _ in phase_checks.phases_vs_model(Compact(c), p, coll, self.dt, steps=1, start=start, p_keys=p_keys):
            pass
        for op in ops:
            self.trace.append(op)
            assert m.apply(op) == 0
            if self.t is not None and self.tm.apply(op) == 0:
                assert self._perform(self.t, op)[0] == 0
        c.sync()
        if self.t is not None:
            self.t.sync()

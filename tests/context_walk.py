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
           The twin is also handed the load sensor's switch and the obstacle's pose -- by the arguments of its last
           sph_obstacle_set_pose.  A pose that has ADVANCED since has no exact way into a fresh context (sph_obstacle_get_pose
           shows the float64 quaternion, sph_obstacle_set_pose takes a float32 one and normalises again;
           tests/test_context_walk_cpu.py pins that), so at such a boundary the walker RE-SEATS the context under test first: one
           extra "kept" call on it, set_obstacle_pose(pivot, float32(shown quaternion), omega), which the numpy record follows by
           obstacle_pose_model.quat_set and the twin repeats; the trace says so.  Long uninterrupted advances of a pose are
           tests/test_gpu_obstacle_pose.py's (fifty steps in lockstep).

  PREFIXES, CALLS, continuation(), fuzz_ops()   the states, the calls that cross them and the long histories, as data: the
           GPU tests run them, the CPU test walks them through a Mirror alone and proves the coverage.

An op is a tuple (name, args...); call_id() names it.  Nothing here peeks into the struct."""
import hashlib

import numpy as np

import mesh_obstacle_cases
import mesh_obstacle_model as mom
import obstacle_model as om
import obstacle_pose_model as pm
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
    "sph_obstacle_build": _NONE,         # ... and its twelve siblings, one row of the document: _set_grid, _clear, _set_motion, _sample,
                                         # _set_pose, _get_pose, _set_sensor, _get_load, _build_mesh, _build_mesh_dev, _mesh_stats
                                         # (walked) and _build_obj (SKIPPED_CALLS)
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

# entry points of a walked row that the walk leaves out, by name and with the reason
SKIPPED_CALLS = {
    "sph_obstacle_build_obj": "a host parser in front of sph_obstacle_build_mesh: tests/test_gpu_obstacle_mesh_host.py has it",
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
          "off": (np.zeros(3, np.float32), np.zeros(3, np.float32)),
          # into the fluid ("on" carries the ramp away from it): the solid kicks particles that are at rest, which a load needs
          "in": (np.array([0.013, -0.007, 0.004], np.float32), np.array([-200.0, 300.0, 100.0], np.float32)),
          # where the mould of ("obstacle_build_mesh_dev",) stands: the fluid's own shape, inverted, a fifth of the box aside
          "mould": (np.array([0.2, 0.12, -0.16], np.float32), np.zeros(3, np.float32))}
CALLER_GRID = {"dims": (23, 21, 19), "origin": np.array([-1.13, -1.11, -1.07], np.float32), "spacing": np.float32(0.1)}
OBSTACLE_OPS = ("obstacle_build", "obstacle_set_grid", "obstacle_motion", "obstacle_clear", "obstacle_sample",
                "obstacle_pose", "obstacle_get_pose", "obstacle_sensor", "obstacle_load",
                "obstacle_build_mesh", "obstacle_mesh_stats", "obstacle_build_mesh_dev")
VIEWS = ("render", "render_surface", "extract_mesh")
MESH = dict(spacing=1.0 / 16.0, radius=1.0 / 8.0)
# the mesh of ("extract_mesh", "coarse"), which feeds ("obstacle_build_mesh_dev",): a quarter of MESH's triangles (numpy voxelises them)
MESH_COARSE = dict(spacing=1.0 / 8.0, radius=3.0 / 16.0)
# ("obstacle_pose", tag): (pivot, quat (w, x, y, z), omega).  The pivot sits inside the ramp of OBSTACLES["both"], in the corner
# where every particle set of this module has particles: a grid turned about it keeps them inside its lattice.  The quaternion
# is skew and not normalised (about 14 degrees); "still" is the same pose with omega = 0.
POSE_PIVOT = (-0.95, -0.99, -0.9)
POSE_QUAT = (0.9, 0.03, -0.09, 0.06)
POSES = {"turning": (POSE_PIVOT, POSE_QUAT, (3.0, -40.0, 11.0)), "still": (POSE_PIVOT, POSE_QUAT, (0.0, 0.0, 0.0))}
# ("obstacle_build_mesh", name): small closed meshes, voxelised on the OBSTACLE_SPACING lattice of the box
WALK_MESHES = {"ico": lambda: mesh_obstacle_cases.icosphere(2, 0.35, (-0.6, -0.8, -0.6), rotation_seed=5)}


def caller_field(seed):
    """the field of ("obstacle_set_grid", seed): a ball in the fluid, roughened -- no distance"""
    x, y, z = (a.astype(np.float64) for a in om.node_positions(CALLER_GRID))
    d = np.sqrt((x[None, None, :] + 0.6) ** 2 + (y[None, :, None] + 0.8) ** 2 + (z[:, None, None] + 0.6) ** 2) - 0.35
    return (d + np.random.default_rng(seed).normal(0.0, 0.02, d.shape)).astype(np.float32)


# ---- numpy models whose result is shared: a build of a mesh on a lattice, the mesh of a particle set --------------------------------
_SHARED = {}


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _grid_key(grid):
    return tuple(int(v) for v in grid["dims"]), _digest(np.asarray(grid["origin"], np.float32)), float(grid["spacing"])


def mesh_field(vertices, triangles, grid, invert=False):
    """(phi, (used, skipped, lost crossings, odd columns)) of mesh_obstacle_model.build, computed once per mesh and lattice"""
    key = ("field", _digest(vertices, triangles), _grid_key(grid), bool(invert))
    if key not in _SHARED:
        phi, stats = mom.build(grid, vertices, triangles, 0, invert)
        phi.setflags(write=False)
        _SHARED[key] = (phi, tuple(int(v) for v in stats))
    return _SHARED[key]


def walk_mesh(name):
    if ("mesh", name) not in _SHARED:
        _SHARED["mesh", name] = WALK_MESHES[name]()
    return _SHARED["mesh", name]


def fluid_mesh(pos, box_min, box_max, radius, params):
    """mesh_model.mesh_of, computed once per particle set (by the bits of the positions), box and parameters"""
    import mesh_model
    key = ("fluid", _digest(pos), tuple(box_min), tuple(box_max), float(radius), tuple(sorted(params.items())))
    if key not in _SHARED:
        _SHARED[key] = mesh_model.mesh_of(pos, box_min, box_max, radius, **params)
    return _SHARED[key]


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
                "obstacle_motion", "obstacle_pose", "obstacle_sensor", "obstacle_build_mesh"): return f"{name}:{op[1]}"
    if name == "extract_mesh" and len(op) > 1: return f"{name}:{op[1]}"
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
        # the pose and the load sensor, by the header's words: the pose belongs to the context like the motion (another grid keeps
        # it, a clear resets it); the sensor is legal without an obstacle; sph_obstacle_clear keeps the switch and zeroes the load
        # and `steps`; `steps` counts the integrates that ran with both a grid and the sensor; while the switch is off nothing is
        # summed, and switching it on again or installing a grid over another keeps the load and `steps` as they are
        self.pose, self.sense, self.load_steps = None, False, 0
        self.posed_sense_steps = 0       # ... of which the context was also posed (what the histories are chosen by)
        self.have_mesh = False           # sph_mesh_extract has run: sph_mesh_dev has pointers for sph_obstacle_build_mesh_dev
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

    def _integrated(self):
        self.have_force = self.have_coll = False
        self.integrated = True
        if self.obstacle is not None:
            self.ob_steps += 1
            self.load_steps += self.sense
            self.posed_sense_steps += self.sense and self.pose is not None

    def _fused(self):
        self._row("force_finish")
        self._integrated()

    def _phase(self, name):
        if name == "hash": self._hash()
        elif name == "sort": self._sort()
        elif name == "build_cells": self.stage = CELLS
        elif name == "density": self.have_dens = True
        elif name == "force": self.have_force = True
        elif name == "collide": self.have_coll = True
        elif name == "integrate": self._integrated()
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
        elif name == "obstacle_clear":             # (the motion and the pose go with it; the sensor's switch stays, its count starts again)
            self.obstacle = self.motion = self.pose = None; self.load_steps = 0; self._row("sph_obstacle_build")
        elif name == "obstacle_sample":
            if self.obstacle is None: return E_STATE
            self._row("sph_obstacle_build")
        elif name == "obstacle_pose": self.pose = None if op[1] == "none" else op[1]; self._row("sph_obstacle_build")
        elif name == "obstacle_sensor": self.sense = bool(op[1]); self._row("sph_obstacle_build")
        elif name in ("obstacle_get_pose", "obstacle_load"): self._row("sph_obstacle_build")
        elif name == "obstacle_build_mesh": self.obstacle = ("mesh", op[1]); self._row("sph_obstacle_build")
        elif name == "obstacle_mesh_stats":        # SPH_E_STATE unless the installed obstacle came from a mesh
            if self.obstacle is None or self.obstacle[0] not in ("mesh", "mesh_dev"): return E_STATE
            self._row("sph_obstacle_build")
        elif name == "obstacle_build_mesh_dev":    # fed by sph_mesh_dev, which returns SPH_E_STATE while no mesh was extracted
            if not self.have_mesh: return E_STATE
            self.obstacle = ("mesh_dev",); self._row("sph_obstacle_build")
        elif name in VIEWS:
            self.have_mesh |= name == "extract_mesh"
            self._row("sph_mesh_extract")
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
    # a moving, turning, sensing obstacle from the start: every call of CALLS meets a context whose pose has already advanced
    # (the boundary re-seats it, see Walker.rebase) and whose sensor buffers exist
    "stepped_posed": dict(before=[("obstacle_build", "both"), ("obstacle_motion", "in"), ("obstacle_pose", "turning"),
                                  ("obstacle_sensor", 1), _UP] + _STEPPED, after=[]),
    # ... and 313 waves (more than one partial run in front of k_obstacle_load) with two mover tiles under the posed push
    "hashed_20k_posed": dict(before=[("obstacle_build", "both"), ("obstacle_pose", "turning"), ("obstacle_sensor", 1),
                                     ("upload", 20000, "flow")] + _STEPPED, after=[("hash",)], capacity=24576, calls="few"),
}
# the prefixes that also run HEAVY (below); all of them are at CELLS, so HEAVY brings the other three stages along
HEAVY_PREFIXES = ("stepped", "cells", "stepped_obstacle", "stepped_posed")
CONTINUATIONS = ("phases", "fci", "step")

# name -> (class, ops, anchor): anchor True = the step that follows also runs against the float64 model; "bare" = the first
# integrate that follows is tests/obstacle_model.py's push applied to the output of a BARE twin (Walker.bare), a context without
# the obstacle.  (A prefix that installs an obstacle runs every call it has with the bare twin, and none against the float64
# model, which knows no obstacle.)
_OB = ("obstacle_build", "both")
_TURN, _SENSE, _MESH = ("obstacle_pose", "turning"), ("obstacle_sensor", 1), ("obstacle_build_mesh", "ico")
_OWN = [("extract_mesh", "coarse"), ("obstacle_build_mesh_dev",), ("obstacle_motion", "mould")]
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
    # the pose, the load sensor and the mesh doors
    "pose_on": ("keep", [_OB, _TURN], "bare"),
    "pose_off": ("keep", [_OB, _TURN, ("obstacle_pose", "none")], "bare"),
    "pose_still_moving": ("keep", [_OB, ("obstacle_motion", "on"), ("obstacle_pose", "still")], "bare"),
    "pose_alone": ("keep", [_TURN], False),                                        # no grid: nothing pushes, the quaternion stays
    "pose_on_caller_grid": ("keep", [("obstacle_set_grid", 52), _TURN], "bare"),
    "pose_on_mesh": ("keep", [_MESH, _TURN], "bare"),
    "sensor_on": ("keep", [_OB, _SENSE], "bare"),
    "sensor_posed": ("keep", [_OB, _TURN, _SENSE], "bare"),
    "sensor_alone": ("keep", [_SENSE, ("obstacle_load",)], False),                 # no grid: legal, reads zeros
    "sensor_off_again": ("keep", [_OB, _SENSE, ("obstacle_sensor", 0)], "bare"),
    "load_read": ("keep", [("obstacle_load",)], False),
    "pose_read": ("keep", [("obstacle_get_pose",)], False),
    "mesh_on": ("keep", [_MESH], "bare"),
    "mesh_stats": ("keep", [_MESH, ("obstacle_mesh_stats",)], "bare"),
    "mesh_stats_none": ("keep", [("obstacle_mesh_stats",)], False),                # refused: no obstacle, or not one from a mesh
    "mesh_from_own_none": ("keep", [("obstacle_build_mesh_dev",)], False),         # refused: no mesh was extracted
    "mesh_replaced": ("keep", [_OB, _MESH], "bare"),
    "posed_remove": ("edit", [_OB, _TURN, _SENSE, ("remove", 0)], "bare"),
    "posed_emit": ("edit", [_OB, _TURN, _SENSE, ("emit", 120, 47, False)], "bare"),
    "posed_set_by_index": ("edit", [_OB, _TURN, _SENSE, ("set_by_index", "both", 36)], "bare"),
    "posed_load_snapshot": ("edit", [_OB, _TURN, _SENSE, ("load_snapshot",)], "bare"),
    "posed_box_moved": ("keep", [_OB, _TURN, _SENSE, ("set_params", "shift")], "bare"),
    # the device door: the context's own last mesh, inverted (a mould of the fluid's shape) and set aside so that it touches some
    # particles and not all.  numpy voxelises a few thousand triangles in seconds, so these calls run under HEAVY_PREFIXES only and
    # reach LOADED, HASHED and SORTED by an edit of velocities (the positions, and so the shared model, stay) or by phase calls
    "mesh_from_own": ("keep", _OWN, "bare"),
    "mesh_from_own_loaded": ("edit", [("set_by_index", "vel", 37)] + _OWN, "bare"),
    "mesh_from_own_hashed": ("keep", [("hash",)] + _OWN, "bare"),
    "mesh_from_own_sorted": ("keep", [("hash",), ("sort",)] + _OWN, "bare"),
    # ... and a mesh that is an edit old: the device buffers the view left behind, voxelised around other particles (the twin, born
    # behind the edit, has no such mesh and is handed the grid through sph_obstacle_set_grid)
    "mesh_from_own_stale": ("edit", [_OWN[0], ("emit", 120, 48, False)] + _OWN[1:], "bare"),
}
HEAVY = ("mesh_from_own", "mesh_from_own_loaded", "mesh_from_own_hashed", "mesh_from_own_sorted", "mesh_from_own_stale")
FEW = ("upload_smaller", "reset_lattice", "set_by_index_both", "emit_auto", "remove_something", "remove_nothing", "remove_emit",
       "emit_remove", "params_box_moved", "precision_mixed", "sort_mode_0", "hash_again", "refused_phase",
       "obstacle_on", "obstacle_off", "obstacle_moving", "obstacle_remove", "obstacle_emit",
       "sensor_posed", "posed_remove", "posed_emit", "mesh_on")


def calls_for(prefix):
    if PREFIXES[prefix].get("calls", "all") != "all":
        return list(FEW)
    return [c for c in CALLS if c not in HEAVY or prefix in HEAVY_PREFIXES]


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
# histories that draw the pose, the sensor and the mesh doors as well (extended="pose"); what each of them holds is said in
# tests/test_context_walk_cpu.py.  The device door is drawn only where it is refused: its numpy model costs seconds per particle set.
FUZZ_SEEDS_POSE = (319, 370, 371, 400, 401, 420)
FUZZ_CAPACITY = 16384


def fuzz_ops(seed, n_ops=40, extended=False):
    """The operation list of one seed: an upload and n_ops calls, each legal or deliberately illegal by the mirror.  extended: a
    quarter of the calls are the obstacle's or a view (drawn first, so the lists of the plain seeds are what they always were);
    extended="pose": three in ten are the pose's, the sensor's or a mesh door's (drawn before those, so the lists of the obstacle
    seeds are what they were as well)."""
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
        if extended == "pose" and rng.random() < 0.3:
            k = int(rng.integers(12))
            if k in (0, 1): push(("obstacle_pose", "turning"))
            elif k == 2: push(("obstacle_pose", "still"))
            elif k == 3: push(("obstacle_pose", "none"))
            elif k in (4, 5): push(("obstacle_sensor", 1))
            elif k == 6: push(("obstacle_sensor", 0))
            elif k == 7: push(("obstacle_load",))
            elif k == 8: push(("obstacle_get_pose",))
            elif k == 9: push(("obstacle_build_mesh", "ico"))
            elif k == 10: push(("obstacle_mesh_stats",))      # refused unless the grid came from a mesh
            elif not m.have_mesh: push(("obstacle_build_mesh_dev",))     # refused: no mesh was extracted
            else: push(("obstacle_get_pose",))
            continue
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


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_NO_POSE = {"pivot": np.zeros(3, np.float32), "q": np.array([1.0, 0.0, 0.0, 0.0]), "omega": np.zeros(3, np.float32)}


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
        # the pose as numpy knows it (never read from the library): kept by pm.quat_set (through pm.pose), pm.quat_step (through
        # pm.advance) alone; pose_args is what the last set_obstacle_pose was given, pose_moved whether an integrate advanced it since
        self.pose, self.pose_args, self.pose_moved = None, None, False
        # the load as numpy knows it: `about` of the last sensing integrate, and J, L where that integrate was anchored (None: it
        # was not, and only the twin can say)
        self.load = {"J": np.zeros(3), "L": np.zeros(3), "about": np.zeros(3, np.float32)}
        self.own_mesh = None             # (vertices, triangles) of the last extract_mesh, by the model
        self.anchor_sensed = self.anchor_kicked = 0
        self.anchor_last = None          # (touched, n) of the last anchored integrate

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
            mp = self.capi.mesh_defaults(**(MESH_COARSE if len(op) > 1 else MESH))
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
        if name == "obstacle_pose": return _rc(c.set_obstacle_pose, None) if op[1] == "none" else _rc(c.set_obstacle_pose, *POSES[op[1]])
        if name == "obstacle_get_pose": return _rc(self.pose_state, c)
        if name == "obstacle_sensor": return _rc(c.set_obstacle_sensor, bool(op[1]))
        if name == "obstacle_load": return _rc(c.obstacle_load)
        if name == "obstacle_build_mesh": return _rc(c.build_obstacle_mesh, *walk_mesh(op[1]), spacing=OBSTACLE_SPACING)
        if name == "obstacle_mesh_stats": return _rc(c.obstacle_mesh_stats)
        if name == "obstacle_build_mesh_dev": return _rc(c.build_obstacle_from_mesh, spacing=OBSTACLE_SPACING, invert=True)
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
        ob_steps, off_before, pose_before = m.ob_steps, self.off, self.pose
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
        for _ in range(m.ob_steps - ob_steps):     # once per integrate with a grid installed: the load's point, then offset and pose
            if m.sense:
                self.load = {"J": None, "L": None, "about": pm.world_pivot(self.pose, self.off)}
            if self.pose is not None:
                self.pose, self.pose_moved = pm.advance(self.pose, self.off, self.u, self.dt)[0], True
            self.off = om.advance(self.off, self.u, self.dt, 1)
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
        elif self.t is not None and name == "obstacle_build_mesh_dev" and not self.tm.have_mesh:
            # the mesh was extracted in front of the twin's boundary: the twin gets the grid through another door, as in _fresh
            _, origin, spacing, _, _, phi = self.obstacle_state(c)
            self.t.set_obstacle_grid(phi, origin, spacing)
            self.tm.apply(("obstacle_set_grid", 0))
            c.sync(); self.t.sync()
        elif self.t is not None and self.tm.apply(op) == 0:
            rc2, _ = self._perform(self.t, op)
            assert rc2 == 0, f"{op}: the twin returned {rc2}"
            c.sync(); self.t.sync()               # lockstep: a sort may look at a count the device has produced
            self._bare_follows(op, m.ob_steps - ob_steps, off_before, pose_before)
        if m.ob_steps > ob_steps and m.sense:     # every integrate of a sensing context: steps, about and, where anchored, J and L
            self._check_load(c.obstacle_load(), f"behind {self.trace[-3:]}")
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
            self.pose = self.pose_args = None
            self.load = {"J": np.zeros(3), "L": np.zeros(3), "about": np.zeros(3, np.float32)}
        elif name == "obstacle_pose":
            if op[1] == "none":
                self.pose = self.pose_args = None
            else:
                self._seat(*POSES[op[1]])
        elif name == "obstacle_get_pose":
            self._check_pose(out, f"{op}")
        elif name == "obstacle_load":
            self._check_load(out, f"{op}")
        elif name in ("obstacle_build_mesh", "obstacle_build_mesh_dev"):      # the lattice of sph_obstacle_build, of the box as it is now
            p = self._params()
            grid = om.lattice(OBSTACLE_SPACING, tuple(p.box_min), tuple(p.box_max), p.particle_radius)
            mesh, invert = (walk_mesh(op[1]), False) if name == "obstacle_build_mesh" else (self.own_mesh, True)
            phi, stats = mesh_field(mesh[0], mesh[1], grid, invert)
            self.ob = {"grid": grid, "phi": phi, "stats": stats}
        elif name == "obstacle_mesh_stats":
            assert out == self.ob["stats"] and out[0] > 100 and not any(out[1:]), f"{op}: {out}, the model {self.ob['stats']}"
        elif name == "obstacle_sample":
            want = pm.sample(self.ob["grid"], self.ob["phi"], self.off, self.pose, sample_points())     # (unposed: obstacle_model.sample)
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

    def pose_state(self, c):
        """(posed, pivot, quat float64, omega, rot) as sph_obstacle_get_pose shows them, posed or not"""
        import ctypes as C
        posed, piv, q, w, rot = C.c_int(), (C.c_float * 3)(), (C.c_double * 4)(), (C.c_float * 3)(), (C.c_float * 9)()
        self.capi._check(c.L.sph_obstacle_get_pose(c.h, C.byref(posed), piv, q, w, rot))
        return (int(posed.value), np.array(list(piv), np.float32), np.array(list(q), np.float64), np.array(list(w), np.float32),
                np.array(list(rot), np.float32).reshape(3, 3))

    def _seat(self, pivot, quat, omega):
        """the record of a pose just set: pm.quat_set of the caller's float32 quaternion"""
        self.pose, self.pose_args, self.pose_moved = pm.pose(pivot, quat, omega), (pivot, quat, omega), False

    def _check_pose(self, got, tag):
        """sph_obstacle_get_pose against the record: without a pose the context reads the identity and zeros"""
        posed, piv, q, w, rot = got
        assert posed == (self.pose is not None) == (self.m.pose is not None), f"posed {posed} {tag}"
        ps = self.pose if self.pose is not None else _NO_POSE
        assert np.array_equal(_bits(piv), _bits(ps["pivot"])) and np.array_equal(_bits(w), _bits(ps["omega"])), f"pivot, omega {tag}"
        assert np.array_equal(_bits64(q), _bits64(ps["q"])), f"quaternion {q}, by numpy {ps['q']} {tag}"
        assert np.array_equal(_bits(rot), _bits(pm.rot_of(ps["q"]))), f"rot {tag}"

    def _check_load(self, got, tag):
        """sph_obstacle_get_load against the record and the mirror's count"""
        assert got["steps"] == self.m.load_steps, f"load steps {got['steps']}, the header's words say {self.m.load_steps} {tag}"
        assert np.array_equal(_bits(got["about"]), _bits(self.load["about"])), f"load about {got['about']}, by numpy {self.load['about']} {tag}"
        for k in ("J", "L"):
            if self.load[k] is not None:
                assert np.array_equal(_bits64(got[k]), _bits64(self.load[k])), f"load {k} {got[k]}, by numpy {self.load[k]} {tag}"

    def _check_obstacle(self, tag):
        """what the library shows of the obstacle against numpy's record, and the twin's against the context's"""
        m = self.m
        pose, load = self.pose_state(self.c), self.c.obstacle_load()
        self._check_pose(pose, tag)
        self._check_load(load, tag)
        for x, y in zip(pose, self.pose_state(self.t)):       # the twin was handed the pose (Walker.rebase) and advances it alike
            assert np.array_equal(np.atleast_1d(x).view(np.uint8), np.atleast_1d(y).view(np.uint8)), f"the twin's pose {tag}"
        if self.tm.load_steps > 0:       # both have summed since the boundary (the twin is younger: not `steps`)
            twin = self.t.obstacle_load()
            assert np.array_equal(_bits64(load["J"]), _bits64(twin["J"])) and np.array_equal(_bits64(load["L"]), _bits64(twin["L"])), \
                f"the twin's load {tag}"
            assert np.array_equal(_bits(load["about"]), _bits(twin["about"])), f"the twin's load about {tag}"
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
        import render_model, surface_model
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
            counts, origin, _, mpos, mnrm, mtri = fluid_mesh(pos, tuple(p.box_min), tuple(p.box_max), R, MESH_COARSE if len(op) > 1 else MESH)
            self.own_mesh = (mpos, mtri)     # what ("obstacle_build_mesh_dev",) voxelises: the library's, by the assertions below
            (dims, got_origin), (nv, nt), got_counts, gpos, gnrm, gtri = out
            assert dims == counts.shape[::-1] and np.array_equal(_bits(got_origin), _bits(origin)), f"{op}: lattice"
            assert nt == len(mtri) > 100 and nv == len(mpos), f"{op}: {nv} vertices, {nt} triangles; the model {len(mpos)}, {len(mtri)}"
            assert np.array_equal(got_counts, counts), f"{op}: counts"
            assert np.array_equal(_bits(gpos), _bits(mpos)) and np.array_equal(_bits(gnrm), _bits(mnrm)), f"{op}: vertices"
            assert np.array_equal(gtri, mtri), f"{op}: triangles"

    # -- the bare twin --------------------------------------------------------------------------------------------------------
    def _bare_follows(self, op, integrates, off_before, pose_before):
        """the bare twin makes the call too, unless it is the obstacle's; behind the first integrate since its boundary the context
        must hold the model's push of the bare twin's output"""
        if self.b is None or op[0] in OBSTACLE_OPS:
            return
        if self.bm.apply(op) == 0:
            assert self._perform(self.b, op)[0] == 0, f"{op}: the bare twin"
            self.b.sync()
        if op[0] in ("integrate", "fci", "step", "step_phased"):
            if self.b_fresh and integrates == 1:
                self._check_against_model(off_before, pose_before)
            self.b_fresh = False

    def _check_against_model(self, off_before, pose_before):
        """the integrate just made is the model's push of the bare twin's output, particle by particle IN SLOT ORDER (the load's
        sums depend on it; the two were uploaded alike and have sorted the same positions): obstacle_model.push, or
        obstacle_pose_model.push wherever the record is posed or sensing -- then also the load's J and L in the header's order"""
        c, p, live, m = self.c, self._params(), self.live, self.m
        tag = f"behind {self.trace[-3:]}"
        (pa, va, ia), (pb, vb, ib) = c.download_owned(), self.b.download_owned()
        assert np.array_equal(ia, ib), f"slot order against the bare twin's {tag}"
        solid = (self.ob["grid"], self.ob["phi"], off_before, self.u)
        walls = (tuple(p.box_min), tuple(p.box_max), p.wall_eps, p.wall_damping)
        st = None
        if pose_before is not None or m.sense:
            st = {}
            want_p, want_v, touched = pm.push(pb, vb, *solid, pose_before, *walls, p.mass, stats=st)
        else:
            want_p, want_v, touched = om.push(pb, vb, *solid, *walls)
        model = "obstacle_model.push" if st is None else "obstacle_pose_model.push"
        assert np.array_equal(_bits(pa), _bits(want_p)), \
            f"positions against {model} of the bare twin's: {int((_bits(pa) != _bits(want_p)).any(axis=1).sum())} of {touched.sum()} touched differ {tag}"
        assert np.array_equal(_bits(va), _bits(want_v)), f"velocities against {model} of the bare twin's {tag}"
        got, bare = c.download(want=("density", "pressure")), self.b.download(want=("density", "pressure"))
        for k in ("density", "pressure"):
            assert np.array_equal(_bits(got[k][live]), _bits(bare[k][live])), f"{k} against the bare twin's {tag}"
        if m.sense:                  # (`about` and `steps` are the record's and the mirror's already: Walker.do)
            self.load["J"], self.load["L"] = pm.load_in_order(st["lane"], st["kicked"], pb.shape[0])
            self._check_load(c.obstacle_load(), tag)
            self.anchor_sensed += 1
            self.anchor_kicked += int(st["kicked"].sum())
        self.anchored += 1
        self.anchor_touched += int(touched.sum())
        self.anchor_last = (int(touched.sum()), pb.shape[0])

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
            tm.obstacle, tm.motion = (None if phi is None else ("grid", "handed")), m.motion
            # the sensor's switch, and the pose by the arguments of its last set (rebase has re-seated a pose that had advanced)
            if m.sense:
                t.set_obstacle_sensor(True)
            if self.pose is not None:
                assert not self.pose_moved
                t.set_obstacle_pose(*self.pose_args)
            tm.sense, tm.pose = m.sense, m.pose
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
        if self.pose is not None and self.pose_moved:
            # sph_obstacle_get_pose shows float64 and sph_obstacle_set_pose takes float32 and normalises again: an advanced
            # pose has no exact way into a fresh context.  So the context under test is RE-SEATED first -- one more "kept"
            # call on it -- with what the twin can be given too, and the record follows by pm.quat_set
            shown = self.pose_state(c)
            self._check_pose(shown, "in front of the re-seat")
            pivot, _, omega = self.pose_args
            quat = tuple(float(v) for v in shown[2].astype(np.float32))
            c.set_obstacle_pose(pivot, quat, omega)
            self._seat(pivot, quat, omega)
            self.trace.append(("re-seat the pose", quat))
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

"""The scenes of tests/test_gpu_render_solids.py as plain numpy -- TEST INFRASTRUCTURE in the style of obstacle_set_cases.py: the
solids of every slot with their looks, the camera, and the model's slots built from them with obstacle_model.rasterise or
mesh_obstacle_model.build (the device's fields bit for bit).  tests/test_solid_render_model_cpu.py holds every scene to the step
budget on the model alone; the GPU tests compare every plane with the model fed with the device's own grids, offsets and poses."""
import functools

import numpy as np

import mesh_obstacle_cases as mc
import mesh_obstacle_model as mm
import obstacle_model as om
import obstacle_pose_model as pm
import solid_render_model as so
from gpufluidsimulator_amd import capi

F = np.float32
BOX, GRID = (2.0, 2.0, 2.0), (32, 32, 32)          # the context: cell edge 1/16
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
S = 1.0 / 16.0                                     # 35 nodes per axis over the box
ZERO = (0.0, 0.0, 0.0)
SKEW = (0.9, 0.2, -0.3, 0.25)                      # (w, x, y, z), not normalised: not axis-aligned
DT = 2e-5


def solid(shapes=None, mesh=None, spacing=S, bounds=None, off=ZERO, u=ZERO, pivot=None, quat=None, omega=ZERO, **look):
    """A solid: analytic shapes, or mesh = (vertices, triangles, band, invert); the motion, the pose (pivot None: unposed) and
    the look (draw, open, color)."""
    return dict(shapes=shapes, mesh=mesh, spacing=spacing, bounds=bounds, off=off, u=u, pivot=pivot, quat=quat, omega=omega,
                look=dict(dict(draw=1, open=0, color=so.DEFAULT_COLOR), **look))


def _cam(w, h, **kw):
    return functools.partial(capi.look_at, w, h, **kw)


SPHERE = solid([om.sphere((0.05, -0.03, 0.02), 0.45)])
_AABOX = mc.case("aligned_box")                    # the box (-0.5, -0.375, -0.25) .. (0.25, 0.5, 0.375) as 12 triangles
# the long floor of the budget scene: 143 x 4 x 4 nodes at s = 1/80, solid below y = -0.5.  A march advances by at least a
# quarter spacing per sample, so no ray can spend 512 samples inside a grid of 48 nodes per axis (its diagonal is 82 spacings:
# 326 samples); the one scene that must exhaust the budget therefore has one long axis, and stays a grid of 2288 nodes.
FLOOR_S = 1.0 / 80.0
FLOOR = solid([om.halfspace((0.0, -0.5, 0.0), (0.0, 1.0, 0.0))], spacing=FLOOR_S, bounds=((-0.875, -0.5125, -0.0125), (0.875, -0.5, 0.0)))

# name -> (camera, {slot: solid}, light, ambient)
SCENES = {
    "sphere": (_cam(96, 72, eye=(1.6, 1.1, 2.2), fovy_deg=35.0), {0: SPHERE}, so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    "sphere_other_side": (_cam(96, 72, eye=(-2.0, 0.4, -1.5), fovy_deg=40.0), {0: SPHERE}, (0.2, 1.0, -0.4), 0.1),
    "box_corner": (_cam(80, 60, eye=(1.5, 1.4, 1.6), fovy_deg=45.0),
                   {0: solid([om.box((0.0, 0.0, 0.0), (0.35, 0.3, 0.25), 0.08)], color=(0.9, 0.5, 0.2))}, so.DEFAULT_LIGHT, 0.25),
    "capsule": (_cam(80, 60, eye=(0.3, 0.8, 2.4), fovy_deg=50.0),
                {2: solid([om.capsule((-0.4, -0.2, 0.1), (0.4, 0.3, -0.1), 0.2)], color=(0.2, 0.8, 0.4))}, (-1.0, 0.5, -1.0), 0.0),
    "ragged_tiles": (_cam(67, 45, eye=(1.6, 1.1, 2.2), fovy_deg=35.0), {0: SPHERE}, so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    # odd sizes and the reference's axis-aligned view: ex = 0 on column 32, ey = 0 on row 24, so D has zero components there
    "axis_aligned": (_cam(65, 49, fovy_deg=35.0), {0: solid([om.sphere((0.0, 0.0, 0.0), 0.45)])}, so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    # slot 1 turns about a skew axis, slot 3 drifts, and they overlap; slot 0 stands in front of both and is not drawn
    "two_slots": (_cam(120, 90, eye=(0.4, 0.9, 2.3), fovy_deg=50.0),
                  {0: solid([om.sphere((0.1, 0.2, 0.9), 0.3)], draw=0),
                   1: solid([om.box((-0.1, 0.0, 0.0), (0.5, 0.08, 0.3))], bounds=((-0.7, -0.2, -0.4), (0.5, 0.2, 0.4)), off=(0.03, -0.02, 0.04),
                            u=(50.0, 0.0, -20.0), pivot=(-0.1, 0.0, 0.0), quat=SKEW, omega=(300.0, -200.0, 4000.0), color=(0.85, 0.3, 0.3)),
                   3: solid([om.sphere((0.15, 0.05, 0.05), 0.3)], off=(-0.01, 0.015, 0.0), u=(-300.0, 600.0, 100.0), color=(0.3, 0.4, 0.9))},
                  so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    # a bowl: the inverted sphere seen from outside its grid.  open: the far inside wall; not open: the face of the grid's box
    "bowl_open": (_cam(80, 60, eye=(0.0, 0.9, 2.6), fovy_deg=50.0), {0: solid([om.sphere(ZERO, 0.8, invert=True)], open=1)},
                  so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    "bowl_closed": (_cam(80, 60, eye=(0.0, 0.9, 2.6), fovy_deg=50.0), {0: solid([om.sphere(ZERO, 0.8, invert=True)], open=0)},
                    so.DEFAULT_LIGHT, so.DEFAULT_AMBIENT),
    # truncated fields from a mesh: beyond W = band * s the field is flat (+-W) and its gradient zero.  Inverted and not open,
    # a ray meets the flat -W at the face of the grid's box: the (0, 1, 0) fallback normal
    "mesh_band2": (_cam(80, 60, eye=(1.5, 1.2, 1.9), fovy_deg=45.0), {0: solid(mesh=_AABOX[:2] + (2, False))}, so.DEFAULT_LIGHT, 0.25),
    "mesh_band3": (_cam(80, 60, eye=(1.5, 1.2, 1.9), fovy_deg=45.0), {1: solid(mesh=_AABOX[:2] + (3, False))}, so.DEFAULT_LIGHT, 0.25),
    "mesh_band3_inverted": (_cam(80, 60, eye=(1.5, 1.2, 1.9), fovy_deg=45.0), {0: solid(mesh=_AABOX[:2] + (3, True))}, so.DEFAULT_LIGHT, 0.25),
    "mesh_band2_bowl": (_cam(80, 60, eye=(1.5, 1.2, 1.9), fovy_deg=45.0), {0: solid(mesh=_AABOX[:2] + (2, True), open=1)}, so.DEFAULT_LIGHT, 0.25),
    # the one scene that exhausts SPH_SOLID_MAX_STEPS: the centre rays graze the floor 0.002 above it, under a quarter spacing,
    # along 142 cells -- 568 samples of a quarter spacing each
    "budget": (_cam(33, 9, eye=(-1.5, -0.498, -0.00625), target=(1.5, -0.498, -0.00625), fovy_deg=1.0), {0: FLOOR}, so.DEFAULT_LIGHT,
               so.DEFAULT_AMBIENT),
}
EXHAUSTS = ("budget",)
# the solid the fluid scenes stand around, and their camera
FLUID_SOLID = solid([om.sphere((0.0, 0.0, 0.0), 0.35)], color=(0.8, 0.7, 0.3))
FLUID_CAM = _cam(120, 90, eye=(0.0, 0.3, 2.4), fovy_deg=45.0)


def pose_of(sd):
    return None if sd["pivot"] is None else pm.pose(sd["pivot"], sd["quat"], sd["omega"])


def grid_of(sd):
    lo, hi = sd["bounds"] if sd["bounds"] is not None else (BMIN, BMAX)
    return om.lattice(sd["spacing"], lo, hi)


@functools.lru_cache(maxsize=None)
def _field(name, k):
    sd = SCENES[name][1][k] if name != "fluid" else FLUID_SOLID
    grid = grid_of(sd)
    if sd["mesh"] is not None:
        v, t, band, invert = sd["mesh"]
        phi = mm.build(grid, v, t, band, invert)[0]
    else:
        phi = om.rasterise(sd["shapes"], grid)
    phi.setflags(write=False)
    return grid, phi


def model_slot(sd, grid, phi, off=None, pose="own"):
    """The model's slot of a solid: grid and phi as the device reports them or (CPU) built here; off and pose as they are NOW."""
    return so.slot(grid, phi, sd["off"] if off is None else off, pose_of(sd) if isinstance(pose, str) else pose, **sd["look"])


def model_slots(name):
    """The slots of a scene as installed (nothing advanced), by the CPU models; shared fields, left unchanged."""
    return {k: model_slot(sd, *_field(name, k)) for k, sd in SCENES[name][1].items()}


def fluid_slot():
    return model_slot(FLUID_SOLID, *_field("fluid", 0))


def fluid_particles():
    """Three blocks of 10 x 10 x 10 around FLUID_SOLID as FLUID_CAM sees it: in front of the sphere, behind it, and a shell of
    particles ON its surface (their sprites' depths lie on either side of the hit's, pixel by pixel)."""
    r = np.random.default_rng(77)
    g = (np.mgrid[0:10, 0:10, 0:10].reshape(3, -1).T.astype(np.float64) - 4.5) * (1.0 / 32.0)
    front = g * (1.0, 1.0, 0.5) + (-0.15, 0.05, 0.8)
    back = g * (0.8, 0.8, 0.5) + (-0.12, -0.12, -0.7)
    d = r.normal(size=(1000, 3))
    d[:, 2], d[:, 0] = np.abs(d[:, 2]), np.abs(d[:, 0])             # the quarter that faces the camera, on its right
    shell = 0.35 * d / np.linalg.norm(d, axis=1, keepdims=True) * r.uniform(0.88, 1.04, (1000, 1))
    return np.concatenate([front, back, shell]).astype(F)


def thin_sheet():
    """A sheet of one layer of particles in front of FLUID_SOLID, wider than the sphere: the solid shows through it."""
    g = np.mgrid[0:48, 0:36].reshape(2, -1).T.astype(np.float64)
    pos = np.stack([(g[:, 0] - 23.5) / 40.0, (g[:, 1] - 17.5) / 40.0 + 0.05, np.full(len(g), 0.6)], axis=1)
    return pos.astype(F)

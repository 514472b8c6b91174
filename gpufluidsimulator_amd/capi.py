"""ctypes binding of the C ABI in include/sph_hip.h (libsph_hip.so).

This is plumbing only: every compute call lands in the hand-written HIP library.  There is
no CPU fallback -- a missing library or a missing gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPH_HIP_LIB", os.path.join(HERE, "libsph_hip.so"))

PHASES = ("z-index", "sort", "b-grid", "dens", "force", "collision", "integrate")
HALO_RECORD_FLOATS = 8


class SphError(RuntimeError):
    pass


# int exchange(void* self, int tag, const void* send_lo, size_t, void* recv_lo, size_t, const void* send_hi, size_t,
#              void* recv_hi, size_t, void* hip_stream)   -- `sph_transport.exchange` of include/sph_hip.h
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                          C.c_void_p, C.c_size_t, C.c_void_p)


class Transport(C.Structure):
    """`sph_transport` of include/sph_hip.h."""
    _fields_ = [("self", C.c_void_p), ("exchange", EXCHANGE_FN), ("host_buffers", C.c_int),
                ("abort", C.CFUNCTYPE(None, C.c_void_p))]


class Params(C.Structure):
    """`sph_params` of include/sph_hip.h."""
    _fields_ = [("box_min", C.c_float * 3), ("box_max", C.c_float * 3), ("grid", C.c_uint32 * 3),
                ("h", C.c_float), ("mass", C.c_float), ("rest_density", C.c_float), ("gas_constant", C.c_float),
                ("viscosity", C.c_float), ("gravity_y", C.c_float), ("wall_eps", C.c_float),
                ("wall_damping", C.c_float), ("restitution", C.c_float), ("collision_param", C.c_float),
                ("particle_radius", C.c_float)]


MAX_COLLIDERS = 8          # SPH_MAX_COLLIDERS


class Collider(C.Structure):
    """`sph_collider` of include/sph_hip.h: one solid sphere."""
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("velocity", C.c_float * 3), ("pad", C.c_float)]


class ColliderBody(C.Structure):
    """`sph_collider_body` of include/sph_hip.h: mass 0 = kinematic, > 0 = a free body under the constant `accel`."""
    _fields_ = [("mass", C.c_float), ("accel", C.c_float * 3)]


MAX_REGIONS = 8            # SPH_MAX_REGIONS
REGION_SPHERE, REGION_BOX, REGION_HALFSPACE = 0, 1, 2


class Region(C.Structure):
    """`sph_region` of include/sph_hip.h: what sph_remove / sph_count_in_regions select by position (32 bytes)."""
    _fields_ = [("kind", C.c_int32), ("a", C.c_float * 3), ("b", C.c_float * 3), ("r", C.c_float)]

    @classmethod
    def sphere(cls, center, radius):
        """d = x - center; d.d < radius^2 (strict)."""
        return cls(REGION_SPHERE, (C.c_float * 3)(*[float(v) for v in center]), (C.c_float * 3)(), float(radius))

    @classmethod
    def box(cls, lo, hi):
        """lo <= x < hi on every axis (half open)."""
        return cls(REGION_BOX, (C.c_float * 3)(*[float(v) for v in lo]), (C.c_float * 3)(*[float(v) for v in hi]), 0.0)

    @classmethod
    def halfspace(cls, point, normal):
        """(x - point) . normal < 0 (strict): the side the normal points away from."""
        return cls(REGION_HALFSPACE, (C.c_float * 3)(*[float(v) for v in point]), (C.c_float * 3)(*[float(v) for v in normal]), 0.0)


MAX_SHAPES = 16                       # SPH_MAX_SHAPES
OBSTACLE_MAX_DIM = 2048               # SPH_OBSTACLE_MAX_DIM
OBSTACLE_MAX_NODES = 1 << 27          # SPH_OBSTACLE_MAX_NODES
OBSTACLE_PUSH_ITERATIONS = 4          # SPH_OBSTACLE_PUSH_ITERATIONS
SHAPE_SPHERE, SHAPE_BOX, SHAPE_CAPSULE, SHAPE_HALFSPACE = 0, 1, 2, 3


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Shape(C.Structure):
    """`sph_shape` of include/sph_hip.h: one analytic solid of sph_obstacle_build (36 bytes)."""
    _fields_ = [("kind", C.c_int32), ("invert", C.c_int32), ("a", C.c_float * 3), ("b", C.c_float * 3), ("r", C.c_float)]

    @classmethod
    def sphere(cls, center, radius, invert=False):
        return cls(SHAPE_SPHERE, int(bool(invert)), _f3(center), _f3((0, 0, 0)), float(radius))

    @classmethod
    def box(cls, center, half_extents, rounding=0.0, invert=False):
        """Axis-aligned, optionally with rounded edges."""
        return cls(SHAPE_BOX, int(bool(invert)), _f3(center), _f3(half_extents), float(rounding))

    @classmethod
    def capsule(cls, end_a, end_b, radius, invert=False):
        return cls(SHAPE_CAPSULE, int(bool(invert)), _f3(end_a), _f3(end_b), float(radius))

    @classmethod
    def halfspace(cls, point, normal, invert=False):
        """Solid on the side the normal points away from."""
        return cls(SHAPE_HALFSPACE, int(bool(invert)), _f3(point), _f3(normal), 0.0)


class ObstacleGrid(C.Structure):
    """`sph_obstacle_grid` of include/sph_hip.h: node (i, j, k) sits at origin + (i, j, k) * spacing; x fastest."""
    _fields_ = [("dims", C.c_uint32 * 3), ("origin", C.c_float * 3), ("spacing", C.c_float)]


class ObstaclePose(C.Structure):
    """`sph_obstacle_pose` of include/sph_hip.h: a pivot of the body frame, the quaternion (w, x, y, z) body -> world, omega in world axes."""
    _fields_ = [("pivot", C.c_float * 3), ("quat", C.c_float * 4), ("omega", C.c_float * 3)]


BODY_FREE_X, BODY_FREE_Y, BODY_FREE_Z, BODY_SPIN, BODY_HINGE = 1, 2, 4, 8, 16     # SPH_BODY_*
BODY_FREE_XYZ = BODY_FREE_X | BODY_FREE_Y | BODY_FREE_Z


class ObstacleBody(C.Structure):
    """`sph_obstacle_body` of include/sph_hip.h (80 bytes): which motions of an obstacle slot the fluid drives, and with what."""
    _fields_ = [("dof", C.c_uint32), ("mass", C.c_float), ("inertia", C.c_float * 3), ("axis", C.c_float * 3),
                ("accel", C.c_float * 3), ("torque", C.c_float * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]

    @classmethod
    def make(cls, dof=0, mass=0.0, inertia=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 0.0), accel=(0.0, 0.0, 0.0), torque=(0.0, 0.0, 0.0),
             lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0)):
        return cls(int(dof), float(mass), _f3(inertia), _f3(axis), _f3(accel), _f3(torque), _f3(lo), _f3(hi))

    def as_dict(self):
        out = {"dof": int(self.dof), "mass": np.float32(self.mass)}
        for f in ("inertia", "axis", "accel", "torque", "lo", "hi"):
            out[f] = np.array(list(getattr(self, f)), np.float32)
        return out


OBSTACLE_MESH_MAX_BAND = 16        # SPH_OBSTACLE_MESH_MAX_BAND
OBSTACLE_MESH_DEFAULT_BAND = 3     # SPH_OBSTACLE_MESH_DEFAULT_BAND


class ObstacleMeshParams(C.Structure):
    """`sph_obstacle_mesh_params` of include/sph_hip.h (sph_obstacle_build_mesh); 0 in a field = its default."""
    _fields_ = [("spacing", C.c_float), ("band", C.c_uint32), ("invert", C.c_int32)]


RENDER_MAX_RADIUS_PX = 64   # SPH_RENDER_MAX_RADIUS_PX
RENDER_MAX_SIZE = 4096      # SPH_RENDER_MAX_SIZE
COLOR_MODES = {"index": 0, "speed": 1, "density": 2}      # SPH_COLOR_*


class Camera(C.Structure):
    """`sph_camera` of include/sph_hip.h: eye space has +x right, +y up, +z forward."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rot", C.c_float * 9), ("trans", C.c_float * 3),
                ("focal_px", C.c_float), ("near_z", C.c_float), ("far_z", C.c_float)]


class RenderStyle(C.Structure):
    """`sph_render_style` of include/sph_hip.h."""
    _fields_ = [("color_mode", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("radius", C.c_float),
                ("index_count", C.c_uint32), ("background", C.c_uint8 * 4)]


class SurfaceStyle(C.Structure):
    """`sph_surface_style` of include/sph_hip.h (sph_render_surface); surface_defaults() fills one."""
    _fields_ = [("smooth_radius_px", C.c_uint32), ("smooth_iterations", C.c_uint32), ("depth_falloff", C.c_float),
                ("flat_color", C.c_int32), ("tint", C.c_float * 3), ("absorb", C.c_float * 3), ("light", C.c_float * 3),
                ("specular", C.c_float)]


class SolidLook(C.Structure):
    """`sph_solid_look` of include/sph_hip.h: how one obstacle slot is drawn."""
    _fields_ = [("draw", C.c_int32), ("open", C.c_int32), ("color", C.c_float * 3)]


class SolidStyle(C.Structure):
    """`sph_solid_style` of include/sph_hip.h (sph_render_set_solids); solid_defaults() fills one."""
    _fields_ = [("slot", SolidLook * 4), ("light", C.c_float * 3), ("ambient", C.c_float)]     # 4: SPH_MAX_OBSTACLES


RENDER_ID_SOLID = 0xFFFFFFF0  # SPH_RENDER_ID_SOLID: the id plane of a pixel won by slot k reads RENDER_ID_SOLID + k
SOLID_MAX_STEPS = 512         # SPH_SOLID_MAX_STEPS
SOLID_BISECTIONS = 6          # SPH_SOLID_BISECTIONS
SURFACE_MAX_RADIUS_PX = 16   # SPH_SURFACE_MAX_RADIUS_PX
SURFACE_MAX_ITERATIONS = 8   # SPH_SURFACE_MAX_ITERATIONS
MESH_MAX_REACH = 8           # SPH_MESH_MAX_REACH
MESH_MAX_DIM = 2048          # SPH_MESH_MAX_DIM
MESH_MAX_NODES = 1 << 27     # SPH_MESH_MAX_NODES


class MeshParams(C.Structure):
    """`sph_mesh_params` of include/sph_hip.h (sph_mesh_extract); 0 in a field = its default."""
    _fields_ = [("spacing", C.c_float), ("radius", C.c_float), ("iso", C.c_float)]


# name -> (restype, argtypes); also the list the symbol-export test walks
_P = C.c_void_p
_U32 = C.c_uint32
SIGNATURES = {
    "sph_abi_version": (C.c_int, []),
    "sph_last_error": (C.c_char_p, []),
    "sph_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "sph_select_device": (C.c_int, [C.c_int]),
    "sph_selected_device": (C.c_int, []),
    "sph_default_params": (None, [C.POINTER(Params), C.POINTER(C.c_float), C.POINTER(_U32)]),
    "sph_grid_dim_for_edge": (_U32, [C.c_float, C.c_float]),
    "sph_create": (C.c_int, [C.POINTER(_P), C.c_int, _U32, C.POINTER(Params)]),
    "sph_create_slab": (C.c_int, [C.POINTER(_P), C.c_int, _U32, C.POINTER(Params), _U32, _U32, _U32]),
    "sph_create_slab_layers": (C.c_int, [C.POINTER(_P), C.c_int, _U32, C.POINTER(Params), _U32, _U32, _U32, _U32]),
    "sph_ghost_layers": (_U32, [_P]),
    "sph_slab_set_protocol": (C.c_int, [_P, C.c_int]),
    "sph_slab_protocol": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_destroy": (None, [_P]),
    "sph_set_stream": (C.c_int, [_P, _P]),
    "sph_set_params": (C.c_int, [_P, C.POINTER(Params)]),
    "sph_get_params": (C.c_int, [_P, C.POINTER(Params)]),
    "sph_sync": (C.c_int, [_P]),
    "sph_num_particles": (_U32, [_P]),
    "sph_capacity": (_U32, [_P]),
    "sph_upload": (C.c_int, [_P, _U32, _P, _P, _P]),
    "sph_set_by_index": (C.c_int, [_P, _U32, _U32, C.c_void_p, C.c_void_p]),
    "sph_reset_lattice": (C.c_int, [_P, C.POINTER(_U32), C.c_int, C.POINTER(C.c_float), C.c_uint64, _U32]),
    "sph_download": (C.c_int, [_P, _U32, _U32, _P, _P, _P, _P]),
    "sph_download_owned": (C.c_int, [_P, _P, _P, _P]),
    "sph_download_forces": (C.c_int, [_P, _U32, _U32, _P, _P, _P, _P]),
    "sph_snapshot_save": (C.c_int, [_P, C.c_char_p]),
    "sph_snapshot_load": (C.c_int, [_P, C.c_char_p]),
    "sph_snapshot_info": (C.c_int, [C.c_char_p, C.POINTER(_U32), C.POINTER(Params)]),
    "sph_set_colliders": (C.c_int, [_P, _U32, C.POINTER(Collider)]),
    "sph_get_colliders": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(Collider)]),
    "sph_set_collider_bodies": (C.c_int, [_P, _U32, C.POINTER(ColliderBody)]),
    "sph_get_collider_impulses": (C.c_int, [_P, C.POINTER(_U32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "sph_emit": (C.c_int, [_P, _U32, _P, _P, _P, C.POINTER(_U32)]),
    "sph_remove": (C.c_int, [_P, _U32, C.POINTER(Region), C.POINTER(_U32), _P, _U32]),
    "sph_count_in_regions": (C.c_int, [_P, _U32, C.POINTER(Region), C.POINTER(_U32)]),
    "sph_camera_look_at": (C.c_int, [C.POINTER(Camera), _U32, _U32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float]),
    "sph_render": (C.c_int, [_P, C.POINTER(Camera), C.POINTER(RenderStyle)]),
    "sph_render_read": (C.c_int, [_P, _P, _P, _P]),
    "sph_render_image_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_U32), C.POINTER(_U32)]),
    "sph_surface_defaults": (None, [C.POINTER(SurfaceStyle)]),
    "sph_render_surface": (C.c_int, [_P, C.POINTER(Camera), C.POINTER(RenderStyle), C.POINTER(SurfaceStyle)]),
    "sph_render_surface_read": (C.c_int, [_P, _P, _P, _P]),
    "sph_solid_defaults": (None, [C.POINTER(SolidStyle)]),
    "sph_render_set_solids": (C.c_int, [_P, C.POINTER(SolidStyle)]),
    "sph_render_get_solids": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(SolidStyle)]),
    "sph_obstacle_lattice": (C.c_int, [_P, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(ObstacleGrid)]),
    "sph_obstacle_build": (C.c_int, [_P, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), _U32, C.POINTER(Shape)]),
    "sph_obstacle_set_grid": (C.c_int, [_P, C.POINTER(ObstacleGrid), _P]),
    "sph_obstacle_clear": (C.c_int, [_P]),
    "sph_obstacle_set_motion": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sph_obstacle_get": (C.c_int, [_P, C.POINTER(ObstacleGrid), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "sph_obstacle_read": (C.c_int, [_P, _P]),
    "sph_obstacle_sample": (C.c_int, [_P, _U32, _P, _P, _P, _P]),
    "sph_obstacle_set_pose": (C.c_int, [_P, C.POINTER(ObstaclePose)]),
    "sph_obstacle_get_pose": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                        C.POINTER(C.c_float)]),
    "sph_obstacle_set_sensor": (C.c_int, [_P, C.c_int]),
    "sph_obstacle_get_load": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
    "sph_obstacle_set_body": (C.c_int, [_P, C.POINTER(ObstacleBody)]),
    "sph_obstacle_get_body": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(ObstacleBody)]),
    "sph_obstacle_build_mesh": (C.c_int,[_P, C.POINTER(ObstacleMeshParams), C.POINTER(C.c_float), C.POINTER(C.c_float), _U32, _P,
                                          _U32, _P]),
    "sph_obstacle_build_mesh_dev": (C.c_int, [_P, C.POINTER(ObstacleMeshParams), C.POINTER(C.c_float), C.POINTER(C.c_float), _U32,
                                              _P, _U32, _P]),
    "sph_obstacle_build_obj": (C.c_int, [_P, C.POINTER(ObstacleMeshParams), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_char_p]),
    "sph_obstacle_mesh_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_obstacle_select": (C.c_int, [_P, _U32]),
    "sph_obstacle_selected": (_U32, [_P]),
    "sph_obstacle_installed": (_U32, [_P, C.POINTER(_U32)]),
    "sph_obstacle_clear_all": (C.c_int, [_P]),
    "sph_mesh_defaults": (None, [C.POINTER(MeshParams)]),
    "sph_mesh_lattice": (C.c_int, [_P, C.POINTER(MeshParams), C.POINTER(_U32), C.POINTER(C.c_float)]),
    "sph_mesh_extract": (C.c_int, [_P, C.POINTER(MeshParams), C.POINTER(_U32), C.POINTER(_U32)]),
    "sph_mesh_read": (C.c_int, [_P, _P, _P, _P]),
    "sph_mesh_dev": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_U32), C.POINTER(_U32)]),
    "sph_mesh_save_obj": (C.c_int, [_P, C.c_char_p]),
    "sph_mesh_field_dims": (C.c_int, [_P, C.POINTER(_U32)]),
    "sph_mesh_field_read": (C.c_int, [_P, _P]),
    "sph_positions_dev": (C.c_int, [_P, C.POINTER(_P)]),
    "sph_download_positions4": (C.c_int, [_P, _P]),
    "sph_get_keys": (C.c_int, [_P, _P]),
    "sph_get_order": (C.c_int, [_P, _P]),
    "sph_get_cell_range": (C.c_int, [_P, _U32, C.POINTER(_U32), C.POINTER(_U32)]),
    "sph_get_cells": (C.c_int, [_P, _U32, _P, _P, _P]),
    "sph_cell_key": (_U32, [_P, _U32, _U32, _U32]),
    "sph_hash": (C.c_int, [_P]),
    "sph_sort": (C.c_int, [_P]),
    "sph_build_cells": (C.c_int, [_P]),
    "sph_density": (C.c_int, [_P]),
    "sph_force": (C.c_int, [_P]),
    "sph_collide": (C.c_int, [_P]),
    "sph_integrate": (C.c_int, [_P, C.c_float]),
    "sph_step": (C.c_int, [_P, C.c_float, _U32]),
    "sph_step_phased": (C.c_int, [_P, C.c_float, _U32]),
    "sph_force_collide_integrate": (C.c_int, [_P, C.c_float]),
    "sph_timing_enable": (C.c_int, [_P, C.c_int]),
    "sph_timing_get": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(_U32)]),
    "sph_timing_reset": (C.c_int, [_P]),
    "sph_last_sort_skipped": (C.c_int, [_P]),
    "sph_sort_stats": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                 C.POINTER(C.c_uint64)]),
    "sph_set_sort_mode": (C.c_int, [_P, C.c_int]),
    "sph_set_direct_hull": (C.c_int, [_P, C.c_uint32]),
    "sph_set_pair_small_launch": (C.c_int, [_P, C.c_uint32]),
    "sph_set_block_order": (C.c_int, [_P, C.c_int, C.c_int, C.c_uint32]),
    "sph_sort_forms": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_test_trust_mover_hint": (C.c_int, [_P]),
    "sph_memory_stats": (None, [C.POINTER(C.c_uint64)]),
    "sph_test_fail_alloc": (None, [C.c_uint32]),
    "sph_test_guard": (None, [C.c_uint32, C.c_int]),
    "sph_test_guard_check": (C.c_int, [C.POINTER(C.c_uint64)]),
    "sph_test_scan": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sph_test_lower_bounds": (C.c_int, [_P, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "sph_set_precision": (C.c_int, [_P, C.c_int]),
    "sph_get_precision": (C.c_int, [_P]),
    "sph_migrants_count": (C.c_int, [_P, C.POINTER(_U32)]),
    "sph_slab_counts": (C.c_int, [_P, C.POINTER(_U32)]),
    "sph_migrants_pack": (C.c_int, [_P, C.POINTER(_P), _U32]),
    "sph_migrants_append": (C.c_int, [_P, _P, _U32]),
    "sph_halo_count": (C.c_int, [_P, C.POINTER(_U32)]),
    "sph_halo_pack": (C.c_int, [_P, C.POINTER(_P), _U32]),
    "sph_halo_pack_counts": (C.c_int, [_P, C.POINTER(_P), _U32, C.POINTER(_U32)]),
    "sph_halo_unpack": (C.c_int, [_P, _P, _U32, _P, _U32]),
    "sph_halo_pack_density": (C.c_int, [_P, C.POINTER(_P), _U32]),
    "sph_halo_unpack_density": (C.c_int, [_P, _P, _P]),
    "sph_layer_histogram": (C.c_int, [_P, _P, _U32]),
    "sph_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "sph_rccl_transport_create": (C.c_int, [C.POINTER(C.POINTER(Transport)), C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sph_rccl_transport_destroy": (None, [C.POINTER(Transport)]),
    "sph_rccl_transport_selftest": (C.c_int, [C.POINTER(Transport), C.c_size_t]),
    "sph_rccl_transport_info": (C.c_int, [C.POINTER(Transport), C.POINTER(C.c_int)]),
    "sph_slab_ping": (C.c_int, [_P, C.c_size_t, _U32, C.POINTER(C.c_double)]),
    "sph_slab_recut": (C.c_int, [_P, _U32, _U32]),
    "sph_slab_recut_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_slab_set_early_force": (C.c_int, [_P, C.c_int]),
    "sph_slab_early_force_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_slab_timing_enable": (C.c_int, [_P, C.c_int]),
    "sph_slab_timing_reset": (C.c_int, [_P]),
    "sph_slab_timing_get": (C.c_int, [_P, C.POINTER(C.c_double)]),
    "sph_slab_test_raise_flag": (C.c_int, [_P, C.c_int]),
    "sph_slab_test_set_hop_seq": (C.c_int, [_P, _U32]),
    "sph_slab_test_hop_state": (C.c_int, [_P, C.POINTER(_U32)]),
    "sph_slab_one_clamped": (C.c_uint64, [C.c_void_p]),
    "sph_slab_in_place_merges": (C.c_uint64, [C.c_void_p]),
    "sph_slab_exchanges": (C.c_uint64, [C.c_void_p]),
    "sph_slab_failed": (C.c_int, [C.c_void_p]),
    "sph_slab_create": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int, C.POINTER(Transport), _U32]),
    "sph_slab_destroy": (None, [_P]),
    "sph_slab_step": (C.c_int, [_P, C.c_float, _U32]),
    "sph_slab_sync": (C.c_int, [_P]),
    "sph_slab_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_slab_counters": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "sph_slab_set_wait_timeout": (C.c_int, [_P, C.c_double]),
    "sph_local_hub_create": (C.c_int, [C.POINTER(_P), C.c_int, C.c_int]),
    "sph_local_hub_destroy": (None, [_P]),
    "sph_local_hub_set_timeout": (C.c_int, [_P, C.c_double]),
    "sph_local_transport_create": (C.c_int, [C.POINTER(C.POINTER(Transport)), _P, C.c_int]),
    "sph_local_transport_destroy": (None, [C.POINTER(Transport)]),
    "sph_loop_transport_create": (C.c_int, [C.POINTER(C.POINTER(Transport)), C.c_float, C.c_double, C.c_double]),
    "sph_loop_transport_destroy": (None, [C.POINTER(Transport)]),
    # include/particleSystem.h: host-only twins of ic.py (used by the C++ class's reset())
    "sph_ic_dam_break": (None, [C.POINTER(_U32), C.POINTER(C.c_float), C.c_int, C.c_uint64, C.c_uint64, _P, _P]),
    "sph_ic_random_box": (None, [C.c_uint64, C.POINTER(C.c_float), C.c_float, _U32, C.c_float, _P, _P]),
}

_lib = None
_torch_first = None     # was torch already imported when libsph_hip.so (and with it /opt/rocm's HIP runtime) was loaded?


def load():
    """dlopen libsph_hip.so (building it first if it is missing) and type its entry points.

    Library order matters in a process that also uses PyTorch: the torch wheel bundles its own HIP/HSA
    runtime and loads it by path.  If libsph_hip.so (linked against /opt/rocm) comes first, torch later
    brings up a second runtime, which finds no device.  Import torch BEFORE the first call of this
    function; then libsph_hip.so binds to the runtime torch has already loaded (same SONAMEs)."""
    global _lib, _torch_first
    if _lib is None:
        import sys
        _torch_first = "torch" in sys.modules
        if not os.path.exists(LIB_PATH):
            from . import build as _b
            _b.build()
        lib = C.CDLL(LIB_PATH)
        lenient = bool(os.environ.get("SPH_HIP_LIB_ALLOW_MISSING"))     # A/B runs against a library of an EARLIER round (profiles/scripts)
        for name, (res, args) in SIGNATURES.items():
            if lenient and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)          # AttributeError = missing export: fail loudly
            fn.restype = res
            fn.argtypes = args
        if lib.sph_abi_version() != 2:
            raise SphError("libsph_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def _check(rc):
    if rc < 0:
        raise SphError(f"libsph_hip error {rc}: {load().sph_last_error().decode()}")
    return rc


def memory_stats():
    """Test hook: (live device bytes, live pinned bytes, live buffers) of this process's library."""
    out = (C.c_uint64 * 3)()
    load().sph_memory_stats(out)
    return tuple(int(v) for v in out)


def fail_alloc(k):
    """Test hook: the k-th allocation from now fails with SPH_E_NOMEM, once; 0 disarms."""
    load().sph_test_fail_alloc(int(k))


def guard(band_bytes, fill=False):
    """Test hook: bands of `band_bytes` (a multiple of 4096; 0: off) around every allocation from now on, filled with a pattern;
    fill=True puts the pattern into every range the library does not clear as well."""
    load().sph_test_guard(int(band_bytes), 1 if fill else 0)


def guard_check():
    """Test hook: (buffers checked, buffers damaged, user bytes of the first damaged one, byte offset of its first damaged word:
    < 0 in front of the user range, >= 0 from its end) over every guarded buffer, live or freed since the last check; repairs."""
    out = (C.c_uint64 * 4)()
    _check(load().sph_test_guard_check(out))
    return int(out[0]), int(out[1]), int(out[2]), C.c_int64(out[3]).value


def default_params(box, grid) -> Params:
    p = Params()
    load().sph_default_params(C.byref(p), (C.c_float * 3)(*[float(b) for b in box]),
                              (C.c_uint32 * 3)(*[int(g) for g in grid]))
    return p


def device_count():
    flag = C.c_int(0)
    n = load().sph_device_count(C.byref(flag))
    return n, bool(flag.value)


def look_at(width, height, eye=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy_deg=60.0, near_z=0.1,
            far_z=100.0) -> Camera:
    """`sph_camera_look_at` (a host helper: no GPU needed).  The defaults are the reference's view (SPH/particles.cpp:64-65,
    324): three units back on +z, looking at the origin, 60 degrees."""
    cam = Camera()
    v3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    _check(load().sph_camera_look_at(C.byref(cam), int(width), int(height), v3(eye), v3(target), v3(up), float(fovy_deg),
                                     float(near_z), float(far_z)))
    return cam


def surface_defaults(**fields) -> SurfaceStyle:
    """`sph_surface_defaults` (a host helper: no GPU needed), with any field replaced: smooth_radius_px, smooth_iterations,
    depth_falloff, flat_color, tint, absorb, light, specular."""
    s = SurfaceStyle()
    load().sph_surface_defaults(C.byref(s))
    for k, v in fields.items():
        if k in ("tint", "absorb", "light"):
            v = (C.c_float * 3)(*[float(x) for x in v])
        elif k not in ("smooth_radius_px", "smooth_iterations", "depth_falloff", "flat_color", "specular"):
            raise TypeError(f"sph_surface_style has no field {k!r}")
        setattr(s, k, v)
    return s


def solid_defaults(looks=None, **fields) -> SolidStyle:
    """`sph_solid_defaults` (a host helper: no GPU needed), with any field replaced: light, ambient; looks: {slot: dict of
    draw, open, color} for the slots that differ."""
    s = SolidStyle()
    load().sph_solid_defaults(C.byref(s))
    for k, v in fields.items():
        if k == "light":
            v = (C.c_float * 3)(*[float(x) for x in v])
        elif k != "ambient":
            raise TypeError(f"sph_solid_style has no field {k!r}")
        setattr(s, k, v)
    for q, look in (looks or {}).items():
        for k, v in look.items():
            if k == "color":
                v = (C.c_float * 3)(*[float(x) for x in v])
            elif k not in ("draw", "open"):
                raise TypeError(f"sph_solid_look has no field {k!r}")
            setattr(s.slot[int(q)], k, v)
    return s


def mesh_defaults(**fields) -> MeshParams:
    """`sph_mesh_defaults` (a host helper: no GPU needed), with any field replaced: spacing, radius, iso."""
    p = MeshParams()
    load().sph_mesh_defaults(C.byref(p))
    for k, v in fields.items():
        if k not in ("spacing", "radius", "iso"):
            raise TypeError(f"sph_mesh_params has no field {k!r}")
        setattr(p, k, float(v))
    return p


class LocalHub:
    """`sph_local_hub`: the rendezvous of the device-to-device transport between slabs of one process (one GPU)."""

    def __init__(self, world, device=0, timeout_s=None):
        h = _P()
        _check(load().sph_local_hub_create(C.byref(h), int(world), int(device)))
        self.h = h
        if timeout_s:
            _check(load().sph_local_hub_set_timeout(self.h, float(timeout_s)))

    def transport(self, rank):
        t = C.POINTER(Transport)()
        _check(load().sph_local_transport_create(C.byref(t), self.h, int(rank)))
        return t

    def close(self):
        if getattr(self, "h", None):
            load().sph_local_hub_destroy(self.h)
            self.h = None


def _f32(a, cols):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(-1, cols)


MAX_OBSTACLES = 4        # SPH_MAX_OBSTACLES


def _slotted(method):
    """An obstacle method with the optional keyword slot=k: select k, call, restore the selection."""
    @functools.wraps(method)
    def call(self, *args, slot=None, **kw):
        if slot is None:
            return method(self, *args, **kw)
        before = self.selected_obstacle()
        self.select_obstacle(slot)
        try:
            return method(self, *args, **kw)
        finally:
            self.select_obstacle(before)
    return call


class Context:
    """One `sph_ctx`: the device state of a particle system (or of one z-slab of it)."""

    def __init__(self, capacity, box=None, grid=None, params: Params | None = None, device=0,
                 slab=None, ghost_capacity=0, ghost_layers=1):
        self.L = load()
        self.params = params if params is not None else default_params(box, grid)
        h = _P()
        if slab is None:
            _check(self.L.sph_create(C.byref(h), device, int(capacity), C.byref(self.params)))
        else:       # ghost_layers = 2: what the one-message slab step needs (sph_slab_set_protocol)
            _check(self.L.sph_create_slab_layers(C.byref(h), device, int(capacity), C.byref(self.params),
                                                 int(slab[0]), int(slab[1]), int(ghost_capacity), int(ghost_layers)))
        self.h = h
        self.capacity = int(capacity)
        self.index_base = 0
        self.index_count = int(capacity)

    def close(self):
        if getattr(self, "h", None):
            self.L.sph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- state ---------------------------------------------------------------------------------
    @property
    def n(self):
        return int(self.L.sph_num_particles(self.h))

    def set_stream(self, stream_handle):
        _check(self.L.sph_set_stream(self.h, _P(stream_handle)))

    def set_params(self, params: Params):
        _check(self.L.sph_set_params(self.h, C.byref(params)))
        self.params = params

    def upload(self, pos, vel=None, index=None):
        pos = _f32(pos, 3)
        n = pos.shape[0]
        vel = _f32(vel, 3) if vel is not None else None
        idx = np.ascontiguousarray(index, dtype=np.uint32) if index is not None else None
        _check(self.L.sph_upload(self.h, n, pos.ctypes.data, vel.ctypes.data if vel is not None else None,
                                 idx.ctypes.data if idx is not None else None))

    def set_by_index(self, first_index, pos=None, vel=None):
        """Overwrite position and/or velocity of the particles with creation indices first_index .. (device side)."""
        pos = None if pos is None else np.ascontiguousarray(pos, dtype=np.float32)
        vel = None if vel is None else np.ascontiguousarray(vel, dtype=np.float32)
        count = (pos if pos is not None else vel).shape[0]
        assert vel is None or pos is None or vel.shape == pos.shape
        _check(self.L.sph_set_by_index(self.h, int(first_index), int(count),
                                       None if pos is None else pos.ctypes.data, None if vel is None else vel.ctypes.data))

    def reset_lattice(self, lattice, jitter=True, jitter_dims=None, start=0, count=None):
        """Dam-break lattice generated on the device (bit-identical to ic.dam_break_lattice)."""
        lat = (_U32 * 3)(*[int(v) for v in lattice])
        total = int(lattice[0]) * int(lattice[1]) * int(lattice[2])
        count = total - start if count is None else count
        jd = (C.c_float * 3)(*[float(v) for v in jitter_dims]) if jitter_dims is not None else None
        _check(self.L.sph_reset_lattice(self.h, lat, 1 if jitter else 0, jd, int(start), int(count)))

    def download(self, index_base=0, count=None, want=("pos", "vel", "density", "pressure")):
        """State by creation index; rows of particles this context does not own stay NaN."""
        count = self.index_count if count is None else count
        out = {}
        for k in want:
            out[k] = np.full((count, 3) if k in ("pos", "vel") else (count,), np.nan, dtype=np.float32)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _check(self.L.sph_download(self.h, int(index_base), int(count), ptr("pos"), ptr("vel"), ptr("density"),
                                   ptr("pressure")))
        return out

    def download_owned(self):
        """(pos[n,3], vel[n,3], index[n]) of the owned particles in slot order."""
        n = self.n
        pos, vel, idx = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.uint32)
        _check(self.L.sph_download_owned(self.h, pos.ctypes.data, vel.ctypes.data, idx.ctypes.data))
        return pos, vel, idx

    def download_forces(self, index_base=0, count=None, force=True, collision=True):
        count = self.index_count if count is None else count
        out = {}
        if force:
            out["fpress"] = np.full((count, 3), np.nan, dtype=np.float32)
            out["fvisc"] = np.full((count, 3), np.nan, dtype=np.float32)
        if collision:
            out["dv"] = np.full((count, 3), np.nan, dtype=np.float32)
            out["count"] = np.full((count,), -1, dtype=np.int32)
        ptr = lambda k: out[k].ctypes.data if k in out else None
        _check(self.L.sph_download_forces(self.h, int(index_base), int(count), ptr("fpress"), ptr("fvisc"), ptr("dv"),
                                          ptr("count")))
        return out

    def save(self, path):
        _check(self.L.sph_snapshot_save(self.h, os.fsencode(path)))

    def load_snapshot(self, path):
        _check(self.L.sph_snapshot_load(self.h, os.fsencode(path)))

    @staticmethod
    def snapshot_info(path):
        n, p = _U32(0), Params()
        _check(load().sph_snapshot_info(os.fsencode(path), C.byref(n), C.byref(p)))
        return int(n.value), p

    def set_colliders(self, centers, radii, velocities=None):
        """Replace the context's solid spheres (include/sph_hip.h: sph_set_colliders): centers (n, 3), radii (n,), velocities
        (n, 3) or None (at rest), in box coordinates; n = 0 clears them.  Every integrate pushes the particles out of them and
        every step advances the centres by dt * velocity."""
        centers = _f32(centers, 3)
        n = centers.shape[0]
        radii = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        velocities = np.zeros((n, 3), np.float32) if velocities is None else _f32(velocities, 3)
        if radii.shape[0] != n or velocities.shape[0] != n:
            raise ValueError("centers, radii and velocities describe different numbers of spheres")
        arr = (Collider * max(n, 1))()
        for j in range(n):
            arr[j].center[:] = [float(v) for v in centers[j]]
            arr[j].radius = float(radii[j])
            arr[j].velocity[:] = [float(v) for v in velocities[j]]
        _check(self.L.sph_set_colliders(self.h, n, arr))

    def set_collider_bodies(self, masses, accels=None):
        """One body per sphere (include/sph_hip.h: sph_set_collider_bodies): masses (n,) -- 0 kinematic, > 0 a free body the
        fluid pushes --, accels (n, 3) or None (zero).  The context is then tracked: collider_impulses() reports what every
        sphere took from the fluid, and the spheres live on the device.  An empty `masses` stops the tracking."""
        masses = np.ascontiguousarray(masses, dtype=np.float32).reshape(-1)
        n = masses.shape[0]
        accels = np.zeros((n, 3), np.float32) if accels is None else _f32(accels, 3)
        if accels.shape[0] != n:
            raise ValueError("masses and accels describe different numbers of spheres")
        arr = (ColliderBody * max(n, 1))()
        for j in range(n):
            arr[j].mass = float(masses[j])
            arr[j].accel[:] = [float(v) for v in accels[j]]
        _check(self.L.sph_set_collider_bodies(self.h, n, arr))

    def collider_impulses(self):
        """(J, steps): J float64 (n, 3), the momentum each sphere took from the fluid in the LAST integrate, and the number
        of integrates since tracking began; ((0, 3) array, 0) on a context that is not tracked.  Synchronises."""
        J = (C.c_double * (3 * MAX_COLLIDERS))()
        n, steps = _U32(), C.c_uint64()
        _check(self.L.sph_get_collider_impulses(self.h, C.byref(n), J, C.byref(steps)))
        return np.array(J[:3 * n.value], np.float64).reshape(-1, 3), int(steps.value)

    def colliders(self):
        """The current spheres, centres advanced: {"centers": (n, 3), "radii": (n,), "velocities": (n, 3)} float32 (on a
        tracked context: the device's centres and velocities; synchronises)."""
        arr = (Collider * MAX_COLLIDERS)()
        n = _U32()
        _check(self.L.sph_get_colliders(self.h, C.byref(n), arr))
        rows = [arr[j] for j in range(n.value)]
        return {"centers": np.array([list(r.center) for r in rows], np.float32).reshape(-1, 3),
                "radii": np.array([r.radius for r in rows], np.float32),
                "velocities": np.array([list(r.velocity) for r in rows], np.float32).reshape(-1, 3)}

    # -- obstacles (whole-domain contexts; include/sph_hip.h: sph_obstacle_build and the calls next to it) -------------------------
    # Every method below marked @_slotted takes an optional slot=k: it selects slot k, calls and restores the selection; without
    # it the call addresses the current selection (slot 0 unless select_obstacle chose another).
    def select_obstacle(self, slot):
        """Every obstacle call from now on addresses `slot` (0..MAX_OBSTACLES - 1)."""
        _check(self.L.sph_obstacle_select(self.h, int(slot)))

    def selected_obstacle(self) -> int:
        return int(self.L.sph_obstacle_selected(self.h))

    def installed_obstacles(self):
        """(count, mask): the slots that hold a grid; bit k of mask = slot k."""
        mask = _U32()
        n = self.L.sph_obstacle_installed(self.h, C.byref(mask))
        return int(n), int(mask.value)

    def clear_obstacles_all(self):
        """clear_obstacle on every slot, and the selection back to 0."""
        _check(self.L.sph_obstacle_clear_all(self.h))

    @staticmethod
    def _bounds(bounds):
        if bounds is None:
            return None, None
        lo, hi = bounds
        return _f3(lo), _f3(hi)

    @_slotted
    def obstacle_lattice(self, spacing=0.0, bounds=None) -> ObstacleGrid:
        """The lattice build_obstacle would use: a host helper.  bounds = (lo, hi) or None (the box)."""
        g = ObstacleGrid()
        lo, hi = self._bounds(bounds)
        _check(self.L.sph_obstacle_lattice(self.h, float(spacing), lo, hi, C.byref(g)))
        return g

    @_slotted
    def build_obstacle(self, shapes, spacing=0.0, bounds=None):
        """Rasterise the union of `shapes` (Shape.sphere / box / capsule / halfspace) on the device and install it as the
        context's obstacle: every later integrate pushes the particles out of it.  spacing 0 = the particle diameter."""
        shapes = list(shapes)
        arr = (Shape * max(len(shapes), 1))(*shapes)
        lo, hi = self._bounds(bounds)
        _check(self.L.sph_obstacle_build(self.h, float(spacing), lo, hi, len(shapes), arr))

    @_slotted
    def set_obstacle_grid(self, phi, origin, spacing):
        """Install the caller's signed distances: phi of shape (n_z, n_y, n_x) (x fastest), float32; negative inside the solid."""
        phi = np.ascontiguousarray(phi, dtype=np.float32)
        if phi.ndim != 3:
            raise ValueError("phi must have the shape (n_z, n_y, n_x)")
        g = ObstacleGrid((_U32 * 3)(phi.shape[2], phi.shape[1], phi.shape[0]), _f3(origin), float(spacing))
        _check(self.L.sph_obstacle_set_grid(self.h, C.byref(g), phi.ctypes.data))

    @_slotted
    def clear_obstacle(self):
        _check(self.L.sph_obstacle_clear(self.h))

    @_slotted
    def set_obstacle_motion(self, offset=None, velocity=None):
        """Offset and / or velocity of the grid (None = keep): the offset advances by dt * velocity once per step."""
        _check(self.L.sph_obstacle_set_motion(self.h, None if offset is None else _f3(offset),
                                              None if velocity is None else _f3(velocity)))

    @_slotted
    def obstacle(self, read=False):
        """None without an obstacle, else {"dims": (n_x, n_y, n_z), "origin", "spacing", "offset", "velocity"} with the advanced
        offset; read=True adds "phi", the installed (clamped) field of shape (n_z, n_y, n_x) (synchronises)."""
        g, off, vel = ObstacleGrid(), (C.c_float * 3)(), (C.c_float * 3)()
        _check(self.L.sph_obstacle_get(self.h, C.byref(g), off, vel))
        if not any(g.dims):
            return None
        out = {"dims": tuple(int(v) for v in g.dims), "origin": np.array(list(g.origin), np.float32),
               "spacing": np.float32(g.spacing), "offset": np.array(list(off), np.float32),
               "velocity": np.array(list(vel), np.float32)}
        if read:
            phi = np.empty(out["dims"][::-1], np.float32)
            _check(self.L.sph_obstacle_read(self.h, phi.ctypes.data))
            out["phi"] = phi
        return out

    @_slotted
    def sample_obstacle(self, points):
        """(phi (n,), normal (n, 3), inside_grid (n,) bool) of the obstacle at `points`, by the rule the particles see: phi =
        +inf and normal 0 outside the grid.  Synchronises."""
        pts = _f32(points, 3)
        n = pts.shape[0]
        phi, nrm, inside = np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty(n, np.uint8)
        _check(self.L.sph_obstacle_sample(self.h, n, pts.ctypes.data, phi.ctypes.data, nrm.ctypes.data, inside.ctypes.data))
        return phi, nrm, inside.astype(bool)

    @_slotted
    def set_obstacle_pose(self, pivot=None, quat=None, omega=(0.0, 0.0, 0.0)):
        """The rigid pose of the obstacle: `pivot` a point of the grid's own (body) frame, `quat` = (w, x, y, z) body -> world
        about it (normalised by the library), `omega` the angular velocity in world axes; the pose advances once per step.
        set_obstacle_pose(None) drops the pose: translation only."""
        if pivot is None:
            _check(self.L.sph_obstacle_set_pose(self.h, None))
            return
        p = ObstaclePose(_f3(pivot), (C.c_float * 4)(*[float(v) for v in quat]), _f3(omega))
        _check(self.L.sph_obstacle_set_pose(self.h, C.byref(p)))

    @_slotted
    def obstacle_pose(self):
        """None without a pose, else {"pivot" (3,) float32, "quat" (4,) float64 (unit, advanced), "omega" (3,) float32,
        "rot" (3, 3) float32 body -> world as the next launch takes it}."""
        posed, piv, q, om, rot = C.c_int(), (C.c_float * 3)(), (C.c_double * 4)(), (C.c_float * 3)(), (C.c_float * 9)()
        _check(self.L.sph_obstacle_get_pose(self.h, C.byref(posed), piv, q, om, rot))
        if not posed.value:
            return None
        return {"pivot": np.array(list(piv), np.float32), "quat": np.array(list(q), np.float64),
                "omega": np.array(list(om), np.float32), "rot": np.array(list(rot), np.float32).reshape(3, 3)}

    @_slotted
    def set_obstacle_sensor(self, on=True):
        """Switch the load sensor: while on, every integrate also sums what the obstacle took from the fluid (obstacle_load)."""
        _check(self.L.sph_obstacle_set_sensor(self.h, int(bool(on))))

    @_slotted
    def obstacle_load(self):
        """{"J" (3,), "L" (3,) float64, "about" (3,) float32, "steps"}: the momentum and the angular momentum about `about` the
        obstacle took in the LAST integrate (divide by dt for force and torque).  Synchronises."""
        J, L, about, steps = (C.c_double * 3)(), (C.c_double * 3)(), (C.c_float * 3)(), C.c_uint64()
        _check(self.L.sph_obstacle_get_load(self.h, J, L, about, C.byref(steps)))
        return {"J": np.array(list(J), np.float64), "L": np.array(list(L), np.float64),
                "about": np.array(list(about), np.float32), "steps": int(steps.value)}

    @_slotted
    def set_obstacle_body(self, body: "ObstacleBody | None" = None, **fields):
        """Give the slot a body (include/sph_hip.h: THE BODY): from then on the fluid drives the motions in `dof`, on the device,
        inside step(dt, n).  `body` is an ObstacleBody, or its fields as keywords (ObstacleBody.make); set_obstacle_body(None)
        with no keyword drops the body (synchronises) and the slot goes on kinematic from where it is.  The slot needs a pose."""
        if body is None and not fields:
            _check(self.L.sph_obstacle_set_body(self.h, None))
            return
        b = body if body is not None else ObstacleBody.make(**fields)
        _check(self.L.sph_obstacle_set_body(self.h, C.byref(b)))

    @_slotted
    def obstacle_body(self):
        """None without a body, else the parameters as they were set: {"dof", "mass", "inertia", "axis", "accel", "torque",
        "lo", "hi"}.  The state is what obstacle() and obstacle_pose() return."""
        has, b = C.c_int(), ObstacleBody()
        _check(self.L.sph_obstacle_get_body(self.h, C.byref(has), C.byref(b)))
        return b.as_dict() if has.value else None

    # -- obstacles from a triangle mesh (include/sph_hip.h: sph_obstacle_build_mesh and the calls next to it) -----------------------
    @_slotted
    def build_obstacle_mesh(self, vertices, triangles, spacing=0.0, band=0, invert=False, bounds=None):
        """Voxelise the closed triangle mesh (vertices (nv, 3) float32, triangles (nt, 3) uint32) on the device into a truncated
        signed distance, `band` nodes wide (0 = 3), and install it as the context's obstacle.  Synchronises."""
        v, t = _f32(vertices, 3), np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        p = ObstacleMeshParams(float(spacing), int(band), int(bool(invert)))
        lo, hi = self._bounds(bounds)
        _check(self.L.sph_obstacle_build_mesh(self.h, C.byref(p), lo, hi, v.shape[0], v.ctypes.data, t.shape[0], t.ctypes.data))

    @_slotted
    def build_obstacle_from_mesh(self, spacing=0.0, band=0, invert=False, bounds=None):
        """The same from the context's own last extract_mesh, through its device pointers: no host trip, no host wait."""
        pos, _, tri, nv, nt = self.mesh_dev()
        p = ObstacleMeshParams(float(spacing), int(band), int(bool(invert)))
        lo, hi = self._bounds(bounds)
        _check(self.L.sph_obstacle_build_mesh_dev(self.h, C.byref(p), lo, hi, nv, pos, nt, tri))

    @_slotted
    def build_obstacle_obj(self, path, spacing=0.0, band=0, invert=False, bounds=None):
        """The same from a Wavefront OBJ file (`v` and `f` lines; polygons are fanned).  Synchronises."""
        p = ObstacleMeshParams(float(spacing), int(band), int(bool(invert)))
        lo, hi = self._bounds(bounds)
        _check(self.L.sph_obstacle_build_obj(self.h, C.byref(p), lo, hi, os.fsencode(path)))

    @_slotted
    def obstacle_mesh_stats(self):
        """(triangles used, triangles skipped, lost crossings, odd columns) of the mesh-built obstacle: a closed mesh has no odd
        column and no lost crossing.  Synchronises."""
        out = (C.c_uint64 * 4)()
        _check(self.L.sph_obstacle_mesh_stats(self.h, out))
        return tuple(int(v) for v in out)

    # -- emitters and drains (whole-domain contexts; include/sph_hip.h: sph_emit, sph_remove, sph_count_in_regions) ------------
    @staticmethod
    def _regions(regions):
        regions = [regions] if isinstance(regions, Region) else list(regions)
        arr = (Region * max(len(regions), 1))()
        for j, r in enumerate(regions):
            arr[j] = r
        return len(regions), arr

    def emit(self, pos, vel=None, index=None):
        """Append particles behind the owned ones; returns the creation index of the first (index=None: consecutive
        indices from the context's next unused one).  The next sort is the full stable sort."""
        pos = _f32(pos, 3)
        n = pos.shape[0]
        vel = _f32(vel, 3) if vel is not None else None
        idx = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1) if index is not None else None
        if (vel is not None and vel.shape[0] != n) or (idx is not None and idx.shape[0] != n):
            raise ValueError("pos, vel and index describe different numbers of particles")
        first = _U32(0)
        _check(self.L.sph_emit(self.h, n, pos.ctypes.data, vel.ctypes.data if vel is not None else None,
                               idx.ctypes.data if idx is not None else None, C.byref(first)))
        return int(first.value)

    def remove(self, regions, max_out=None):
        """Delete the owned particles inside any of the regions (a Region or up to 8 of them); the survivors keep their slot
        order.  Returns the creation indices of the removed particles in slot order (the first max_out of them)."""
        m, arr = self._regions(regions)
        max_out = self.n if max_out is None else int(max_out)
        out = np.empty(max(max_out, 1), dtype=np.uint32)
        cnt = _U32(0)
        _check(self.L.sph_remove(self.h, m, arr, C.byref(cnt), out.ctypes.data, max_out))
        self.last_removed = int(cnt.value)
        return out[:min(self.last_removed, max_out)].copy()

    def count_in(self, regions):
        """Number of owned particles inside any of the regions (nothing changes)."""
        m, arr = self._regions(regions)
        cnt = _U32(0)
        _check(self.L.sph_count_in_regions(self.h, m, arr, C.byref(cnt)))
        return int(cnt.value)

    # -- pictures (whole-domain contexts; include/sph_hip.h: sph_render, sph_render_read, sph_render_image_dev) ----------------
    def render(self, camera: Camera, color="index", lo=0.0, hi=1.0, radius=0.0, background=(0, 0, 0, 255), index_count=0):
        """Queue one render of the owned particles as sphere sprites (asynchronous).  color: "index" (the reference's
        colouring), "speed" or "density", the last two mapped from [lo, hi] onto the ramp; radius 0: the particle radius."""
        st = self._render_style(color, lo, hi, radius, background, index_count)
        _check(self.L.sph_render(self.h, C.byref(camera), C.byref(st)))

    @staticmethod
    def _render_style(color="index", lo=0.0, hi=1.0, radius=0.0, background=(0, 0, 0, 255), index_count=0):
        if color not in COLOR_MODES:
            raise ValueError(f"color {color!r}: one of {sorted(COLOR_MODES)}")
        return RenderStyle(COLOR_MODES[color], float(lo), float(hi), float(radius), int(index_count),
                           (C.c_uint8 * 4)(*[int(v) for v in background]))

    def render_surface(self, camera: Camera, surface: "SurfaceStyle | None" = None, **style):
        """Queue one render of the owned particles as a surface (asynchronous): sphere depth, thickness, smoothed depth,
        normals, a water-like shading.  surface: a SurfaceStyle (None: surface_defaults()); style: the keywords of render().
        read_image() then gives the RGBA image, the front particle's id and the SMOOTHED depth; read_surface() the rest."""
        sf = surface_defaults() if surface is None else surface
        st = self._render_style(**style)
        _check(self.L.sph_render_surface(self.h, C.byref(camera), C.byref(st), C.byref(sf)))

    def set_render_solids(self, style: "SolidStyle | None"):
        """While a style is set, render() and render_surface() also draw every installed obstacle slot whose look has draw != 0
        (`sph_render_set_solids`); None switches the solids off, the default.  Launches and allocates nothing."""
        _check(self.L.sph_render_set_solids(self.h, None if style is None else C.byref(style)))

    def render_solids(self):
        """The SolidStyle that is set, as it was given; None while the solids are off."""
        on, s = C.c_int(0), SolidStyle()
        _check(self.L.sph_render_get_solids(self.h, C.byref(on), C.byref(s)))
        return s if on.value else None

    def read_surface(self):
        """(raw_depth[h, w] float32, thickness_q[h, w] uint32, normals[h, w, 3] float32) of the last surface render;
        synchronises."""
        _, w, h = self.image_dev()
        raw, thick, normal = np.empty((h, w), np.float32), np.empty((h, w), np.uint32), np.empty((h, w, 3), np.float32)
        _check(self.L.sph_render_surface_read(self.h, raw.ctypes.data, thick.ctypes.data, normal.ctypes.data))
        return raw, thick, normal

    def read_image(self):
        """(rgba[h, w, 4] uint8, id[h, w] uint32, depth[h, w] float32) of the last render; synchronises."""
        _, w, h = self.image_dev()
        rgba, ident, depth = np.empty((h, w, 4), np.uint8), np.empty((h, w), np.uint32), np.empty((h, w), np.float32)
        _check(self.L.sph_render_read(self.h, rgba.ctypes.data, ident.ctypes.data, depth.ctypes.data))
        return rgba, ident, depth

    def image_dev(self):
        """(device pointer of the RGBA8 image of the last render, width, height)."""
        p, w, h = _P(), _U32(), _U32()
        _check(self.L.sph_render_image_dev(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, int(w.value), int(h.value)

    # -- geometry (whole-domain contexts; include/sph_hip.h: sph_mesh_extract and the calls next to it) --------------------------
    def mesh_lattice(self, params: "MeshParams | None" = None):
        """((n_x, n_y, n_z), origin float32[3]) of the lattice extract_mesh would use (a host helper)."""
        dims, origin = (_U32 * 3)(), (C.c_float * 3)()
        _check(self.L.sph_mesh_lattice(self.h, None if params is None else C.byref(params), dims, origin))
        return tuple(int(v) for v in dims), np.array(list(origin), np.float32)

    def extract_mesh(self, params: "MeshParams | None" = None):
        """Extract the surface of the owned particles as a triangle mesh on the device (params None: mesh_defaults());
        returns (vertices, triangles).  Waits once for the two counts."""
        nv, nt = _U32(0), _U32(0)
        _check(self.L.sph_mesh_extract(self.h, None if params is None else C.byref(params), C.byref(nv), C.byref(nt)))
        return int(nv.value), int(nt.value)

    def mesh_dev(self):
        """(positions, normals, triangles: device pointers or None; vertices; triangles) of the last mesh."""
        a, b, t, nv, nt = _P(), _P(), _P(), _U32(), _U32()
        _check(self.L.sph_mesh_dev(self.h, C.byref(a), C.byref(b), C.byref(t), C.byref(nv), C.byref(nt)))
        return a.value, b.value, t.value, int(nv.value), int(nt.value)

    def read_mesh(self):
        """(pos[nv, 3] float32, normal[nv, 3] float32, tri[nt, 3] uint32) of the last mesh; synchronises."""
        *_, nv, nt = self.mesh_dev()
        pos, nrm, tri = np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32), np.empty((nt, 3), np.uint32)
        _check(self.L.sph_mesh_read(self.h, pos.ctypes.data, nrm.ctypes.data, tri.ctypes.data))
        return pos, nrm, tri

    def mesh_field(self):
        """The counts of the lattice of the last extract_mesh, uint32[n_z, n_y, n_x]; synchronises."""
        dims = (_U32 * 3)()
        _check(self.L.sph_mesh_field_dims(self.h, dims))
        out = np.empty((dims[2], dims[1], dims[0]), np.uint32)
        _check(self.L.sph_mesh_field_read(self.h, out.ctypes.data))
        return out

    def save_obj(self, path):
        """The last mesh as a Wavefront OBJ file (v, vn, f a//a b//b c//c)."""
        _check(self.L.sph_mesh_save_obj(self.h, os.fsencode(path)))

    def positions4(self):
        out = np.empty((self.capacity, 4), dtype=np.float32)
        _check(self.L.sph_download_positions4(self.h, out.ctypes.data))
        return out

    def positions_dev(self):
        p = _P()
        _check(self.L.sph_positions_dev(self.h, C.byref(p)))
        return p.value

    def keys(self):
        out = np.empty(self.n, dtype=np.uint32)
        _check(self.L.sph_get_keys(self.h, out.ctypes.data))
        return out

    def order(self):
        out = np.empty(self.n, dtype=np.uint32)
        _check(self.L.sph_get_order(self.h, out.ctypes.data))
        return out

    def cells(self, max_cells=None):
        max_cells = self.n + 16 if max_cells is None else max_cells
        k = np.empty(max_cells, dtype=np.uint32)
        s = np.empty(max_cells, dtype=np.uint32)
        c = np.empty(max_cells, dtype=np.uint32)
        m = _check(self.L.sph_get_cells(self.h, max_cells, k.ctypes.data, s.ctypes.data, c.ctypes.data))
        m = min(m, max_cells)
        return k[:m], s[:m], c[:m]

    def cell_range(self, cell):
        """(start, end) of one cell of the table, relative to the first installed slot; (0, 0) = empty."""
        a, b = _U32(), _U32()
        _check(self.L.sph_get_cell_range(self.h, int(cell), C.byref(a), C.byref(b)))
        return a.value, b.value

    def cell_key(self, x, y, z):
        return int(self.L.sph_cell_key(self.h, int(x), int(y), int(z)))

    # -- phases ---------------------------------------------------------------------------------
    def hash(self): _check(self.L.sph_hash(self.h))
    def sort(self): _check(self.L.sph_sort(self.h))
    def build_cells(self): _check(self.L.sph_build_cells(self.h))
    def density(self): _check(self.L.sph_density(self.h))
    def force(self): _check(self.L.sph_force(self.h))
    def collide(self): _check(self.L.sph_collide(self.h))
    def integrate(self, dt): _check(self.L.sph_integrate(self.h, float(dt)))
    def step(self, dt, n=1): _check(self.L.sph_step(self.h, float(dt), int(n)))
    def step_phased(self, dt, n=1): _check(self.L.sph_step_phased(self.h, float(dt), int(n)))
    def sync(self): _check(self.L.sph_sync(self.h))

    # -- timing ---------------------------------------------------------------------------------
    def timing(self, on=True): _check(self.L.sph_timing_enable(self.h, 1 if on else 0))
    def timing_reset(self): _check(self.L.sph_timing_reset(self.h))

    def sort_skipped(self):
        """True if the last sort found no particle in a new cell and did nothing (no synchronisation)."""
        return bool(self.L.sph_last_sort_skipped(self.h))

    def sort_stats(self):
        """{'sorts', 'merges', 'skips', 'last_movers', 'movers_total'}: how often the sort took the merge path and
        how many particles changed cell (see sph_hip.h)."""
        a, b, k, m, t = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        _check(self.L.sph_sort_stats(self.h, C.byref(a), C.byref(b), C.byref(k), C.byref(m), C.byref(t)))
        return {"sorts": a.value, "merges": b.value, "skips": k.value, "last_movers": m.value, "movers_total": t.value}

    def set_precision(self, mixed_f16=False):
        """False: fp32 (the reference's precision); True: BASELINE config 5 -- fp32 state, packed-fp16 pair arithmetic
        and per-row accumulators in the density / force traversals."""
        _check(self.L.sph_set_precision(self.h, 1 if mixed_f16 else 0))

    def set_sort_mode(self, merge=True):
        """merge=False/0: full radix sort every step (the SPH_SORT_MERGE=0 behaviour); True/1: merge while few
        particles change cell; 2: merge whatever the count (tests)."""
        _check(self.L.sph_set_sort_mode(self.h, int(merge)))

    def trust_mover_hint(self):
        """Test hook: after set_by_index / upload the next movers' sorts launch both forms; this takes that back."""
        _check(self.L.sph_test_trust_mover_hint(self.h))

    def test_scan(self, values):
        """Test hook: (exclusive prefix sums, total) of a uint32 or uint64 array by the library's one-block scan."""
        v = np.ascontiguousarray(values)
        assert v.ndim == 1 and v.dtype in (np.uint32, np.uint64), v.dtype
        out, total = np.empty_like(v), np.zeros(1, v.dtype)
        _check(self.L.sph_test_scan(self.h, 8 * v.dtype.itemsize, v.size, v.ctypes.data, out.ctypes.data, total.ctypes.data))
        return out, total[0]

    def test_lower_bounds(self, keys, targets):
        """Test hook: for each of up to 32 uint32 targets, the first index of the sorted uint32 `keys` whose key is >= it (len(keys)
        if there is none), by the library's lower-bounds kernel."""
        k, t = np.ascontiguousarray(keys), np.ascontiguousarray(targets)
        assert k.ndim == 1 and t.ndim == 1 and k.dtype == np.uint32 and t.dtype == np.uint32, (k.dtype, t.dtype)
        out = np.empty(t.size, np.uint32)
        _check(self.L.sph_test_lower_bounds(self.h, k.ctypes.data, k.size, t.ctypes.data, t.size, out.ctypes.data))
        return out

    def sort_forms(self):
        """Movers' sorts launched as (both forms, one-block sort alone, multi-block passes alone)."""
        out = (C.c_uint64 * 3)()
        _check(self.L.sph_sort_forms(self.h, out))
        return tuple(int(v) for v in out)

    def set_block_order(self, xcd=True, ztile=True, strip_blocks_log2=4):
        """Order in which the pair kernels' workgroups take the slots (performance only; see sph_set_block_order)."""
        _check(self.L.sph_set_block_order(self.h, int(bool(xcd)), int(bool(ztile)), int(strip_blocks_log2)))

    def set_direct_hull(self, slots=512):
        """Rows of the neighbour passes whose staged hull would exceed `slots` are read straight from global memory
        (0: all of them, 0xFFFFFFFF: none); same bits either way."""
        _check(self.L.sph_set_direct_hull(self.h, int(slots) & 0xFFFFFFFF))

    def set_pair_small_launch(self, slots):
        """A context with fewer than `slots` owned particles launches the neighbour passes in 128-thread workgroups (0: never,
        0xFFFFFFFF: always; default 524288); same bits either way."""
        _check(self.L.sph_set_pair_small_launch(self.h, int(slots) & 0xFFFFFFFF))

    def timing_get(self):
        ms = (C.c_float * len(PHASES))()
        steps = _U32(0)
        _check(self.L.sph_timing_get(self.h, ms, C.byref(steps)))
        return {PHASES[k]: float(ms[k]) for k in range(len(PHASES))}, int(steps.value)

    # -- slab halo (device pointers: ints, e.g. torch.Tensor.data_ptr()) ----------------------------
    def _pair(self, fn, *a):
        cnt = (_U32 * 2)()
        _check(fn(self.h, cnt, *a))
        return int(cnt[0]), int(cnt[1])

    def slab_counts(self):
        cnt = (_U32 * 4)()
        _check(self.L.sph_slab_counts(self.h, cnt))
        return tuple(int(v) for v in cnt)

    def force_collide_integrate(self, dt): _check(self.L.sph_force_collide_integrate(self.h, float(dt)))

    def migrants_count(self): return self._pair(self.L.sph_migrants_count)
    def halo_count(self): return self._pair(self.L.sph_halo_count)

    def migrants_pack(self, buf_lo, buf_hi, capacity):
        _check(self.L.sph_migrants_pack(self.h, (_P * 2)(buf_lo, buf_hi), int(capacity)))

    def migrants_append(self, buf, n):
        _check(self.L.sph_migrants_append(self.h, _P(buf), int(n)))

    def halo_pack(self, buf_lo, buf_hi, capacity, counts=None):
        if counts is None:
            _check(self.L.sph_halo_pack(self.h, (_P * 2)(buf_lo, buf_hi), int(capacity)))
        else:
            _check(self.L.sph_halo_pack_counts(self.h, (_P * 2)(buf_lo, buf_hi), int(capacity),
                                               (_U32 * 2)(int(counts[0]), int(counts[1]))))

    def halo_unpack(self, lo, n_lo, hi, n_hi):
        _check(self.L.sph_halo_unpack(self.h, _P(lo), int(n_lo), _P(hi), int(n_hi)))

    def halo_pack_density(self, buf_lo, buf_hi, capacity):
        _check(self.L.sph_halo_pack_density(self.h, (_P * 2)(buf_lo, buf_hi), int(capacity)))

    def halo_unpack_density(self, lo, hi):
        _check(self.L.sph_halo_unpack_density(self.h, _P(lo), _P(hi)))

    def layer_histogram(self):
        n = int(self.params.grid[2])
        out = np.zeros(n, dtype=np.uint32)
        _check(self.L.sph_layer_histogram(self.h, out.ctypes.data, n))
        return out

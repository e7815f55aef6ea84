"""Python host side of the C-ABI in include/solver2d_amd.h (ctypes over solver2d_amd/libs2amd.so).

The mirror of the reference's plug point: `Solver.solve(params, bodies, contacts, joints)` is
`s2Solve_<Variant>(world, context)` (reference src/solvers.h:70-79) on wire arrays.  There is no
CPU path here: if the HIP library is missing or no GPU is visible the constructor raises.
"""
import ctypes
import os

import numpy as np

from . import wire

_HERE = os.path.dirname(os.path.abspath(__file__))
# S2AMD_LIB: another build of the same C-ABI (experiments: `make -C solver2d_amd/csrc variant NAME=...`)
LIB_PATH = os.environ.get("S2AMD_LIB") or os.path.join(_HERE, "libs2amd.so")
# The tolerance-mode build: the same sources with -ffp-contract=fast (FMA contraction).  Not bit-equal to the reference;
# within the tolerances tests/test_gpu_fast.py states and checks.  A library of its own so that one process can hold both.
FAST_LIB_PATH = os.environ.get("S2AMD_FAST_LIB") or os.path.join(_HERE, "libs2amd_fast.so")

EXPORTS = [
    "s2amd_api_version", "s2amd_build_flags", "s2amd_device_count", "s2amd_device_bus_id", "s2amd_last_error", "s2amd_create", "s2amd_destroy",
    "s2amd_solve", "s2amd_upload", "s2amd_step_resident", "s2amd_download", "s2amd_save_bodies",
    "s2amd_restore_bodies", "s2amd_get_contact_order", "s2amd_get_joint_order", "s2amd_get_writable_bodies", "s2amd_get_stats",
    "s2amd_set_option", "s2amd_export_poses", "s2amd_export_poses_async", "s2amd_export_bodies_async", "s2amd_export_wait", "s2amd_measure_dominant", "s2amd_refit_shapes", "s2amd_find_pairs", "s2amd_synchronize", "s2amd_update_contacts", "s2amd_find_islands", "s2amd_color_constraints",
    "s2amd_world_upload", "s2amd_world_step", "s2amd_world_download", "s2amd_world_find_pairs", "s2amd_world_set_contacts",
    "s2amd_device_alloc", "s2amd_device_free", "s2amd_device_read", "s2amd_world_separated", "s2amd_world_download_boxes", "s2amd_world_set_refit_order", "s2amd_world_download_step", "s2amd_world_set_tree", "s2amd_world_get_tree",
    "s2amd_world_set_report", "s2amd_world_touch_events", "s2amd_world_touching", "s2amd_world_body_sums",
    "s2amd_world_set_joint_report", "s2amd_world_joint_states", "s2amd_world_joint_limit_events", "s2amd_world_body_joint_sums", "s2amd_world_joint_summary",
    "s2amd_world_set_shape_report", "s2amd_world_set_shape_view", "s2amd_world_shape_draws", "s2amd_world_shape_view_events", "s2amd_world_shape_summary",
    "s2amd_world_set_body_report", "s2amd_world_set_rest_thresholds", "s2amd_world_body_states", "s2amd_world_body_rest_events", "s2amd_world_islands",
    "s2amd_world_body_summary",
    "s2amd_world_set_metrics", "s2amd_world_metrics", "s2amd_world_metrics_history",
    "s2amd_world_ray_cast", "s2amd_world_point_probe", "s2amd_world_query_boxes",
    "s2amd_world_closest_shape", "s2amd_world_shapes_in_range",
    "s2amd_world_collide_shape", "s2amd_world_deepest_contact",
    "s2amd_world_cast_shape", "s2amd_world_cast_shape_all", "s2amd_world_move_shapes",
    "s2amd_world_edit", "s2amd_world_apply_fields", "s2amd_world_set_fields", "s2amd_world_field_states",
    "s2amd_world_set_actuators", "s2amd_world_set_actions", "s2amd_world_import_actions", "s2amd_world_actuator_states", "s2amd_world_actuator_counts",
    "s2amd_device_write",
    "s2amd_world_set_observers", "s2amd_world_set_observation_report", "s2amd_world_observations", "s2amd_world_export_observations",
    "s2amd_world_export_observations_async", "s2amd_world_observer_states", "s2amd_world_observer_counts",
    "s2amd_world_set_episodes", "s2amd_world_set_episode_report", "s2amd_world_episode_rewards", "s2amd_world_episode_flags",
    "s2amd_world_export_episode_step", "s2amd_world_export_episode_step_async", "s2amd_world_episode_states", "s2amd_world_episode_rule_states",
    "s2amd_world_episode_events", "s2amd_world_episode_counts",
    "s2amd_world_set_resets", "s2amd_world_set_reset_report", "s2amd_world_reset_agents", "s2amd_world_reset_states", "s2amd_world_reset_counts",
    "s2amd_world_set_sensors", "s2amd_world_set_sensor_report", "s2amd_world_sensor_inside", "s2amd_world_sensor_events", "s2amd_world_sensor_states",
    "s2amd_world_set_ray_sensors", "s2amd_world_set_ray_report", "s2amd_world_ray_states", "s2amd_world_ray_ranges", "s2amd_world_export_ray_ranges",
    "s2amd_world_ray_events",
    "s2amd_world_set_grid_sensors", "s2amd_world_set_grid_report", "s2amd_world_grid_categories", "s2amd_world_grid_shapes", "s2amd_world_grid_occupancy",
    "s2amd_world_export_grid_occupancy", "s2amd_world_grid_states",
    "s2amd_get_strip_owners", "s2amd_get_resident_kernel", "s2amd_variant_family_count", "s2amd_get_variant_family", "s2amd_get_variant_entry",
    "s2amd_sharded_create", "s2amd_sharded_destroy", "s2amd_sharded_shard_count", "s2amd_sharded_solver", "s2amd_sharded_upload", "s2amd_sharded_step",
    "s2amd_sharded_download", "s2amd_sharded_read_bodies", "s2amd_sharded_reshard", "s2amd_sharded_get_partition",
    "s2amd_sharded_step_async", "s2amd_sharded_wait", "s2amd_sharded_get_step_ops", "s2amd_sharded_count_ops",
]

_libs = {}


class S2AmdError(RuntimeError):
    pass


def load(fast=False):
    """Load libs2amd.so (fast=True: libs2amd_fast.so).  Raises if it has not been built (python __graft_entry__.py /
    make -C solver2d_amd/csrc)."""
    path = FAST_LIB_PATH if fast else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise S2AmdError("HIP extension %s is missing: build it with `make -C solver2d_amd/csrc` "
                         "(there is no CPU fallback)" % path)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.s2amd_api_version.restype = ctypes.c_int
    L.s2amd_device_count.restype = ctypes.c_int
    L.s2amd_last_error.restype = ctypes.c_char_p
    L.s2amd_build_flags.restype = ctypes.c_char_p
    L.s2amd_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.s2amd_destroy.argtypes = [vp]
    L.s2amd_destroy.restype = None
    L.s2amd_solve.argtypes = [vp, ctypes.POINTER(wire.StepParams), vp, i32, vp, i32, vp, i32]
    L.s2amd_upload.argtypes = [vp, vp, i32, vp, i32, vp, i32]
    L.s2amd_step_resident.argtypes = [vp, ctypes.POINTER(wire.StepParams)]
    L.s2amd_download.argtypes = [vp, vp, i32, vp, i32, vp, i32]
    L.s2amd_save_bodies.argtypes = [vp]
    L.s2amd_restore_bodies.argtypes = [vp]
    L.s2amd_synchronize.argtypes = [vp]
    L.s2amd_get_contact_order.argtypes = [vp, vp, i32, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_get_joint_order.argtypes = [vp, vp, i32, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_get_writable_bodies.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_get_strip_owners.argtypes = [vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_get_resident_kernel.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_variant_family_count.restype = ctypes.c_int
    L.s2amd_get_variant_family.argtypes = [i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_get_variant_entry.argtypes = [i32, i32, ctypes.POINTER(i32), i32, ctypes.POINTER(ctypes.c_uint64)]
    L.s2amd_get_stats.argtypes = [vp, ctypes.POINTER(wire.StepStats)]
    L.s2amd_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    L.s2amd_export_poses.argtypes = [vp, vp, i32]
    L.s2amd_export_poses_async.argtypes = [vp, vp, i32, i32]
    L.s2amd_export_bodies_async.argtypes = [vp, vp, i32, i32]
    L.s2amd_export_wait.argtypes = [vp, i32]
    L.s2amd_measure_dominant.argtypes = [vp, ctypes.POINTER(wire.StepParams), i32, ctypes.POINTER(ctypes.c_float),
                                         ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_refit_shapes.argtypes = [vp, vp, i32, vp, i32, vp]
    L.s2amd_find_pairs.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_update_contacts.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp]
    L.s2amd_world_upload.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp]
    L.s2amd_world_step.argtypes = [vp, ctypes.POINTER(wire.StepParams), ctypes.POINTER(wire.WorldStepInfo)]
    L.s2amd_world_find_pairs.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_set_contacts.argtypes = [vp, vp, i32, vp, vp]
    L.s2amd_world_separated.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_download_boxes.argtypes = [vp, vp, i32]
    L.s2amd_world_set_refit_order.argtypes = [vp, vp, i32]
    L.s2amd_world_set_tree.argtypes = [vp, i32, vp, i32, i32]
    L.s2amd_world_get_tree.argtypes = [vp, i32, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_download.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp]
    L.s2amd_world_set_report.argtypes = [vp, i32]
    L.s2amd_world_touch_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_touching.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_body_sums.argtypes = [vp, vp, i32]
    L.s2amd_world_set_joint_report.argtypes = [vp, i32]
    L.s2amd_world_joint_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_joint_limit_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_body_joint_sums.argtypes = [vp, vp, i32]
    L.s2amd_world_joint_summary.argtypes = [vp, vp]
    L.s2amd_world_set_shape_report.argtypes = [vp, i32]
    L.s2amd_world_set_shape_view.argtypes = [vp, vp]
    L.s2amd_world_shape_draws.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_shape_view_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_shape_summary.argtypes = [vp, vp]
    L.s2amd_world_set_body_report.argtypes = [vp, i32]
    L.s2amd_world_set_rest_thresholds.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.s2amd_world_body_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_body_rest_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_islands.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_body_summary.argtypes = [vp, vp]
    L.s2amd_world_set_metrics.argtypes = [vp, i32, i32]
    L.s2amd_world_metrics.argtypes = [vp, vp]
    L.s2amd_world_metrics_history.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_ray_cast.argtypes = [vp, vp, i32, vp]
    L.s2amd_world_point_probe.argtypes = [vp, vp, i32, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_query_boxes.argtypes = [vp, vp, i32, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_closest_shape.argtypes = [vp, vp, i32, vp]
    L.s2amd_world_shapes_in_range.argtypes = [vp, vp, i32, vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_collide_shape.argtypes = [vp, vp, i32, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_deepest_contact.argtypes = [vp, vp, i32, vp]
    L.s2amd_world_cast_shape.argtypes = [vp, vp, i32, vp]
    L.s2amd_world_cast_shape_all.argtypes = [vp, vp, i32, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_move_shapes.argtypes = [vp, vp, i32, vp, vp]
    L.s2amd_world_edit.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_apply_fields.argtypes = [vp, vp, i32, vp]
    L.s2amd_world_set_fields.argtypes = [vp, vp, i32]
    L.s2amd_world_field_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_set_actuators.argtypes = [vp, vp, i32, i32]
    L.s2amd_world_set_actions.argtypes = [vp, vp, i32, i32]
    L.s2amd_world_import_actions.argtypes = [vp, vp, i32, i32]
    L.s2amd_world_actuator_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_actuator_counts.argtypes = [vp, vp]
    L.s2amd_device_write.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.s2amd_world_set_observers.argtypes = [vp, vp, i32, i32, i32]
    L.s2amd_world_set_observation_report.argtypes = [vp, i32]
    L.s2amd_world_observations.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_export_observations.argtypes = [vp, vp, i32]
    L.s2amd_world_export_observations_async.argtypes = [vp, vp, i32, i32]
    L.s2amd_world_observer_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_observer_counts.argtypes = [vp, vp]
    L.s2amd_world_set_episodes.argtypes = [vp, vp, i32, i32, vp]
    L.s2amd_world_set_episode_report.argtypes = [vp, i32]
    L.s2amd_world_episode_rewards.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_episode_flags.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_export_episode_step.argtypes = [vp, vp, vp, i32]
    L.s2amd_world_export_episode_step_async.argtypes = [vp, vp, vp, i32, i32]
    L.s2amd_world_episode_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_episode_rule_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_episode_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_episode_counts.argtypes = [vp, vp]
    L.s2amd_world_set_resets.argtypes = [vp, vp, i32, vp, i32, i32, ctypes.c_uint32]
    L.s2amd_world_set_reset_report.argtypes = [vp, i32]
    L.s2amd_world_reset_agents.argtypes = [vp, vp, i32]
    L.s2amd_world_reset_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_reset_counts.argtypes = [vp, vp]
    L.s2amd_world_set_sensors.argtypes = [vp, vp, i32]
    L.s2amd_world_set_sensor_report.argtypes = [vp, i32, i32]
    L.s2amd_world_sensor_inside.argtypes = [vp, vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_sensor_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_sensor_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_set_ray_sensors.argtypes = [vp, vp, i32]
    L.s2amd_world_set_ray_report.argtypes = [vp, i32]
    L.s2amd_world_ray_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_ray_ranges.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_export_ray_ranges.argtypes = [vp, vp, i32]
    L.s2amd_world_ray_events.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_set_grid_sensors.argtypes = [vp, vp, i32]
    L.s2amd_world_set_grid_report.argtypes = [vp, i32]
    L.s2amd_world_grid_categories.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_grid_shapes.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_grid_occupancy.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_world_export_grid_occupancy.argtypes = [vp, vp, i32]
    L.s2amd_world_grid_states.argtypes = [vp, vp, i32, ctypes.POINTER(i32)]
    L.s2amd_device_alloc.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(vp)]
    L.s2amd_device_free.argtypes = [vp, vp]
    L.s2amd_device_read.argtypes = [vp, vp, vp, ctypes.c_uint64]
    L.s2amd_find_islands.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, ctypes.POINTER(i32)]
    L.s2amd_color_constraints.argtypes = [vp, vp, i32, vp, i32, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_sharded_create.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.s2amd_sharded_destroy.argtypes = [vp]
    L.s2amd_sharded_destroy.restype = None
    L.s2amd_sharded_shard_count.argtypes = [vp]
    L.s2amd_sharded_solver.argtypes = [vp, i32]
    L.s2amd_sharded_solver.restype = vp
    L.s2amd_sharded_upload.argtypes = [vp, vp, i32, vp, i32, vp, i32]
    L.s2amd_sharded_step.argtypes = [vp, ctypes.POINTER(wire.StepParams)]
    L.s2amd_sharded_step_async.argtypes = [vp, ctypes.POINTER(wire.StepParams)]
    L.s2amd_sharded_wait.argtypes = [vp]
    L.s2amd_sharded_get_step_ops.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.s2amd_sharded_count_ops.argtypes = [i32, i32, ctypes.POINTER(i32)]
    L.s2amd_sharded_download.argtypes = [vp, vp, i32, vp, i32, vp, i32]
    L.s2amd_sharded_read_bodies.argtypes = [vp, i32, vp, i32]
    L.s2amd_sharded_reshard.argtypes = [vp, vp, i32, vp, i32]
    L.s2amd_sharded_get_partition.argtypes = [vp, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    if L.s2amd_api_version() != wire.API_VERSION:
        raise S2AmdError("libs2amd.so API version %d != %d" % (L.s2amd_api_version(), wire.API_VERSION))
    if fast and not L.s2amd_build_flags().decode().count("contract=fast"):
        raise S2AmdError("%s is not a tolerance-mode build (%s)" % (path, L.s2amd_build_flags().decode()))
    _libs[path] = L
    return L


def device_count():
    return load().s2amd_device_count()


def device_bus_id(device):
    buf = ctypes.create_string_buffer(64)
    _check(load().s2amd_device_bus_id(int(device), buf, 64))
    return buf.value.decode()


def _check(rc, L=None):
    if rc != 0:
        raise S2AmdError("s2amd error %d: %s" % (rc, (L or load()).s2amd_last_error().decode(errors="replace")))


def variant_families(fast=False):
    """{kernel family: tuple of its key's field names} of the variant tables (s2amd_get_variant_family)."""
    L = load(fast)
    out = {}
    for f in range(L.s2amd_variant_family_count()):
        kernel, fields = ctypes.c_char_p(), ctypes.c_char_p()
        _check(L.s2amd_get_variant_family(f, ctypes.byref(kernel), ctypes.byref(fields), None, None), L)
        out[kernel.value.decode()] = tuple(fields.value.decode().split(","))
    return out


def variant_census(fast=False):
    """{kernel family: {key tuple: count}}: every entry of the variant tables of the register-resident soft kernels and how often a launcher
    of this process has selected it so far (host-side selections -- an eager launch or a capture; the replays of a captured step graph are not
    counted: s2amd_get_variant_entry).  Counters never reset: compare two calls."""
    L = load(fast)
    out = {}
    for f in range(L.s2amd_variant_family_count()):
        kernel, length, entries = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32()
        _check(L.s2amd_get_variant_family(f, ctypes.byref(kernel), None, ctypes.byref(length), ctypes.byref(entries)), L)
        family = out.setdefault(kernel.value.decode(), {})
        key, count = (ctypes.c_int32 * length.value)(), ctypes.c_uint64()
        for e in range(entries.value):
            _check(L.s2amd_get_variant_entry(f, e, key, length.value, ctypes.byref(count)), L)
            family[tuple(key)] = int(count.value)
    return out


_env_options_logged = False


def env_options():
    """S2AMD_OPTIONS="key=value,key=value": options for every solver this process creates (bisecting a difference
    without editing the caller).  Validated here -- a malformed entry raises naming it -- and logged once to stderr,
    because it silently changes every solver of the process, the parity tests' included."""
    global _env_options_logged
    text = os.environ.get("S2AMD_OPTIONS", "")
    out = []
    for kv in filter(None, (e.strip() for e in text.split(","))):
        k, eq, v = kv.partition("=")
        try:
            if not eq or not k.strip():
                raise ValueError
            out.append((k.strip(), int(v)))
        except ValueError:
            raise S2AmdError("S2AMD_OPTIONS: entry %r is not key=integer" % kv) from None
    if out and not _env_options_logged:
        import sys
        print("[s2amd] S2AMD_OPTIONS applied to every solver: %s" % ", ".join("%s=%d" % e for e in out), file=sys.stderr)
        _env_options_logged = True
    return out


class Solver:
    """One device-resident world (one HIP stream).  Arrays are numpy structured arrays of the
    dtypes in solver2d_amd.wire and are mutated in place, like the reference mutates its pools."""

    def __init__(self, device=0, graph=True, profile=False, fast=False):
        """fast=True: the tolerance-mode build (libs2amd_fast.so, FMA contraction on; results within the stated
        tolerances of the oracle) instead of the bit-exact one."""
        L = load(fast=fast)
        h = ctypes.c_void_p()
        _check(L.s2amd_create(int(device), ctypes.byref(h)), L)
        self._L = L
        self._h = h
        self.fast = bool(fast)
        try:
            self.set_option("graph", 1 if graph else 0)
            self.set_option("profile", 1 if profile else 0)
            for k, v in env_options():
                self.set_option(k, v)
        except Exception:
            self.close()
            raise

    def _ck(self, rc):
        _check(rc, self._L)

    def close(self):
        if getattr(self, "_h", None):
            self._L.s2amd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def writable_bodies(self, body_capacity):
        """(writable uint8[nb], solver class): the bodies the coloured sweeps write -- what one colour must not share."""
        out = np.zeros(int(body_capacity), dtype=np.uint8)
        cls = ctypes.c_int32()
        self._ck(self._L.s2amd_get_writable_bodies(self._h, wire.as_ptr(out), len(out), ctypes.byref(cls)))
        return out, cls.value

    def set_option(self, key, value):
        self._ck(self._L.s2amd_set_option(self._h, key.encode(), int(value)))

    @staticmethod
    def _args(bodies, contacts, joints):
        for arr, dt in ((bodies, wire.body_dtype), (contacts, wire.contact_dtype), (joints, wire.joint_dtype)):
            if arr.dtype != dt or not arr.flags["C_CONTIGUOUS"]:
                raise ValueError("array must be a contiguous %s array" % (dt.names,))
        return (wire.as_ptr(bodies), len(bodies), wire.as_ptr(contacts), len(contacts), wire.as_ptr(joints), len(joints))

    def solve(self, params, bodies, contacts, joints):
        """== s2Solve_<params.solverType>(world, context): upload, solve, download; in place."""
        self._ck(self._L.s2amd_solve(self._h, ctypes.byref(params), *self._args(bodies, contacts, joints)))
        return bodies, contacts, joints

    def upload(self, bodies, contacts, joints):
        self._ck(self._L.s2amd_upload(self._h, *self._args(bodies, contacts, joints)))

    def step_resident(self, params):
        self._ck(self._L.s2amd_step_resident(self._h, ctypes.byref(params)))

    def download(self, bodies, contacts, joints):
        self._ck(self._L.s2amd_download(self._h, *self._args(bodies, contacts, joints)))
        return bodies, contacts, joints

    def save_bodies(self):
        self._ck(self._L.s2amd_save_bodies(self._h))

    def restore_bodies(self):
        self._ck(self._L.s2amd_restore_bodies(self._h))

    def export_poses(self, device_ptr, capacity):
        """{position, rot} per body into a caller-owned device buffer (float32[capacity, 4])."""
        self._ck(self._L.s2amd_export_poses(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity)))

    def export_bodies_async(self, device_ptr, capacity, slot):
        """Two float4 per body -- {position, rot}, {linearVelocity, angularVelocity, 0} -- enqueued like export_poses_async."""
        self._ck(self._L.s2amd_export_bodies_async(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity), int(slot)))

    def export_poses_async(self, device_ptr, capacity, slot):
        """export_poses enqueued behind the steps already on the solver's stream; pair with export_wait(slot)."""
        self._ck(self._L.s2amd_export_poses_async(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity), int(slot)))

    def export_wait(self, slot):
        self._ck(self._L.s2amd_export_wait(self._h, int(slot)))

    def device_alloc(self, nbytes):
        """A zeroed device buffer owned by the caller (an int address); free it with device_free."""
        p = ctypes.c_void_p()
        self._ck(self._L.s2amd_device_alloc(self._h, int(nbytes), ctypes.byref(p)))
        return int(p.value)

    def device_free(self, ptr):
        self._ck(self._L.s2amd_device_free(self._h, ctypes.c_void_p(int(ptr))))

    def device_read(self, ptr, shape, dtype=np.float32):
        out = np.zeros(shape, dtype=dtype)
        self._ck(self._L.s2amd_device_read(self._h, wire.as_ptr(out.reshape(-1)), ctypes.c_void_p(int(ptr)), out.nbytes))
        return out

    def device_write(self, ptr, values):
        """The bytes of a numpy array into device memory at `ptr` (device_alloc, or any device pointer), behind the solver's stream."""
        values = np.ascontiguousarray(values)
        self._ck(self._L.s2amd_device_write(self._h, ctypes.c_void_p(int(ptr)), wire.as_ptr(values.reshape(-1)), values.nbytes))

    def measure_dominant(self, params, repeats=20):
        """(us per launch, launches per sweep, constraints per launch) of the dominant kernel; see
        s2amd_measure_dominant."""
        us, n, c = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
        self._ck(self._L.s2amd_measure_dominant(self._h, ctypes.byref(params), int(repeats), ctypes.byref(us), ctypes.byref(n), ctypes.byref(c)))
        return us.value, n.value, c.value

    def refit_shapes(self, bodies, shapes, origins):
        """Stage 4 of s2World_Step on wire arrays (in place): origins, tight and fat AABBs, `enlarged`."""
        assert shapes.dtype == wire.shape_dtype and origins.dtype == np.float32 and origins.shape == (len(bodies), 2)
        self._ck(self._L.s2amd_refit_shapes(self._h, wire.as_ptr(bodies), len(bodies), wire.as_ptr(shapes), len(shapes), wire.as_ptr(origins)))
        return shapes, origins

    def update_contacts(self, bodies, origins, shapes, pairs, contacts):
        """Stage 3 of s2World_Step (s2UpdateContact per live contact) on wire arrays, in place; returns status int32[nc]."""
        assert pairs.dtype == wire.pair_state_dtype and contacts.dtype == wire.contact_dtype and len(pairs) == len(contacts)
        assert shapes.dtype == wire.shape_dtype
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        assert origins.shape == (len(bodies), 2)
        status = np.zeros(len(contacts), dtype=np.int32)
        self._ck(self._L.s2amd_update_contacts(self._h, wire.as_ptr(bodies), len(bodies), wire.as_ptr(origins), wire.as_ptr(shapes), len(shapes),
                                            wire.as_ptr(pairs), wire.as_ptr(contacts), len(contacts), wire.as_ptr(status)))
        return status

    # ---- resident world: stage 3 -> solve -> stage 4 chained in HBM ----
    def world_upload(self, bodies, contacts, joints, shapes, pairs, origins):
        assert shapes.dtype == wire.shape_dtype and pairs.dtype == wire.pair_state_dtype and len(pairs) == len(contacts)
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        assert origins.shape == (len(bodies), 2)
        self._ck(self._L.s2amd_world_upload(self._h, *self._args(bodies, contacts, joints), wire.as_ptr(shapes), len(shapes), wire.as_ptr(pairs),
                                         wire.as_ptr(origins)))
        self._world_bodies = len(bodies)

    def world_step(self, params):
        """One s2World_Step minus pair creation on the resident world; returns the step's counters as a dict."""
        info = wire.WorldStepInfo()
        self._ck(self._L.s2amd_world_step(self._h, ctypes.byref(params), ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in wire.WorldStepInfo._fields_}

    def world_find_pairs(self):
        """Stage 1's new pairs for the shapes the last refit moved: int32[n, 2] sorted by (A, B)."""
        cap = 1024
        while True:
            out = np.zeros((cap, 2), dtype=np.int32)
            n = ctypes.c_int32()
            rc = self._L.s2amd_world_find_pairs(self._h, wire.as_ptr(out), cap, ctypes.byref(n))
            if rc == -5 and n.value > cap:  # S2AMD_E_CAPACITY
                cap = n.value
                continue
            self._ck(rc)
            return out[: n.value].copy()

    def world_set_refit_order(self, order):
        """The order the caller's refit visits the movable shapes in (= the move buffer's order)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        self._ck(self._L.s2amd_world_set_refit_order(self._h, wire.as_ptr(order), len(order)))

    def world_set_tree(self, body_type, nodes, root):
        """One of the reference's three broad-phase trees (s2TreeNode records, wire.tree_node_dtype) onto the device."""
        nodes = np.ascontiguousarray(nodes)
        assert nodes.dtype == wire.tree_node_dtype
        self._ck(self._L.s2amd_world_set_tree(self._h, int(body_type), wire.as_ptr(nodes), len(nodes), int(root)))

    def world_get_tree(self, body_type, node_capacity):
        """(nodes, root) of a device tree as the reference would hold it now."""
        nodes = np.zeros(int(node_capacity), dtype=wire.tree_node_dtype)
        root = ctypes.c_int32()
        self._ck(self._L.s2amd_world_get_tree(self._h, int(body_type), wire.as_ptr(nodes), len(nodes), ctypes.byref(root)))
        return nodes, root.value

    def world_download_boxes(self, shape_capacity):
        """s2amdShapeBox of every resident shape slot after the last world_step."""
        out = np.zeros(int(shape_capacity), dtype=wire.shape_box_dtype)
        self._ck(self._L.s2amd_world_download_boxes(self._h, wire.as_ptr(out), len(out)))
        return out

    def world_separated(self, expected=64):
        """Contact slots the last world_step destroyed (their pairs separated), ascending."""
        out = np.zeros(max(int(expected), 1), dtype=np.int32)
        n = ctypes.c_int32()
        rc = self._L.s2amd_world_separated(self._h, wire.as_ptr(out), len(out), ctypes.byref(n))
        if rc == -5:
            out = np.zeros(n.value, dtype=np.int32)
            rc = self._L.s2amd_world_separated(self._h, wire.as_ptr(out), len(out), ctypes.byref(n))
        self._ck(rc)
        return out[: n.value].copy()

    def world_set_contacts(self, slots, contacts, pairs):
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        contacts = np.ascontiguousarray(contacts)
        pairs = np.ascontiguousarray(pairs)
        assert contacts.dtype == wire.contact_dtype and pairs.dtype == wire.pair_state_dtype and len(slots) == len(contacts) == len(pairs)
        self._ck(self._L.s2amd_world_set_contacts(self._h, wire.as_ptr(slots), len(slots), wire.as_ptr(contacts), wire.as_ptr(pairs)))

    def world_download(self, bodies, contacts, joints, shapes, pairs, origins):
        """Fills the given arrays (same sizes as uploaded) and returns them with the last stage-3 status."""
        origins = np.ascontiguousarray(origins, dtype=np.float32)
        status = np.zeros(len(contacts), dtype=np.int32)
        self._ck(self._L.s2amd_world_download(self._h, *self._args(bodies, contacts, joints), wire.as_ptr(shapes), len(shapes), wire.as_ptr(pairs),
                                           wire.as_ptr(origins), wire.as_ptr(status)))
        return bodies, contacts, joints, shapes, pairs, origins, status

    # ---- scene queries on the resident world: the world as it stands now, nothing resident changes ----
    def _world_best(self, fn, records, dtype, hit_dtype):
        """One answer per record: hit_dtype[len(records)]."""
        records = np.ascontiguousarray(records)
        assert records.dtype == dtype
        hits = np.zeros(len(records), dtype=hit_dtype)
        self._ck(fn(self._h, wire.as_ptr(records), len(records), wire.as_ptr(hits)))
        return hits

    def _world_lists(self, fn, records, dtype, payload_dtype, expected, distances=False):
        """A list per record: (offsets[len + 1], payload); with distances=True fn takes a float array behind the payload, and the answer is
        (offsets, payload, distances).  Asked again with the total the library states when it answers S2AMD_E_CAPACITY."""
        records = np.ascontiguousarray(records)
        assert records.dtype == dtype
        offsets = np.zeros(len(records) + 1, dtype=np.int32)
        cap = max(int(expected), 1)
        while True:
            payload = np.zeros(cap, dtype=payload_dtype)
            beside = np.zeros(cap, dtype=np.float32) if distances else None
            n = ctypes.c_int32()
            out = (wire.as_ptr(payload), wire.as_ptr(beside)) if distances else (wire.as_ptr(payload),)
            rc = fn(self._h, wire.as_ptr(records), len(records), wire.as_ptr(offsets), *out, cap, ctypes.byref(n))
            if rc == -5 and n.value > cap:  # S2AMD_E_CAPACITY
                cap = n.value
                continue
            self._ck(rc)
            if distances:
                return offsets, payload[: n.value].copy(), beside[: n.value].copy()
            return offsets, payload[: n.value].copy()

    def world_ray_cast(self, rays):
        """Closest hit of every ray (wire.ray_dtype) -> wire.ray_hit_dtype[len(rays)]; shape == -1: no hit."""
        return self._world_best(self._L.s2amd_world_ray_cast, rays, wire.ray_dtype, wire.ray_hit_dtype)

    def world_point_probe(self, probes, expected=None):
        """The shapes that contain each point (wire.point_probe_dtype): (offsets[len + 1], shapes), ascending by slot per probe."""
        return self._world_lists(self._L.s2amd_world_point_probe, probes, wire.point_probe_dtype, np.int32, expected or 4 * len(probes) + 64)

    def world_query_boxes(self, boxes, expected=None):
        """The shapes whose fat box overlaps each box (wire.box_query_dtype): (offsets[len + 1], shapes), ascending by slot per box."""
        return self._world_lists(self._L.s2amd_world_query_boxes, boxes, wire.box_query_dtype, np.int32, expected or 16 * len(boxes) + 64)

    # ---- proximity queries on the resident world: s2ShapeDistance between a caller's proxy and the shapes near it ----
    def world_closest_shape(self, queries):
        """The in-range shape of least distance for every query (wire.proximity_query_dtype) -> wire.proximity_hit_dtype[len(queries)];
        shape == -1: nothing within maxDistance."""
        return self._world_best(self._L.s2amd_world_closest_shape, queries, wire.proximity_query_dtype, wire.proximity_hit_dtype)

    def world_shapes_in_range(self, queries, distances=False, expected=None):
        """The shapes within maxDistance of each query: (offsets[len + 1], shapes), ascending by slot per query; with distances=True
        (offsets, shapes, distances).  Asked again with the total the library states when it answers S2AMD_E_CAPACITY."""
        fn = self._L.s2amd_world_shapes_in_range
        if not distances:
            fn = lambda h, q, count, offsets, shapes, cap, total: self._L.s2amd_world_shapes_in_range(h, q, count, offsets, shapes, None, cap, total)  # noqa: E731
        return self._world_lists(fn, queries, wire.proximity_query_dtype, np.int32, expected or 8 * len(queries) + 64, distances=bool(distances))

    # ---- contact queries on the resident world: the reference's manifolds between a caller's shape and the shapes near it ----
    def world_deepest_contact(self, queries):
        """The hit of least separation for every query (wire.contact_query_dtype) -> wire.contact_hit_dtype[len(queries)];
        shape == -1: the query touches nothing."""
        return self._world_best(self._L.s2amd_world_deepest_contact, queries, wire.contact_query_dtype, wire.contact_hit_dtype)

    def world_collide_shape(self, queries, expected=None):
        """The manifolds of each query against the shapes it touches: (offsets[len + 1], hits), ascending by slot per query.  Asked again
        with the total the library states when it answers S2AMD_E_CAPACITY."""
        return self._world_lists(self._L.s2amd_world_collide_shape, queries, wire.contact_query_dtype, wire.contact_hit_dtype, expected or 4 * len(queries) + 64,
                                 distances=None)

    # ---- shape casts on the resident world: a caller's proxy swept along a vector, conservative advancement over s2ShapeDistance ----
    def world_cast_shape(self, casts):
        """The hit of least fraction for every cast (wire.shape_cast_dtype) -> wire.shape_cast_hit_dtype[len(casts)];
        shape == -1: the sweep reaches nothing up to maxFraction."""
        return self._world_best(self._L.s2amd_world_cast_shape, casts, wire.shape_cast_dtype, wire.shape_cast_hit_dtype)

    def world_cast_shape_all(self, casts, expected=None):
        """Every shape each cast hits: (offsets[len + 1], hits), ascending by slot per cast.  Asked again with the total the library
        states when it answers S2AMD_E_CAPACITY."""
        return self._world_lists(self._L.s2amd_world_cast_shape_all, casts, wire.shape_cast_dtype, wire.shape_cast_hit_dtype, expected or 4 * len(casts) + 64,
                                 distances=None)

    # ---- move-and-slide on the resident world: cast, stop a skin short, clip to the plane met, cast again -- all on the device ----
    def world_move_shapes(self, movers, planes=True):
        """Where every mover (wire.mover_dtype) ends and what it slid against -> (wire.mover_result_dtype[len(movers)],
        wire.mover_plane_dtype[len(movers), 8]); with planes=False the library is given no plane array and the answer is the results."""
        movers = np.ascontiguousarray(movers)
        assert movers.dtype == wire.mover_dtype
        results = np.zeros(len(movers), dtype=wire.mover_result_dtype)
        out = np.zeros((len(movers), wire.MOVER_MAX_ITERATIONS), dtype=wire.mover_plane_dtype) if planes else None
        self._ck(self._L.s2amd_world_move_shapes(self._h, wire.as_ptr(movers), len(movers), wire.as_ptr(results), wire.as_ptr(out) if planes else None))
        return (results, out) if planes else results

    # ---- world edits: the reference's eight per-frame setters applied to the resident records, the structure kept ----
    def world_edit(self, edits, want_skipped=True):
        """Applies wire.world_edit_dtype records (wire.edit_*) to the resident bodies and joints in list order, behind the last step and
        before the next.  Returns how many were skipped (a free slot, a joint of the other type); with want_skipped=False the call only
        enqueues, reads nothing back and returns None."""
        edits = np.ascontiguousarray(edits)
        assert edits.dtype == wire.world_edit_dtype
        skipped = ctypes.c_int32(-1)
        self._ck(self._L.s2amd_world_edit(self._h, wire.as_ptr(edits), len(edits), ctypes.byref(skipped) if want_skipped else None))
        return skipped.value if want_skipped else None

    # ---- actuators on the resident world (s2amd_world_set_actuators, ...): channels of a device-side action vector drive every step ----
    def world_set_actuators(self, actuators, channels):
        """Replaces the whole persistent list (wire.actuator_dtype; an empty one clears it) and zeroes the action buffer of `channels`
        floats: every world_step applies the list in front of the persistent fields."""
        actuators = np.ascontiguousarray(actuators)
        assert actuators.dtype == wire.actuator_dtype
        self._ck(self._L.s2amd_world_set_actuators(self._h, wire.as_ptr(actuators) if len(actuators) else None, len(actuators), int(channels)))
        self._world_actuators = len(actuators)

    def world_set_actions(self, values, first=0):
        """Host values into channels [first, first + len(values)) of the action buffer; enqueued, no wait."""
        values = np.ascontiguousarray(values, dtype=np.float32)
        self._ck(self._L.s2amd_world_set_actions(self._h, wire.as_ptr(values) if len(values) else None, int(first), len(values)))

    def world_import_actions(self, device_ptr, count, first=0):
        """`count` floats from device memory (device_alloc, or a torch tensor's data_ptr() whose producer stream has been synchronised)
        into channels [first, first + count) of the action buffer; enqueued, no wait."""
        self._ck(self._L.s2amd_world_import_actions(self._h, ctypes.c_void_p(int(device_ptr)), int(first), int(count)))

    def world_actuator_states(self):
        """wire.actuator_state_dtype records, one per actuator of the list, of the last world_step's pass."""
        return self._world_list(self._L.s2amd_world_actuator_states, wire.actuator_state_dtype, getattr(self, "_world_actuators", 0))

    def world_actuator_counts(self):
        """int32[4]: actuators per status {APPLIED, DISABLED, SKIPPED, NONFINITE} of the last world_step's pass."""
        counts = np.zeros(4, dtype=np.int32)
        self._ck(self._L.s2amd_world_actuator_counts(self._h, wire.as_ptr(counts)))
        return counts

    # ---- observers on the resident world (s2amd_world_set_observers, ...): the world's state as a device-side observation vector ----
    def world_set_observers(self, observers, channels, frames=1):
        """Replaces the whole persistent list (wire.observer_dtype; an empty one clears it): every world_step with the observation report
        on writes a vector of `channels` floats, kept for the last `frames` reporting steps."""
        observers = np.ascontiguousarray(observers)
        assert observers.dtype == wire.observer_dtype
        self._ck(self._L.s2amd_world_set_observers(self._h, wire.as_ptr(observers) if len(observers) else None, len(observers), int(channels), int(frames)))
        self._world_observers = (len(observers), int(frames), int(channels)) if len(observers) else (0, 0, 0)

    def world_set_observation_report(self, flags):
        """wire.OBSERVATION_REPORT_VECTOR | _STATES: what the next world_step reports (0: nothing, and the history stands still)."""
        self._ck(self._L.s2amd_world_set_observation_report(self._h, int(flags)))

    def world_observations(self):
        """float32[frames, channels] of the last world_step: frame 0 is that step, frame k the k-th reporting step before it."""
        _, frames, channels = getattr(self, "_world_observers", (0, 0, 0))
        return self._world_list(self._L.s2amd_world_observations, np.float32, frames * channels).reshape(frames, channels)

    def world_export_observations(self, device_ptr, capacity):
        """world_observations' bytes into a device buffer (device_alloc, or a torch tensor's data_ptr()) of `capacity` floats; waits."""
        self._ck(self._L.s2amd_world_export_observations(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity)))

    def world_export_observations_async(self, device_ptr, capacity, slot=0):
        """The same copy enqueued behind the steps on the solver's stream, with an event in `slot`; pair with export_wait(slot)."""
        self._ck(self._L.s2amd_world_export_observations_async(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity), int(slot)))

    def world_observer_states(self):
        """wire.observer_state_dtype records, one per observer of the list, of the last world_step's pass."""
        return self._world_list(self._L.s2amd_world_observer_states, wire.observer_state_dtype, getattr(self, "_world_observers", (0, 0, 0))[0])

    def world_observer_counts(self):
        """int32[4]: observers per status {OBSERVED, DISABLED, SKIPPED, SOURCE_OFF} of the last world_step's pass."""
        counts = np.zeros(4, dtype=np.int32)
        self._ck(self._L.s2amd_world_observer_counts(self._h, wire.as_ptr(counts)))
        return counts

    # ---- episodes on the resident world (s2amd_world_set_episodes, ...): rewards, termination and the episode accounting on the device ----
    def world_set_episodes(self, rules, agents, step_limits=None):
        """Replaces the whole persistent list (wire.episode_rule_dtype) over `agents` agents, with one step limit per agent (None or 0:
        no limit); agents = 0 clears it.  Every world_step with the episode report on gives one reward and one flags word per agent."""
        rules = np.ascontiguousarray(rules)
        assert rules.dtype == wire.episode_rule_dtype
        limits = None if step_limits is None else np.ascontiguousarray(step_limits, dtype=np.int32)
        assert limits is None or len(limits) == int(agents)
        self._ck(self._L.s2amd_world_set_episodes(self._h, wire.as_ptr(rules) if len(rules) else None, len(rules), int(agents),
                                                  wire.as_ptr(limits) if limits is not None and len(limits) else None))
        self._world_episodes = (len(rules), int(agents))

    def world_set_episode_report(self, flags):
        """wire.EPISODE_REPORT_STEP | _STATES | _RULE_STATES | _EVENTS: what the next world_step reports (0: nothing, and no episode advances)."""
        self._ck(self._L.s2amd_world_set_episode_report(self._h, int(flags)))

    def world_episode_rewards(self):
        """float32[agents]: the rewards of the last world_step."""
        return self._world_list(self._L.s2amd_world_episode_rewards, np.float32, getattr(self, "_world_episodes", (0, 0))[1])

    def world_episode_flags(self):
        """int32[agents]: wire.EPISODE_TERMINATED | _TRUNCATED | _TIME_LIMIT of the last world_step."""
        return self._world_list(self._L.s2amd_world_episode_flags, np.int32, getattr(self, "_world_episodes", (0, 0))[1])

    def world_export_episode_step(self, rewards_ptr, flags_ptr, capacity):
        """The two arrays above into device buffers (device_alloc, or a torch tensor's data_ptr()) of `capacity` entries each; waits."""
        self._ck(self._L.s2amd_world_export_episode_step(self._h, ctypes.c_void_p(int(rewards_ptr)), ctypes.c_void_p(int(flags_ptr)), int(capacity)))

    def world_export_episode_step_async(self, rewards_ptr, flags_ptr, capacity, slot=0):
        """The same copies enqueued behind the steps on the solver's stream, with an event in `slot`; pair with export_wait(slot)."""
        self._ck(self._L.s2amd_world_export_episode_step_async(self._h, ctypes.c_void_p(int(rewards_ptr)), ctypes.c_void_p(int(flags_ptr)), int(capacity), int(slot)))

    def world_episode_states(self):
        """wire.episode_state_dtype records, one per agent: this step's flags and reward, and the episode accounting."""
        return self._world_list(self._L.s2amd_world_episode_states, wire.episode_state_dtype, getattr(self, "_world_episodes", (0, 0))[1])

    def world_episode_rule_states(self):
        """wire.episode_rule_state_dtype records, one per rule in list order, of the last world_step's pass."""
        return self._world_list(self._L.s2amd_world_episode_rule_states, wire.episode_rule_state_dtype, getattr(self, "_world_episodes", (0, 0))[0])

    def world_episode_events(self, expected=16):
        """wire.episode_event_dtype records: the agents whose episode ended in the last world_step, ascending."""
        return self._world_list(self._L.s2amd_world_episode_events, wire.episode_event_dtype, expected)

    def world_episode_counts(self):
        """int32[8]: rules per status {EVALUATED, DISABLED, SKIPPED, SOURCE_OFF}, then agents done, terminated, truncated, at the time limit."""
        counts = np.zeros(8, dtype=np.int32)
        self._ck(self._L.s2amd_world_episode_counts(self._h, wire.as_ptr(counts)))
        return counts

    # ---- resets on the resident world (s2amd_world_set_resets, ...): finished agents restart on the device ----
    def world_set_resets(self, bodies, joints, agents, seed=0):
        """Replaces the whole persistent list (wire.reset_body_dtype and wire.reset_joint_dtype records, e.g. wire.resets_from_world) over
        `agents` agents; agents = 0 clears it.  `seed` keys the jitter."""
        bodies, joints = np.ascontiguousarray(bodies), np.ascontiguousarray(joints)
        assert bodies.dtype == wire.reset_body_dtype and joints.dtype == wire.reset_joint_dtype
        self._ck(self._L.s2amd_world_set_resets(self._h, wire.as_ptr(bodies) if len(bodies) else None, len(bodies), wire.as_ptr(joints) if len(joints) else None,
                                                len(joints), int(agents), int(seed) & 0xFFFFFFFF))
        self._world_resets = int(agents)

    def world_set_reset_report(self, flags):
        """wire.RESET_ON_EPISODE_END: every world_step resets the agents whose episode ended in it, behind its episode pass;
        wire.RESET_REPORT_STATES opens world_reset_states.  0: a step enqueues nothing."""
        self._ck(self._L.s2amd_world_set_reset_report(self._h, int(flags)))

    def world_reset_agents(self, agents=None):
        """The reset pass between steps for the agents listed (None: every agent); enqueued like an edit, waits for nothing."""
        if agents is None:
            self._ck(self._L.s2amd_world_reset_agents(self._h, None, wire.RESET_ALL))
            return
        agents = np.ascontiguousarray(agents, dtype=np.int32)
        self._ck(self._L.s2amd_world_reset_agents(self._h, wire.as_ptr(agents) if len(agents) else None, len(agents)))

    def world_reset_states(self):
        """wire.reset_state_dtype records, one per agent: how often it has been reset, and whether the last pass did."""
        return self._world_list(self._L.s2amd_world_reset_states, wire.reset_state_dtype, getattr(self, "_world_resets", 0))

    def world_reset_counts(self):
        """int32[8] of the last pass: agents reset, bodies applied, bodies skipped, joints applied, joints skipped, shapes moved,
        contacts emptied, source off."""
        counts = np.zeros(8, dtype=np.int32)
        self._ck(self._L.s2amd_world_reset_counts(self._h, wire.as_ptr(counts)))
        return counts

    # ---- force fields on the resident world (s2amd_world_apply_fields, s2amd_world_set_fields): writes addressed by region ----
    def world_apply_fields(self, fields, want_states=True):
        """Applies wire.field_dtype records (wire.field_*) to the resident bodies once, in list order, behind the last step and before
        the next.  Returns one wire.field_state_dtype record per field; with want_states=False the call only enqueues, reads nothing
        back and returns None."""
        fields = np.ascontiguousarray(fields)
        assert fields.dtype == wire.field_dtype
        states = np.zeros(len(fields), dtype=wire.field_state_dtype) if want_states else None
        self._ck(self._L.s2amd_world_apply_fields(self._h, wire.as_ptr(fields) if len(fields) else None, len(fields),
                                                  wire.as_ptr(states) if want_states and len(fields) else None))
        return states

    def world_set_fields(self, fields):
        """Replaces the whole persistent list (wire.field_dtype; an empty one clears it): every world_step applies it in front of its
        stage 3.  The list holds across uploads."""
        fields = np.ascontiguousarray(fields)
        assert fields.dtype == wire.field_dtype
        self._ck(self._L.s2amd_world_set_fields(self._h, wire.as_ptr(fields) if len(fields) else None, len(fields)))
        self._world_fields = len(fields)

    def world_field_states(self):
        """wire.field_state_dtype records, one per field of the persistent list, of the last world_step's application."""
        return self._world_list(self._L.s2amd_world_field_states, wire.field_state_dtype, getattr(self, "_world_fields", 0))

    # ---- the reports of the resident world: the three shapes their getters have ----
    def _world_list(self, fn, dtype, expected):
        """One counted list: grown to the count the library states when it answers S2AMD_E_CAPACITY (the count is set, nothing was consumed)."""
        cap = max(int(expected), 1)
        while True:
            out = np.zeros(cap, dtype=dtype)
            n = ctypes.c_int32()
            rc = fn(self._h, wire.as_ptr(out), cap, ctypes.byref(n))
            if rc == -5 and n.value > cap:  # S2AMD_E_CAPACITY
                cap = n.value
                continue
            self._ck(rc)
            return out[: n.value].copy()

    def _world_event_pair(self, fn, expected):
        """Two counted lists of int32 codes, grown the same way."""
        cap_a = cap_b = max(int(expected), 1)
        while True:
            a, b = np.zeros(cap_a, dtype=np.int32), np.zeros(cap_b, dtype=np.int32)
            na, nb = ctypes.c_int32(), ctypes.c_int32()
            rc = fn(self._h, wire.as_ptr(a), cap_a, ctypes.byref(na), wire.as_ptr(b), cap_b, ctypes.byref(nb))
            if rc == -5 and (na.value > cap_a or nb.value > cap_b):  # S2AMD_E_CAPACITY
                cap_a, cap_b = max(cap_a, na.value), max(cap_b, nb.value)
                continue
            self._ck(rc)
            return a[: na.value].copy(), b[: nb.value].copy()

    def _world_record(self, fn, dtype):
        """One record."""
        out = np.zeros(1, dtype=dtype)
        self._ck(fn(self._h, wire.as_ptr(out)))
        return out[0]

    # ---- contact report of the resident world (s2amd_world_set_report): what touches what, and how hard ----
    def world_set_report(self, flags):
        """wire.REPORT_* bits: what every world_step from the next one on compacts on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_report(self._h, int(flags)))

    def world_touch_events(self, expected=64):
        """(began, ended): the contact slots that started / stopped touching in the last world_step, each ascending."""
        return self._world_event_pair(self._L.s2amd_world_touch_events, expected)

    def world_touching(self, expected=1024):
        """wire.touching_contact_dtype records of the contacts touching after the last world_step, ascending by slot."""
        return self._world_list(self._L.s2amd_world_touching, wire.touching_contact_dtype, expected)

    def world_body_sums(self, body_capacity=None):
        """wire.body_contact_sum_dtype per body slot: net contact impulse, normal load and touching count after the last world_step
        (body_capacity: that of the upload, which is the default)."""
        if body_capacity is None:
            body_capacity = getattr(self, "_world_bodies", 0)
        out = np.zeros(int(body_capacity), dtype=wire.body_contact_sum_dtype)
        self._ck(self._L.s2amd_world_body_sums(self._h, wire.as_ptr(out), len(out)))
        return out

    # ---- joint report of the resident world (s2amd_world_set_joint_report): joint states, limit events, reactions ----
    def world_set_joint_report(self, flags):
        """wire.JOINT_REPORT_* bits: what every world_step from the next one on compacts on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_joint_report(self._h, int(flags)))

    def world_joint_states(self, expected=256):
        """wire.joint_state_dtype records of the live joint slots after the last world_step, ascending by slot."""
        return self._world_list(self._L.s2amd_world_joint_states, wire.joint_state_dtype, expected)

    def world_joint_limit_events(self, expected=64):
        """(began, ended): the codes 2 * slot + side (0 lower, 1 upper) of the joint limits that became / stopped being active in the
        last world_step, each ascending."""
        return self._world_event_pair(self._L.s2amd_world_joint_limit_events, expected)

    def world_body_joint_sums(self, body_capacity=None):
        """wire.body_joint_sum_dtype per body slot: net joint impulse, axial impulse and joint count after the last world_step
        (body_capacity: that of the upload, which is the default)."""
        if body_capacity is None:
            body_capacity = getattr(self, "_world_bodies", 0)
        out = np.zeros(int(body_capacity), dtype=wire.body_joint_sum_dtype)
        self._ck(self._L.s2amd_world_body_joint_sums(self._h, wire.as_ptr(out), len(out)))
        return out

    def world_joint_summary(self):
        """One wire.joint_summary_dtype record: joint counts, limits active, the largest anchor gap after the last world_step."""
        return self._world_record(self._L.s2amd_world_joint_summary, wire.joint_summary_dtype)

    # ---- shape report of the resident world (s2amd_world_set_shape_report): draw records, view events, bounds ----
    def world_set_shape_report(self, flags):
        """wire.SHAPE_REPORT_* bits: what every world_step from the next one on compacts on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_shape_report(self._h, int(flags)))

    def world_set_shape_view(self, box):
        """The view box (lower.x, lower.y, upper.x, upper.y) the report culls to from the next world_step on; None: every live shape."""
        if box is None:
            self._ck(self._L.s2amd_world_set_shape_view(self._h, None))
            return
        box = np.ascontiguousarray(box, dtype=np.float32)
        assert box.shape == (4,)
        self._ck(self._L.s2amd_world_set_shape_view(self._h, wire.as_ptr(box)))

    def world_shape_draws(self, expected=1024):
        """wire.shape_draw_dtype records of the live shapes in view after the last world_step, ascending by shape slot."""
        return self._world_list(self._L.s2amd_world_shape_draws, wire.shape_draw_dtype, expected)

    def world_shape_view_events(self, expected=64):
        """(entered, left): the shape slots that came into / went out of view in the last world_step, each ascending."""
        return self._world_event_pair(self._L.s2amd_world_shape_view_events, expected)

    def world_shape_summary(self):
        """One wire.shape_summary_dtype record: shape counts, shapes in view, the movable and the in-view bounds after the last world_step."""
        return self._world_record(self._L.s2amd_world_shape_summary, wire.shape_summary_dtype)

    # ---- body report of the resident world (s2amd_world_set_body_report): states, rest events, islands ----
    def world_set_body_report(self, flags):
        """wire.BODY_REPORT_* bits: what every world_step from the next one on compacts on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_body_report(self._h, int(flags)))

    def world_set_rest_thresholds(self, linear_speed, angular_speed, seconds):
        """At rest: speed <= linear_speed and |w| <= angular_speed for `seconds`; holds from the next world_step on."""
        self._ck(self._L.s2amd_world_set_rest_thresholds(self._h, float(np.float32(linear_speed)), float(np.float32(angular_speed)), float(np.float32(seconds))))

    def world_body_states(self, expected=1024):
        """wire.body_state_dtype records of the reported bodies (under MOVED_ONLY: the moved ones) after the last world_step, ascending by slot."""
        return self._world_list(self._L.s2amd_world_body_states, wire.body_state_dtype, expected)

    def world_body_rest_events(self, expected=64):
        """(rested, woke): the body slots that came to rest / woke up in the last world_step, each ascending."""
        return self._world_event_pair(self._L.s2amd_world_body_rest_events, expected)

    def world_islands(self, expected=256):
        """wire.island_state_dtype records of the islands of the world as it stands after the last world_step, by lowest body slot."""
        return self._world_list(self._L.s2amd_world_islands, wire.island_state_dtype, expected)

    def world_body_summary(self):
        """One wire.body_summary_dtype record: body, rest and island counts, the largest island, the fastest body after the last world_step."""
        return self._world_record(self._L.s2amd_world_body_summary, wire.body_summary_dtype)

    # ---- step metrics of the resident world (s2amd_world_set_metrics): one record per step, kept in a ring on the device ----
    def world_set_metrics(self, flags, history_length=1):
        """wire.METRICS_* bits: what every world_step from the next one on reduces to one record (0: nothing, the default); the ring keeps
        the last `history_length` records (1..wire.METRICS_MAX_HISTORY).  Every call restarts the recorder."""
        self._ck(self._L.s2amd_world_set_metrics(self._h, int(flags), int(history_length)))

    def world_metrics(self):
        """One wire.step_metrics_dtype record: the last world_step's."""
        return self._world_record(self._L.s2amd_world_metrics, wire.step_metrics_dtype)

    def world_metrics_history(self, expected=wire.METRICS_MAX_HISTORY):
        """wire.step_metrics_dtype records of the steps the ring still holds, oldest first, in one read."""
        return self._world_list(self._L.s2amd_world_metrics_history, wire.step_metrics_dtype, expected)

    # ---- sensor report of the resident world (s2amd_world_set_sensors, s2amd_world_set_sensor_report): inside, entered, left ----
    def world_set_sensors(self, sensors):
        """Replaces the whole list of sensors (wire.sensor_dtype; an empty one clears it).  The list holds across uploads."""
        sensors = np.ascontiguousarray(sensors)
        assert sensors.dtype == wire.sensor_dtype
        self._ck(self._L.s2amd_world_set_sensors(self._h, wire.as_ptr(sensors) if len(sensors) else None, len(sensors)))
        self._world_sensors = len(sensors)

    def world_set_sensor_report(self, flags, list_capacity=0):
        """wire.SENSOR_REPORT_* bits: what every world_step from the next one on evaluates on the device (0: nothing, the default);
        list_capacity sizes the device lists a step writes and never changes an answer."""
        self._ck(self._L.s2amd_world_set_sensor_report(self._h, int(flags), int(list_capacity)))

    def world_sensor_inside(self, expected=64):
        """(offsets[sensors + 1], shapes): the shape slots inside each sensor after the last world_step, ascending per sensor.  Asked again
        with the total the library states when it answers S2AMD_E_CAPACITY."""
        offsets = np.zeros(getattr(self, "_world_sensors", 0) + 1, dtype=np.int32)
        cap = max(int(expected), 1)
        while True:
            shapes = np.zeros(cap, dtype=np.int32)
            n = ctypes.c_int32()
            rc = self._L.s2amd_world_sensor_inside(self._h, wire.as_ptr(offsets), wire.as_ptr(shapes), cap, ctypes.byref(n))
            if rc == -5 and n.value > cap:  # S2AMD_E_CAPACITY
                cap = n.value
                continue
            self._ck(rc)
            return offsets, shapes[: n.value].copy()

    def world_sensor_events(self, expected=64):
        """(entered, left): wire.sensor_event_dtype records of the (sensor, shape) pairs that came inside / went out in the last world_step,
        each ascending by (sensor, shape).  Asked again with the counts the library states when it answers S2AMD_E_CAPACITY."""
        cap_a = cap_b = max(int(expected), 1)
        while True:
            a, b = np.zeros(cap_a, dtype=wire.sensor_event_dtype), np.zeros(cap_b, dtype=wire.sensor_event_dtype)
            na, nb = ctypes.c_int32(), ctypes.c_int32()
            rc = self._L.s2amd_world_sensor_events(self._h, wire.as_ptr(a), cap_a, ctypes.byref(na), wire.as_ptr(b), cap_b, ctypes.byref(nb))
            if rc == -5 and (na.value > cap_a or nb.value > cap_b):  # S2AMD_E_CAPACITY
                cap_a, cap_b = max(cap_a, na.value), max(cap_b, nb.value)
                continue
            self._ck(rc)
            return a[: na.value].copy(), b[: nb.value].copy()

    def world_sensor_states(self, expected=None):
        """wire.sensor_state_dtype records, one per sensor in list order, after the last world_step."""
        return self._world_list(self._L.s2amd_world_sensor_states, wire.sensor_state_dtype, expected or getattr(self, "_world_sensors", 0))

    # ---- ray report of the resident world (s2amd_world_set_ray_sensors, s2amd_world_set_ray_report): states, ranges, events ----
    def world_set_ray_sensors(self, rays):
        """Replaces the whole list of ray sensors (wire.ray_sensor_dtype; an empty one clears it).  The list holds across uploads."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == wire.ray_sensor_dtype
        self._ck(self._L.s2amd_world_set_ray_sensors(self._h, wire.as_ptr(rays) if len(rays) else None, len(rays)))
        self._world_rays = len(rays)

    def world_set_ray_report(self, flags):
        """wire.RAY_REPORT_* bits: what every world_step from the next one on casts on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_ray_report(self._h, int(flags)))

    def world_ray_states(self, expected=None):
        """wire.ray_state_dtype records, one per ray in list order, after the last world_step."""
        return self._world_list(self._L.s2amd_world_ray_states, wire.ray_state_dtype, expected or getattr(self, "_world_rays", 0))

    def world_ray_ranges(self, expected=None):
        """float32[rays]: the hit fraction (maxFraction on a miss) of every ray in list order, after the last world_step."""
        return self._world_list(self._L.s2amd_world_ray_ranges, np.float32, expected or getattr(self, "_world_rays", 0))

    def world_export_ray_ranges(self, device_ptr, capacity):
        """world_ray_ranges' bytes into a device buffer (device_alloc, or a torch tensor's data_ptr()) of `capacity` floats."""
        self._ck(self._L.s2amd_world_export_ray_ranges(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity)))

    def world_ray_events(self, expected=64):
        """wire.ray_event_dtype records of the rays whose hit shape changed in the last world_step, ascending by ray."""
        return self._world_list(self._L.s2amd_world_ray_events, wire.ray_event_dtype, expected)

    # ---- grid report of the resident world (s2amd_world_set_grid_sensors, s2amd_world_set_grid_report): per-cell images, states ----
    def world_set_grid_sensors(self, grids):
        """Replaces the whole list of occupancy grids (wire.grid_sensor_dtype; an empty one clears it).  The list holds across uploads."""
        grids = np.ascontiguousarray(grids)
        assert grids.dtype == wire.grid_sensor_dtype
        self._ck(self._L.s2amd_world_set_grid_sensors(self._h, wire.as_ptr(grids) if len(grids) else None, len(grids)))
        self._world_grids = len(grids)
        self._world_grid_cells = int((grids["width"].astype(np.int64) * grids["height"]).sum())

    def world_set_grid_report(self, flags):
        """wire.GRID_REPORT_* bits: what every world_step from the next one on rasterises on the device (0: nothing, the default)."""
        self._ck(self._L.s2amd_world_set_grid_report(self._h, int(flags)))

    def world_grid_categories(self, expected=None):
        """uint32[cells]: the OR of categoryBits over each cell's hits, grids in list order, cell (i, j) at firstCell + j * width + i."""
        return self._world_list(self._L.s2amd_world_grid_categories, np.uint32, expected or getattr(self, "_world_grid_cells", 0))

    def world_grid_shapes(self, expected=None):
        """int32[cells]: the lowest hit slot of each cell, or -1."""
        return self._world_list(self._L.s2amd_world_grid_shapes, np.int32, expected or getattr(self, "_world_grid_cells", 0))

    def world_grid_occupancy(self, expected=None):
        """float32[cells]: 1.0 where a cell has a hit, else 0.0."""
        return self._world_list(self._L.s2amd_world_grid_occupancy, np.float32, expected or getattr(self, "_world_grid_cells", 0))

    def world_export_grid_occupancy(self, device_ptr, capacity):
        """world_grid_occupancy's bytes into a device buffer (device_alloc, or a torch tensor's data_ptr()) of `capacity` floats."""
        self._ck(self._L.s2amd_world_export_grid_occupancy(self._h, ctypes.c_void_p(int(device_ptr)), int(capacity)))

    def world_grid_states(self, expected=None):
        """wire.grid_state_dtype records, one per grid in list order, after the last world_step."""
        return self._world_list(self._L.s2amd_world_grid_states, wire.grid_state_dtype, expected or getattr(self, "_world_grids", 0))

    def find_islands(self, bodies, contacts, joints):
        """(island_of_body int32[nb], island_count): connected components over the movable bodies, on the device."""
        island = np.full(len(bodies), -2, dtype=np.int32)
        n = ctypes.c_int32()
        self._ck(self._L.s2amd_find_islands(self._h, wire.as_ptr(bodies), len(bodies), wire.as_ptr(contacts), len(contacts), wire.as_ptr(joints),
                                         len(joints), wire.as_ptr(island), ctypes.byref(n)))
        return island, n.value

    def color_constraints(self, bodies, contacts):
        """(color_of_contact int32[nc], color_count, rounds): deterministic Jones-Plassmann colouring on the device."""
        colour = np.full(len(contacts), -2, dtype=np.int32)
        n, r = ctypes.c_int32(), ctypes.c_int32()
        self._ck(self._L.s2amd_color_constraints(self._h, wire.as_ptr(bodies), len(bodies), wire.as_ptr(contacts), len(contacts), wire.as_ptr(colour),
                                              ctypes.byref(n), ctypes.byref(r)))
        return colour, n.value, r.value

    def find_pairs(self, bodies, shapes, moved, existing, joints):
        """New broad-phase pairs as int32[n, 2] sorted by (A, B); see s2amd_find_pairs."""
        existing = np.ascontiguousarray(existing, dtype=np.int32).reshape(-1, 2)
        moved = np.ascontiguousarray(moved, dtype=np.uint8)
        cap = 4096
        while True:
            out = np.zeros((cap, 2), dtype=np.int32)
            n = ctypes.c_int32()
            rc = self._L.s2amd_find_pairs(self._h, wire.as_ptr(bodies), len(bodies), wire.as_ptr(shapes), len(shapes), wire.as_ptr(moved),
                                         wire.as_ptr(existing), len(existing), wire.as_ptr(joints), len(joints), wire.as_ptr(out), cap,
                                         ctypes.byref(n))
            if rc == -5 and n.value > cap:
                cap = n.value
                continue
            self._ck(rc)
            return out[: n.value].copy()

    def _order(self, fn):
        n, nc = ctypes.c_int32(), ctypes.c_int32()
        self._ck(fn(self._h, None, 0, None, 0, ctypes.byref(n), ctypes.byref(nc)))
        order = np.zeros(max(n.value, 1), dtype=np.int32)
        offsets = np.zeros(nc.value + 1, dtype=np.int32)
        self._ck(fn(self._h, order.ctypes.data, len(order), offsets.ctypes.data, len(offsets), ctypes.byref(n), ctypes.byref(nc)))
        return order[: n.value].copy(), offsets

    def contact_order(self):
        """(order, colorOffsets) of the last step; see s2amd_get_contact_order."""
        return self._order(self._L.s2amd_get_contact_order)

    def strip_owners(self, body_capacity):
        """(ownerStrip, onSeam, stripCount): see s2amd_get_strip_owners."""
        owner = np.full(max(body_capacity, 1), -1, dtype=np.int32)
        seam = np.full(max(body_capacity, 1), -1, dtype=np.int32)
        n = ctypes.c_int32()
        self._ck(self._L.s2amd_get_strip_owners(self._h, owner.ctypes.data, seam.ctypes.data, len(owner), ctypes.byref(n)))
        return owner[:body_capacity], seam[:body_capacity], n.value

    def resident_kernel(self):
        """(kernel, rounds) of the resident islands in the last step; see s2amd_get_resident_kernel."""
        kernel, rounds = ctypes.c_int32(), ctypes.c_int32()
        self._ck(self._L.s2amd_get_resident_kernel(self._h, ctypes.byref(kernel), ctypes.byref(rounds)))
        return kernel.value, rounds.value

    def joint_order(self):
        return self._order(self._L.s2amd_get_joint_order)

    def synchronize(self):
        """Waits for the steps enqueued under option "async" and raises a deferred device error."""
        self._ck(self._L.s2amd_synchronize(self._h))

    def stats(self):
        st = wire.StepStats()
        self._ck(self._L.s2amd_get_stats(self._h, ctypes.byref(st)))
        return {k: getattr(st, k) for k, _ in wire.StepStats._fields_}


class _BorrowedSolver(Solver):
    """A shard's s2amdSolver as a Solver object (orders, stats, options): owned by the ShardedSolver, never destroyed from here."""

    def __init__(self, L, handle):
        self._L, self._h, self.fast = L, ctypes.c_void_p(handle), False

    def close(self):
        self._h = None


class ShardedSolver:
    """include/solver2d_amd.h: s2amd_sharded_* -- one process, one shard per entry of `devices` (HIP ordinals; the same ordinal more
    than once = logical shards on one GPU).  The world's islands are found on the device and bin-packed onto the shards; a step is every
    shard's s2Solve_* plus ONE exchange of the owned body records between the devices.  Arrays as for Solver."""

    def __init__(self, devices, fast=False):
        L = load(fast=fast)
        devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
        h = ctypes.c_void_p()
        _check(L.s2amd_sharded_create(devs, len(devices), ctypes.byref(h)), L)
        self._L, self._h = L, h
        self.shards = len(devices)
        self.body_capacity = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.s2amd_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        _check(rc, self._L)

    def shard(self, i):
        """The Solver of shard i (borrowed: queries and options only)."""
        h = self._L.s2amd_sharded_solver(self._h, int(i))
        if not h:
            raise S2AmdError("no shard %d" % i)
        return _BorrowedSolver(self._L, h)

    def upload(self, bodies, contacts, joints):
        self._ck(self._L.s2amd_sharded_upload(self._h, *Solver._args(bodies, contacts, joints)))
        self.body_capacity = len(bodies)

    def step(self, params):
        self._ck(self._L.s2amd_sharded_step(self._h, ctypes.byref(params)))

    def step_async(self, params):
        """The step enqueued on the shards' streams, nothing waited for (wait() collects)."""
        self._ck(self._L.s2amd_sharded_step_async(self._h, ctypes.byref(params)))

    def wait(self):
        self._ck(self._L.s2amd_sharded_wait(self._h))

    def step_ops(self):
        """(stream operations the last step enqueued, host waits since, exchange form: 0 stores / 1 rccl / 2 peer copies)"""
        ops, waits, ex = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._ck(self._L.s2amd_sharded_get_step_ops(self._h, ctypes.byref(ops), ctypes.byref(waits), ctypes.byref(ex)))
        return ops.value, waits.value, ex.value

    def download(self, bodies, contacts, joints):
        self._ck(self._L.s2amd_sharded_download(self._h, *Solver._args(bodies, contacts, joints)))
        return bodies, contacts, joints

    def read_bodies(self, shard=0):
        """float32[bodies, 8] {position, rot, linearVelocity, angularVelocity, 0} of the WHOLE world as shard `shard`'s device holds it."""
        out = np.zeros((self.body_capacity, 8), dtype=np.float32)
        self._ck(self._L.s2amd_sharded_read_bodies(self._h, int(shard), wire.as_ptr(out.reshape(-1)), self.body_capacity))
        return out

    def reshard(self, contacts=None, joints=None):
        for arr, dt in ((contacts, wire.contact_dtype), (joints, wire.joint_dtype)):
            if arr is not None and (arr.dtype != dt or not arr.flags["C_CONTIGUOUS"]):
                raise ValueError("array must be a contiguous %s array" % (dt.names,))
        self._ck(self._L.s2amd_sharded_reshard(self._h, wire.as_ptr(contacts) if contacts is not None else None, len(contacts) if contacts is not None else 0,
                                               wire.as_ptr(joints) if joints is not None else None, len(joints) if joints is not None else 0))

    def partition(self):
        """(shard_of_body int32[bodies] (-1: owned by nobody), island_count, reshards so far)"""
        out = np.full(max(self.body_capacity, 1), -1, dtype=np.int32)
        n, r = ctypes.c_int32(), ctypes.c_int32()
        self._ck(self._L.s2amd_sharded_get_partition(self._h, out.ctypes.data, len(out), ctypes.byref(n), ctypes.byref(r)))
        return out[: self.body_capacity], n.value, r.value

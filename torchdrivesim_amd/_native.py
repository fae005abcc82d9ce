"""
ctypes binding of libtdship.so (C ABI: include/tdship.h).  The library is built in-tree by
``torchdrivesim_amd/csrc/Makefile`` (``python -c "import __graft_entry__ as g; g.build()"``).

There is deliberately NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
"""
import contextlib
import ctypes
import enum
import functools
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libtdship.so')
#: the same sources built with -DTDS_TESTING: the product plus the hooks of the header's "testing hooks" section (tools/, tests/ only)
TESTING_LIB_PATH = os.path.join(_HERE, 'lib', 'libtdship_testing.so')
CSRC = os.path.join(_HERE, 'csrc')

METRIC_IOU, METRIC_DISCS = 0, 1
OUT_F32, OUT_U8 = 0, 1
OUT_MASK_U8, OUT_MASK_BITS = 2, 3     # semantic masks (tds_raster_scene_masks): 0 / 1 bytes, packed bits
RASTER_NO_TRIM = 1
RASTER_REWRITE_ALL = 2
RASTER_HAS_CAMERA_PREP = 4
RASTER_NO_SMALL_FACES = 8
RASTER_HAS_HELPER_STREAM = 16


class RasterDebug(enum.IntFlag):
    """the flags of tds_raster_set_debug (testing build): TDS_RASTER_DBG_* of include/tdship.h"""
    NO_STATIC = 1
    NO_ACTORS = 2
    NO_STORE = 4
    NO_EDGES = 8
    NO_SCAN = 16
    NO_BINNED = 32
    NO_BITS = 64
    STATS = 128
    NO_EDGE_WALK = 256
    NO_SETUP = 512
    NO_PROJECT = 1024
    MINWG3 = 2048
    XCD_CLOCKS = 4096
    NO_SPLIT = 8192
    SPLIT = 16384
    NO_SHORT_PATH = 32768
    GRID8 = 65536
    GRID4 = 131072
    WHOLE_4WAVES = 262144
    NO_8WAVES = 524288
    WIDEST_STRIPS = 1048576
    NO_EXTRA_STRIP = 2097152
    PROLOGUE_TWICE = 4194304
    DROP_SMALL = 8388608
    SMALL_FREE_SLOPES = 16777216
    SMALL_NO_MIDDLE_ROW = 33554432
    HELPER = 67108864
    NO_ACTOR_WAVE = 134217728

_lib = None


class RasterAux(ctypes.Structure):
    """tds_raster_aux_t (include/tdship.h): optional outputs of tds_raster_scene for a later backward pass"""
    _fields_ = [('index_slices', ctypes.c_void_p), ('index_slices_bytes', ctypes.c_int64), ('keys', ctypes.c_uint32 * 16),
                ('n_keys', ctypes.c_int32), ('index_bits', ctypes.c_int32), ('flags', ctypes.c_int32), ('coverage_maintained', ctypes.c_int32),
                ('coverage', ctypes.c_void_p), ('coverage_bytes', ctypes.c_int64)]


class RasterAuxPrep(RasterAux):
    """tds_raster_aux_t with the two fields appended to it for the table of prepared scan set-ups; the library reads them only when `flags` has
    RASTER_HAS_CAMERA_PREP, so the shorter RasterAux stays a valid argument"""
    _fields_ = [('camera_prep', ctypes.c_void_p), ('camera_prep_bytes', ctypes.c_int64)]


class RasterAuxHelper(RasterAuxPrep):
    """tds_raster_aux_helper_t: tds_raster_aux_t and, behind it, the two fields of the helper launch -- the stream whose CUs the persistent launch may
    use as well (in) and the workgroups of the second enqueue (out, 0: none was made); read and written only when `flags` has
    RASTER_HAS_HELPER_STREAM"""
    _fields_ = [('helper_stream', ctypes.c_void_p), ('helper_workgroups', ctypes.c_int64)]


# One declaration per entry point of include/tdship.h, its parameters under the header's names (tests/test_abi.py holds the table to the header).
# Kinds: f32* f64* u8* i32* i64* = device pointer to such elements (a dense CUDA tensor of that dtype), void* = device pointer to what the call says,
# host* = pointer into host memory (arrays, structs, out-parameters), handle = an object of the library, stream = the hipStream_t; else C scalars.
_ABI = '''
tds_version()
tds_last_error(host* buf, size_t n)
tds_bicycle_step_f32(f32* state, f32* action, f32* lr, f32* out, int64 n, float dt, float max_acc, float max_steer, int left_handed, int no_reversing, stream stream)
tds_bicycle_step_bwd_f32(f32* state, f32* action, f32* lr, f32* grad_out, f32* grad_state, f32* grad_action, f32* grad_lr, int64 n, float dt, float max_acc, float max_steer,
    int left_handed, int no_reversing, stream stream)
tds_simple_step_f32(f32* state, f32* action, f32* out, int64 n, float dt, host* norm, int oriented, stream stream)
tds_simple_step_bwd_f32(f32* state, f32* action, f32* grad_out, f32* grad_state, f32* grad_action, int64 n, float dt, host* norm, int oriented, stream stream)
tds_unicycle_step_f32(f32* state, f32* action, f32* out, int64 n, float dt, float max_acc, float max_yaw_rate, stream stream)
tds_unicycle_step_bwd_f32(f32* state, f32* action, f32* grad_out, f32* grad_state, f32* grad_action, int64 n, float dt, float max_acc, float max_yaw_rate, stream stream)
tds_collision_f32(f32* boxes, f32* sc, u8* present, f32* out, i64* overlap, i32* partner, int64 B, int64 A, int64 N, int metric, stream stream)
tds_collision_bwd_f32(f32* boxes, f32* sc, u8* present, f32* grad_out, f32* grad_boxes, f32* grad_sc, int64 B, int64 A, int64 N, int metric, stream stream)
tds_overlap_count_f32(f32* boxes, f32* sc, u8* present, f64* out, int64 B, int64 A, stream stream)
tds_pairwise_overlap_f32(f32* box1, f32* sc1, f32* box2, f32* sc2, f32* out, int64 n, int metric, stream stream)
tds_pairwise_discs_f32(f32* box1, f32* sc1, f32* box2, f32* sc2, f32* out, int64 n, int num_discs, stream stream)
tds_box2corners_f32(f32* box, f32* sc, f32* corners, int64 n, stream stream)
tds_occlusion_mask_f32(f32* state, f32* size, u8* present, u8* out, int64 B, int64 A, int64 E, stream stream)
tds_map_create(host* verts, host* faces, host* face_z, host* face_rgb, int64 V, int64 F, host* levels, int n_levels, float cell_size, host* out)
tds_map_destroy(handle map)
tds_map_info(handle map, host* info)
tds_map_info_ex(handle map, host* info, int n_words)
tds_map_keys(handle map, host* keys, int cap, host* n)
tds_mapset_create(host* maps, int n, host* out)
tds_mapset_destroy(handle set)
tds_mapset_keys(handle set, host* keys, int cap, host* n)
tds_rows_hash_u64(void* rows, int64 n_rows, int64 row_bytes, int64 row_stride_bytes, uint64 seed, i64* out, stream stream)
tds_rows_equal_u8(void* rows, int64 n_rows, int64 row_bytes, int64 row_stride_bytes, i32* rep, u8* equal, stream stream)
tds_offroad_f32(handle map, f32* state, f32* lenwid, f32* sc, u8* present, f32* out, int64 n_agents, float threshold, stream stream)
tds_offroad_bwd_f32(handle map, f32* state, f32* lenwid, f32* sc, u8* present, f32* grad_out, f32* grad_state, f32* grad_lenwid, f32* grad_sc, int64 n_agents, float threshold,
    stream stream)
tds_offroad_multi_f32(handle set, i32* scene_map, int64 agents_per_scene, f32* state, f32* lenwid, f32* sc, u8* present, f32* out, int64 n_agents, float threshold,
    stream stream)
tds_offroad_multi_bwd_f32(handle set, i32* scene_map, int64 agents_per_scene, f32* state, f32* lenwid, f32* sc, u8* present, f32* grad_out, f32* grad_state, f32* grad_lenwid,
    f32* grad_sc, int64 n_agents, float threshold, stream stream)
tds_raster_index_slices_bytes(int64 n_img, int res, host* bytes)
tds_raster_coverage_bytes(int64 n_img, int res, host* bytes)
tds_raster_camera_prep_bytes(int64 n_img, int res, int out_mode, int n_keys, host* bytes)
tds_raster_scene(handle map, f32* state, f32* agent_sc, f32* tmpl, i32* actor_key, u8* mask, f32* cam_xy, f32* cam_sc, int64 B, int64 Nc, int64 N, float scale, int res,
    int out_mode, void* out, void* workspace, int64 workspace_bytes, host* actor_keys, int n_actor_keys, int actor_key_per_camera, f32* extra_tri, i32* extra_key,
    int64 n_extra, host* aux, stream stream)
tds_raster_scene_multi(handle set, i32* scene_map, f32* state, f32* agent_sc, f32* tmpl, i32* actor_key, u8* mask, f32* cam_xy, f32* cam_sc, int64 B, int64 Nc, int64 N,
    float scale, int res, int out_mode, void* out, void* workspace, int64 workspace_bytes, host* actor_keys, int n_actor_keys, int actor_key_per_camera, f32* extra_tri,
    i32* extra_key, int64 n_extra, host* aux, stream stream)
tds_raster_scene_masks(handle map, f32* state, f32* agent_sc, f32* tmpl, i32* actor_key, u8* mask, f32* cam_xy, f32* cam_sc, int64 B, int64 Nc, int64 N, float scale, int res,
    int out_mode, void* out, void* workspace, int64 workspace_bytes, host* actor_keys, int n_actor_keys, f32* extra_tri, i32* extra_key, int64 n_extra, host* key_channels,
    int n_channels, host* aux, stream stream)
tds_raster_scene_masks_multi(handle set, i32* scene_map, f32* state, f32* agent_sc, f32* tmpl, i32* actor_key, u8* mask, f32* cam_xy, f32* cam_sc, int64 B, int64 Nc, int64 N,
    float scale, int res, int out_mode, void* out, void* workspace, int64 workspace_bytes, host* actor_keys, int n_actor_keys, f32* extra_tri, i32* extra_key, int64 n_extra,
    host* key_channels, int n_channels, host* aux, stream stream)
tds_raster_scene_workspace_bytes(int64 n_img, int res, host* bytes)
tds_raster_scene_workspace_bytes_for(int64 n_img, int res, int out_mode, int n_keys, host* bytes)
tds_buffer_create(int64 bytes, int device, int flags, host* out)
tds_buffer_ptr(handle buf)
tds_buffer_info(handle buf, host* bytes, host* chunks, host* spread)
tds_buffer_destroy(handle buf)
tds_torch_alloc(size_t size, int device, stream stream)
tds_torch_free(void* ptr, size_t size, int device, stream stream)
tds_stream_create(int device, host* cu_mask, int n_words, host* stream)
tds_stream_destroy(int device, handle stream)
tds_device_cu_count(int device, host* cus)
tds_stream_places(stream stream, i32* places, int n)
tds_raster_scene_bwd_f32(f32* state, f32* agent_sc, f32* tmpl, u8* mask, f32* cam_xy, f32* cam_sc, f32* image, f32* grad_out, int64 B, int64 Nc, int64 N, float scale, int res,
    f32* grad_agent, f32* grad_cam, f32* grad_tmpl, stream stream)
tds_raster_scene_bwd_idx_f32(f32* state, f32* agent_sc, f32* tmpl, u8* mask, f32* cam_xy, f32* cam_sc, i32* index_slices, host* keys, int n_keys, f32* grad_out,
    int64 grad_out_stride, int64 B, int64 Nc, int64 N, float scale, int res, f32* grad_agent, f32* grad_cam, f32* grad_color, f32* grad_tmpl, stream stream)
tds_raster_mesh(f32* verts, f32* attrs, i32* faces, int64 n_img, int64 V, int64 F, f32* cam_xy, f32* cam_sc, host* levels, int n_levels, float scale, int res, int out_mode,
    void* out, int flags, stream stream)
tds_lanelet_centerline_f64(host* left, int n_left, host* right, int n_right, host* out, host* n_out)
tds_lanes_create(host* poly_xy, host* poly_start, host* cl_xyz, host* cl_start, host* flags, int n_lanelets, float cell_size, float max_tolerance, host* out)
tds_lanes_destroy(handle lanes)
tds_lanes_info(handle lanes, host* info)
tds_laneset_create(host* lanes, int n, host* out)
tds_laneset_destroy(handle set)
tds_wrong_way_f32(handle set, i32* scene_map, int64 agents_per_scene, f32* state, f32* recenter_offset, u8* present, f32* out, int64 n_agents, float direction_angle_threshold,
    float lanelet_dist_tolerance, stream stream)
tds_wrong_way_grad_f32(handle set, i32* scene_map, int64 agents_per_scene, f32* state, f32* recenter_offset, u8* present, f32* out, f32* dloss_dpsi, int64 n_agents,
    float direction_angle_threshold, float lanelet_dist_tolerance, stream stream)
tds_lanelet_directions_f64(handle set, i32* scene_map, int64 points_per_scene, f64* xy, f64* dirs, f64* dists, i32* count, u8* status, int max_dirs, int64 n_points,
    float lanelet_dist_tolerance, stream stream)
tds_spawn_on_lanes_f32(handle set, i32* scene_map, i64* scene_ids, int64 n_scenes, int agents_per_scene, f32* attributes, f32* occupied, f32* occupied_sc, u8* occupied_mask,
    int n_occupied, uint64 seed, float min_speed, float max_speed, float gap_long, float gap_lat, int max_attempts, f32* state, f32* sc, u8* placed, i32* attempts,
    stream stream)
tds_lanes_set_successors(handle lanes, host* succ_start, host* succ_items)
tds_lane_snap(handle lanes, f32* xy, f32* sc, i32* lane, f64* arc, f32* lateral, int64 n_poses, float tolerance, stream stream)
tds_lane_snap_multi(handle set, i32* scene_map, int64 poses_per_scene, f32* xy, f32* sc, i32* lane, f64* arc, f32* lateral, int64 n_poses, float tolerance, stream stream)
tds_lane_follow_step(handle lanes, i64* scene_ids, int64 B, int64 N, int64 E, f32* boxes, f32* ent_sc, f32* ent_speed, u8* ent_present, i32* self_index, f32* npc_size,
    f32* desired_speed, u8* npc_present, i32* lane, f64* arc, i32* hops, f32* state, f32* sc, i32* leader, uint64 seed, float dt, float horizon, float lateral_margin,
    host* idm, stream stream)
tds_lane_follow_step_multi(handle set, i32* scene_map, i64* scene_ids, int64 B, int64 N, int64 E, f32* boxes, f32* ent_sc, f32* ent_speed, u8* ent_present, i32* self_index,
    f32* npc_size, f32* desired_speed, u8* npc_present, i32* lane, f64* arc, i32* hops, f32* state, f32* sc, i32* leader, uint64 seed, float dt, float horizon,
    float lateral_margin, host* idm, stream stream)
tds_lane_conflicts_f64(handle lanes, f64* table, float clearance, float step, stream stream)
tds_lane_give_way_multi(handle set, i32* scene_map, i64* scene_ids, i64* tables, int64 B, int64 N, i32* lane, f64* arc, i32* hops, f32* state, f32* npc_size, u8* npc_present,
    int64 S, i32* line_lane, f64* line_arc, u8* line_red, uint64 seed, float horizon, float b_max, float creep_speed, f64* stop_at, i32* yield_to, stream stream)
tds_lane_follow_step_stops_multi(handle set, i32* scene_map, i64* scene_ids, int64 B, int64 N, int64 E, f32* boxes, f32* ent_sc, f32* ent_speed, u8* ent_present,
    i32* self_index, f32* npc_size, f32* desired_speed, u8* npc_present, i32* lane, f64* arc, i32* hops, f32* state, f32* sc, i32* leader, f64* stop_at, uint64 seed,
    float dt, float horizon, float lateral_margin, host* idm, stream stream)
tds_route_sample_multi(handle set, i32* scene_map, i64* scene_ids, int64 B, int64 A, i32* lane, f64* arc, f64* distance, u8* present, u8* mask, uint64 seed, i32* route_lanes,
    i32* route_n, f64* start_arc, f64* end_arc, f64* offsets, f64* length, i32* cursor, f64* stored, u8* completed, stream stream)
tds_route_progress_multi(handle set, i32* scene_map, int64 B, int64 A, f32* xy, int64 xy_stride, f32* sc, u8* present, i32* route_lanes, i32* route_n, f64* start_arc,
    f64* end_arc, f64* offsets, f64* length, i32* cursor, f64* stored, u8* completed, float goal_tolerance, float off_route_distance, int n_lookahead, float spacing,
    f32* progress, f32* advance, f32* lateral, f32* heading, f32* remaining, u8* reached, u8* off_route, f32* lookahead, stream stream)
tds_route_progress_bwd_multi(handle set, i32* scene_map, int64 B, int64 A, f32* xy, int64 xy_stride, f32* sc, u8* present, i32* route_lanes, i32* route_n, f64* start_arc,
    f64* end_arc, f64* offsets, f64* length, i32* piece, f32* g_progress, f32* g_advance, f32* g_lateral, f32* g_heading, f32* g_remaining, f32* g_lookahead, int n_lookahead,
    float spacing, f32* g_xy, f32* g_sc, stream stream)
tds_route_points_multi(handle set, i32* scene_map, int64 B, int64 A, int64 Q, i32* route_lanes, i32* route_n, f64* start_arc, f64* end_arc, f64* offsets, f64* length, f64* q,
    f32* points, stream stream)
tds_lane_distances_f64(handle lanes, f64* to_go, stream stream)
tds_route_to_multi(handle set, i32* scene_map, i64* tables, int64 B, int64 A, i32* lane, f64* arc, i32* dest_lane, f64* dest_arc, u8* present, u8* mask, i32* route_lanes,
    i32* route_n, f64* start_arc, f64* end_arc, f64* offsets, f64* length, i32* cursor, f64* stored, u8* completed, f64* rest, stream stream)
tds_range_scan_f32(handle map, f32* boxes, f32* sc, u8* present, f32* ray_sc, f32* agent_range, f32* road_range, i32* hit, int64 B, int64 A, int64 E, int R, float max_range,
    float gap_tolerance, stream stream)
tds_range_scan_multi_f32(handle set, i32* scene_map, f32* boxes, f32* sc, u8* present, f32* ray_sc, f32* agent_range, f32* road_range, i32* hit, int64 B, int64 A, int64 E,
    int R, float max_range, float gap_tolerance, stream stream)
tds_range_scan_bwd_f32(handle map, f32* boxes, f32* sc, u8* present, f32* ray_sc, f32* road_range, f32* g_agent, f32* g_road, f32* g_boxes, f32* g_sc, f32* g_ray_sc,
    i32* choice, f32* road_edge, int64 B, int64 A, int64 E, int R, float max_range, float gap_tolerance, stream stream)
tds_range_scan_bwd_multi_f32(handle set, i32* scene_map, f32* boxes, f32* sc, u8* present, f32* ray_sc, f32* road_range, f32* g_agent, f32* g_road, f32* g_boxes, f32* g_sc,
    f32* g_ray_sc, i32* choice, f32* road_edge, int64 B, int64 A, int64 E, int R, float max_range, float gap_tolerance, stream stream)
tds_neighbors_f32(f32* boxes, f32* sc, f32* speed, u8* present, u8* visible, f32* features, i32* index, int64 B, int64 A, int64 E, int K, float max_distance, stream stream)
tds_neighbors_bwd_f32(f32* boxes, f32* sc, f32* speed, i32* index, f32* g_features, f32* g_boxes, f32* g_sc, f32* g_speed, int64 B, int64 A, int64 E, int K, stream stream)
tds_lights_step(f64* duration, i32* next_phase, i32* n_phases, u8* colour, i32* phase, f64* remaining, i64* state, f32* time_to_change, u8* mask, int64 B, int64 M, int64 P,
    int64 N, host* dt, int advance, stream stream)
tds_lights_reset(i32* n_phases, f64* duration, i32* phase, f64* remaining, u8* mask, i64* scene_ids, int64 B, int64 M, int64 P, uint64 seed, stream stream)
tds_stop_lines_f32(f32* agent_xy, f32* agent_sc, u8* agent_present, f32* lines, f32* line_sc, u8* mask, i64* state, f32* time_to_change, f32* features, i32* index,
    i32* slot_state, int64 B, int64 A, int64 N, int K, float max_distance, int ahead_only, float min_cos, stream stream)
tds_stop_lines_bwd_f32(f32* agent_xy, f32* agent_sc, f32* lines, f32* line_sc, i32* index, f32* g_features, f32* g_xy, f32* g_sc, int64 B, int64 A, int64 N, int K,
    stream stream)
tds_lane_observations_multi(handle set, i32* scene_map, f32* agent_xy, f32* agent_sc, u8* present, f32* features, f32* points, i32* n_valid, i32* index, int64 B, int64 A,
    int K, int P, float spacing, float max_distance, stream stream)
tds_lane_observations_bwd_multi(handle set, i32* scene_map, f32* agent_xy, f32* agent_sc, i32* index, f32* g_features, f32* g_points, f32* g_xy, f32* g_sc, int64 B, int64 A,
    int K, int P, float spacing, stream stream)
tds_time_to_collision_f32(f32* boxes, f32* sc, f32* speed, u8* present, u8* visible, f32* ttc, i32* index, int64 B, int64 A, int64 E, int K, float horizon,
    float margin, stream stream)
tds_time_to_collision_bwd_f32(f32* boxes, f32* sc, f32* speed, i32* index, f32* g_ttc, f32* g_boxes, f32* g_sc, f32* g_speed, int64 B, int64 A, int64 E, int K,
    float margin, stream stream)
'''

#: entry points that only libtdship_testing.so exports (include/tdship.h, "testing hooks")
_TESTING_ABI = '''
tds_raster_set_strip_width(int tw)
tds_raster_set_bits_waves(int n)
tds_raster_set_list_lds(int lds_kb)
tds_raster_set_list_waves(int waves)
tds_raster_set_debug(int flags)
tds_raster_set_helper_min_items(int items_per_workgroup)
tds_raster_get_helper_stats(host* out1)
tds_raster_get_actor_wave_stats(host* out1)
tds_raster_get_stats(host* out16)
tds_raster_get_prep_stats(host* out2)
tds_raster_get_small_stats(host* out16)
tds_raster_plan(int64 n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices, int64 workspace_bytes, int cus, int force_tw,
    int bits_waves, int list_waves, int list_lds_kb, int debug, host* out)
tds_raster_plan_small_lane(int64 n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices, int64 workspace_bytes, int cus,
    int force_tw, int bits_waves, int list_waves, int list_lds_kb, int debug, int small_faces, host* small_lane)
tds_testing_set_near_lists(int enabled)
tds_stop_lines_bwd_set_row_lanes(int lanes)
'''

ELEMENTS = {'f32*': torch.float32, 'f64*': torch.float64, 'u8*': torch.uint8, 'i32*': torch.int32, 'i64*': torch.int64, 'void*': None}
SCALARS = {'int': ctypes.c_int, 'int64': ctypes.c_int64, 'uint64': ctypes.c_uint64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _parse(abi):
    """name -> [(kind, parameter name), ...]"""
    decls = {name: [tuple(p.split()) for p in params.split(',') if p.strip()] for name, params in re.findall(r'(\w+)\((.*?)\)', abi, flags=re.S)}
    assert all(k in ELEMENTS or k in SCALARS or k in ('host*', 'handle', 'stream') for d in decls.values() for k, _ in d)
    return decls


DECLARATIONS, TESTING_DECLARATIONS = _parse(_ABI), _parse(_TESTING_ABI)
# name -> argtypes: every pointer kind is a void *
_SIGNATURES = {name: [SCALARS.get(k, ctypes.c_void_p) for k, _ in d] for name, d in DECLARATIONS.items()}
_TESTING_SIGNATURES = {name: [SCALARS.get(k, ctypes.c_void_p) for k, _ in d] for name, d in TESTING_DECLARATIONS.items()}
#: entry points that do not return an error code
_RESTYPES = {'tds_buffer_ptr': ctypes.c_void_p, 'tds_torch_alloc': ctypes.c_void_p, 'tds_torch_free': None}


def build(force=False):
    """Compile every HIP source for gfx950 into torchdrivesim_amd/lib/libtdship.so (hipcc cross-compiles without a GPU)."""
    cmd = ['make', '-C', CSRC, '-j', str(min(8, os.cpu_count() or 1))]
    if force:
        cmd.append('-B')
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _load(path, signatures):
    if not os.path.exists(path):
        raise RuntimeError(
            f'{path} is missing: the HIP extension has not been built. Run '
            '`python -c "import __graft_entry__ as g; g.build()"` (needs hipcc). There is no CPU fallback.')
    try:
        L = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError(f'cannot load {path}: {e}') from e
    for name, argtypes in signatures.items():
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    return L


def lib():
    global _lib
    if _lib is None:
        _lib = _load(LIB_PATH, _SIGNATURES)
    return _lib


_testing_lib = None


def testing_lib():
    """libtdship_testing.so (tools/ and tests/ only; the product never loads it)"""
    global _testing_lib
    if _testing_lib is None:
        _testing_lib = _load(TESTING_LIB_PATH, {**_SIGNATURES, **_TESTING_SIGNATURES})
    return _testing_lib


@contextlib.contextmanager
def testing():
    """Route every call of this process through the testing build for the duration of the block (handles created inside must be
    used and dropped inside: the two libraries are separate images).  Yields the testing library for its hooks."""
    global _lib
    saved, _lib = _lib, testing_lib()
    try:
        yield _lib
    finally:
        _lib = saved


def last_error():
    buf = ctypes.create_string_buffer(512)
    lib().tds_last_error(buf, 512)
    return buf.value.decode(errors='replace')


E_INVAL, E_HIP, E_NOMEM, E_LIMIT = -1, -2, -3, -4          # TDS_EINVAL, TDS_EHIP, TDS_ENOMEM, TDS_ELIMIT of include/tdship.h
BUFFER_DENSE = 1
SPAWN_MAX_BOXES = 2048           # TDS_SPAWN_MAX_BOXES
FOLLOW_MAX_HOPS, FOLLOW_MAX_ENTITIES = 8, 1024       # TDS_FOLLOW_MAX_HOPS, TDS_FOLLOW_MAX_ENTITIES
CONFLICT_MAX_LANELETS, GIVE_WAY_MAX_NPCS = 2048, 1024    # TDS_CONFLICT_MAX_LANELETS, TDS_GIVE_WAY_MAX_NPCS
ROUTE_MAX_LANES, ROUTE_MAX_LOOKAHEAD = 16, 32       # TDS_ROUTE_MAX_LANES, TDS_ROUTE_MAX_LOOKAHEAD
ROUTE_MAX_GRAPH = 2048                               # TDS_ROUTE_MAX_GRAPH
NEIGHBORS_MAX_K, NEIGHBORS_MAX_ENTITIES = 32, 1024   # TDS_NEIGHBORS_MAX_K, TDS_NEIGHBORS_MAX_ENTITIES
LIGHTS_MAX_MACHINES, LIGHTS_MAX_PHASES, LIGHTS_MAX_LIGHTS = 256, 64, 1024      # TDS_LIGHTS_MAX_MACHINES, TDS_LIGHTS_MAX_PHASES, TDS_LIGHTS_MAX_LIGHTS
LIGHTS_MAX_SKIPS, STOP_LINES_MAX_K = 1024, 32        # TDS_LIGHTS_MAX_SKIPS, TDS_STOP_LINES_MAX_K
LANE_OBS_MAX_K, LANE_OBS_MAX_POINTS = 32, 32         # TDS_LANE_OBS_MAX_K, TDS_LANE_OBS_MAX_POINTS
LANE_OBS_MAX_HOPS, LANE_OBS_MAX_LANELETS = 8, 2048   # TDS_LANE_OBS_MAX_HOPS, TDS_LANE_OBS_MAX_LANELETS
TTC_MAX_K, TTC_MAX_ENTITIES = 32, 1024               # TDS_TTC_MAX_K, TDS_TTC_MAX_ENTITIES


class TdsError(RuntimeError):
    """A C-ABI entry point returned a negative code (`.code`; the message is tds_last_error's).  A RuntimeError, the type the reference
    handles around rendering (rendering/base.py:190-201)."""

    def __init__(self, what, code, message):
        super().__init__(f'{what} failed (code {code}): {message}')
        self.code = code


def check(rc, what):
    if rc != 0:
        raise TdsError(what, rc, last_error())


def stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@functools.lru_cache(maxsize=None)
def _device_pointer(dtype, name):
    """what `call` does to the argument of a device-pointer parameter: a tensor is refused unless the kernels can read it as it is (dtype None:
    any element type) and becomes its address; None, numbers and ctypes values pass through"""
    def convert(t):
        if not isinstance(t, torch.Tensor):
            return t
        if not t.is_cuda:
            raise RuntimeError(f'{name}: torchdrivesim_amd kernels run on an MI355X; got a {t.device} tensor (no CPU fallback)')
        if dtype is not None and t.dtype != dtype:
            raise RuntimeError(f'{name}: expected {dtype}, got {t.dtype}')
        if not t.is_contiguous():
            raise RuntimeError(f'{name}: tensor must be contiguous')
        return ctypes.c_void_p(t.data_ptr())
    return convert


def dev_ptr(t, dtype, name):
    """Device pointer of a dense tensor; refuses anything the kernels cannot read as-is."""
    return _device_pointer(dtype, name)(t)


def _stream_arg(s):
    return s.cuda_stream if isinstance(s, torch.cuda.Stream) else s


# name -> (one converter per parameter -- None: the argument is passed on as it is --, whether the last parameter is the launch stream)
_MARSHAL = {name: (tuple(_stream_arg if k == 'stream' else _device_pointer(ELEMENTS[k], p) if k in ELEMENTS else None for k, p in d),
                   bool(d) and d[-1][0] == 'stream') for name, d in {**DECLARATIONS, **TESTING_DECLARATIONS}.items()}


def call(name, device, *args):
    """Run a C-ABI entry point with `device` current, its arguments converted as the declaration says.  A launch stream that is the last
    parameter may be left out: torch's current stream of `device` (a stream that is given must belong to `device`)."""
    convert, stream_last = _MARSHAL[name]
    missing = len(convert) - len(args)
    if missing and not (missing == 1 and stream_last):
        raise TypeError(f'{name} takes {len(convert)} arguments, got {len(args)}')
    args = [a if c is None else c(a) for c, a in zip(convert, args)]
    if missing:
        args.append(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        rc = getattr(lib(), name)(*args)
    check(rc, name)

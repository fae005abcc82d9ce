/*
 * tdship.h -- C ABI of libtdship.so, the MI355X (gfx950) implementation of the torchdrivesim hot path.
 *
 * The reference (inverted-ai/torchdrivesim v0.2.3) is pure Python on torch and has no FFI of its own; each
 * entry point below names the reference function whose inner loop it replaces (file:line into the reference
 * checkout).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (torch tensors, `.data_ptr()`), except
 *     in tds_map_create / tds_grid_*(), which take HOST arrays (map preparation happens once per map);
 *   - tensors are dense, row-major, fp32 / int32 / uint8 as stated; shapes are given in comments;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); kernels are enqueued on it and the call
 *     returns without synchronising; calls are re-entrant per device;
 *   - return value: 0 on success, a negative TDS_E* code otherwise (never throws); tds_last_error() returns the
 *     message for the calling thread.  The Python host raises RuntimeError on any non-zero code, so
 *     BirdviewRenderer.render_frame's `except RuntimeError` (rendering/base.py:190-201) still applies;
 *   - sin/cos of agent and camera headings are INPUTS ([sin, cos] pairs), computed by the caller with torch on the
 *     same device, exactly where the reference calls torch.sin/torch.cos (simulator.py:940, utils.py:40-53,
 *     _iou_utils.py:290-291); all remaining arithmetic is IEEE-754 binary32 with one rounding per operation in the
 *     reference's order (no FMA contraction) so integer / boolean outputs can be compared bit for bit.
 */
#ifndef TDSHIP_H
#define TDSHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDS_ABI_VERSION 1

#define TDS_OK 0
#define TDS_EINVAL (-1)     /* bad argument (null pointer, negative size, unsupported resolution ...) */
#define TDS_EHIP (-2)       /* a HIP runtime call or kernel launch failed */
#define TDS_ENOMEM (-3)
#define TDS_ELIMIT (-4)     /* a documented capacity was exceeded (e.g. more than 255 rendering levels) */

int tds_version(void);
/* copies the calling thread's last error message (NUL terminated) into buf; returns its length */
int tds_last_error(char *buf, size_t n);

/* ------------------------------------------------------------------------------------------------------------
 * K1  kinematic models                                                                   kinematic.py:328-523
 * state / out: n x 4 [x, y, psi, v]  (n = B*A agents);  `out` must not alias `state` (the reference replaces the
 * state tensor, it never mutates it: kinematic.py:477, pack_state = torch.stack).
 * ---------------------------------------------------------------------------------------------------------- */

/* KinematicBicycle.step (kinematic.py:462-477) and BicycleNoReversing.step (:513-523, no_reversing != 0).
 * action: n x 2 normalised [acceleration, steering];  lr: n. */
int tds_bicycle_step_f32(const float *state, const float *action, const float *lr, float *out, int64_t n,
                         float dt, float max_acc, float max_steer, int left_handed, int no_reversing, void *stream);
/* backward of the above: grad_out n x 4 -> grad_state n x 4, grad_action n x 2, grad_lr n (any may be NULL) */
int tds_bicycle_step_bwd_f32(const float *state, const float *action, const float *lr, const float *grad_out,
                             float *grad_state, float *grad_action, float *grad_lr, int64_t n, float dt, float max_acc,
                             float max_steer, int left_handed, int no_reversing, void *stream);

/* SimpleKinematicModel.step (:362-367) / OrientedKinematicModel.step (:384-389, oriented != 0).
 * action: n x 4 normalised, norm: 4 host floats [max_dx, max_dx, max_dpsi, max_dv]. */
int tds_simple_step_f32(const float *state, const float *action, float *out, int64_t n, float dt, const float *norm,
                        int oriented, void *stream);
int tds_simple_step_bwd_f32(const float *state, const float *action, const float *grad_out, float *grad_state,
                            float *grad_action, int64_t n, float dt, const float *norm, int oriented, void *stream);

/* UnicycleModel.step -- named by the north star, absent from the reference: action n x 2 normalised
 * [acceleration, yaw rate]: v += a dt; x += v cos(psi) dt; y += v sin(psi) dt; psi += w dt. */
int tds_unicycle_step_f32(const float *state, const float *action, float *out, int64_t n, float dt, float max_acc,
                          float max_yaw_rate, void *stream);
int tds_unicycle_step_bwd_f32(const float *state, const float *action, const float *grad_out, float *grad_state,
                              float *grad_action, int64_t n, float dt, float max_acc, float max_yaw_rate, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K2a  collisions                     simulator.py:1064-1109,1161-1194; _iou_utils.py:42-367; infractions.py:378-545
 * ---------------------------------------------------------------------------------------------------------- */
#define TDS_METRIC_IOU 0
#define TDS_METRIC_DISCS 1

/* Simulator.compute_collision for all exposed agents of all scenes at once.
 *   boxes   B x N x 5  [x, y, length, width, psi]   all agents = A exposed agents followed by N-A NPCs
 *   sc      B x N x 2  [sin, cos] of the angle the metric uses: psi (iou) or psi + pi/2*(width > length) (discs)
 *   present B x N      uint8 (already restricted to the requested agent types, simulator.py:1086-1089)
 *   out     B x A      collision_i = sum_j o_ij present_j - max_j o_ij present_j   
 *   overlap B x A      uint64 bit j set iff o_ij present_j > 0, j != i   (NULL to skip; requires N <= 64)
 *   partner B x A      int32 arg-max_j!=i of o_ij present_j, -1 if none   (NULL to skip)   [new outputs, SURVEY R8]
 *                      ties: the LOWEST j != i that attains the largest o_ij present_j > 0 */
int tds_collision_f32(const float *boxes, const float *sc, const uint8_t *present, float *out, uint64_t *overlap,
                      int32_t *partner, int64_t B, int64_t A, int64_t N, int metric, void *stream);
/* backward: grad_out B x A -> grad_boxes B x N x 5 (psi column = 0), grad_sc B x N x 2; both are OVERWRITTEN */
int tds_collision_bwd_f32(const float *boxes, const float *sc, const uint8_t *present, const float *grad_out,
                          float *grad_boxes, float *grad_sc, int64_t B, int64_t A, int64_t N, int metric, void *stream);

/* The `nograd` metric (simulator.py:1111-1149 -> infractions.py:352-375, 429-500; the reference asks shapely for
 * `intersection(...).area != 0` pair by pair on the host): out B x A float64 = number of OTHER present agents whose rectangle shares
 * area with agent i's, 0 for an absent agent.  boxes B x A x 5, sc B x A x 2 = [sin psi, cos psi], present B x A uint8.  Corners as
 * infractions.rectangle_vertices in float32; the predicate (no separating edge line, touching does not count) in float64. */
int tds_overlap_count_f32(const float *boxes, const float *sc, const uint8_t *present, double *out, int64_t B, int64_t A, void *stream);

/* iou_differentiable (infractions.py:307-324) / collision_detection_with_discs (:503-545), element-wise over n pairs.
 * box1, box2: n x 5; sc1, sc2: n x 2 as above. */
int tds_pairwise_overlap_f32(const float *box1, const float *sc1, const float *box2, const float *sc2, float *out,
                             int64_t n, int metric, void *stream);

/* collision_detection_with_discs(box1, box2, num_discs) for a number of discs other than the default 5 (infractions.py:378-426,
 * 503-545): odd, 3 .. 25 (torch.cdist changes its formulation above 25 points) */
int tds_pairwise_discs_f32(const float *box1, const float *sc1, const float *box2, const float *sc2, float *out, int64_t n,
                           int num_discs, void *stream);

/* box2corners_th (_iou_utils.py:270-299): box n x 5, sc n x 2 -> corners n x 4 x 2 */
int tds_box2corners_f32(const float *box, const float *sc, float *corners, int64_t n, void *stream);

/* StandardSensingObservationNoise.get_noisy_present_mask (observation_noise.py:89-132, utils.line_circle_intersection :139-187):
 *   state B x E x 4 (exposed agents first, then NPCs), size B x E x 2, present B x E uint8
 *   out   B x A x E uint8: present[b,e] and no other entity o (o != e, o != a) whose disc of radius width/2 touches the segment
 *         from ego a to entity e */
int tds_occlusion_mask_f32(const float *state, const float *size, const uint8_t *present, uint8_t *out, int64_t B, int64_t A, int64_t E,
                           void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Static map handle: triangle mesh + uniform grid, built once per map and per device.
 * Replaces the per-call `mesh.expand(...)` / `RGBMesh.concat([background.expand(Nc), ...])` dataflow of
 * infractions.py:220-226 and mesh.py:1147-1156.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct tds_map tds_map_t;

/* HOST inputs: verts V x 2, faces F x 3 (indices into verts; padded faces [0,0,0] allowed, mesh.py:69),
 * face_z F (rendering level of the face's FIRST vertex, cv2.py:44-46), face_rgb F (colour of the first vertex already
 * quantised as cv2.py:50: 0x00RRGGBB), levels: n_levels distinct rendering levels sorted DESCENDING that contain every
 * face_z and every actor level that will be rendered with this map (<= 255).  face_z / face_rgb / levels may be NULL
 * for a map that is only used by tds_offroad_f32; such a map also gets per-cell nearest-face candidate lists (exact),
 * which make the off-road query one short linear walk, and a bounding-volume hierarchy over its faces for points beyond the lists' grid.  cell_size <= 0 selects the default (8 m).
 * The handle lives on the CURRENT HIP device. */
int tds_map_create(const float *verts, const int32_t *faces, const float *face_z, const uint32_t *face_rgb, int64_t V,
                   int64_t F, const float *levels, int n_levels, float cell_size, tds_map_t **out);
int tds_map_destroy(tds_map_t *map);
/* info[0..7] = V, F, grid nx, grid ny, number of grid entries, device bytes held, n_levels, number of nearest-face candidates
 * (EIGHT words, as in every release of this header but round 5's, which wrote ten through this symbol: see INTEGRATION.md, "ABI notes") */
int tds_map_info(const tds_map_t *map, int64_t *info);
/* the first `n_words` of: the eight words above, then [8] entries of the rendering grid (lone faces + pairs, tds_common.h: QuadEntry),
 * [9] pairs of same-key faces that share an edge; words beyond TDS_MAP_INFO_WORDS read 0 */
#define TDS_MAP_INFO_WORDS 10
int tds_map_info_ex(const tds_map_t *map, int64_t *info, int n_words);
/* the distinct face keys of the map (HOST array of `cap` entries; *n receives their number, -1 when there are more than 64): with the caller's
 * actor keys they decide which rasteriser serves a launch -- at most 15 keys in all: the bit-plane kernels -- and with it how much scratch
 * tds_raster_scene can use (tds_raster_scene_workspace_bytes_for) */
int tds_map_keys(const tds_map_t *map, uint32_t *keys, int cap, int *n);

/* Map sets: batches whose scenes have DIFFERENT meshes (the reference supports them as a collated, padded mesh batch, mesh.py:69,
 * 113-123).  A set is a device array of the views of several maps of ONE device that were created with the SAME `levels` table; the
 * maps must outlive the set.  `scene_map` (device, B int32) of the *_multi entry points says which map of the set scene b uses. */
typedef struct tds_mapset tds_mapset_t;
int tds_mapset_create(const tds_map_t *const *maps, int n, tds_mapset_t **out);
int tds_mapset_destroy(tds_mapset_t *set);
int tds_mapset_keys(const tds_mapset_t *set, uint32_t *keys, int cap, int *n);      /* tds_map_keys over the union of the set's maps */

/* Which scenes of a collated batch share a mesh.  The reference pads every element of a collated mesh batch to the largest one
 * (mesh.py:172-200 `pad`, :113-123 / :232-245 `collate`), so two scenes on the same map hold identical rows, byte for byte; it then carries
 * B private copies through every batch operation (simulator.py:444-511).  These two let the host group the B rows of a DEVICE tensor by content
 * without a copy to the host, so that it builds one tds_map_t per DISTINCT mesh:
 *   tds_rows_hash_u64   out[r] = 64-bit content hash of row r (rows of `row_bytes` bytes -- a multiple of 4 -- `row_stride_bytes` apart);
 *                       `seed` selects the hash function (two seeds: 128 bits);
 *   tds_rows_equal_u8   equal[r] = 0 where row r differs from row rep[r] (the caller presets `equal` to 1): the exact confirmation of a
 *                       grouping by hash.
 * rows, out, rep, equal: device pointers. */
int tds_rows_hash_u64(const void *rows, int64_t n_rows, int64_t row_bytes, int64_t row_stride_bytes, uint64_t seed, uint64_t *out, void *stream);
int tds_rows_equal_u8(const void *rows, int64_t n_rows, int64_t row_bytes, int64_t row_stride_bytes, const int32_t *rep, uint8_t *equal, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K2b  offroad              simulator.py:1035-1044; infractions.py:86-229 (pure-torch path, squared distances)
 *   state B x A x 4, lenwid B x A x 2, sc B x A x 2 ([sin,cos] of psi), present B x A uint8 or NULL,
 *   out B x A = sum over the 4 corners of threshold(min over faces of squared distance) [* present]
 * ---------------------------------------------------------------------------------------------------------- */
int tds_offroad_f32(const tds_map_t *map, const float *state, const float *lenwid, const float *sc,
                    const uint8_t *present, float *out, int64_t n_agents, float threshold, void *stream);
/* backward: grad_out n -> grad_state n x 4 (x, y columns; psi, v = 0), grad_lenwid n x 2, grad_sc n x 2 (overwritten) */
int tds_offroad_bwd_f32(const tds_map_t *map, const float *state, const float *lenwid, const float *sc,
                        const uint8_t *present, const float *grad_out, float *grad_state, float *grad_lenwid,
                        float *grad_sc, int64_t n_agents, float threshold, void *stream);

/* the same for scenes with different maps: agent a belongs to scene a / agents_per_scene, which uses map scene_map[scene] of the set */
int tds_offroad_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, int64_t agents_per_scene, const float *state, const float *lenwid,
                          const float *sc, const uint8_t *present, float *out, int64_t n_agents, float threshold, void *stream);
int tds_offroad_multi_bwd_f32(const tds_mapset_t *set, const int32_t *scene_map, int64_t agents_per_scene, const float *state,
                              const float *lenwid, const float *sc, const uint8_t *present, const float *grad_out, float *grad_state,
                              float *grad_lenwid, float *grad_sc, int64_t n_agents, float threshold, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K3  bird's-eye-view rasteriser, CV2 semantics
 *     simulator.py:920-1033 -> mesh.py:1053-1157 -> rendering/base.py:167-204 -> rendering/cv2.py:27-70
 * ---------------------------------------------------------------------------------------------------------- */
#define TDS_OUT_F32 0      /* reference-faithful float32 image with values 0..255 */
#define TDS_OUT_U8 1       /* same values as uint8 (separate mode, 4x fewer bytes) */
#define TDS_OUT_MASK_U8 2    /* semantic masks, one 0 / 1 byte per pixel and channel (tds_raster_scene_masks) */
#define TDS_OUT_MASK_BITS 3  /* semantic masks, one bit per pixel and channel (tds_raster_scene_masks) */

/* Fused scene path used by Simulator.render / render_egocentric: the static map comes from the handle, the actor
 * mesh is generated on the fly from agent state (never materialised per camera).
 *   state     B x N x 4   all agents (exposed + NPCs)
 *   agent_sc  B x N x 2   [sin, cos] of psi
 *   tmpl      B x N x 7 x 2   actor template verts in the agent frame (mesh.py:911-996), built once by the host
 *   actor_key B x N x 2   uint32 (rank << 24 | 0x00RRGGBB) for (body, direction) faces, rank = 1 + index of the
 *                         part's rendering level in the map's `levels`; a key of 0 removes the part (quads without a direction
 *                         triangle, e.g. the stop lines of traffic controls, mesh.py:1007-1035)
 *   mask      B x Nc x N  uint8, present & rendering mask (simulator.py:946-948)
 *   cam_xy    B x Nc x 2, cam_sc B x Nc x 2 [sin, cos]
 *   scale = 2 / fov (rendering/base.py:149), res = H = W
 *   out       B x Nc x 3 x H x W   float32 or uint8 (out_mode)
 * Equal-level faces of different colour are ordered by packed colour (documented tie-break).
 *
 * workspace: optional DEVICE scratch (tds_raster_scene_workspace_bytes) for the two-kernel forms -- a first kernel scans the map grid
 * once per camera and lists the surviving faces, a second one rasterises from the lists: per-strip lists for the packed-key kernels
 * (more than 15 keys), one list of up to 1 636 faces or pairs of faces per camera (20 bytes each) for the bit-plane kernels up to 160 x 160 (float32; above 116 x 116 only multiples of 16) / 216 x 216 (uint8),
 * where that form is faster than the fused kernel (above, the fused kernel runs and the recommended size holds no lists).  A list that overflows only sends its camera (or strip) to the kernel that scans for
 * itself: the pixels never depend on the size of the scratch.  With workspace == NULL every launch scans the grid itself (same pixels,
 * slower at low resolutions).  The scratch carries no state between calls.
 * Launch shape of the bit-plane kernels: the fused kernel at three workgroups per CU is a PERSISTENT launch: its workgroups take cameras
 * from per-XCD work queues, 64 bytes at the END of the workspace that the call clears in stream order right before the launch (a one-wave
 * kernel).  The library owns no device memory besides the handles of tds_map_create & co. and allocates nothing in
 * any per-call entry point, so every call can be captured into a HIP graph.  Two calls that may run at the same time (different
 * streams) need a workspace each.  With workspace == NULL the same kernel runs one workgroup per camera (about 1 % slower at 256 x 256).
 * The workspace must be 16-byte aligned.
 *
 * actor_keys: optional HOST array of the distinct values occurring in `actor_key` (one per agent type and part).  When it is
 * given and the scene (map + actors) uses at most 16 distinct keys, the bit-plane kernel is used: one bit per pixel and key in
 * LDS, a whole camera per workgroup, spans painted with one ds_or.  Same pixels as the other paths.
 *
 * actor_key_per_camera != 0: `actor_key` is B x Nc x N x 2 -- every camera sees its own colours, the fused form of generate()'s
 * custom_agent_colors (mesh.py:1092-1099; only the body faces take the custom colour there).
 *
 * extra_tri / extra_key / n_extra: optional per-camera triangles, B x Nc x n_extra x 3 x 2 float32 WORLD coordinates and
 * B x Nc x n_extra uint32 keys (0 = no triangle) -- the fused form of generate()'s waypoint discs (mesh.py:1120-1145), which differ
 * from camera to camera.  Their keys must be listed in `actor_keys` for the bit-plane kernel to be used. */
/* aux (may be NULL): optional outputs for a later backward pass (tds_raster_scene_bwd_idx_f32).
 *   index_slices  DEVICE buffer of tds_raster_index_slices_bytes(B * Nc, res) bytes, or NULL.  When given, the call must be servable by
 *                 the bit-plane kernel (float32 output, res a multiple of 4, at most 15 distinct keys with `actor_keys` listed) -- else
 *                 TDS_ELIMIT -- and receives, per pixel, the 1-based position of the winning key in `keys` (0 = background) as bit-slices:
 *                 uint32 [camera][x / 32][y / 4][slice 0..3][y % 4], bit x % 32; 64 B per (word column, row quad), slices >= index_bits
 *                 are zero.  x, y = OpenCV pixel coordinates = the last two axes of `out`.
 *   keys, n_keys, index_bits   filled by the call (HOST): the ascending key table of the launch (n_keys = 0 when another kernel ran)
 *   flags         input: TDS_RASTER_NO_TRIM draws every face as the reference does with trim_mesh_before_rendering = False */
#define TDS_RASTER_NO_TRIM 1   /* trim_mesh_before_rendering = False (rendering/cv2.py:15,32-41): keep faces without a vertex in view */
/* Coverage record (optional): lets a render into a buffer that still holds an EARLIER render of this library skip the 128-byte lines that
 * held only background then and hold only background now (a loop that renders into a ring of buffers: about half the lines at 256 x 256).
 *   coverage        DEVICE buffer of at least tds_raster_coverage_bytes(B * Nc, res) bytes, 16-byte aligned, or NULL.  It belongs to ONE
 *                   output buffer: a 64-byte header (magic, res, cameras, the address of `out`, the background's bits per channel, the mode of the
 *                   launch in flight) and uint32 [camera][x / 32][y / 32], bit x % 32 = "the line of column x, rows 32 (y / 32) .. + 31 holds a
 *                   covered pixel" (x, y as for index_slices; one line per channel, all three share the bit).  The call checks the header on the
 *                   device, in stream order: a record that was never written, or written for another resolution, camera count or `out`, makes
 *                   the launch store every line; either way the launch leaves a valid record of what `out` holds now.  Needs no clearing.
 *   coverage_bytes  size of that buffer (too small for the call: TDS_EINVAL)
 *   flags           TDS_RASTER_REWRITE_ALL: store every line whatever the record says, and still record the coverage
 *   coverage_maintained   filled by the call (HOST): 1 when the launch maintained the record.  The rule: a float32 image whose side is a multiple of
 *                   32, no index_slices, and the launch is the fused bit-plane kernel in 4-wave workgroups at three per CU (its LDS per workgroup lies
 *                   between 40 and 52 KiB: e.g. five keys at 256 x 256, nine keys there in two strips, seven keys at 192 x 192).  0: any other launch
 *                   (uint8 output, the masks, other sides, the split form up to 160 x 160, 8-wave workgroups -- six or seven keys at 256 x 256 --,
 *                   four workgroups per CU -- five keys at 192 x 192, eight keys at 256 x 256 in half strips --, more than 15 keys): every pixel was
 *                   stored and the record was NOT touched: it no longer describes `out` and must not be passed again without TDS_RASTER_REWRITE_ALL.
 * THE CONTRACT IS THE CALLER'S: between two calls that pass the same record without TDS_RASTER_REWRITE_ALL nothing but this library's
 * renders with that record may have written to `out` -- the skipped lines are assumed to hold the background (0.0f) the earlier call left
 * there.  aux == NULL or coverage == NULL: every pixel is stored, as before. */
#define TDS_RASTER_REWRITE_ALL 2
/* Prepared scan set-ups (optional): a scratch table that lets the persistent bit-plane launch compute each camera's scan set-up (trim polygon,
 * grid window, grid rows) once, in a small kernel in front of it, instead of in every wave of the camera's workgroup.
 *   camera_prep        DEVICE buffer of at least tds_raster_camera_prep_bytes(B * Nc, res, out_mode, n_keys) bytes, 16-byte aligned, or NULL.  The
 *                      call writes it and reads it in stream order; it carries nothing from call to call, and two launches that may overlap in
 *                      time must not share one.  It is NOT part of the workspace.
 *   camera_prep_bytes  size of that buffer
 *   flags              TDS_RASTER_HAS_CAMERA_PREP: the struct the caller passes HAS these two fields.  They were appended to a struct that ended
 *                      with coverage_bytes (112 bytes); the library reads past that only when the flag is set, so a caller built against the
 *                      shorter struct stays valid and simply gets no table.
 * The pixels never depend on it: no flag, NULL, a buffer that is too small or misaligned, or a call served by another launch (uint8 or float32 in 8-wave
 * workgroups or at four workgroups per CU, the split form, the masks, packed keys) renders exactly as before and leaves the buffer alone. */
#define TDS_RASTER_HAS_CAMERA_PREP 4
/*   flags              TDS_RASTER_NO_SMALL_FACES: every face goes through the face queue.  Without it the persistent 4-wave bit-plane launches paint
 *                      the faces that lie inside the image and span at most TDS_RASTER_SMALL_ROWS rows on the lane that scanned them, where enough
 *                      lanes of a scan step hold one; the pixels are the same either way. */
#define TDS_RASTER_NO_SMALL_FACES 8
/* Helper launch (optional): a second stream whose CUs the persistent bit-plane launch may use as well.  A caller that keeps the launch's stream off
 * some CUs for other kernels (tds_stream_create with a CU mask: the infraction metrics beside the launch) passes the stream confined to those CUs; the
 * call then enqueues the SAME kernel with the same arguments a second time, on that stream, sized for its CUs (three workgroups per CU).  Its workgroups
 * take work items from the launch's queues like all the others -- whatever is left when they start, which is when the kernels enqueued on that stream
 * before the call have ended -- and exit at once when nothing is.  The pixels never depend on it.
 *   helper_stream      the hipStream_t (in).  Used only when ALL of this holds, else the call makes its one launch as before: the launch is the fused
 *                      bit-plane kernel of a colour image (float32 or uint8) in persistent 4-wave workgroups over all the cameras (not the masks, not the
 *                      split form or the launch over its overflowed cameras, not four workgroups per CU or eight waves, not a call with index_slices);
 *                      a workspace was given (the queues live there); helper_stream and `stream` are two different, non-NULL streams and helper_stream
 *                      may use at least one CU; the launch has at least 4 work items (camera, strip) per workgroup of its own grid (shorter launches
 *                      would wait for the other stream longer than they gain); neither stream is capturing (a captured graph keeps the single launch).
 *   helper_workgroups  filled by the call (HOST): workgroups of the second enqueue, 0 = none was made.
 *   flags              TDS_RASTER_HAS_HELPER_STREAM: the struct the caller passes is a tds_raster_aux_helper_t (below): tds_raster_aux_t with these two
 *                      fields behind it (the two of TDS_RASTER_HAS_CAMERA_PREP are still read only with their own flag).  Appended like those, so
 *                      the shorter structs stay valid.
 * Ordering, all inside the call: the helper stream waits for an event recorded on `stream` behind everything the call enqueues in front of the launch
 * (queue clear, coverage header, prepared set-ups), and `stream` waits for an event recorded on the helper stream behind the second enqueue before the
 * call returns -- so whatever follows the call in `stream`'s order (the next call's queue clear, a free of the workspace, of `out` or of an input)
 * follows BOTH enqueues.  The call blocks nothing on the host.  The events are created once per (device, stream, helper stream) and kept for the life
 * of the process.  A HIP error while forking or joining: TDS_EHIP (after a failed fork nothing is enqueued on the helper stream). */
#define TDS_RASTER_HAS_HELPER_STREAM 16
typedef struct tds_raster_aux {
    uint32_t *index_slices;
    int64_t index_slices_bytes;
    uint32_t keys[16];
    int32_t n_keys;
    int32_t index_bits;
    int32_t flags;              /* in: TDS_RASTER_* */
    int32_t coverage_maintained;    /* out */
    uint32_t *coverage;         /* in */
    int64_t coverage_bytes;     /* in */
    void *camera_prep;          /* in; read only with TDS_RASTER_HAS_CAMERA_PREP */
    int64_t camera_prep_bytes;  /* in; read only with TDS_RASTER_HAS_CAMERA_PREP */
} tds_raster_aux_t;
/* tds_raster_aux_t with the two fields of the helper launch appended (offsets 128 and 136): what a caller that sets TDS_RASTER_HAS_HELPER_STREAM passes
 * as `aux`, its address cast to tds_raster_aux_t *.  The library looks behind the 128 bytes only under that flag. */
typedef struct tds_raster_aux_helper {
    tds_raster_aux_t aux;
    void *helper_stream;        /* in */
    int64_t helper_workgroups;  /* out */
} tds_raster_aux_helper_t;
int tds_raster_index_slices_bytes(int64_t n_img, int res, int64_t *bytes);
/* bytes of the coverage record of n_img images of res x res (0: no lines are tracked at this resolution -- res is no multiple of 32) */
int tds_raster_coverage_bytes(int64_t n_img, int res, int64_t *bytes);
/* bytes of the table of prepared scan set-ups for n_img images of res x res in `out_mode` with `n_keys` distinct keys (-1: not known): one
 * record per camera and strip of the launch; 0 where no launch of that shape takes the table.  Bad arguments: TDS_EINVAL. */
int tds_raster_camera_prep_bytes(int64_t n_img, int res, int out_mode, int n_keys, int64_t *bytes);

int tds_raster_scene(const tds_map_t *map, const float *state, const float *agent_sc, const float *tmpl,
                     const uint32_t *actor_key, const uint8_t *mask, const float *cam_xy, const float *cam_sc,
                     int64_t B, int64_t Nc, int64_t N, float scale, int res, int out_mode, void *out, void *workspace,
                     int64_t workspace_bytes, const uint32_t *actor_keys, int n_actor_keys, int actor_key_per_camera,
                     const float *extra_tri, const uint32_t *extra_key, int64_t n_extra, tds_raster_aux_t *aux, void *stream);
/* tds_raster_scene for scenes with different maps: scene b is drawn over map scene_map[b] of the set (one launch for the batch) */
int tds_raster_scene_multi(const tds_mapset_t *set, const int32_t *scene_map, const float *state, const float *agent_sc, const float *tmpl,
                           const uint32_t *actor_key, const uint8_t *mask, const float *cam_xy, const float *cam_sc, int64_t B, int64_t Nc,
                           int64_t N, float scale, int res, int out_mode, void *out, void *workspace, int64_t workspace_bytes,
                           const uint32_t *actor_keys, int n_actor_keys, int actor_key_per_camera,
                           const float *extra_tri, const uint32_t *extra_key, int64_t n_extra, tds_raster_aux_t *aux, void *stream);
/* Semantic bird's-eye masks: the same scene and arguments as tds_raster_scene / _multi (without actor_key_per_camera: the actors' keys are
 * those of their types), but instead of an image a stack of C = n_channels binary channels.  Channel c is set at pixel (x, y) exactly when
 * the colour image would paint there a face whose key has bit c set in its key_channels word -- the same fill, trim rule (TDS_RASTER_NO_TRIM
 * in aux->flags), mask, masked-agent dot, per-camera triangles as the colour call, but WITHOUT occlusion: a road channel stays set under a car.
 *   key_channels  HOST array, one uint32 channel set per entry of the launch's key table: the distinct values of the map's keys (tds_map_keys,
 *                 over the set for _multi) and of actor_keys, in ascending order.  1 <= n_channels <= 32.
 *   out_mode      TDS_OUT_MASK_U8:   out = B x Nc x C x H x W bytes, 0 or 1, in the memory order of the colour image (x, y = the last two axes)
 *                 TDS_OUT_MASK_BITS: out = B x Nc x C x ceil(W / 32) x H uint32 words: bit i of word (xw, y) is pixel (32 xw + i, y);
 *                                    padding bits are 0.  16-byte aligned.
 *   workspace     required: tds_raster_scene_workspace_bytes_for(B * Nc, res, out_mode, n_keys) bytes.  The call writes its channel table there
 *                 in stream order (nothing is allocated: the call can be captured into a HIP graph).
 * The masks are streamed out of the bit-plane kernels, with the plan of the uint8 image of the same shape: a scene with more than 15 distinct
 * keys is TDS_ELIMIT.  actor_keys must be listed when N > 0 or n_extra > 0; aux->index_slices must be NULL (TDS_EINVAL otherwise). */
int tds_raster_scene_masks(const tds_map_t *map, const float *state, const float *agent_sc, const float *tmpl,
                           const uint32_t *actor_key, const uint8_t *mask, const float *cam_xy, const float *cam_sc,
                           int64_t B, int64_t Nc, int64_t N, float scale, int res, int out_mode, void *out, void *workspace,
                           int64_t workspace_bytes, const uint32_t *actor_keys, int n_actor_keys,
                           const float *extra_tri, const uint32_t *extra_key, int64_t n_extra, const uint32_t *key_channels, int n_channels,
                           tds_raster_aux_t *aux, void *stream);
int tds_raster_scene_masks_multi(const tds_mapset_t *set, const int32_t *scene_map, const float *state, const float *agent_sc, const float *tmpl,
                                 const uint32_t *actor_key, const uint8_t *mask, const float *cam_xy, const float *cam_sc, int64_t B, int64_t Nc,
                                 int64_t N, float scale, int res, int out_mode, void *out, void *workspace, int64_t workspace_bytes,
                                 const uint32_t *actor_keys, int n_actor_keys, const float *extra_tri, const uint32_t *extra_key, int64_t n_extra,
                                 const uint32_t *key_channels, int n_channels, tds_raster_aux_t *aux, void *stream);
/* recommended scratch size for n_img = B * Nc cameras at this resolution (0 if the fast path cannot be used): enough for every path */
int tds_raster_scene_workspace_bytes(int64_t n_img, int res, int64_t *bytes);
/* the same for a launch of which the caller knows the number of distinct keys (map keys + actor keys, tds_map_keys): with at most 15 the
 * bit-plane kernels run, which use the face lists up to 160 x 160 (float32; above 116 x 116 only multiples of 16) / 216 x 216 (uint8) only and above nothing but the 64 bytes of
 * work queues -- 128 bytes instead of 32 KB per camera at 256 x 256.  n_keys < 0 or > 15: as tds_raster_scene_workspace_bytes. */
/* The mask modes: the uint8 image's size and 256 bytes for the channel table. */
int tds_raster_scene_workspace_bytes_for(int64_t n_img, int res, int out_mode, int n_keys, int64_t *bytes);

/* ------------------------------------------------------------------------------------------------------------
 * Output buffers with spread-out physical pages (no reference counterpart: rendering/cv2.py:52 allocates a numpy image per call).
 *
 * The rasteriser is bound by the HBM write stream, and what a write stream reaches on MI355X depends on the PHYSICAL pages under the
 * buffer: a large hipMalloc is served at 1, 15/16 or 7/8 of the rate for as long as it lives, whatever its virtual address and whatever
 * the store pattern (about one 51.5 GB allocation in three is at 7/8); a buffer whose physical pages are spread over twice its size
 * hardly ever is (one of 100 probed, at 15/16; DESIGN_HISTORY.md section 4, tools/alloc_probe.hip).  tds_buffer_create builds such a buffer: chunks of 8 MiB created alternately
 * with spacer chunks that are released once the buffer is mapped (hipMemCreate / hipMemMap; needs twice the size free while it runs,
 * and falls back to dense chunks when that is not there).  Below 256 MiB, or with TDS_BUFFER_DENSE, it is one hipMalloc.
 * These are explicit create / destroy calls like tds_map_create: no per-step entry point allocates.
 * tds_torch_alloc / tds_torch_free have the signatures torch.cuda.memory.CUDAPluggableAllocator binds
 * (void *(size_t, int device, stream), void(void *, size_t, int device, stream)): a torch memory pool over them hands such buffers to
 * `torch.empty`, cached and stream-ordered by torch's allocator like any other block (torchdrivesim_amd/rendering/hip.py: image_pool).
 * ---------------------------------------------------------------------------------------------------------- */
#define TDS_BUFFER_DENSE 1      /* plain hipMalloc whatever the size */
typedef struct tds_buffer tds_buffer_t;
int tds_buffer_create(int64_t bytes, int device, int flags, tds_buffer_t **out);
void *tds_buffer_ptr(const tds_buffer_t *buf);                         /* device pointer, valid until tds_buffer_destroy */
int tds_buffer_info(const tds_buffer_t *buf, int64_t *bytes, int64_t *chunks, int *spread);      /* any output may be NULL */
int tds_buffer_destroy(tds_buffer_t *buf);
void *tds_torch_alloc(size_t size, int device, void *stream);          /* NULL on failure */
void tds_torch_free(void *ptr, size_t size, int device, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Streams confined to a part of the device's CUs (no reference counterpart).
 *
 * The persistent raster launch holds every CU it may use until its last image is out, so nothing runs beside it -- unless it is kept off
 * a few CUs.  tds_stream_create makes a stream whose kernels only run on the CUs of `cu_mask` (hipExtStreamCreateWithCUMask: bit i of the
 * mask is CU i / 8 of XCD i % 8 on MI355X; `n_words` 32-bit words, 8 for 256 CUs; NULL = all CUs).  A loop renders on a stream that leaves
 * four CUs per XCD out and computes its metrics on a stream confined to those 32: the write-bound launch loses nothing (tools/cu_mask_probe.hip)
 * and the metrics run beside it (Simulator.overlap_infractions = 'reserved').  tds_raster_scene sizes its persistent launch for the CUs of the
 * stream it is given.  Explicit create / destroy, like the other handles.
 * ---------------------------------------------------------------------------------------------------------- */
int tds_stream_create(int device, const uint32_t *cu_mask, int n_words, void **stream);
int tds_stream_destroy(int device, void *stream);
int tds_device_cu_count(int device, int *cus);
/* Where do the kernels of `stream` run?  Enqueues `n` one-wave workgroups that each keep their CU busy for a moment and write
 * XCC_ID << 16 | (HW_ID bits 15..8: SE, SH, CU) of the CU they ran on to places[blockIdx] (device memory, n words).  With n of a few
 * thousand every CU the stream may use shows up.  The caller synchronises and reads; the mask layout documented above is an observation of
 * one MI355X in SPX mode, and this is how the host verifies it on the device at hand before it relies on it (_ops.reserved_streams). */
int tds_stream_places(void *stream, uint32_t *places, int n);


/* Backward of tds_raster_scene with respect to the poses of the actors and cameras.  The CV2 backend of the reference has no
 * gradient (rendering/cv2.py:27-70 runs in numpy); this one is build-defined (edge sampling of the actors' outlines against the
 * forward image, DESIGN.md "K3 backward") and plays the role of the pytorch3d backend's soft-blend gradient
 * (rendering/pytorch3d.py:57-119) for policy learning through the renderer.
 *   image, grad_out  B x Nc x 3 x H x W float32: the forward output (TDS_OUT_F32) and the incoming gradient
 *   grad_agent       B x Nc x N x 4   [d/dx, d/dy, d/dsin(psi), d/dcos(psi)] of actor n as seen by camera c (caller sums over c)
 *   grad_cam         B x Nc x 4       [d/dcx, d/dcy, d/dsin, d/dcos] of the camera: every colour boundary of the image moves with it
 *   grad_tmpl        optional (NULL to skip), B x Nc x N x 7 x 2: d/d(template vertex v) of actor n as seen by camera c -- the actor's
 *                    outline in its own frame (mesh.py:911-996).  The caller sums over c and chains to the actor's length and width
 *                    through the construction of the template.
 * All outputs are overwritten. */
int tds_raster_scene_bwd_f32(const float *state, const float *agent_sc, const float *tmpl, const uint8_t *mask, const float *cam_xy,
                             const float *cam_sc, const float *image, const float *grad_out, int64_t B, int64_t Nc, int64_t N,
                             float scale, int res, float *grad_agent, float *grad_cam, float *grad_tmpl, void *stream);

/* The same gradient computed from the forward's key-index slices (tds_raster_aux_t) instead of the forward image: the incoming gradient
 * is read only next to colour boundaries.  keys / n_keys: HOST, the key table the forward launch reported.
 * grad_color (optional, NULL to skip): B x Nc x 16 x 4 -- entry [i][ch] (ch 0..2 = R, G, B; [3] = 0) is the gradient with respect to
 * channel ch of the colour shown for key index i (0 = background, i >= 1: keys[i - 1]) in that camera: the sum of grad_out over the
 * pixels whose winning key it is (exact: the image is colour[index] pixel by pixel).  Asking for it reads grad_out in full.
 * grad_out_stride: floats between the gradient images of consecutive cameras -- 3 res^2 for a dense B x Nc x 3 x H x W gradient, 0 when
 * ONE 3 x H x W image is the gradient of every camera (losses like image.sum() or a fixed linear read-out hand back a broadcast). */
int tds_raster_scene_bwd_idx_f32(const float *state, const float *agent_sc, const float *tmpl, const uint8_t *mask, const float *cam_xy,
                                 const float *cam_sc, const uint32_t *index_slices, const uint32_t *keys, int n_keys, const float *grad_out,
                                 int64_t grad_out_stride, int64_t B, int64_t Nc, int64_t N, float scale, int res, float *grad_agent,
                                 float *grad_cam, float *grad_color, float *grad_tmpl, void *stream);

/* Generic BirdviewRenderer.render_rgb_mesh (rendering/base.py:206-212) for an arbitrary per-camera RGB mesh:
 *   verts n_img x V x 3 (x, y, z), attrs n_img x V x 3 in [0,1], faces n_img x F x 3 int32,
 *   levels: n_levels HOST floats sorted descending containing every z in use (<= 255)
 *   out   n_img x 3 x H x W  (CHW, i.e. already permuted as render_frame returns it, base.py:202-203)
 *   flags TDS_RASTER_* (0: the trim rule of cv2.py:32-41 is applied) */
int tds_raster_mesh(const float *verts, const float *attrs, const int32_t *faces, int64_t n_img, int64_t V, int64_t F,
                    const float *cam_xy, const float *cam_sc, const float *levels, int n_levels, float scale, int res,
                    int out_mode, void *out, int flags, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Wrong-way query           simulator.py:607-630 (compute_wrong_way); infractions.py:232-304 (lanelet_orientation_loss);
 *                           lanelet2.py:108-180 (find_lanelet_directions, find_direction)
 * The reference keeps a lanelet2.core.LaneletMap (Lanelet2 C++ objects, not part of the reference's sources) and queries it agent by
 * agent.  Here a map is flattened once into a LANE TABLE and a batch is one kernel launch.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct tds_lanes tds_lanes_t;
typedef struct tds_laneset tds_laneset_t;

/* Centre line of one lanelet (`lanelet.centerline`, lanelet2.py:128): HOST arrays, bounds n x 3 float64 in travel order, out must hold
 * (n_left + n_right + 1) x 3 doubles, *n_out = number of points written (0 when a bound is empty). */
int tds_lanelet_centerline_f64(const double *left, int n_left, const double *right, int n_right, double *out, int *n_out);

/* tds_lanes_create also keeps, per centre-line point, the cumulative 3-D length of its line (float64, summed front to back) and the list of
 * lanelets a point can be drawn on, for tds_spawn_on_lanes_f32. */
/* HOST inputs: poly_xy P x 2 float64 = outline rings (left bound followed by the reversed right bound), lanelet l owns points
 * poly_start[l] .. poly_start[l+1]; cl_xyz C x 3 float64 = centre lines, cl_start likewise; flags (n_lanelets, may be NULL): bit 0 =
 * the lanelet carries one of the tags to exclude (infractions.py:21).  cell_size <= 0 selects the default (8 m).  Queries may use
 * any lanelet_dist_tolerance up to max_tolerance.  The handle lives on the CURRENT HIP device. */
int tds_lanes_create(const double *poly_xy, const int32_t *poly_start, const double *cl_xyz, const int32_t *cl_start,
                     const int32_t *flags, int n_lanelets, float cell_size, float max_tolerance, tds_lanes_t **out);
int tds_lanes_destroy(tds_lanes_t *lanes);
/* info[0..3] = lanelets, grid nx, grid ny, device bytes held */
int tds_lanes_info(const tds_lanes_t *lanes, int64_t *info);
/* the lane tables of a batch (`lanelet_maps: List[Optional[LaneletMap]]`, infractions.py:232): a device array of views; the tables must
 * outlive the set */
int tds_laneset_create(const tds_lanes_t *const *lanes, int n, tds_laneset_t **out);
int tds_laneset_destroy(tds_laneset_t *set);

/* lanelet_orientation_loss [* present]:
 *   state n x 4 (x, y, psi, v); agent a belongs to scene a / agents_per_scene, which uses table scene_map[scene] of the set
 *   (device int32; a negative entry = `None`, loss 0; NULL = table 0 for every scene); recenter_offset (scenes x 2 or NULL) is added to
 *   the position (infractions.py:271-273); present (n uint8 or NULL) multiplies the result (simulator.py:624).
 *   out n = min over the lanelets within lanelet_dist_tolerance of -cos(d) * [|d| > direction_angle_threshold],
 *   d = normalize_angle(lanelet direction - psi); 0 without such a lanelet, when one of them carries an excluded tag, or when
 *   find_direction fails (LaneletError, infractions.py:290-294). */
int tds_wrong_way_f32(const tds_laneset_t *set, const int32_t *scene_map, int64_t agents_per_scene, const float *state,
                      const float *recenter_offset, const uint8_t *present, float *out, int64_t n_agents,
                      float direction_angle_threshold, float lanelet_dist_tolerance, void *stream);
/* tds_wrong_way_f32 plus one more output, the same kernel with one more pointer: out has the bits of tds_wrong_way_f32, and
 *   dloss_dpsi n = d out / d psi with the lanelet whose loss the minimum keeps held fixed: -sinf(d) where |d| > direction_angle_threshold, else 0
 *   (normalize_angle has derivative 1).  Of equal losses the first in table order wins (the winner is tracked with a strict <; a NaN loss -- a NaN psi -- gives way to a
 *   later one exactly as fminf drops it).  Exactly 0
 *   wherever the loss is forced to 0: no lanelet, an excluded tag, a failed find_direction, an absent agent, a scene without a table.
 *   The position is a constant, as in the reference (it passes through float() there, infractions.py:270-287): x and y get no gradient. */
int tds_wrong_way_grad_f32(const tds_laneset_t *set, const int32_t *scene_map, int64_t agents_per_scene, const float *state,
                           const float *recenter_offset, const uint8_t *present, float *out, float *dloss_dpsi, int64_t n_agents,
                           float direction_angle_threshold, float lanelet_dist_tolerance, void *stream);
/* find_lanelet_directions for a batch of points (xy n x 2 float64, as the reference passes host doubles): dirs / dists n x max_dirs
 * float64 (direction and distance of the first max_dirs lanelets found, in table order), count n (number found, may exceed max_dirs; 0 when excluded), status n uint8 (bit 0: find_direction
 * failed for some lanelet, bit 1: a lanelet with an excluded tag is within tolerance) */
int tds_lanelet_directions_f64(const tds_laneset_t *set, const int32_t *scene_map, int64_t points_per_scene, const double *xy,
                               double *dirs, double *dists, int32_t *count, uint8_t *status, int max_dirs, int64_t n_points,
                               float lanelet_dist_tolerance, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * On-lane scene initialisation            behavior/heuristic.py:10-53 (heuristic_initialize); lanelet2.py:183-208
 *                                         (pick_random_point_and_orientation); infractions.py:503-545 (the acceptance test)
 * The reference places one agent after the other in ONE scene, one torch call and one Lanelet2 query per attempt.  Here a batch of scenes is
 * one launch: one wavefront per scene, 64 attempts of the current agent at once.
 *   set, scene_map     lane tables as for tds_wrong_way_f32 (a negative entry, or a table without an eligible lanelet -- at least two
 *                      centre-line points and a finite positive length --, places nothing)
 *   scene_ids          n_scenes int64 (device) or NULL = 0 .. n_scenes-1: the identity of each scene in the random stream
 *   attributes         n_scenes x A x 3  [length, width, lr] (lr is not read)
 *   occupied           n_scenes x M x 5 boxes [x, y, length, width, psi] that are already there, NOT yet inflated by the gap, or NULL (M = 0);
 *   occupied_sc        n_scenes x M x 2 [sin, cos] of the angle the disc metric uses for the INFLATED box: psi + pi/2 * (width + gap_lat >
 *                      length + gap_long); occupied_mask n_scenes x M uint8 or NULL (all present)
 *   state              n_scenes x A x 4 [x, y, psi, speed];  sc n_scenes x A x 2 [sin, cos] of the heading, taken from the unit vector of
 *                      the lane's local direction (psi = atan2 of the same vector);  placed n_scenes x A uint8;
 *   attempts           n_scenes x A int32: candidates drawn for the agent (max_attempts for the one that found no place, 0 = never reached)
 * Candidate (agent i, attempt a) of scene id s: Philox4x32-10, key = (seed low, seed high), counter = (s low, s high, i, a) -> r0..r3;
 * eligible lanelet (r0 * n_eligible) >> 32, arc length = length * (r1 + 0.5) * 2^-32 (float64), speed = min_speed + (max_speed - min_speed) *
 * ((r2 >> 8) * 2^-24) (float32).  Agents are placed in index order; agent i takes the candidate with the LOWEST attempt index whose 5-disc
 * value (tds_pairwise_overlap_f32, TDS_METRIC_DISCS) against every present occupied box and every agent 0 .. i-1 -- each grown by
 * [gap_long, gap_lat] -- is not > 0.  In a scene where agent i finds none in max_attempts, agents i .. are not placed (rows of zeros).
 * agents_per_scene + n_occupied <= TDS_SPAWN_MAX_BOXES (the boxes of a scene live in LDS, 24 bytes each).  Every output is written in
 * full; nothing is allocated and nothing synchronises. */
#define TDS_SPAWN_MAX_BOXES 2048
int tds_spawn_on_lanes_f32(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t n_scenes,
                           int agents_per_scene, const float *attributes, const float *occupied, const float *occupied_sc,
                           const uint8_t *occupied_mask, int n_occupied, uint64_t seed, float min_speed, float max_speed,
                           float gap_long, float gap_lat, int max_attempts, float *state, float *sc, uint8_t *placed,
                           int32_t *attempts, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Lane-following NPC traffic (no reference counterpart: the definition is this library's own; float64 model:
 * tests/lane_follow_model.py).
 *
 * The lane graph of a table: lanelet l is followed by the lanelets succ_items[succ_start[l] .. succ_start[l + 1]) (HOST arrays, n_lanelets + 1
 * and succ_start[n_lanelets] int32, indices into the table, ascending per lanelet).  Set once, right after tds_lanes_create and before the
 * table joins a set; a second call is TDS_EINVAL. */
int tds_lanes_set_successors(tds_lanes_t *lanes, const int32_t *succ_start, const int32_t *succ_items);

/* A pose onto a lane: xy n x 2 [x, y], sc n x 2 [sin psi, cos psi] (computed by the caller with torch, like every angle of this header).
 * Candidates are the lanelets whose outline contains the point or lies within `tolerance` of it (the test of tds_wrong_way_f32), that carry
 * no excluded tag and are eligible in the sense of tds_spawn_on_lanes_f32.  Per candidate: the foot = the closest point of the 2-D centre
 * line (earliest segment on ties), t = the unit direction of the foot's segment, score = cos psi * t.x + sin psi * t.y.  The candidate with
 * the largest score wins (lowest index on ties) and must have a score > 0:
 *   lane n int32     index of the lanelet in the table, -1 without such a candidate
 *   arc n float64    cum[k] + u * (cum[k + 1] - cum[k]) on the table's cumulative lengths, k the foot's segment, u its parameter in [0, 1]
 *   lateral n        signed offset from the foot's segment line, left positive
 * Pose i belongs to scene i / poses_per_scene (the _multi form; scene_map as for tds_wrong_way_f32).  Float64 throughout. */
int tds_lane_snap(const tds_lanes_t *lanes, const float *xy, const float *sc, int32_t *lane, double *arc, float *lateral, int64_t n_poses,
                  float tolerance, void *stream);
int tds_lane_snap_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t poses_per_scene, const float *xy, const float *sc,
                        int32_t *lane, double *arc, float *lateral, int64_t n_poses, float tolerance, void *stream);

/* One step of N NPCs per scene that follow the lane graph at the speed the Intelligent Driver Model gives them; one launch, one wavefront per NPC.
 *   entities      boxes B x E x 5 [x, y, length, width, psi] (psi is not read), ent_sc B x E x 2 [sin, cos], ent_speed B x E, ent_present B x E
 *                 uint8: everything an NPC may have to brake for, AS IT WAS BEFORE THE STEP (a Jacobi update: the kernel writes none of them)
 *   self_index    B x N int32 or NULL: the entity row that is the NPC itself (skipped); npc_size B x N x 2 [length, width];
 *                 desired_speed B x N (v0 > 0); npc_present B x N uint8
 *   lane, arc, hops   B x N int32 / float64 / int32, IN AND OUT: lanelet, arc length on it, lanelet transitions made so far
 *   state         B x N x 4 [x, y, psi, speed], in and out (only speed is read); sc B x N x 2 [sin, cos] of the new pose = the unit vector of
 *                 its segment; leader B x N int32: the entity braked for, -1 none, -2 the end of the lane, -3 the junction it gives way at
 *                 (tds_lane_follow_step_stops_multi only)
 * Path: from (lane, arc) along the centre line (2-D) to the lanelet's end, then along the successor chosen for hop `hops`, `hops + 1`, ...:
 * succ[(r0 * n_succ) >> 32], r0 the first word of Philox4x32-10 with key (seed low ^ 0x4C414E45, seed high ^ 0x464F4C57) and counter (scene id
 * low, scene id high, NPC index, hop).  It ends with the segment in which `horizon` metres are covered, after TDS_FOLLOW_MAX_HOPS successors,
 * or after 256 segments; a lanelet without a (drivable) successor ends it with a standing obstacle of zero length at its end.
 * Leader: every other present entity gives five points (centre, corners); each is projected onto the path (closest point over all segments,
 * earliest on ties) -> path distance d and distance e from the path; it blocks iff d > 0 and e <= width / 2 + lateral_margin.  The leader is
 * the entity with the smallest d (lowest index on ties), gap = d - length / 2, v_lead = its speed * max(0, cos) of the angle between its heading
 * and the path's direction at that foot.  IDM with idm = [T, s0, a, b, b_max]: gap = max(gap, 0.1), s* = s0 + max(0, v T + v (v - v_lead) /
 * (2 sqrt(a b))), acc = max(-b_max, a (1 - (v / v0)^4 - (s* / gap)^2)) (no last term without a leader); v' = max(0, v + acc dt) rounded to
 * binary32, ds = (v + v') / 2 dt, arc += ds; while arc >= the lanelet's length: arc -= length, lane = successor, hops += 1 (at most
 * TDS_FOLLOW_MAX_HOPS times); at a dead end arc = length and v' = 0.  Rows with lane < 0, not present, or whose desired_speed is not > 0 (NaN
 * included): nothing but leader = -1 is written.
 * Float64 with + - * / sqrt only; psi alone is an atan2.  E > TDS_FOLLOW_MAX_ENTITIES is TDS_ELIMIT; a negative or non-finite dt, horizon,
 * lateral_margin or IDM parameter is TDS_EINVAL before any launch.  Nothing is allocated, nothing synchronises, every loop is bounded. */
#define TDS_FOLLOW_MAX_HOPS 8
#define TDS_FOLLOW_MAX_ENTITIES 1024
int tds_lane_follow_step(const tds_lanes_t *lanes, const int64_t *scene_ids, int64_t B, int64_t N, int64_t E, const float *boxes,
                         const float *ent_sc, const float *ent_speed, const uint8_t *ent_present, const int32_t *self_index,
                         const float *npc_size, const float *desired_speed, const uint8_t *npc_present, int32_t *lane, double *arc,
                         int32_t *hops, float *state, float *sc, int32_t *leader, uint64_t seed, float dt, float horizon,
                         float lateral_margin, const float *idm, void *stream);
int tds_lane_follow_step_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t N, int64_t E,
                               const float *boxes, const float *ent_sc, const float *ent_speed, const uint8_t *ent_present,
                               const int32_t *self_index, const float *npc_size, const float *desired_speed, const uint8_t *npc_present,
                               int32_t *lane, double *arc, int32_t *hops, float *state, float *sc, int32_t *leader, uint64_t seed, float dt,
                               float horizon, float lateral_margin, const float *idm, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Giving way at junctions (no reference counterpart: the definition is this library's own; float64 model:
 * tests/give_way_model.py; the expressions: csrc/tds_conflicts.h).  Float64 with + - * / sqrt only.  DRIVABLE = eligible in the sense of
 * tds_spawn_on_lanes_f32; len(l) = the last `cum` of l's centre line.
 *
 * tds_lane_conflicts_f64 fills table, L x (L + 2) float64 owned by the caller (L = the table's lanelets), laid out as
 *   exit      L x L   exit[a][b] at table[a * L + b]
 *   zone_in   L       at table[L * L + a]
 *   zone_out  L       at table[L * L + L + a]
 * For every drivable lanelet a: samples k = 0 .. min(floor(len(a) / step), 2^20) at arcs s_k = (double)k * step, the point of each as in
 * tds_lane_follow_step's pose (the segment that holds s_k on `cum`, t = (s_k - cum[i]) / its 3-D length), 2-D.  For every drivable b that is
 * not EXCLUDED -- b == a, b a successor of a, a a successor of b, a and b successors of a common lanelet -- a sample HITS b iff the least
 * squared distance from it to b's 2-D centre-line segments (the foot of tds_lane_snap) is <= clearance * clearance.  exit[a][b] = the last
 * s_k that hits b, -1 without one (and for every other pair); zone_in[a] = the least over b of the first s_k that hits b, +inf without one;
 * zone_out[a] = the greatest exit[a][b], -1 without one.  a and b CONFLICT iff exit[a][b] >= 0 and exit[b][a] >= 0.  One launch, a workgroup
 * per lanelet.  clearance or step not finite or not > 0 is TDS_EINVAL before any launch, L > TDS_CONFLICT_MAX_LANELETS is TDS_ELIMIT, a table
 * without a successor graph TDS_EINVAL.
 *
 * tds_lane_give_way_multi decides, for the N NPCs of every scene as they are BEFORE the step, who stops before which junction; one launch, a
 * workgroup per scene.  lane, arc, hops, state (B x N x 4, only speed is read), npc_size, npc_present, scene_ids, seed: as for
 * tds_lane_follow_step_multi, whose route stream is used, so that the successors drawn here are the ones that kernel takes.  tables: per lane
 * table of the set the address of its conflict table (int64, 0 = none).  Stop lines (S >= 0 per scene): line_lane B x S int32 (-1: on no
 * lane), line_arc B x S float64, line_red B x S uint8.  Outputs: stop_at B x N float64 (+inf: none), yield_to B x N int32 (-1: none).
 *   Path: l_0 = lane, start_0 = -arc; l_(k+1) = the successor drawn for hop hops + k, start_(k+1) = start_k + len(l_k); it ends when
 *   start_(k+1) >= horizon, after TDS_FOLLOW_MAX_HOPS successors, or at a successor that is not drivable.  With half = length / 2:
 *   Junction: the first l_k with zone_out[l_k] >= 0, start_k + zone_out[l_k] + half > 0 and start_k + zone_in[l_k] <= horizon.  Then
 *   D = start_k + zone_in[l_k], gap = D - half, COMMITTED iff gap <= 0 or v * v >= 2 * b_max * gap, t = max(gap, 0) / max(v, creep_speed).
 *   Rows that are absent, whose lane is not drivable, whose scene has no table, or without a junction take no part.
 *   HELD: not committed, and a stop line with line_red set, line_lane == l_k' for a k' <= k, 0 < start_k' + line_arc < start_k + zone_out[l_k].
 *   NPC i (junction p, not committed) GIVES WAY to j != i (junction q) iff j is not held, exit[q][p] >= 0 and exit[p][q] >= 0,
 *   start_j + exit[q][p] + half_j > 0, and j is committed or (t_j, j) < (t_i, i) lexicographically.  Then stop_at[i] = D_i and yield_to[i] =
 *   the lowest such j.
 * N > TDS_GIVE_WAY_MAX_NPCS is TDS_ELIMIT; horizon or b_max negative or not finite, creep_speed not finite or not > 0 is TDS_EINVAL before any
 * launch.  Nothing is allocated, nothing synchronises, every loop is bounded, no atomics.
 *
 * tds_lane_follow_step_stops_multi is tds_lane_follow_step_multi with one more input, stop_at B x N float64 or NULL (NULL: that entry point
 * bit for bit): after the leader and the dead end, a finite stop_at gives gap_s = stop_at - length / 2, and if there is no leader so far or
 * gap_s < gap: leader = -3, gap = gap_s, v_lead = 0. */
#define TDS_CONFLICT_MAX_LANELETS 2048
#define TDS_GIVE_WAY_MAX_NPCS 1024
int tds_lane_conflicts_f64(const tds_lanes_t *lanes, double *table, float clearance, float step, void *stream);
int tds_lane_give_way_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, const int64_t *tables, int64_t B,
                            int64_t N, const int32_t *lane, const double *arc, const int32_t *hops, const float *state, const float *npc_size,
                            const uint8_t *npc_present, int64_t S, const int32_t *line_lane, const double *line_arc, const uint8_t *line_red,
                            uint64_t seed, float horizon, float b_max, float creep_speed, double *stop_at, int32_t *yield_to, void *stream);
int tds_lane_follow_step_stops_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t N,
                                     int64_t E, const float *boxes, const float *ent_sc, const float *ent_speed, const uint8_t *ent_present,
                                     const int32_t *self_index, const float *npc_size, const float *desired_speed,
                                     const uint8_t *npc_present, int32_t *lane, double *arc, int32_t *hops, float *state, float *sc,
                                     int32_t *leader, const double *stop_at, uint64_t seed, float dt, float horizon, float lateral_margin,
                                     const float *idm, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Route goals (no reference counterpart: the definition is this library's own; float64 model: tests/route_model.py).
 * Everything is float64 with + - * / sqrt only.  Centre lines are 2-D for geometry; arc lengths are on the table's cumulative 3-D lengths
 * `cum` (the convention of tds_lane_snap, so its arc, or one drawn by tds_spawn_on_lanes_f32, is directly usable).  w_i = cum[i + 1] - cum[i].
 *
 * A route (one row = one agent, B x A rows) is n <= TDS_ROUTE_MAX_LANES lanelets route_lanes[0 .. n) (unused entries -1).  Piece j carries
 * the arc interval [a_j, b_j]: a_0 = start_arc, a_j = 0 otherwise; b_(n-1) = end_arc, b_j = the lanelet's length otherwise.  offsets[j] =
 * sum_(i<j) (b_i - a_i), summed front to back (unused entries 0); length = offsets[n].
 *
 * Sampling, from (lane, arc) with requested length D: a = arc clamped to [0, the lanelet's length], rem = D, off = 0; for j = 0 .. 15:
 * lanes[j] = l, offsets[j] = off; if rem <= len(l) - a: end_arc = a + rem, off += end_arc - a, stop; else off += len(l) - a, rem -= len(l) - a,
 * end_arc = len(l); stop at j = 15 (the cap) or at a dead end; else l = the successor for hop j, a = 0.  The successor is
 * succ[(r0 * n_succ) >> 32], r0 the first word of Philox4x32-10 with key (seed low ^ 0x524F5554, seed high ^ 0x474F414C) and counter (scene id
 * low, scene id high, agent index, hop) (not drawn where n_succ = 1).  As in tds_lane_follow_step the draw is over ALL successors: a lanelet
 * without a successor is a dead end, and so is one whose drawn successor is not eligible in the sense of tds_spawn_on_lanes_f32 or carries an
 * excluded tag -- such successors are skipped by ending the route, never by drawing again.  length then records the shortfall.  A row with
 * lane < 0 (or not eligible), an absent row (present == 0), a D that is not > 0 or not finite, a scene without a lane table, or a route whose
 * length is not > 0 gets n = 0 (start_arc = end_arc = length = 0).  Every sampled row also gets cursor = 0, stored = 0, completed = 0; rows
 * with mask == 0 are left untouched (mask NULL: every row).
 *
 * Progress of a pose (x, y, [s, c] = [sin psi, cos psi]) with cursor k (the piece the agent was last found on; never decreases): candidates
 * are the segments of pieces k .. min(k + 2, n - 1).  Segment i of piece j (points P_i, P_(i+1), d = P_(i+1) - P_i in 2-D) is clipped to its
 * piece: ulo = a_j > cum[i] ? (a_j - cum[i]) / w_i : 0, uhi = b_j < cum[i + 1] ? (b_j - cum[i]) / w_i : 1; it is skipped unless d.d > 0, w_i > 0
 * and uhi > ulo.  u = min(max(((x - P_i.x) d.x + (y - P_i.y) d.y) / d.d, ulo), uhi), foot F = P_i + u d, e2 = |F - (x, y)|^2.  The foot is the
 * candidate with the smallest e2, the earliest (piece, segment) on ties.  With t = d / sqrt(d.d) and arc_foot = cum[i] + u w_i:
 *   progress  = offsets[j] + (arc_foot - a_j);   advance = progress - stored, then stored = progress (so advance is measured from the route's
 *               start on the first call after sampling: 0 up to rounding for the pose the route was sampled from)
 *   lateral   = t.x (y - P_i.y) - t.y (x - P_i.x), left positive;   heading = [s t.x - c t.y, c t.x + s t.y] (sin, cos of the heading error)
 *   remaining = length - progress;  reached = remaining <= goal_tolerance;  completed |= reached (sticky);
 *   off_route = sqrt(e2) > off_route_distance;  cursor = j
 * The point at route arc q: q clamped to [0, length] (a q that is not > 0 is 0); piece j = the last one with offsets[j] <= q; lanelet arc =
 * a_j + (q - offsets[j]); segment i = clip(searchsorted(cum, arc, right) - 1, 0, points - 2); u = (arc - cum[i]) / w_i (0 where w_i is not > 0);
 * the point is P_i + u d.  Lookahead point m = 0 .. n_lookahead-1 is the point at progress + (m + 1) * spacing in the agent's frame:
 * [dx c + dy s, dy c - dx s], (dx, dy) = point - (x, y).  Float outputs are rounded to binary32 once, at the end.
 * Rows without a route, absent rows and scenes without a table get zeros everywhere, heading = [0, 1], reached = completed = off_route = 0 and
 * keep cursor and stored; a row whose pose can be weighed against no candidate (NaN) gets the same outputs and keeps completed as well.
 *   xy            row i reads [x, y] at xy[i * xy_stride], xy_stride >= 2 (4 for a B x A x 4 state); sc B x A x 2 [sin, cos]; present B x A uint8 or NULL
 *   lookahead     B x A x n_lookahead x 2, n_lookahead <= TDS_ROUTE_MAX_LOOKAHEAD
 * tds_route_points_multi: q B x A x Q float64 route arcs -> points B x A x Q x 2, world frame ([0, 0] for rows without a route).
 * One launch each; nothing is allocated, nothing synchronises, every loop is bounded whatever the tensors hold.  A negative or non-finite
 * goal_tolerance, off_route_distance or spacing, n_lookahead outside [0, 32] or xy_stride < 2 is TDS_EINVAL before any launch. */
#define TDS_ROUTE_MAX_LANES 16
#define TDS_ROUTE_MAX_LOOKAHEAD 32
int tds_route_sample_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t A,
                           const int32_t *lane, const double *arc, const double *distance, const uint8_t *present, const uint8_t *mask,
                           uint64_t seed, int32_t *route_lanes, int32_t *route_n, double *start_arc, double *end_arc, double *offsets,
                           double *length, int32_t *cursor, double *stored, uint8_t *completed, void *stream);
int tds_route_progress_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, const float *xy, int64_t xy_stride,
                             const float *sc, const uint8_t *present, const int32_t *route_lanes, const int32_t *route_n,
                             const double *start_arc, const double *end_arc, const double *offsets, const double *length, int32_t *cursor,
                             double *stored, uint8_t *completed, float goal_tolerance, float off_route_distance, int n_lookahead,
                             float spacing, float *progress, float *advance, float *lateral, float *heading, float *remaining,
                             uint8_t *reached, uint8_t *off_route, float *lookahead, void *stream);
int tds_route_points_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, int64_t Q, const int32_t *route_lanes,
                           const int32_t *route_n, const double *start_arc, const double *end_arc, const double *offsets,
                           const double *length, const double *q, float *points, void *stream);

/* Differentiable route progress (float64 torch-autograd model: tests/route_grad_model.py): the gradients of progress, advance,
 * remaining, lateral, heading and lookahead of tds_route_progress_multi to the pose, [x, y] and [s, c] = [sin psi, cos psi] (psi gets its
 * gradient through the caller's sin / cos, as everywhere in this header).  The discrete choices of the forward are constants of
 * differentiation: the piece, the segment, which clamp is active, and the lookahead's pieces and segments.
 *
 * The foot.  In the winning segment i of piece j, with d = P_(i+1) - P_i, l2 = d.d, w = w_i, ulo, uhi as above: u_raw = ((x - P_i.x) d.x +
 * (y - P_i.y) d.y) / l2; u moves with the pose iff ulo <= u_raw <= uhi (equality counts as interior, the rule of torch.clamp); then
 * D = d progress / d[x, y] = (w d) / l2, otherwise D = 0.  With t = d / sqrt(l2) and the incoming gradients g_*:
 *   gp    = (g_progress + g_advance) - g_remaining      advance differentiates as progress (the stored progress of the previous step is a
 *                                                       constant), remaining as its negative
 *   g_xy  = gp D + g_lateral [-t.y, t.x]                lateral is measured against the segment's LINE: this holds clamped or not
 *   g_sc  = [g_heading.s t.x + g_heading.c t.y, g_heading.c t.x - g_heading.s t.y]
 * Lookahead point m, with q = progress + (m + 1) * spacing, (px, py) the point at q, inside segment k of its piece with e = P_(k+1) - P_k, and
 * (gox, goy) its incoming gradient: q moves with progress iff 0 < q <= length (the complement of the two clamps of the point at a route arc);
 * then Q = d[px, py] / dq = e / w_k (0 where w_k is not > 0), otherwise Q = 0.  With (ex, ey) = (px - x, py - y):
 *   gq    = gox (Q.x c + Q.y s) + goy (Q.y c - Q.x s)
 *   g_xy += [(goy s - gox c) + gq D.x, gq D.y - (gox s + goy c)];   g_sc += [gox ey - goy ex, gox ex + goy ey]
 * Float64, + - * / and the forward's sqrt of l2 only; the foot's terms and the n_lookahead points' are summed in a fixed order (a result is the
 * same bits from run to run) and each of the four outputs of a row is rounded to binary32 once.  Exact zeros: rows without a foot (a pose no
 * segment can be weighed against: NaN), absent rows, rows with n = 0, scenes without a table.  No gradients to the route tensors, no double
 * backward.
 *   piece         B x A int32: the cursor as tds_route_progress_multi LEFT it for these poses.  No segment is saved: piece `piece` (clamped to
 *                 [0, n - 1]) alone is searched, with the forward's candidates and tie rule, which finds the forward's foot again -- it lay in
 *                 that piece, and a row that found nothing in the window finds nothing in a part of it
 *   g_progress, g_advance, g_lateral, g_remaining B x A, g_heading B x A x 2, g_lookahead B x A x n_lookahead x 2: each may be NULL = zero
 *   g_xy, g_sc    B x A x 2 float32, written in full
 * Everything else as tds_route_progress_multi reads it.  One launch; nothing is allocated, nothing synchronises, every loop is bounded whatever
 * the tensors hold.  n_lookahead outside [0, 32], a negative or non-finite spacing, xy_stride < 2 or a null output is TDS_EINVAL before any
 * launch. */
int tds_route_progress_bwd_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, const float *xy, int64_t xy_stride,
                                 const float *sc, const uint8_t *present, const int32_t *route_lanes, const int32_t *route_n,
                                 const double *start_arc, const double *end_arc, const double *offsets, const double *length,
                                 const int32_t *piece, const float *g_progress, const float *g_advance, const float *g_lateral,
                                 const float *g_heading, const float *g_remaining, const float *g_lookahead, int n_lookahead, float spacing,
                                 float *g_xy, float *g_sc, void *stream);

/* Routes to a destination: shortest paths on the lane graph (float64 model: tests/route_to_model.py).  Float64, + and
 * compares only.  A lanelet is USABLE if it is eligible in the sense of tds_spawn_on_lanes_f32 and carries no excluded tag; len(l) is its
 * cumulative 3-D length, the last `cum` of its centre line.
 *
 * tds_lane_distances_f64 fills to_go, L x L float64 owned by the caller (L = the table's lanelets): to_go[t][l] is the distance from the
 * START of lanelet l to the START of lanelet t along usable lanelets: to_go[t][t] = 0, otherwise to_go[t][l] = len(l) + min over the usable
 * successors s of l of to_go[t][s], +inf where t cannot be reached; the row and the column of a lanelet that is not usable are +inf
 * throughout, its diagonal entry included.  This is the least fixed point of a monotone operator, so it does not depend on the order of
 * relaxation.  One launch, a workgroup per destination, at most L sweeps each.  L > TDS_ROUTE_MAX_GRAPH is TDS_ELIMIT, a table without a
 * successor graph TDS_EINVAL.
 *
 * tds_route_to_multi deals every row (B x A) the shortest route from (lane, arc) to (dest_lane, dest_arc), into the route tensors and the
 * state of tds_route_sample_multi plus rest (B x A float64).  tables: per lane table of the set the address of its to_go (int64, 0 = none).
 * With l0 = lane, t = dest_lane, a0 = arc clamped to [0, len(l0)], b = dest_arc clamped to [0, len(t)] (a value that is not > 0 is 0):
 *   no route (n = 0, rest = +inf): an absent row (present == 0), l0 or t not usable, a scene without a lane table or whose table has no to_go;
 *   t == l0 and b >= a0: one piece, start_arc = a0, end_arc = b, rest = 0;
 *   otherwise piece 0 runs from a0 to the end of l0, and for j = 0 .. 15, at the end of piece j on lanelet l: next = the usable successor s
 *   of l with the smallest to_go[t][s], the first in succ_items order on ties (a destination behind the agent on its own lanelet is reached
 *   round the graph this way); no successor with a finite value: no route, rest = +inf; next == t and b == 0: the route ends here, rest = 0;
 *   j == 15: the route ends here, TRUNCATED, rest = to_go[t][next] + b; next == t: piece j + 1 = t with end_arc = b, rest = 0; else l = next.
 * offsets and length are summed front to back as in sampling (length is not a table entry bit for bit); a route whose length is not > 0
 * is no route (n = 0; rest keeps its 0: the agent stands at its destination).  Every dealt row also gets cursor = 0, stored = 0,
 * completed = 0; rows with mask == 0 are left untouched (mask NULL: every row).  One launch, a thread per row; nothing is allocated, nothing
 * synchronises, every loop is bounded.  Not covered: lane changes (edges to adjacent lanes), more than TDS_ROUTE_MAX_LANES lanelets in one
 * stored route (continue from its end), costs other than length. */
#define TDS_ROUTE_MAX_GRAPH 2048
int tds_lane_distances_f64(const tds_lanes_t *lanes, double *to_go, void *stream);
int tds_route_to_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *tables, int64_t B, int64_t A, const int32_t *lane,
                       const double *arc, const int32_t *dest_lane, const double *dest_arc, const uint8_t *present, const uint8_t *mask,
                       int32_t *route_lanes, int32_t *route_n, double *start_arc, double *end_arc, double *offsets, double *length,
                       int32_t *cursor, double *stored, uint8_t *completed, double *rest, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K5  range scans (no reference counterpart: the definition is this library's own, DESIGN.md "K5"; float64 model: tests/range_scan_model.py)
 * R rays per exposed agent, from its centre, ray k of agent a along the unit vector [cos, sin] = ray_sc[b, a, k, (1, 0)] -- the caller computes
 * [sin, cos] of psi_a + off_k with torch, like every other angle of this header.
 *   boxes       B x E x 5  [x, y, length, width, psi]   all entities = A exposed agents followed by E - A NPCs (psi is not read)
 *   sc          B x E x 2  [sin, cos] of psi;  present B x E uint8;  ray_sc B x A x R x 2
 *   agent_range B x A x R  smallest t >= 0 at which the ray enters the rectangle of another present entity (slab test in the rectangle's
 *                          frame; 0 from inside one); max_range without such a t below max_range
 *   road_range  B x A x R  length of the ray's initial stretch on the map's faces: the least fixed point of F <- max{b_f : a_f <= F + gap_tolerance}
 *                          from F = 0, [a_f, b_f] = where the ray meets the closed face f, over the faces of positive area; capped at max_range;
 *                          ("positive area" is the one test that is NOT binary32: the cross product of two edges in float64 on the float32
 *                          vertices, so that kernel and model drop the same faces; every range is binary32 + - * /)
 *                          max_range everywhere without a map (map == NULL)
 *   hit         B x A x R  int32: the entity that defines agent_range if agent_range < max_range and agent_range <= road_range (lowest index
 *                          on a tie), -2 if road_range < max_range and road_range < agent_range, -1 if both are max_range
 * Rows of exposed agents that are not present: max_range, max_range, -1.  Any of the three outputs may be NULL; without agent_range the rectangles
 * are not tested and hit is computed as if agent_range were max_range.  The map is a geometry-only or a rendering map: only its grid is read.
 * E <= TDS_SCAN_MAX_ENTITIES (the boxes of a scene live in LDS, 32 bytes each).  Nothing is allocated and nothing synchronises; every loop of the
 * kernel is bounded whatever the inputs hold. */
#define TDS_SCAN_MAX_ENTITIES 1024
int tds_range_scan_f32(const tds_map_t *map, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,
                       float *agent_range, float *road_range, int32_t *hit, int64_t B, int64_t A, int64_t E, int R,
                       float max_range, float gap_tolerance, void *stream);
/* the same for scenes with different maps: scene b uses map scene_map[b] of the set (an index outside the set: as without a map) */
int tds_range_scan_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, const float *boxes, const float *sc, const uint8_t *present,
                             const float *ray_sc, float *agent_range, float *road_range, int32_t *hit, int64_t B, int64_t A, int64_t E, int R,
                             float max_range, float gap_tolerance, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K5b  differentiable range scans: the backward of K5 (float64 torch-autograd model: tests/range_scan_grad_model.py; the
 * per-ray derivatives and the edge rule are stated once, in csrc/tds_scan_grad.h, and their numpy restatement in tests/test_scan_grad_host.py
 * equals them bit for bit).
 * Inputs: map, boxes, sc, present, ray_sc, max_range, gap_tolerance as K5 read them ([sin, cos] are independent inputs; the map, max_range and
 * gap_tolerance are constants); road_range B x A x R as K5 wrote it; g_agent, g_road B x A x R float32, the incoming gradients (either may be
 * NULL: that part contributes nothing).
 * Outputs, each optional (NULL):
 *   g_boxes   B x E x 5      to [x, y, length, width, psi]; the psi column is 0: psi is not read, it gets its gradient through sc and ray_sc
 *   g_sc      B x E x 2      to [sin, cos] of every entity
 *   g_ray_sc  B x A x R x 2  to [sin, cos] of every ray
 *   choice    B x A x R x 2  int32 witness: [the entity that defines agent_range or -1, the slab that binds: 0 none, 1 x (length), 2 y (width)]
 *   road_edge B x A x R x 4  float32 witness: [x_i, y_i, x_j, y_j], the world end points of the edge road_range ends on, (x_i, y_i) <= (x_j, y_j)
 *                            lexicographically; NaN where the road contributes nothing
 * With every gradient output NULL the call only writes the witness ("which rectangle side and which road edge a ray ends on"), and g_agent,
 * g_road may be NULL.
 * Precision: every discrete choice is made again in binary32 with K5's own code on K5's own inputs; all derivative arithmetic and all sums are
 * binary64 on the widened float32 inputs, summed in a fixed order and rounded to binary32 once, on the store.  No atomics: two runs give the
 * same bits.
 * Agent part, ray (a, k) of a present observer, with K5's names for entity j: (rx, ry) = origin - centre_j, lx = rx c + ry s, ly = ry c - rx s,
 * ex = dx c + dy s, ey = dy c - dx s, hl, hw the half sizes.  Constants: the entity that defines agent_range (K5's: the lowest index on a tie,
 * whether or not the road is nearer -- hit does not always name it), the slab that binds in K5's order 0, x, y (the y slab binds if its entry
 * exceeds max(0, x entry), else the x slab if its entry exceeds 0, else nothing; a slab with e == 0 never binds), the entry side sigma = -sign(e).
 * Differentiated: t = (sigma h - l) / e of the binding slab, to x, y of the observer, to x, y, length, width (h = size / 2), [sin, cos] of entity
 * j and to [dx, dy] of the ray.  A ray without an entity below max_range, with t0 == 0 (origin inside a rectangle, the clamp binds) or of an
 * absent observer contributes exactly zero whatever comes in, NaN and inf included.
 * Road part: a ray contributes iff 0 < road_range < max_range.  road_range then equals, bit for bit, the far end `hi` of the line-triangle
 * interval of a positive-area face listed in the cells around the end of the stretch r(road_range) (K5's cell rule and margin).  ONE pass over
 * those lists: candidates are the (face, edge) pairs whose face has positive area and hi == road_range and whose edge crosses the line at
 * u == road_range (binary32, K5's arithmetic); every edge is oriented so that its first end point is lexicographically (x, y) the smaller and
 * the smallest 4-tuple (x_i, y_i, x_j, y_j) is taken -- a rule that does not depend on the grid.  Differentiated on that orientation:
 * t = u_i + (u_j - u_i) w_i / (w_i - w_j), p = v - o, u = d . p, w = d x p, to x, y of the observer and to [dx, dy] of the ray; the edge is a
 * constant.  road_range == 0 (origin off the road), road_range >= max_range (capped), no map and absent observers give exactly zero; so does a
 * ray for which no candidate reproduces road_range, and its road_edge says so (NaN).
 * Per entity j each gradient is the binary64 sum, chunk of 256 rays after chunk of the scene's A * R: the rays that end on j in ray order, then
 * (j < A) the observer terms of j's own rays in ray order.  Every output is written in full; the row of an entity no ray touches is exactly 0.
 * Argument rules, limits and codes are K5's, before any launch; the road part needs road_range; B * E == 0 or no output at all is a successful
 * no-op.  One launch; nothing is allocated and nothing synchronises; every loop of the kernel is bounded whatever the inputs hold.  The
 * launch asks for 80 bytes of LDS per entity + 17 KiB: 97 KiB at TDS_SCAN_MAX_ENTITIES. */
int tds_range_scan_bwd_f32(const tds_map_t *map, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,
                           const float *road_range, const float *g_agent, const float *g_road, float *g_boxes, float *g_sc, float *g_ray_sc,
                           int32_t *choice, float *road_edge, int64_t B, int64_t A, int64_t E, int R, float max_range, float gap_tolerance,
                           void *stream);
/* the same for scenes with different maps, as tds_range_scan_multi_f32 */
int tds_range_scan_bwd_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, const float *boxes, const float *sc, const uint8_t *present,
                                 const float *ray_sc, const float *road_range, const float *g_agent, const float *g_road, float *g_boxes,
                                 float *g_sc, float *g_ray_sc, int32_t *choice, float *road_edge, int64_t B, int64_t A, int64_t E, int R,
                                 float max_range, float gap_tolerance, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K6  neighbour observations (no reference counterpart: the definition is this library's own; binary32 model, equal bit for
 * bit: tests/neighbors_model.py).  For every exposed agent the K nearest other entities within max_distance, nearest first, in its own frame.
 * Entities are those of tds_range_scan_f32: the A exposed agents followed by E - A NPCs.
 *   boxes    B x E x 5      [x, y, length, width, psi]; psi is not read
 *   sc       B x E x 2      [sin, cos] of psi;  speed B x E;  present B x E uint8
 *   visible  B x A x E      uint8, optional: non-zero = observer a may see entity e; NULL = everything is visible
 *   features B x A x K x 8  float32;  index B x A x K int32
 * Arithmetic: binary32 throughout, every + - * rounded once (the build passes -ffp-contract=off), so a numpy-float32 model that does the same
 * operations in the same order reproduces the outputs bit for bit.
 * Candidates of observer a (a < A, present[b, a] set) in scene b: every e != a with present[b, e] set, visible[b, a, e] != 0 where visible is
 * given, and d2 <= r2, where dx = x_e - x_a, dy = y_e - y_a, d2 = dx*dx + dy*dy and r2 = max_distance * max_distance, computed once on the
 * host in float32.  A NaN d2 fails the comparison: no candidate.  max_distance = +inf is allowed: every finite pose is then a candidate.
 * Selection: the K candidates with the smallest (d2, e) -- equal d2 is broken by the lower entity index; slot 0 is the nearest.
 * Slot k, 8 floats (32 bytes: two aligned 16-byte stores), with (s, c) the observer's [sin, cos], (se, ce) the neighbour's, v_a / v_e the speeds:
 *   0, 1  x = dx*c + dy*s,  y = dy*c - dx*s                      (the convention of the route lookahead)
 *   2, 3  sin_rel = se*c - ce*s,  cos_rel = ce*c + se*s
 *   4, 5  vx = v_e*cos_rel - v_a,  vy = v_e*sin_rel              (the neighbour's velocity minus the observer's, in the observer's frame)
 *   6, 7  the neighbour's length and width, copied
 * index holds the entity of the slot, -1 for an empty slot; the features of an empty slot are all 0; the row of an observer that is not
 * present is entirely empty; every output is written in full.
 * 1 <= K <= TDS_NEIGHBORS_MAX_K, max_distance not negative and not NaN, A <= E: else TDS_EINVAL before any launch; E > TDS_NEIGHBORS_MAX_ENTITIES
 * (the entities of a scene live in LDS, 32 bytes each) is TDS_ELIMIT; B * A == 0 is a successful no-op.  One launch; nothing is allocated and
 * nothing synchronises; every loop of the kernel is bounded by E and K whatever the tensors hold. */
#define TDS_NEIGHBORS_MAX_K 32
#define TDS_NEIGHBORS_MAX_ENTITIES 1024
int tds_neighbors_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                      float *features, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float max_distance, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K6b  differentiable neighbour observations: the backward of K6 (float64 torch-autograd model: tests/neighbors_grad_model.py;
 * the slot gradient is stated once, in csrc/tds_neighbors_grad.h, and its numpy restatement in tests/test_neighbors_grad_host.py equals it bit
 * for bit).
 * Inputs: boxes, sc, speed as K6 read them; index B x A x K int32 as K6 wrote it; g_features B x A x K x 8 float32, the incoming gradient.
 * Outputs: g_boxes B x E x 5 (the psi column is 0: psi is not read, it gets its gradient through [sin, cos]), g_sc B x E x 2, g_speed B x E.
 * s and c are independent inputs.  Constants of differentiation: which entity is in a slot and the max_distance cut, visible, the order of
 * the slots.
 * Slot (b, a, k) with e = index[b, a, k] is FILLED iff 0 <= e < E and e != a.  Every other slot -- empty, an index that is garbage --
 * contributes exactly zero whatever its g_features holds (a NaN, an infinity), and nothing is read at its index.  A filled slot whose inputs
 * or incoming gradients are not finite propagates what IEEE arithmetic gives.
 * With K6's names, f2 = se*c - ce*s, f3 = ce*c + se*s, and g0 .. g7 the incoming gradient of the slot's features, every operation binary64 on
 * the widened float32 values and rounded once, in this order:
 *   G2 = g2 + g5*v_e, G3 = g3 + g4*v_e;  px = g0*c - g1*s, py = g0*s + g1*c
 *   to entity e:    x: px, y: py, length: g6, width: g7, sin: G2*c + G3*s, cos: G3*c - G2*s, speed: g4*f3 + g5*f2
 *   to observer a:  x: -px, y: -py, sin: ((g0*dy - g1*dx) - G2*ce) + G3*se, cos: ((g0*dx + g1*dy) + G2*se) + G3*ce, speed: -g4
 * Per entity j each of its seven gradients is the binary64 sum over the filled slots of the scene whose index is j (entity side) and over the
 * filled slots of j's own row (observer side, j < A), rounded to binary32 once.  The order of the sum is fixed (16 lanes per entity: per lane
 * the slots that name j in slot order, then the lane's slots of j's own row, then a butterfly over the 16 lanes); no atomics: two runs give the same bits.  Every
 * output is written in full; the row of an entity no filled slot touches is exactly 0.
 * Argument rules, limits and codes are K6's (max_distance is not an argument); B * E == 0 is a successful no-op; with A == 0 index and
 * g_features may be NULL and every row is written as zeros.  One launch; nothing is allocated and nothing synchronises; every loop of the
 * kernel is bounded by A, E and K whatever index holds. */
int tds_neighbors_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_features,
                          float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K7  traffic lights on the device (models, equal bit for bit: tests/lights_model.py).
 *
 * (a) The programmes.  M machines of at most P phases drive N lights; the tables are shared by the B scenes of a batch, the clocks are per scene:
 *   duration    M x P float64     seconds of phase p of machine m (rows of shorter machines are padded)
 *   next_phase  M x P int32       LIST POSITION of the phase that follows (what TrafficLightStateMachine.tick indexes its list with)
 *   n_phases    M int32           phases of machine m, 1 .. P
 *   colour      M x P x N uint8   the state light n shows in that phase, 255 where the phase does not name the light
 *   phase       B x M int32       in and out: list position of the current phase;  remaining B x M float64, in and out: seconds left in it
 *   state       B x N int64, time_to_change B x N float32: out;  mask B uint8 or NULL: scenes with a zero are left exactly as they are
 * tds_lights_step, for every masked scene:
 *   1. with `advance` non-zero every machine does, in float64 with + - and comparisons only, p its phase and r its remaining time:
 *        left = r - dt;  if left > 0: r = left.  Otherwise at most TDS_LIGHTS_MAX_SKIPS times:
 *          nxt = next_phase[m][p], span = duration[m][nxt];
 *          if left == 0: p = nxt, r = span, stop;
 *          left += span;  if left > 0: p = nxt, r = left if left <= span else span, stop;
 *          p = nxt;
 *        and when the cap is exhausted p = nxt, r = span.  This is TrafficLightStateMachine.tick operation for operation (the one copy of it that
 *        host and device compile is csrc/tds_lights.h).
 *   2. then every light n takes colour[m][p_m][n] of the LAST machine m (the highest index) whose current phase names it -- the order of the
 *      host's merged.update -- and time_to_change[b, n] is that machine's remaining time rounded to binary32.  A light that no current phase
 *      names keeps what it had.  advance == 0 does step 2 alone.
 * dt points to ONE double in host memory, read before the launch (a scalar of the call; the kernel gets the value).
 * tds_lights_reset puts every machine of the masked scenes at the beginning of phase (r0 * n_phases[m]) >> 32, r0 the first word of
 * Philox4x32-10 with key (seed low ^ 0x4C494748, seed high ^ 0x54535452) and counter (scene id low, scene id high, m, 0), and sets remaining to
 * that phase's duration; state and time_to_change follow with tds_lights_step(advance = 0).
 * M > TDS_LIGHTS_MAX_MACHINES, P > TDS_LIGHTS_MAX_PHASES or N > TDS_LIGHTS_MAX_LIGHTS is TDS_ELIMIT; a negative or non-finite dt is TDS_EINVAL
 * before any launch; B == 0 is a successful no-op.  One launch each, nothing is allocated, nothing synchronises; every index read from device
 * memory (phase, next_phase, n_phases) is clamped to its table before use and every loop is bounded whatever the tables hold. */
#define TDS_LIGHTS_MAX_MACHINES 256
#define TDS_LIGHTS_MAX_PHASES 64
#define TDS_LIGHTS_MAX_LIGHTS 1024
#define TDS_LIGHTS_MAX_SKIPS 1024
int tds_lights_step(const double *duration, const int32_t *next_phase, const int32_t *n_phases, const uint8_t *colour, int32_t *phase,
                    double *remaining, int64_t *state, float *time_to_change, const uint8_t *mask, int64_t B, int64_t M, int64_t P, int64_t N,
                    const double *dt, int advance, void *stream);
int tds_lights_reset(const int32_t *n_phases, const double *duration, int32_t *phase, double *remaining, const uint8_t *mask,
                     const int64_t *scene_ids, int64_t B, int64_t M, int64_t P, uint64_t seed, void *stream);

/* (b) Stop-line observations (no reference counterpart).  For every exposed agent the K nearest stop lines of one traffic control within
 * max_distance between centres, nearest first, in the agent's frame; K6's conventions.
 *   agent_xy B x A x 2, agent_sc B x A x 2 [sin, cos], agent_present B x A uint8
 *   lines B x N x 5 [x, y, length, width, psi] (psi is not read), line_sc B x N x 2 [sin, cos] of psi, mask B x N uint8 (0: padding)
 *   state B x N int64 (the control's state), time_to_change B x N float32 or NULL (read as 0)
 *   features B x A x K x 8 float32, index B x A x K int32, slot_state B x A x K int32
 * Binary32 throughout, every operation rounded once.  With (s, c) the observer's [sin, cos] and (sl, cl) the line's:
 *   dx = x_n - x_a, dy = y_n - y_a, d2 = dx*dx + dy*dy;  x = dx*c + dy*s, y = dy*c - dx*s;  sin_rel = sl*c - cl*s, cos_rel = cl*c + sl*s.
 * Candidates of a present observer: the lines n with mask[b, n] set, d2 <= r2 (r2 = max_distance * max_distance, computed once on the host in
 * float32), with ahead_only x >= 0, and cos_rel >= min_cos (-inf: no such filter).  A NaN fails every test.  Selection: the K smallest (d2, n).
 * Slot k: x, y, sin_rel, cos_rel, length, width, time_to_change[b, n], sqrt(d2) (correctly rounded); index = n; slot_state = state[b, n] as
 * int32.  Empty slots are all 0 with index -1 and slot_state -1; the row of an absent observer is all empty; every output is written in full.
 * 1 <= K <= TDS_STOP_LINES_MAX_K, max_distance not negative and not NaN, min_cos not NaN: else TDS_EINVAL; N > TDS_LIGHTS_MAX_LIGHTS (the lines of
 * a scene live in LDS, 32 bytes each) is TDS_ELIMIT; B * A == 0 is a successful no-op.  One launch, nothing allocated, nothing synchronises. */
#define TDS_STOP_LINES_MAX_K 32
int tds_stop_lines_f32(const float *agent_xy, const float *agent_sc, const uint8_t *agent_present, const float *lines, const float *line_sc,
                       const uint8_t *mask, const int64_t *state, const float *time_to_change, float *features, int32_t *index,
                       int32_t *slot_state, int64_t B, int64_t A, int64_t N, int K, float max_distance, int ahead_only, float min_cos,
                       void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K7b  differentiable stop-line observations: the backward of K7 (b) (float64 torch-autograd model:
 * tests/stop_lines_grad_model.py; the slot gradient and the order of a row's sum are stated once, in csrc/tds_stop_lines_grad.h, and their numpy
 * restatement in tests/test_stop_lines_grad_host.py equals them bit for bit).
 * Inputs: agent_xy, agent_sc, lines, line_sc as K7 read them; index B x A x K int32 as K7 wrote it; g_features B x A x K x 8 float32, the
 * incoming gradient, which must start at a multiple of 16 bytes (else TDS_EINVAL).
 * Outputs: g_xy B x A x 2, g_sc B x A x 2: the gradients to the observing agent's own x, y and [sin, cos].  s and c are independent inputs.  The
 * lines are constants and get nothing.  Constants of differentiation: which line is in a slot and the order of the slots, the max_distance
 * cut, ahead_only, min_cos, mask.
 * Slot (b, a, k) with n = index[b, a, k] is FILLED iff 0 <= n < N.  Every other slot -- empty, an index that is garbage -- contributes exactly
 * zero whatever its g_features holds (a NaN, an infinity), and nothing is read at its index.  A filled slot whose inputs or incoming gradients
 * are not finite propagates what IEEE arithmetic gives.
 * With K7's names, and g0 .. g7 the incoming gradient of the slot's features, every operation binary64 on the widened float32 values and
 * rounded once, in this order:
 *   dx = x_n - x_a, dy = y_n - y_a;  r = sqrt(dx*dx + dy*dy)  (recomputed: not the forward's rounded distance)
 *   q = g7 / r, and exactly 0 where r == 0  (an agent standing exactly on a line's centre gets no NaN from the distance)
 *   to x_a:  -(g0*c - g1*s) - q*dx          to y_a:  -(g0*s + g1*c) - q*dy
 *   to s:    ((g0*dy - g1*dx) - g2*cl) + g3*sl      to c:  ((g0*dx + g1*dy) + g2*sl) + g3*cl
 * length, width and time_to_change are copies of constants: g4, g5 and g6 go nowhere and are not read.
 * Per observer each of its four gradients is the binary64 sum over its K slots, rounded to binary32 once.  The order of the sum is fixed: 4
 * lanes per observer; lane l starts from +0 and adds its filled slots l, l + 4, l + 8, ... in that order; then two rounds m = 2, 1 in which lane l
 * takes (its sum) + (the sum of lane l ^ m); lane 0 has the result.  No atomics: two runs give the same bits.  Every output is written in full;
 * the rows of an observer without a filled slot -- an absent agent's among them -- are exactly 0.
 * Argument rules, limits and codes are K7's (max_distance, ahead_only and min_cos are not arguments); B * A == 0 is a successful no-op.  One
 * launch; nothing is allocated and nothing synchronises; every loop of the kernel is bounded by A, N and K whatever index holds. */
int tds_stop_lines_bwd_f32(const float *agent_xy, const float *agent_sc, const float *lines, const float *line_sc, const int32_t *index,
                           const float *g_features, float *g_xy, float *g_sc, int64_t B, int64_t A, int64_t N, int K, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K8  lane observations (no reference counterpart: the definition is this library's own; float64 model, equal bit for bit:
 * tests/lane_obs_model.py).  For every exposed agent the K nearest lanelets of its scene's lane table within max_distance of their centre
 * lines, nearest first; each slot is the foot on the centre line in the agent's frame plus a polyline of P points ahead of the foot that
 * follows the lane graph while the way is unambiguous.
 *   agent_xy B x A x 2, agent_sc B x A x 2 [sin, cos], present B x A uint8
 *   features B x A x K x 8 float32, points B x A x K x P x 2 float32, n_valid B x A x K int32, index B x A x K int32
 * Arithmetic: binary64 on the lane table, every + - * / sqrt rounded once (the build passes -ffp-contract=off); the poses are read as float32
 * and widened; every output float is the double result rounded once to binary32.
 * Observer (b, a) with pose (x, y) and heading (s, c): its row is EMPTY if present[b, a] == 0, the scene has no lane table (scene_map[b]
 * outside the set), or any of x, y, s, c is a NaN.
 * Candidates: every lanelet l of the table that is eligible in the sense of tds_spawn_on_lanes_f32 (>= 2 centre-line points, a finite positive
 * length) and carries no excluded tag (flag bit 0) -- the rule of tds_lane_snap.
 * Foot: the closest point of the lanelet's 2-D centre line, found as tds_lane_snap finds it.  Segment i from (ax, ay) with (dx, dy) to the next point:
 *   l2 = dx*dx + dy*dy;  u = l2 > 0 ? ((x - ax)*dx + (y - ay)*dy) / l2 : 0, clamped to [0, 1] (a NaN: 0);
 *   fx = ax + u*dx - x, fy = ay + u*dy - y;  d2 = fx*fx + fy*fy.
 * The segments in ascending order, the first d2 below +inf starts, a strictly smaller d2 replaces it: sb is the earliest segment of the smallest
 * d2.  A lanelet none of whose d2 is below +inf (all NaN or +inf) is no candidate.
 * In range: d2 <= r2, r2 = (double)max_distance * (double)max_distance.  max_distance = +inf is allowed.
 * Selection: the K candidates in range with the smallest (bits of (float)d2, l) -- equal binary32 distance is broken by the lower lanelet index;
 * slot 0 is the nearest.
 * Slot features, 8 floats (two aligned 16-byte stores), with (tx, ty) = (dx, dy) / sqrt(l2) of segment sb, (0, 0) if l2 == 0, and cum the
 * lanelet's cumulative 3-D lengths (cum[last] = its length):
 *   0, 1  fx*c + fy*s,  fy*c - fx*s                  the foot in the observer's frame (the convention of the route lookahead and of K6)
 *   2, 3  sin_rel = ty*c - tx*s,  cos_rel = tx*c + ty*s   the lane's direction at the foot against the heading (an oncoming lane: cos_rel < 0)
 *   4     arc = cum[sb] + u*(cum[sb + 1] - cum[sb])  (the expression of tds_lane_snap)
 *   5     remaining = cum[last] - arc
 *   6     lateral = tx*(y - ay) - ty*(x - ax)        (left positive, as tds_lane_snap)
 *   7     distance = sqrt(d2)
 * Slot points: point j lies at q_j = arc + (double)j * (double)spacing along the lane.  The walk of point j starts on cur = l with base = 0 and
 * no hops made; len(cur) = cum[last] of cur.  While q_j - base > len(cur): if cur has exactly ONE successor in the lane graph, that successor is
 * a candidate in the sense above and fewer than TDS_LANE_OBS_MAX_HOPS hops were made, then base += len(cur), cur = the successor, one more
 * hop; otherwise the point is invalid -- and so are all later ones, the walk of a later point passing through the same states.  A valid point:
 *   pos = q_j - base;  k = clip(searchsorted(cum, pos, 'right') - 1, 0, n - 2);  w = cum[k + 1] - cum[k];  t = w > 0 ? (pos - cum[k]) / w : 0;
 *   wx = px_k + t*(px_(k+1) - px_k), wy likewise (the convention of the route points);  ex = wx - x, ey = wy - y;
 *   the point is (ex*c + ey*s, ey*c - ex*s).
 * n_valid is the number of valid points: at least 1 in a filled slot (point 0 is the centre-line point at arc); invalid points are (0, 0).  A
 * fork or a dead end ends the polyline; the branches are slots of their own where they are in range.  A table without a lane graph
 * (tds_lanes_set_successors) has no successors.
 * index is the lanelet of the slot in its scene's table, -1 for an empty slot, whose features and points are 0 and whose n_valid is 0.  Every
 * output is written in full.
 * 1 <= K <= TDS_LANE_OBS_MAX_K, 1 <= P <= TDS_LANE_OBS_MAX_POINTS, spacing finite and positive, max_distance not negative and not NaN: else
 * TDS_EINVAL before any launch; a table of more than TDS_LANE_OBS_MAX_LANELETS lanelets (the limit of tds_lane_distances_f64) is TDS_ELIMIT;
 * a set of several tables needs scene_map; B * A == 0 is a successful no-op.  One launch; nothing is allocated and nothing synchronises;
 * every loop of the kernel is bounded by the table's sizes, K, P or the hop limit whatever the tensors hold. */
#define TDS_LANE_OBS_MAX_K 32
#define TDS_LANE_OBS_MAX_POINTS 32
#define TDS_LANE_OBS_MAX_HOPS 8
#define TDS_LANE_OBS_MAX_LANELETS 2048
int tds_lane_observations_multi(const tds_laneset_t *set, const int32_t *scene_map, const float *agent_xy, const float *agent_sc,
                                const uint8_t *present, float *features, float *points, int32_t *n_valid, int32_t *index, int64_t B,
                                int64_t A, int K, int P, float spacing, float max_distance, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K8b  differentiable lane observations: the backward of K8 (float64 torch-autograd model: tests/lane_obs_grad_model.py; the
 * contributions of a slot and of a point are stated once, in csrc/tds_lane_obs_grad.h, and their numpy restatement in
 * tests/test_lane_obs_grad_host.py equals them bit for bit).  The map is constant: the gradient goes to the observing agent's own pose alone.
 * Inputs: agent_xy, agent_sc as K8 read them; index B x A x K int32 as K8 wrote it; g_features B x A x K x 8 and g_points B x A x K x P x 2
 * float32, the incoming gradients -- either may be NULL, which reads as all zero.
 * g_features must be 16-byte aligned and g_points 8-byte aligned (a slot's features are read as two 16-byte loads, a point as one of 8).
 * Outputs: g_xy B x A x 2 and g_sc B x A x 2 float32.  Every element is written; the row of an observer with no contributing slot is exactly 0.
 * s and c are independent inputs.  Constants of differentiation: which lanelet is in a slot and the order of the slots, the max_distance cut,
 * the foot's segment sb, whether u was clamped, and for every point its validity, the lanelet its walk ends on and the segment k there.
 * Slot (b, a, k) with l = index[b, a, k] is FILLED iff the scene has a lane table, 0 <= l < n of that table and l is a candidate in K8's sense
 * (eligible, no excluded tag, a d2 below +inf for this pose) and none of x, y, s, c is a NaN.  Every other slot -- empty, an index that is
 * garbage, a scene without a table, a NaN pose -- contributes exactly zero whatever its incoming gradients hold (a NaN, an infinity), and nothing is read at its index.  Whether a
 * point is valid comes from redoing K8's walk with K8's arithmetic (n_valid is not an input); an invalid point contributes exactly zero.  A
 * filled slot or valid point whose incoming gradient is not finite propagates what IEEE arithmetic gives.
 * With K8's names, every operation binary64 on the widened float32 values and rounded once, in this order.  Per filled slot, with (dx, dy), l2,
 * (fx, fy), d2 of segment sb, (tx, ty), W = cum[sb + 1] - cum[sb], and g0 .. g7 the incoming gradient of its features:
 *   u0 = l2 > 0 ? ((x - ax)*dx + (y - ay)*dy) / l2 : 0;  m = l2 > 0 and 0 < u0 < 1                 (the unclamped u: a NaN gives m = 0)
 *   a = m ? ((W*dx) / l2, (W*dy) / l2) : (0, 0)                                                      (d arc / d(x, y))
 *   qx = g0*c - g1*s, qy = g0*s + g1*c;  tq = tx*qx + ty*qy;  G = g4 - g5;  dist = sqrt(d2)
 *   x: ((m ? tq*tx - qx : -qx) + G*a.x) - g6*ty, then - g7*(fx / dist) iff dist > 0
 *   y: ((m ? tq*ty - qy : -qy) + G*a.y) + g6*tx, then - g7*(fy / dist) iff dist > 0
 *   sin: (g0*fy - g1*fx) + (g3*ty - g2*tx);   cos: (g0*fx + g1*fy) + (g2*ty + g3*tx)
 * (d f / d(x, y) = m t t^T - I.  distance's term m*(f.t)*t / dist is left out: f is perpendicular to t wherever m = 1, so the term is zero in
 * exact arithmetic.  An agent exactly on a centre line, dist == 0, gets nothing through feature 7 and no NaN.)
 * Per valid point j of the slot on segment k of its final lanelet, w = cum[k + 1] - cum[k], with (gx, gy) its incoming gradient:
 *   h = w > 0 ? ((px_(k+1) - px_k) / w, (py_(k+1) - py_k) / w) : (0, 0);  rx = gx*c - gy*s, ry = gx*s + gy*c;  hr = hx*rx + hy*ry
 *   x: hr*a.x - rx;  y: hr*a.y - ry;  sin: gx*ey - gy*ex;  cos: gx*ex + gy*ey
 * (hr * a is the polyline sliding along the lane as the agent moves; it vanishes where the foot is clamped.)
 * Per observer each of its four gradients is the binary64 sum of these contributions, rounded to binary32 once, in a fixed order: 64 lanes;
 * lane i first takes the features of slot i (i < K), then the pairs (slot, point) = i, i + 64, ... of the row-major K x P pairs in ascending
 * order, each sum starting at 0; then a butterfly over the 64 lanes (xor 32, 16, 8, 4, 2, 1).  No atomics: two runs give the same bits.
 * Argument rules, limits and codes are K8's (max_distance and present are not arguments: an absent observer's slots are empty); B * A == 0 is a
 * successful no-op.  One launch; nothing is allocated and nothing synchronises; every loop of the kernel is bounded by the table's sizes, K, P
 * or the hop limit whatever index holds. */
int tds_lane_observations_bwd_multi(const tds_laneset_t *set, const int32_t *scene_map, const float *agent_xy, const float *agent_sc,
                                    const int32_t *index, const float *g_features, const float *g_points, float *g_xy, float *g_sc, int64_t B,
                                    int64_t A, int K, int P, float spacing, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K9  time to collision (no reference counterpart: the definition is this library's own; float64 model, equal bit for bit:
 * tests/ttc_model.py; the pair test is stated once, in csrc/tds_ttc.h).  For every exposed agent the K other entities it would touch first
 * within `horizon` seconds, soonest first, and when -- every entity keeping its velocity v * [cos psi, sin psi] and its heading.
 * Inputs are those of tds_neighbors_f32 (K6): boxes B x E x 5 (psi is not read), sc B x E x 2 [sin, cos], speed B x E, present B x E uint8,
 * visible B x A x E uint8 or NULL.  Outputs: ttc B x A x K float32, index B x A x K int32.
 * Arithmetic: the float32 inputs are widened exactly; binary64 throughout; only + - * /, fabs and comparisons, each rounded once (the build
 * passes -ffp-contract=off); a result is rounded to binary32 once, at the end.
 * Observer a (a < A) against entity e, with (x, y, l, w, s, c, v) of each: e != a; present[b, a] and present[b, e] set; visible[b, a, e] != 0
 * where visible is given; all seven values of both finite -- tested first: a non-finite entity is no candidate, a non-finite observer has an
 * empty row.  Then
 *   hla = 0.5*l_a + margin, hwa = 0.5*w_a + margin   (the observer grows by the margin on every side);  hle = 0.5*l_e, hwe = 0.5*w_e
 *   dx = x_e - x_a, dy = y_e - y_a;  rvx = v_e*c_e - v_a*c_a, rvy = v_e*s_e - v_a*s_a;  lo = -inf, hi = +inf
 * and for the four axes (nx, ny) = (c_a, s_a), (-s_a, c_a), (c_e, s_e), (-s_e, c_e), in this order:
 *   p = dx*nx + dy*ny;  w = rvx*nx + rvy*ny
 *   R = hla*|c_a*nx + s_a*ny| + hwa*|c_a*ny - s_a*nx| + hle*|c_e*nx + s_e*ny| + hwe*|c_e*ny - s_e*nx|     summed left to right
 *   w == 0:  no candidate if |p| > R, else the axis constrains nothing
 *   else:    t0 = (-R - p)/w, t1 = (R - p)/w, swapped if t0 > t1;  if (t0 > lo) lo = t0;  if (t1 < hi) hi = t1
 * The pair is a candidate iff lo <= hi && hi >= 0 && lo <= (double)horizon; its time is t = lo > 0 ? lo : 0.0 (never -0.0; 0 for a pair that
 * overlaps already) and ttc = (float)t.
 * Selection: the K candidates with the smallest (bits of ttc, e) -- equal float32 times are broken by the lower entity index; slot 0 is the
 * soonest.  Empty slots hold +inf and -1; the row of an observer that is absent or not finite is entirely empty; every output is written in full.
 * 1 <= K <= TDS_TTC_MAX_K, horizon not negative and not NaN (+inf is allowed), margin finite, A <= E: else TDS_EINVAL before any launch;
 * E > TDS_TTC_MAX_ENTITIES (the entities of a scene live in LDS, 32 bytes each) is TDS_ELIMIT; B * A == 0 is a successful no-op.  Negative
 * sizes or margins get no special case: the arithmetic decides.  One launch; nothing is allocated and nothing synchronises; every loop of the
 * kernel is bounded by E and K whatever the tensors hold. */
#define TDS_TTC_MAX_K 32
#define TDS_TTC_MAX_ENTITIES 1024
int tds_time_to_collision_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                              float *ttc, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float horizon, float margin, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * K9b  differentiable time to collision: the backward of K9 (float64 torch-autograd model: tests/ttc_grad_model.py; the pair
 * gradient is stated once, in csrc/tds_ttc_grad.h, and its numpy restatement in that model equals it bit for bit).
 * Inputs: boxes, sc, speed as K9 read them; index B x A x K int32 as K9 wrote it; g_ttc B x A x K float32, the incoming gradient of ttc.
 * Outputs: g_boxes B x E x 5 (the psi column is 0: psi is not read, it gets its gradient through [sin, cos]), g_sc B x E x 2, g_speed B x E.
 * s and c are independent inputs; margin and horizon get no gradient.
 * Slot (b, a, k) with e = index[b, a, k] CONTRIBUTES iff 0 <= e < E and e != a, all seven values of both boxes are finite, and lo > 0, where
 * lo is K9's, recomputed with K9's binary64 expressions over the axes with w != 0 (the observer grown by margin).  Every other slot -- empty,
 * a pair that overlaps already (t = 0), an index that is garbage -- contributes exactly zero whatever its g_ttc holds (a NaN, an infinity).
 * The forward's discrete choices are constants: the binding axis n = (nx, ny) is the FIRST of the four axes, in K9's order, whose t0 (after the
 * swap) equals lo -- K9's strict t0 > lo update; sigma = sign(w) on it; the signs of the four fabs arguments of R, with sign(0) = 0.  Then
 * t = lo = (-sigma*R - p)/w, and with N = sigma*R + p + t*w:  d t = -dN/w at constant t, that is with q = d + t*rv
 *   dt = -( sigma*dR + n.dd + t*(n.drv) + q.dn ) / w.
 * The 14 partials, every operation binary64 and rounded once, in this order (a: observer, e: other; hl, hw as in K9):
 *   a1 = c_a*nx + s_a*ny, a2 = c_a*ny - s_a*nx, e1 = c_e*nx + s_e*ny, e2 = c_e*ny - s_e*nx;  inv = -1/w
 *   ka1 = sigma*(hla*sign(a1)), ka2 = sigma*(hwa*sign(a2)), ke1 = sigma*(hle*sign(e1)), ke2 = sigma*(hwe*sign(e2))
 *   qx = dx + t*rvx, qy = dy + t*rvy
 *   gnx = ((ka1*c_a - ka2*s_a) + (ke1*c_e - ke2*s_e)) + qx;  gny = ((ka1*s_a + ka2*c_a) + (ke1*s_e + ke2*c_e)) + qy
 *   nca = (ka1*nx + ka2*ny) - t*(v_a*nx), nsa = (ka1*ny - ka2*nx) - t*(v_a*ny), nce = (ke1*nx + ke2*ny) + t*(v_e*nx), nse = (ke1*ny - ke2*nx) + t*(v_e*ny)
 *   axis 0: nca += gnx, nsa += gny;  axis 1: nsa -= gnx, nca += gny;  axis 2: nce += gnx, nse += gny;  axis 3: nse -= gnx, nce += gny
 *   x_e: nx*inv, y_e: ny*inv, x_a: -(nx*inv), y_a: -(ny*inv);  length_a: (sigma*(0.5*|a1|))*inv, width_a: (sigma*(0.5*|a2|))*inv, length_e and
 *   width_e likewise with e1, e2;  sin_a: nsa*inv, cos_a: nca*inv, sin_e: nse*inv, cos_e: nce*inv;  speed_a: -((t*a1)*inv), speed_e: (t*e1)*inv.
 * Per entity j each of its seven gradients is the binary64 sum of g_ttc[slot] * partial over the contributing slots of j's own row (observer
 * side, j < A) and of every slot of the scene whose index is j (other side), rounded to binary32 once.  The order of the sum is fixed (per lane
 * in slot order, then a butterfly over the lanes); no atomics: two runs give the same bits.  Every output is written in full; the row of an
 * entity with no contribution is exactly 0.
 * Argument rules, limits and codes are K9's (horizon is not an argument); B * E == 0 is a successful no-op; with A == 0 index and g_ttc may be
 * NULL.  One launch; nothing is allocated and nothing synchronises; every loop of the kernel is bounded by A, E and K whatever index holds, and
 * an index outside [0, E) is never dereferenced. */
int tds_time_to_collision_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_ttc,
                                  float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, float margin, void *stream);

/* ---- testing hooks ------------------------------------------------------------------------------------------------------------
 * NOT part of the product: libtdship.so exports none of these.  They exist in libtdship_testing.so, the same sources compiled with
 * -DTDS_TESTING, which tools/ (ablations, work counters) and a few tests (forcing the slow code paths) load instead. */
/* The flags of tds_raster_set_debug (ablations, work counters and forced launch forms of K3, the scene rasteriser).  Defined in both builds:
 * the product's kernels name them too, where TDS_DBG() compiles them out. */
#define TDS_RASTER_DBG_NO_STATIC 1             /* no static map */
#define TDS_RASTER_DBG_NO_ACTORS 2             /* no actors */
#define TDS_RASTER_DBG_NO_STORE 4              /* no store of the image */
#define TDS_RASTER_DBG_NO_EDGES 8              /* no outline edges: no edge classes and no walk */
#define TDS_RASTER_DBG_NO_SCAN 16              /* no scan conversion */
#define TDS_RASTER_DBG_NO_BINNED 32            /* never the binned packed-key path */
#define TDS_RASTER_DBG_NO_BITS 64              /* never the bit planes */
#define TDS_RASTER_DBG_STATS 128               /* work counters on (tds_raster_get_stats) */
#define TDS_RASTER_DBG_NO_EDGE_WALK 256        /* the edge classes stay, only the walk of outline edges goes */
#define TDS_RASTER_DBG_NO_SETUP 512            /* no per-face set-up (nothing is painted) */
#define TDS_RASTER_DBG_NO_PROJECT 1024         /* walk the grid but project nothing */
#define TDS_RASTER_DBG_MINWG3 2048             /* the 170-VGPR instantiation everywhere */
#define TDS_RASTER_DBG_XCD_CLOCKS 4096         /* the work counters hold per-XCD finish [0..7] and ~start [8..15] wall clocks (100 MHz) */
#define TDS_RASTER_DBG_NO_SPLIT 8192           /* never the split form (K3s + K3r) */
#define TDS_RASTER_DBG_SPLIT 16384             /* the split form wherever a workspace allows it */
#define TDS_RASTER_DBG_NO_SHORT_PATH 32768     /* K3r without its short path for small faces */
#define TDS_RASTER_DBG_GRID8 65536             /* the persistent launch with 8 workgroups per CU (round 3's surplus) instead of the resident number */
#define TDS_RASTER_DBG_GRID4 131072            /* ... with 4 */
#define TDS_RASTER_DBG_WHOLE_4WAVES 262144     /* an image whose planes do not fit three workgroups per CU (six and more keys at 256 x 256): whole in
                                                  4-wave workgroups instead of whole in 8-wave ones */
#define TDS_RASTER_DBG_NO_8WAVES 524288        /* ... in half-image strips instead */
#define TDS_RASTER_DBG_WIDEST_STRIPS 1048576   /* strips as wide as the LDS allows instead of equal ones (nine and more keys) */
#define TDS_RASTER_DBG_NO_EXTRA_STRIP 2097152  /* never one strip more than necessary (nine and more keys) */
#define TDS_RASTER_DBG_PROLOGUE_TWICE 4194304  /* the fused bit-plane kernel runs its per-item prologue (trim polygon, scan window, grid rows) a second
                                                  time and drops the result: the difference to a plain launch is what the prologue costs */
#define TDS_RASTER_DBG_DROP_SMALL 8388608      /* the fused bit-plane kernel drops, instead of queueing, every accepted face with all three vertices inside
                                                  the image and at most TDS_RASTER_SMALL_ROWS rows: the difference to a plain launch is what these
                                                  faces cost on the general path */
#define TDS_RASTER_DBG_SMALL_FREE_SLOPES 16777216  /* the on-lane block for small faces takes the packed vertices for its three slopes instead of computing
                                                  them: wrong pixels, timing and counters only -- the difference to a plain launch is what the slopes cost */
#define TDS_RASTER_DBG_SMALL_NO_MIDDLE_ROW 33554432 /* ... paints the row of the middle vertex, where it lies between the others, as a row of part 1: wrong
                                                  pixels -- the difference is what that row's own expressions cost */
#define TDS_RASTER_DBG_HELPER 67108864         /* never set by a caller: the testing build sets it in the arguments of the helper enqueue (tds_raster_aux_helper_t::
                                                  helper_stream), so that the work counters can tell its items (tds_raster_get_helper_stats) */
#define TDS_RASTER_DBG_NO_ACTOR_WAVE 134217728 /* the persistent 4-wave bit-plane kernel leaves a work item's agents, and the masked agents' dot, to ONE wave
                                                  of the workgroup (chosen by the item number: one lane per agent for the distance cull, faces for the
                                                  visible agents only) while the others start on the map at once; with this flag every wave culls and
                                                  projects its share of the agents, as the other launches do.  Same pixels. */
#ifndef TDS_RASTER_SMALL_ROWS
#define TDS_RASTER_SMALL_ROWS 7                /* rows (yb - yt + 1) of the largest face that is small: the persistent bit-plane kernel paints such faces
                                                  on the lane that scanned them; the flag above and the counters below go by the same test */
#endif

#ifdef TDS_TESTING
/* force the LDS strip width of K3 (0 = automatic, else 8 .. 128 output rows) */
int tds_raster_set_strip_width(int tw);
/* waves per workgroup of the bit-plane raster kernel (4 or 8) */
int tds_raster_set_bits_waves(int n);
/* K3r, the list rasteriser of the split bit-plane path: LDS budget per workgroup in KiB (sets the strip width) */
int tds_raster_set_list_lds(int lds_kb);
/* K3r: waves per workgroup (2 or 4; 0 = chosen by the size of a strip) */
int tds_raster_set_list_waves(int waves);
/* ablation switches of K3: an OR of the TDS_RASTER_DBG_* flags above */
int tds_raster_set_debug(int flags);
/* the helper launch (tds_raster_aux_helper_t::helper_stream) is made from this many work items per workgroup of the launch's own grid on (product: 4; >= 0) */
int tds_raster_set_helper_min_items(int items_per_workgroup);
/* read and reset the counter of work items that workgroups of the helper enqueue rendered (TDS_RASTER_DBG_STATS); the two counters of
 * tds_raster_get_prep_stats count every item, whichever enqueue took it */
int tds_raster_get_helper_stats(unsigned long long *out1);
/* read and reset the counter of work items of the persistent 4-wave bit-plane launches whose agents were served by one wave of the workgroup
 * (TDS_RASTER_DBG_STATS): every item of a launch with agents, 0 with TDS_RASTER_DBG_NO_ACTOR_WAVE */
int tds_raster_get_actor_wave_stats(unsigned long long *out1);
/* read and reset the 16 work counters of the bit-plane kernel */
int tds_raster_get_stats(unsigned long long *out16);
/* read and reset the two counters of the prepared scan set-ups (TDS_RASTER_DBG_STATS): work items of the persistent bit-plane launches that used
 * their record of tds_raster_aux_t::camera_prep, and work items that computed their set-up in the kernel */
int tds_raster_get_prep_stats(unsigned long long *out2);
/* read and reset the 16 counters of small faces (TDS_RASTER_DBG_STATS; fused bit-plane kernels; a face is small as TDS_RASTER_DBG_DROP_SMALL says).
 * A chunk is one step of a wave through the static map (up to 64 grid entries).  [0] chunks, [1] faces accepted in them, [2] small ones among those,
 * [3] accepted faces of the other producers (actors, per-camera triangles), [4] small ones among those, [5..12] chunks by their number of small
 * faces: 0, 1-8, 9-16, 17-24, 25-32, 33-40, 41-48, 49-64, [13] small faces in chunks that hold at least as many as the on-lane path asks for (25),
 * [14] chunks without an accepted face,
 * [15] faces painted on the lane that scanned them (persistent launches). */
int tds_raster_get_small_stats(unsigned long long *out16);
/* which launches tds_raster_scene makes for a call of this shape (its plan_raster_scene, with explicit knobs: those of the four setters above).
 * n_keys: distinct keys (-1: more than 15); workspace_bytes: as the caller passes it (0: none).
 * form: 0 bit planes, 1 split (K3s + K3r + the bit planes over overflowed cameras), 2 packed keys binned, 3 packed keys fused, 4 TDS_ELIMIT.
 * The mask modes (tds_raster_scene_masks): the uint8 plan with the pair table taken off lds / lds_s; 4 where that plan takes packed keys. */
typedef struct {
    int form, tw, strips, twp, nwv, nb, minwg, emit, four_per_cu, persist, tws, lw;
    int64_t lds, lds_s, grid, caps, off_counts, off_lists, off_lists3;
} tds_raster_plan_t;
int tds_raster_plan(int64_t n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices, int64_t workspace_bytes,
                    int cus, int force_tw, int bits_waves, int list_waves, int list_lds_kb, int debug, tds_raster_plan_t *out);
/* the same call: does its launch paint small faces on the lane that scanned them?  small_faces: 0 = the caller passed TDS_RASTER_NO_SMALL_FACES.
 * 1 exactly for the 4-wave bit-plane instantiations at three workgroups per CU (minwg 3) of a colour image, else 0. */
int tds_raster_plan_small_lane(int64_t n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices,
                               int64_t workspace_bytes, int cus, int force_tw, int bits_waves, int list_waves, int list_lds_kb, int debug,
                               int small_faces, int *small_lane);
/* 0: maps created from now on carry no nearest-face candidate lists (K2b then walks grid rings) */
int tds_testing_set_near_lists(int enabled);
/* the lanes that share an observer in K7b's launch: 4 (the product's), 16 or 1 -- the shapes that were measured against each other; the order of
 * a row's sum, and so the last bits, follow the choice */
int tds_stop_lines_bwd_set_row_lanes(int lanes);
#endif

#ifdef __cplusplus
}
#endif
#endif /* TDSHIP_H */

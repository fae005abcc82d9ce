// K3's host-only entry points: the sizes a caller allocates by (tds_raster_*_bytes) and, in the testing build, the knobs and the planner as it
// is (tds_raster_set_*, tds_raster_plan).  No kernel in here; the calculations are tds_raster_plan.h's, the launches raster.hip's.
#include "tds_common.h"
#include "tds_raster_plan.h"

using namespace tds_raster;

#ifdef TDS_TESTING
// ---- testing build only (include/tdship.h, section "testing hooks"): absent from libtdship.so --------------------------------
RasterKnobs tds_raster::g_knobs = DEFAULT_KNOBS;

// force the strip width (0 = automatic)
TDS_EXPORT int tds_raster_set_strip_width(int tw) {
    TDS_CHECK_ARG(tw == 0 || tw == 8 || tw == 16 || tw == 32 || tw == 64 || tw == 96 || tw == 128, "strip width must be 0, 8, 16, 32, 64, 96 or 128");
    g_knobs.force_tw = tw;
    return TDS_OK;
}

// waves per workgroup of the bit-plane kernel (4 or 8)
TDS_EXPORT int tds_raster_set_bits_waves(int n) {
    TDS_CHECK_ARG(n == 4 || n == 8, "waves per workgroup must be 4 or 8");
    g_knobs.bits_waves = n;
    return TDS_OK;
}

// K3r (the list rasteriser of the split bit-plane path): the LDS a workgroup may take in KiB, which sets the strip width
TDS_EXPORT int tds_raster_set_list_lds(int lds_kb) {
    TDS_CHECK_ARG(lds_kb >= 16 && lds_kb <= 150, "tds_raster_set_list_lds: 16..150 KiB");
    g_knobs.list_lds_kb = lds_kb;
    return TDS_OK;
}

// K3r: waves per workgroup (2 or 4; 0 = chosen by the size of a strip)
TDS_EXPORT int tds_raster_set_list_waves(int waves) {
    TDS_CHECK_ARG(waves == 0 || waves == 2 || waves == 4, "tds_raster_set_list_waves: 0, 2 or 4");
    g_knobs.list_waves = waves;
    return TDS_OK;
}

// ablation switches, see CommonArgs::debug
TDS_EXPORT int tds_raster_set_debug(int flags) {
    g_knobs.debug = flags;
    return TDS_OK;
}

// work items per workgroup of the main grid from which the helper launch is made (tds_raster_aux_t::helper_stream)
TDS_EXPORT int tds_raster_set_helper_min_items(int items_per_workgroup) {
    TDS_CHECK_ARG(items_per_workgroup >= 0, "tds_raster_set_helper_min_items: a count >= 0");
    g_knobs.helper_min_items_per_wg = items_per_workgroup;
    return TDS_OK;
}

// plan_raster_scene with explicit knobs; workspace_bytes as a caller passes it (the queue tail is cut off here, as in the launch)
TDS_EXPORT int tds_raster_plan(int64_t n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices,
                               int64_t workspace_bytes, int cus, int force_tw, int bits_waves, int list_waves, int list_lds_kb, int debug,
                               tds_raster_plan_t *out) {
    TDS_CHECK_ARG(out && n_img > 0 && res > 0 && res <= 4096 && n_keys >= -1 && n_keys <= MAX_KEYS && cus > 0 &&
                  (out_mode == TDS_OUT_F32 || out_mode == TDS_OUT_U8 || is_mask_mode(out_mode)), "tds_raster_plan: bad arguments");
    const PlanInput in = {n_img, res, out_mode, n_keys, keys_listed != 0, actors != 0, extra != 0, want_slices != 0, lists_room(workspace_bytes, is_mask_mode(out_mode)), cus};
    const RasterPlan p = plan_raster_scene(in, RasterKnobs{force_tw, bits_waves, list_waves, list_lds_kb, debug, HELPER_MIN_ITEMS_PER_WG});
    *out = tds_raster_plan_t{(int)p.form, p.tw, p.strips, p.twp, p.nwv, p.nb, p.nwv == 4 ? (p.four_per_cu ? 4 : 3) : 0, want_slices && p.form == RasterForm::Bits,
                             p.four_per_cu, p.persist, p.tws, p.lw, (int64_t)p.lds, (int64_t)p.lds_s, p.grid, p.caps, p.ws.counts, p.ws.lists, p.ws.lists3};
    return TDS_OK;
}

// whether the launch of that plan paints small faces on the scan lane (RasterPlan::small_lane), for a caller that allows it or not
TDS_EXPORT int tds_raster_plan_small_lane(int64_t n_img, int res, int out_mode, int n_keys, int keys_listed, int actors, int extra, int want_slices,
                                          int64_t workspace_bytes, int cus, int force_tw, int bits_waves, int list_waves, int list_lds_kb, int debug,
                                          int small_faces, int *small_lane) {
    TDS_CHECK_ARG(small_lane && n_img > 0 && res > 0 && res <= 4096 && n_keys >= -1 && n_keys <= MAX_KEYS && cus > 0 &&
                  (out_mode == TDS_OUT_F32 || out_mode == TDS_OUT_U8 || is_mask_mode(out_mode)), "tds_raster_plan_small_lane: bad arguments");
    PlanInput in = {n_img, res, out_mode, n_keys, keys_listed != 0, actors != 0, extra != 0, want_slices != 0, lists_room(workspace_bytes, is_mask_mode(out_mode)), cus};
    in.small_faces = small_faces != 0;
    const RasterPlan p = plan_raster_scene(in, RasterKnobs{force_tw, bits_waves, list_waves, list_lds_kb, debug, HELPER_MIN_ITEMS_PER_WG});
    *small_lane = (p.form == RasterForm::Bits || p.form == RasterForm::Split) && p.small_lane ? 1 : 0;
    return TDS_OK;
}
#endif  // TDS_TESTING

TDS_EXPORT int tds_raster_index_slices_bytes(int64_t n_img, int res, int64_t *bytes) {
    TDS_CHECK_ARG(bytes, "tds_raster_index_slices_bytes: null output");
    TDS_CHECK_ARG(n_img >= 0 && res > 0 && res <= 4096, "tds_raster_index_slices_bytes: bad sizes");
    *bytes = index_slices_bytes(n_img, res);
    return TDS_OK;
}

TDS_EXPORT int tds_raster_coverage_bytes(int64_t n_img, int res, int64_t *bytes) {
    TDS_CHECK_ARG(bytes, "tds_raster_coverage_bytes: null output");
    TDS_CHECK_ARG(n_img >= 0 && res > 0 && res <= 4096, "tds_raster_coverage_bytes: bad sizes");
    *bytes = coverage_bytes(n_img, res);
    return TDS_OK;
}

TDS_EXPORT int tds_raster_scene_workspace_bytes(int64_t n_img, int res, int64_t *bytes) {
    TDS_CHECK_ARG(bytes, "tds_raster_scene_workspace_bytes: null output");
    TDS_CHECK_ARG(res > 0 && res <= 4096 && n_img >= 0, "tds_raster_scene_workspace_bytes: bad arguments");
    *bytes = workspace_bytes(n_img, res, g_knobs);
    return TDS_OK;
}

TDS_EXPORT int tds_raster_scene_workspace_bytes_for(int64_t n_img, int res, int out_mode, int n_keys, int64_t *bytes) {
    TDS_CHECK_ARG(bytes, "tds_raster_scene_workspace_bytes_for: null output");
    TDS_CHECK_ARG(res > 0 && res <= 4096 && n_img >= 0, "tds_raster_scene_workspace_bytes_for: bad arguments");
    TDS_CHECK_ARG(out_mode == TDS_OUT_F32 || out_mode == TDS_OUT_U8 || is_mask_mode(out_mode), "tds_raster_scene_workspace_bytes_for: unknown output mode %d", out_mode);
    *bytes = workspace_bytes_for(n_img, res, out_mode, n_keys, g_knobs);
    return TDS_OK;
}

TDS_EXPORT int tds_raster_camera_prep_bytes(int64_t n_img, int res, int out_mode, int n_keys, int64_t *bytes) {
    TDS_CHECK_ARG(bytes, "tds_raster_camera_prep_bytes: null output");
    *bytes = 0;
    TDS_CHECK_ARG(n_img >= 0 && n_img < ((int64_t)1 << 31) && res > 0 && res <= 4096, "tds_raster_camera_prep_bytes: bad sizes");
    TDS_CHECK_ARG(out_mode == TDS_OUT_F32 || out_mode == TDS_OUT_U8 || is_mask_mode(out_mode), "tds_raster_camera_prep_bytes: unknown output mode %d", out_mode);
    TDS_CHECK_ARG(n_keys >= -1 && n_keys <= MAX_KEYS, "tds_raster_camera_prep_bytes: n_keys must be -1 (not known) .. %d", MAX_KEYS);
    *bytes = camera_prep_bytes(n_img, res, out_mode, n_keys, g_knobs);
    return TDS_OK;
}

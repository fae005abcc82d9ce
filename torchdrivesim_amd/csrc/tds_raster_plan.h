// The launch planning of K3, the scene rasteriser (raster.hip): the knobs, where the work queues, the mask table and the split and binned lists
// lie in the caller's workspace, the form and shape of the launches (plan_raster_scene), and the byte counts behind the tds_raster_*_bytes
// entry points (raster_host.hip).  A pure host calculation -- it decides which bytes of the workspace the kernels write.  Nothing of HIP in
// here: a host compiler takes this file as it is, and tests/raster_plan_host.cpp sweeps the plans on the CPU, with the sanitizers too.
// The constants are the ones the planner shares with the kernels; raster.hip reads them from here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/tdship.h"

namespace tds_raster {

constexpr int RWAVES = 4;
constexpr int QCAP = 64;                          // per-wave face queue (entries): key + 3 packed vertices
constexpr int Q_DW = 4 * QCAP;
constexpr int BLOCK_CAP = 256;                    // per-wave list of (face, block) pairs
constexpr int WAVE_LDS_DW = Q_DW + BLOCK_CAP;
constexpr int MAX_STRIPS = 128;                   // strips per image that K3a bins
constexpr int MAX_KEYS = 15;                      // key indices 1..15 fit 4 bits (0 = background)
constexpr int EQCAP = 128;                        // ring of queued outline edges per wave (power of two, >= 2 * 64)
constexpr int BITS_WAVE_LDS_DW = Q_DW + 64 + 2 * EQCAP;   // per wave: face queue + owner markers + edge ring
constexpr int BITS_FIXED_DW = 20;                 // [0..14] ascending key table, [15] next chunk of the grid scan, [16] the work item taken next,
                                                  // [17] queues this workgroup has found empty
constexpr int COV_HEADER_DW = 16;                 // header of a coverage record (raster.hip, beside COV_MODE)
constexpr int MASK_TABLE_DW = 64;                 // the channel table of a mask launch (raster.hip, MaskTable)
constexpr int64_t MASK_TABLE_BYTES = MASK_TABLE_DW * 4;
constexpr int64_t PREP_RECORD_BYTES = 336;        // sizeof(PrepRecord): one prepared scan set-up (raster.hip holds the two equal)

inline int bits_index_bits(int K) { return K <= 3 ? 2 : (K <= 7 ? 3 : 4); }
inline size_t bits_lds_bytes(int K, int res, int twp, int nwaves, int out_mode) {
    size_t plane_dw = ((size_t)K * res * (twp / 32) + 3) & ~(size_t)3;
    size_t P = (size_t)1 << (2 * bits_index_bits(K));
    size_t tab_dw = 3 * P * (out_mode == TDS_OUT_F32 ? 2 : 1);
    return (plane_dw + tab_dw + BITS_FIXED_DW + (size_t)nwaves * BITS_WAVE_LDS_DW) * 4;
}
// The knobs of K3 that the testing hooks set (include/tdship.h, "testing hooks"), constants in the product: the strip width (0: automatic),
// waves per workgroup of the bit-plane kernel and of K3r (0: by image size), K3r's LDS budget in KiB (it takes the widest strip that fits), and
// the TDS_RASTER_DBG_* flags; helper_min_items_per_wg: the helper launch is made from that many work items per workgroup of the main grid on
// (plan_raster_scene, at helper_grid, says why 4).
struct RasterKnobs { int force_tw, bits_waves, list_waves, list_lds_kb, debug, helper_min_items_per_wg; };
constexpr int HELPER_MIN_ITEMS_PER_WG = 4;
constexpr RasterKnobs DEFAULT_KNOBS = {0, 4, 0, 40, 0, HELPER_MIN_ITEMS_PER_WG};
#ifdef TDS_TESTING
extern __attribute__((visibility("hidden"))) RasterKnobs g_knobs;    // one per library, defined in raster_host.hip: every launch reads what the hooks set
#else
constexpr RasterKnobs g_knobs = DEFAULT_KNOBS;
#endif

// The work queues of a persistent bit-plane launch: 8 counters (64 bytes) that must be zero when the kernel starts.  They live at the
// END of the caller's workspace (tds_raster_scene_workspace_bytes provides for them) and are cleared in stream order right before the
// launch.  Two launches that may overlap in time must not share a workspace; that already holds for the face lists.  The library allocates
// nothing per call.  (They are cleared by tds::zero_async, a kernel: see there why not hipMemsetAsync.)
constexpr int64_t QUEUE_BYTES = 64;
// where the queues start in a workspace of `bytes` (what lies before is left for the lists); -1: no room for them
inline int64_t queue_offset(int64_t bytes) { return bytes < QUEUE_BYTES + 64 ? -1 : (bytes - QUEUE_BYTES) & ~(int64_t)63; }
// the workspace that leaves `lists` bytes for the lists and room for the queues after them
inline int64_t with_queue_tail(int64_t lists) { return ((lists + 63) & ~(int64_t)63) + QUEUE_BYTES + 64; }
// what the lists may use of a workspace of `bytes` (0: none): all that lies before the queues -- and, in a mask call, before the channel table
// (MASK_TABLE_BYTES right in front of the queues)
inline int64_t lists_room(int64_t bytes, bool masks) {
    const int64_t q = queue_offset(bytes);
    return q < 0 ? 0 : (masks ? std::max<int64_t>(q - MASK_TABLE_BYTES, 0) : q);
}

// The workspace of the split form: a marker list (`poisoned`, n_img + 1 words) at 0, a count per camera, then `caps` poly records per camera,
// each 16 bytes in `lists` (flags, P0, P1, P2) and 4 in `lists3` (P3).  The recommended workspace (tds_raster_scene_workspace_bytes*)
// counts LIST_CAPS records of 16 bytes while the launch divides what it gets by 20, so LIST_CAPS = 2048 yields about 1636 records per
// camera.  Kept as it was measured: a change moves which cameras overflow to the fused kernel.
struct SplitLayout { int64_t counts, lists, lists3, caps; };        // byte offsets; records per camera
// caps < 0: as many as `bytes` hold (a multiple of 4, at most 8192; 0 when none fit)
inline SplitLayout split_layout(int64_t n_img, int64_t caps, int64_t bytes = 0) {
    const int64_t counts = ((n_img + 1) * 4 + 255) & ~(int64_t)255, lists = (counts + n_img * 4 + 255) & ~(int64_t)255;
    if (caps < 0) caps = bytes > lists ? std::min<int64_t>(((bytes - lists) / (n_img * 20)) & ~(int64_t)3, 8192) : 0;
    return {counts, lists, lists + n_img * caps * 16, caps};
}

// workgroups of a persistent launch: exactly as many as are resident at a time -- three per CU (168 VGPRs: three waves per SIMD), fewer when
// the LDS of one exceeds a third of the CU's 160 KiB.  (A surplus of waiting workgroups costs: DESIGN_HISTORY.md, appendix R6; fewer than the
// resident number, or head / tail items in strips, do not pay either: profiles/r06_tail_attempts.log.)
inline int64_t resident_workgroups(int cus, size_t lds_bytes, const RasterKnobs &k) {
    const size_t granted = (lds_bytes + 2047) & ~(size_t)2047;                  // LDS is granted in 2 KiB steps
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(3, (size_t)(160 * 1024) / std::max<size_t>(granted, 1)));
    // (testing build, GRID8 / GRID4: 8 / 4 workgroups per CU -- the surplus of round 3)
    return (int64_t)cus * ((k.debug & TDS_RASTER_DBG_GRID8) ? 8 : ((k.debug & TDS_RASTER_DBG_GRID4) ? 4 : per_cu));
}

inline size_t lds_bytes(int tw, int res) { return ((size_t)tw * res + (size_t)RWAVES * WAVE_LDS_DW) * sizeof(uint32_t); }

// strip width: the widest of {64,32,16,8} whose tile leaves room for two workgroups per CU (160 KiB LDS), else one
inline int pick_tw(int res) {
    const int cands[4] = {64, 32, 16, 8};
    for (int tw : cands)
        if (lds_bytes(tw, res) <= 80 * 1024) return tw;
    for (int tw : cands)
        if (lds_bytes(tw, res) <= 160 * 1024) return tw;
    return 0;
}
// strip width of the packed-key kernels (0: the resolution does not fit)
inline int strip_width(int res, const RasterKnobs &k) { return (k.force_tw && k.force_tw <= 64) ? k.force_tw : pick_tw(res); }

constexpr int DEFAULT_CAPS = 512;         // faces per strip list that the recommended workspace provides
constexpr int LIST_CAPS = 2048;           // faces per camera list of the split bit-plane path that the recommended workspace provides
// The split form (K3s + K3r) serves resolutions up to these; above, the fused launch hides the scan behind its write stream or its row loops.
// ONE sweep on one build and box (round 6, tools/split_threshold_sweep.sh, B = 1024 x 64, ms per call, fused / split -- each pair from one process;
// profiles/r06_split_threshold_sweep.log):
//   float32   96 4.00 / 2.72   104 4.09 / 3.02   112 4.13 / 3.24   116 4.14 / 3.98   120 4.19 / 4.46   124 4.18 / 4.20   128 4.12 / 3.24   136 4.33 / 5.38
//            144 4.36 / 3.93   152 4.46 / 5.03   160 4.48 / 4.28   168 5.11 / 6.20   176 4.80 / 5.02   192 4.97 / 5.48
//   uint8    128 3.99 / 2.91   160 4.16 / 3.38   176 4.51 / 3.70   192 4.50 / 4.14   208 4.69 / 4.33   216 4.65 / 4.38   224 4.94 / 5.18 (7.35 once the strip no longer
//            holds the whole image)   256 5.09 / 5.64
// float32: K3r is bound by its write stream from about 116 x 116 on and pays for output columns (res x 4 bytes) that straddle 64-byte sectors, so above
// SPLIT_ANY_RES_F32 the split form is taken only where res is a multiple of 16 (split_serves).
constexpr int SPLIT_MAX_RES_F32 = 160, SPLIT_ANY_RES_F32 = 116, SPLIT_MAX_RES_U8 = 216;
inline bool split_serves(int res, bool f32) {
    if (!f32) return res <= SPLIT_MAX_RES_U8;
    return res <= SPLIT_ANY_RES_F32 || (res <= SPLIT_MAX_RES_F32 && (res & 15) == 0);
}

// Bits: the bit-plane kernel (raster_scene_bits_kernel), the whole image or strips of it; Split: K3s (scan_faces_kernel) + K3r
// (raster_list_bits_kernel) + the bit-plane kernel over the cameras whose list overflowed; packed keys Binned (K3a bin_faces_kernel + K3b
// raster_scene_list_kernel) or Fused (raster_scene_kernel); Error: TDS_ELIMIT
enum class RasterForm { Bits, Split, Binned, Fused, Error };

struct PlanInput {
    int64_t n_img;
    int res, out_mode, n_keys;  // n_keys: distinct keys of the scene (its map(s) and the listed actor keys); -1: more than MAX_KEYS
    bool keys_listed, actors, extra, want_slices;   // the caller listed the actors' keys; N > 0; n_extra > 0; index slices wanted
    int64_t workspace_bytes;    // what the lists may use, the queue tail cut off; 0: no workspace, or no room for the queues
    int cus;                    // CUs the launch may use
    bool small_faces = true;    // the caller lets small faces be painted on the lane that scanned them (off: TDS_RASTER_NO_SMALL_FACES)
    int helper_cus = 0;         // CUs of a helper stream the launch may use as well (tds_raster_aux_helper_t::helper_stream); 0: there is none -- no such stream,
                                // the call's own stream, a stream without a CU, or a stream that is capturing (raster.hip: helper_stream_cus)
};

struct RasterPlan {
    RasterForm form;
    const char *error;          // Error: the message (a format that may take MAX_KEYS)
    int tw, strips;             // strip width of the packed-key kernels; strips per image of the raster launch
    int twp, nwv, nb;           // bit planes: strip width (32-padded), waves per workgroup, index bits,
    size_t lds;                 // LDS per workgroup,
    bool four_per_cu, persist;  // the MINWG = 4 instantiation (one workgroup per item) instead of MINWG = 3, a persistent launch over the queues
    int64_t grid, caps;         // workgroups of the raster launch; faces per list (Split: per camera, Binned: per strip)
    SplitLayout ws;             // Split: the workspace layout; Binned: the strip lists at ws.lists, their counts at 0
    int tws, lw; size_t lds_s;  // Split: strip width, waves and LDS per workgroup of K3r
    bool small_lane;            // the bit-plane kernel paints small faces on the lane that scanned them (raster.hip: drain_bits)
    int64_t helper_grid;        // workgroups of the second enqueue of the persistent launch, on the helper stream; 0: none
};

// A pure function of the call's shape and the knobs: no HIP call, no global.  tests/test_raster_plan.py pins its choices,
// tests/test_raster_plan_host.py the layouts it hands the kernels.
inline bool is_mask_mode(int out_mode) { return out_mode == TDS_OUT_MASK_U8 || out_mode == TDS_OUT_MASK_BITS; }

inline RasterPlan plan_raster_scene(const PlanInput &in, const RasterKnobs &k) {
    // the masks take the plan of the uint8 image of the same shape; only their LDS is smaller (no pair table).  They are streamed out of the
    // bit-plane kernels only.
    if (is_mask_mode(in.out_mode)) {
        PlanInput u8 = in;
        u8.out_mode = TDS_OUT_U8;
        RasterPlan p = plan_raster_scene(u8, k);
        if (p.form == RasterForm::Bits || p.form == RasterForm::Split) {
            const size_t tab = (size_t)3 * ((size_t)1 << (2 * p.nb)) * 4;
            p.lds -= tab;
            if (p.form == RasterForm::Split) p.lds_s -= tab;
            p.small_lane = false;                       // the mask instantiations queue every face
            p.helper_grid = 0;                          // ... and are enqueued once
        } else if (p.form != RasterForm::Error) {
            p.form = RasterForm::Error;
            p.error = "tds_raster_scene_masks: the masks come from the bit-plane kernels only (at most %d distinct keys, listed by the caller)";
        }
        return p;
    }
    RasterPlan p{};
    const int res = in.res, full = (res + 31) & ~31;
    p.tw = strip_width(res, k);
    p.strips = (res + p.tw - 1) / p.tw;
    p.grid = in.n_img * p.strips;
    // fastest path: bit planes, when the scene uses at most MAX_KEYS distinct keys and the caller listed the actors' keys
    if ((in.keys_listed || !(in.actors || in.extra)) && in.n_keys > 0 && !(k.debug & TDS_RASTER_DBG_NO_BITS)) {
        auto lds_of = [&](int twp, int nwv) { return bits_lds_bytes(in.n_keys, res, twp, nwv, in.out_mode); };
        // strip width: the whole (32-padded) image if the planes fit 64 KiB, else the widest multiple of 32 that does
        int twp = full;
        while (twp > 32 && (size_t)in.n_keys * res * (twp / 8) > 64 * 1024) twp -= 32;
        // ... in strips of EQUAL width (nine keys at 256 x 256: 192 + 64 columns left the second strip's workgroups a third of the work and the first
        // one's two per CU -- 10.4 ms; 128 + 128 at three per CU: profiles/r06_more_keys.log)
        // and, where one more strip lets three workgroups share a CU instead of two, in one more (ten keys: 3 x 96 columns).
        if (twp < full && !(k.debug & TDS_RASTER_DBG_WIDEST_STRIPS)) {
            const int n_strips = (res + twp - 1) / twp;
            auto equal_width = [&](int n) { return (((res + n - 1) / n) + 31) & ~31; };
            twp = equal_width(n_strips);
            if (lds_of(twp, k.bits_waves) > 52 * 1024 && equal_width(n_strips + 1) >= 64 && lds_of(equal_width(n_strips + 1), k.bits_waves) <= 52 * 1024 &&
                !(k.debug & TDS_RASTER_DBG_NO_EXTRA_STRIP))
                twp = equal_width(n_strips + 1);
        }
        int nwv = k.bits_waves;
        // Three workgroups per CU need at most 52 KiB each (160 KiB of LDS, allocated in 2 KiB steps): five keys at 256 x 256 just fit.
        // A whole image that does not (six keys and more: two agent types, traffic lights, waypoints) -- measured at B = 1024 x 64, 256 x 256,
        // six / seven keys, float32 | uint8 ms (profiles/r06_more_keys.log):
        //     two half-image strips, four 128-VGPR workgroups per CU (each strip scans the grid for itself)   7.79 / 7.86 | 6.88 / 6.98
        //     the whole image, two 4-wave workgroups per CU (persistent)                                       7.62 / 7.71 | 6.90 / 6.99
        //     the whole image, two 8-WAVE workgroups per CU (sixteen waves per CU instead of eight)            7.61 / 7.63 | 6.25 / 6.32
        // so: eight waves on the whole image where two such workgroups fit a CU (80 KiB each: up to seven keys at 256 x 256), else half strips
        // (eight keys: 7.72 against 7.75 for the whole image in 4-wave workgroups; five keys at 320 x 320: 2.76 against 2.84; and differentiable
        // calls, whose index slices the 4-wave kernel writes).  Eight waves also rule out the split form below (uint8, 192 - 216 px, 8 - 10 keys).
        if (twp == full && twp >= 128 && lds_of(twp, nwv) > 52 * 1024 && !(k.debug & TDS_RASTER_DBG_WHOLE_4WAVES)) {
            const int half = ((twp / 2) + 31) & ~31;
            if (nwv == 4 && !in.want_slices && lds_of(twp, 8) <= 80 * 1024 && !(k.debug & TDS_RASTER_DBG_NO_8WAVES)) nwv = 8;
            else if (lds_of(half, nwv) <= 52 * 1024) twp = half;
        }
        if (k.force_tw >= 32 && k.force_tw < twp) twp = k.force_tw;     // tuning hook
        if (lds_of(twp, nwv) <= 150 * 1024) {
            p.form = RasterForm::Bits; p.twp = twp; p.nwv = nwv; p.nb = bits_index_bits(in.n_keys); p.lds = lds_of(twp, nwv);
            p.strips = (res + twp - 1) / twp; p.grid = in.n_img * p.strips;
            // differentiable calls: float32, four waves; the instantiation that also stores the index slices
            if (in.want_slices && nwv != 4) { p.form = RasterForm::Error; p.error = "tds_raster_scene: index slices need the 4-wave bit-plane kernel"; return p; }
            // ---- the split form (K3s + K3r) where the launch is not bound by the write stream (where it pays: the sweep beside SPLIT_MAX_RES_*) ----
            const bool f32 = in.out_mode == TDS_OUT_F32;
            bool split = !in.want_slices && nwv == 4 && in.workspace_bytes > 0 && split_serves(res, f32);
            if (k.debug & TDS_RASTER_DBG_NO_SPLIT) split = false;
            if (k.debug & TDS_RASTER_DBG_SPLIT) split = !in.want_slices && nwv == 4 && in.workspace_bytes > 0;
            if (split) p.ws = split_layout(in.n_img, -1, in.workspace_bytes);
            if (split && p.ws.caps >= 128) {
                // strip width of K3r: the widest multiple of 32 columns whose workgroup stays within the LDS budget (four workgroups per CU);
                // waves: two up to 104 x 104 float32 / 128 x 128 uint8 pixels of a strip, four above (the sweep is DESIGN_HISTORY.md, appendix R7)
                int lw = k.list_waves, tws = full;
                if (lw == 0) lw = (int64_t)res * tws <= (f32 ? 104 * 104 : 128 * 128) ? 2 : 4;
                while (tws > 32 && lds_of(tws, lw) > (size_t)k.list_lds_kb * 1024) tws -= 32;
                // (more keys than the sweep's five can push a large image over the LDS budget: K3r in several strips per camera loses to
                // the fused kernel from about 160 x 160 on -- uint8 224: 7.35 against 4.94 ms -- unless the testing build forces the form)
                const bool narrowed = tws < full && res >= 160 && !(k.debug & TDS_RASTER_DBG_SPLIT);
                if (lds_of(tws, lw) <= 150 * 1024 && !narrowed) { p.form = RasterForm::Split; p.tws = tws; p.lw = lw; p.lds_s = lds_of(tws, lw); p.caps = p.ws.caps; }
            }
            // the instantiations for three workgroups per CU are persistent launches: their workgroups take (camera, strip) items from per-XCD
            // queues (see claim_work); the others get one workgroup per item, and so do all without a workspace (there is no queue).  The launch
            // over the cameras K3s marked (normally none) takes its items from a queue: a persistent instantiation.
            p.four_per_cu = nwv == 4 && !in.want_slices && p.form != RasterForm::Split && p.lds <= 40 * 1024 && !(k.debug & TDS_RASTER_DBG_MINWG3);
            p.persist = nwv == 4 && !p.four_per_cu && in.workspace_bytes > 0;
            if (p.persist) p.grid = std::min(p.form == RasterForm::Split ? 512 : p.grid, resident_workgroups(in.cus, p.lds, k));
            // Small faces on the scan lane: the 4-wave instantiations for three workgroups per CU have the block (issue-bound launches: 5.98 -> 5.76 ms
            // at the headline, uint8 4.89 -> 4.69; the launch that stores every line of a float32 image is bound by HBM and neither gains nor loses
            // beyond its spread: DESIGN.md section 6), the 8-wave and the 128-VGPR instantiations do not; the caller may switch it off.
            p.small_lane = in.small_faces && nwv == 4 && !p.four_per_cu;
            // The helper enqueue: the same kernel once more on a stream confined to CUs the launch's own stream is kept off (the metric stream of
            // Simulator.overlap_infractions = 'reserved'), as many workgroups as are resident there.  They claim items from the same queues, so only
            // the persistent launch over ALL the cameras of a colour image takes it: not the launch over the cameras K3s marked (one short queue),
            // not a call that stores index slices, none without queues.  And only a launch long enough: the helper workgroups start when the helper
            // stream's earlier kernels have ended and the call's stream waits for them at the end, so a launch of a few items per workgroup can only
            // lose the cross-stream waits (tens of microseconds) -- from HELPER_MIN_ITEMS_PER_WG items per workgroup of the main grid on.
            // (Why 4: DESIGN.md section 6, the table of launch times at B = 16, 64 and 256 with and without the helper.)
            if (p.form == RasterForm::Bits && p.persist && !in.want_slices && in.helper_cus > 0 &&
                in.n_img * p.strips >= (int64_t)k.helper_min_items_per_wg * p.grid)
                p.helper_grid = resident_workgroups(in.helper_cus, p.lds, k);
            return p;
        }
    }
    if (in.want_slices) {
        p.form = RasterForm::Error; p.error = "tds_raster_scene: index slices are produced by the bit-plane kernel only (at most %d distinct keys, listed by the caller)";
        return p;
    }
    // general path: bin once per camera (K3a), then rasterise per strip from the lists (K3b)
    if (in.workspace_bytes > 0 && !(k.debug & TDS_RASTER_DBG_NO_BINNED) && p.strips <= MAX_STRIPS) {
        int64_t caps = std::min<int64_t>((in.workspace_bytes / p.grid - (int64_t)sizeof(uint32_t)) / 16, 4096);      // 16: a poly record
        if (caps >= 64) {
            p.ws.lists = (p.grid * (int64_t)sizeof(uint32_t) + 255) & ~(int64_t)255;
            // the counts' 256-byte alignment can cost up to 252 bytes: with fewer than 16 strip lists to spread them over, more than one record each
            while (p.ws.lists + p.grid * caps * 16 > in.workspace_bytes) --caps;
            p.form = RasterForm::Binned; p.caps = caps; return p;
        }
    }
    p.form = RasterForm::Fused; return p;
}

// ---- the byte counts of the sizing entry points (raster_host.hip checks the arguments) ----
// the index slices of n_img images of res x res (0: none at this resolution -- it must be a multiple of 4)
inline int64_t index_slices_bytes(int64_t n_img, int res) { return (res & 3) ? 0 : n_img * (int64_t)((res + 31) / 32) * (int64_t)(res / 4) * 64; }
// bytes of the coverage record of n_img float32 images of res x res (0: no record at this resolution -- lines are tracked where res is a multiple of 32)
inline int64_t coverage_bytes(int64_t n_img, int res) {
    return (res & 31) ? 0 : (int64_t)COV_HEADER_DW * 4 + n_img * (int64_t)(res >> 5) * (int64_t)(res >> 5) * 4;
}

// the recommended workspace when the keys are not known: the strip lists of the binned form or the camera lists of the split form, whichever are larger
inline int64_t workspace_bytes(int64_t n_img, int res, const RasterKnobs &k) {
    const int tw = strip_width(res, k);
    int64_t lists = 0;
    if (tw != 0 && (res + tw - 1) / tw <= MAX_STRIPS) lists = n_img * ((res + tw - 1) / tw) * (DEFAULT_CAPS * 16 + 4);
    // the split bit-plane path, LIST_CAPS faces per camera, where the split form can be chosen for either output type (testing: anywhere)
#ifndef TDS_TESTING
    if (split_serves(res, true) || split_serves(res, false))
#endif
    lists = std::max(lists, split_layout(n_img, LIST_CAPS).lists3);
    return with_queue_tail(lists);
}

// ... for an output mode (float32, uint8 or a mask mode) and a number of keys (outside 0..MAX_KEYS: not known)
inline int64_t workspace_bytes_for(int64_t n_img, int res, int out_mode, int n_keys, const RasterKnobs &k) {
    // the masks: the uint8 image's workspace and the channel table in front of the queues
    if (is_mask_mode(out_mode)) return workspace_bytes_for(n_img, res, TDS_OUT_U8, n_keys, k) + MASK_TABLE_BYTES;
    if (n_keys < 0 || n_keys > MAX_KEYS) return workspace_bytes(n_img, res, k);
    // the bit-plane kernels: face lists where the split form can run for this output type, the work queues of the persistent launch always
    int64_t lists = 0;
#ifndef TDS_TESTING
    if (split_serves(res, out_mode == TDS_OUT_F32))
#endif
        lists = split_layout(n_img, LIST_CAPS).lists3;
    return with_queue_tail(lists);
}

// The table of prepared scan set-ups is sized before the device is known: for a whole MI355X.  (The CU count only caps a persistent launch's
// grid; whether the plan is one, and its strips, do not depend on it.)
constexpr int PREP_PLAN_CUS = 256;
// The table of prepared scan set-ups (tds_raster_aux_t::camera_prep): one record per work item (camera, strip) of the launch that takes it -- the
// fused bit-plane kernel in persistent 4-wave workgroups; 0 where the call is served by another launch.  The strips are the plan's: of a plain
// and of a differentiable call (which may cut the image in two where the plain call takes eight waves) the larger count.
inline int64_t camera_prep_bytes(int64_t n_img, int res, int out_mode, int n_keys, const RasterKnobs &k) {
    if (is_mask_mode(out_mode) || n_keys <= 0 || n_img == 0) return 0;
    // (with the workspace the library recommends: where that makes the plan the split form, no table)
    const int64_t ws_bytes = workspace_bytes_for(n_img, res, out_mode, n_keys, k);
    int64_t items = 0;
    for (int slices = 0; slices < (out_mode == TDS_OUT_F32 ? 2 : 1); ++slices) {
        const PlanInput in = {n_img, res, out_mode, n_keys, true, true, false, slices != 0, lists_room(ws_bytes, false), PREP_PLAN_CUS};
        const RasterPlan p = plan_raster_scene(in, k);
        if (p.form == RasterForm::Bits && p.persist) items = std::max<int64_t>(items, n_img * p.strips);
    }
    return items * PREP_RECORD_BYTES;
}

}  // namespace tds_raster

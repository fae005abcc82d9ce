// The rule that decides whether the persistent bit-plane launch is enqueued a second time on a helper stream (torchdrivesim_amd/csrc/
// tds_raster_plan.h: plan_raster_scene, RasterPlan::helper_grid), swept on the host over the plans of tests/raster_plan_host.cpp -- every
// shape once with and once without a helper stream of 0, 1, 32 or 256 CUs, and with the threshold knob at 0, at the product's value and far
// above it.  Built and run by tests/test_helper_plan_host.py, plain and with the sanitizers.  Prints how many plans took the helper, one line per
// invariant that failed (with its first counter-example) and the plan of the headline launch; exit status 1 if an invariant failed.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "tds_raster_plan.h"

using namespace tds_raster;

namespace {

struct Failure { long count; std::string first; };
std::map<std::string, Failure> failures;
const PlanInput *g_in;
int g_threshold;

void expect(bool ok, const char *what) {
    if (ok) return;
    Failure &f = failures[what];
    if (f.count++ == 0) {
        char buf[256];
        snprintf(buf, sizeof buf, "n_img %lld res %d out_mode %d n_keys %d slices %d room %lld cus %d helper_cus %d threshold %d", (long long)g_in->n_img,
                 g_in->res, g_in->out_mode, g_in->n_keys, (int)g_in->want_slices, (long long)g_in->workspace_bytes, g_in->cus, g_in->helper_cus, g_threshold);
        f.first = buf;
    }
}

// every field but helper_grid
bool same_launch(RasterPlan a, RasterPlan b) {
    a.helper_grid = b.helper_grid = 0;
    return a.form == b.form && a.error == b.error && a.tw == b.tw && a.strips == b.strips && a.twp == b.twp && a.nwv == b.nwv && a.nb == b.nb && a.lds == b.lds &&
           a.four_per_cu == b.four_per_cu && a.persist == b.persist && a.grid == b.grid && a.caps == b.caps && a.ws.counts == b.ws.counts &&
           a.ws.lists == b.ws.lists && a.ws.lists3 == b.ws.lists3 && a.ws.caps == b.ws.caps && a.tws == b.tws && a.lw == b.lw && a.lds_s == b.lds_s &&
           a.small_lane == b.small_lane;
}

}  // namespace

int main() {
    const int modes[4] = {TDS_OUT_F32, TDS_OUT_U8, TDS_OUT_MASK_U8, TDS_OUT_MASK_BITS};
    const int64_t cameras[4] = {3, 32, 512, 65536};
    const int cu_counts[2] = {224, 256};
    const int helper_cu_counts[4] = {0, 1, 32, 256};
    const int thresholds[3] = {0, HELPER_MIN_ITEMS_PER_WG, 1 << 20};
    long plans = 0, helped = 0;
    for (int r = 1; r <= 523; ++r) {
        const int res = r <= 520 ? r : 1024 << (r - 521);
        for (int n_keys = -1; n_keys <= MAX_KEYS; ++n_keys)
            for (int out_mode : modes)
                for (int64_t n_img : cameras) {
                    const bool masks = is_mask_mode(out_mode);
                    for (int threshold : thresholds) {
                        RasterKnobs k = DEFAULT_KNOBS;
                        k.helper_min_items_per_wg = threshold;
                        g_threshold = threshold;
                        const int64_t recommended = workspace_bytes_for(n_img, res, out_mode, n_keys, k);
                        for (int64_t bytes : {(int64_t)0, recommended}) {
                            const int64_t room = lists_room(bytes, masks);
                            for (int slices = 0; slices < (out_mode == TDS_OUT_F32 ? 2 : 1); ++slices)
                                for (int cus : cu_counts) {
                                    PlanInput in = {n_img, res, out_mode, n_keys, true, true, false, slices != 0, room, cus};
                                    g_in = &in;
                                    const RasterPlan alone = plan_raster_scene(in, k);
                                    expect(alone.helper_grid == 0, "no helper stream: helper_grid == 0");
                                    for (int hc : helper_cu_counts) {
                                        in.helper_cus = hc;
                                        const RasterPlan p = plan_raster_scene(in, k);
                                        ++plans;
                                        expect(same_launch(p, alone), "the helper stream changes nothing else of the plan");
                                        expect(p.helper_grid >= 0, "helper_grid >= 0");
                                        if (p.helper_grid == 0) {
                                            // the only reasons for none
                                            const bool could = p.form == RasterForm::Bits && p.persist && !in.want_slices && !masks && hc > 0;
                                            expect(!could || n_img * p.strips < (int64_t)threshold * p.grid, "a plan that could take the helper and is long enough takes it");
                                            continue;
                                        }
                                        ++helped;
                                        expect(hc > 0, "helper: a helper stream with CUs");
                                        expect(p.form == RasterForm::Bits, "helper: the fused bit-plane form (not split, not packed keys)");
                                        expect(p.persist && room > 0, "helper: persistent, with queues in a workspace");
                                        expect(p.nwv == 4 && !p.four_per_cu, "helper: 4-wave workgroups at three per CU (not eight waves, not four per CU)");
                                        expect(!in.want_slices, "helper: no index slices");
                                        expect(!masks && (out_mode == TDS_OUT_F32 || out_mode == TDS_OUT_U8), "helper: a colour image, not the masks");
                                        expect(n_img * p.strips >= (int64_t)threshold * p.grid, "helper: items >= threshold x main grid");
                                        expect(p.helper_grid == resident_workgroups(hc, p.lds, k), "helper: as many workgroups as are resident on the helper's CUs");
                                        if (p.lds <= 52 * 1024) expect(p.helper_grid == 3 * (int64_t)hc, "helper: helper_grid == 3 x helper CUs");
                                        expect(p.helper_grid <= 3 * (int64_t)hc, "helper: at most three workgroups per CU");
                                    }
                                }
                        }
                    }
                }
    }
    printf("plans %ld helped %ld\n", plans, helped);
    for (const auto &f : failures) printf("FAILED %s: %ld plans, first %s\n", f.first.c_str(), f.second.count, f.second.first.c_str());
    // the headline launch (65 536 cameras of 256 x 256 float32, five keys, 224 CUs + 32), the same with 32 cameras, and the 128 x 128 split form
    const RasterKnobs k = DEFAULT_KNOBS;
    for (const int64_t n_img : {(int64_t)65536, (int64_t)32}) {
        PlanInput in = {n_img, 256, TDS_OUT_F32, 5, true, true, false, false, lists_room(workspace_bytes_for(n_img, 256, TDS_OUT_F32, 5, k), false), 224};
        in.helper_cus = 32;
        const RasterPlan p = plan_raster_scene(in, k);
        printf("cameras %lld grid %lld helper_grid %lld\n", (long long)n_img, (long long)p.grid, (long long)p.helper_grid);
    }
    PlanInput in = {65536, 128, TDS_OUT_F32, 5, true, true, false, false, lists_room(workspace_bytes_for(65536, 128, TDS_OUT_F32, 5, k), false), 224};
    in.helper_cus = 32;
    const RasterPlan p = plan_raster_scene(in, k);
    printf("128 px form %d helper_grid %lld\n", (int)p.form, (long long)p.helper_grid);
    return failures.empty() ? 0 : 1;
}

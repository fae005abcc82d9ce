// The rasteriser's launch planning (torchdrivesim_amd/csrc/tds_raster_plan.h) swept on the host: every plan's workspace layout must stay
// inside the room the plan was given, its LDS inside the CU's, its shapes among the kernels' instantiations.  Built and run by
// tests/test_raster_plan_host.py, plain and with the sanitizers.  Prints the plans per form, one line per invariant that failed (with its
// first counter-example) and the binned layout of the smallest call; exit status 1 if an invariant failed.
#include <cstdio>
#include <map>
#include <string>

#include "tds_raster_plan.h"

using namespace tds_raster;

namespace {

struct Failure { long count; std::string first; };
std::map<std::string, Failure> failures;
const PlanInput *g_in;
int64_t g_bytes;

void expect(bool ok, const char *what) {
    if (ok) return;
    Failure &f = failures[what];
    if (f.count++ == 0) {
        char buf[256];
        snprintf(buf, sizeof buf, "n_img %lld res %d out_mode %d n_keys %d listed %d slices %d workspace %lld cus %d", (long long)g_in->n_img, g_in->res,
                 g_in->out_mode, g_in->n_keys, (int)g_in->keys_listed, (int)g_in->want_slices, (long long)g_bytes, g_in->cus);
        f.first = buf;
    }
}

constexpr size_t KiB = 1024;

void check_plan(const PlanInput &in, const RasterPlan &p, int64_t q) {
    const int64_t n = in.n_img, room = in.workspace_bytes;
    switch (p.form) {
    case RasterForm::Error:
        expect(p.error != nullptr, "error: a message");
        return;
    case RasterForm::Bits:
    case RasterForm::Split:
        expect(p.lds <= 150 * KiB, "bits: lds <= 150 KiB");
        expect(p.twp > 0 && p.twp % 32 == 0 && (int64_t)p.strips * p.twp >= in.res, "bits: twp a multiple of 32, strips * twp >= res");
        expect(p.nb == bits_index_bits(in.n_keys), "bits: nb == bits_index_bits(n_keys)");
        expect(p.nwv == 4 || p.nwv == 8, "bits: nwv 4 or 8");
        expect(p.grid >= 1, "bits: grid >= 1");
        if (p.form == RasterForm::Bits) expect(p.grid <= n * p.strips, "bits: grid <= n_img * strips");
        expect(!p.persist || q >= 0, "bits: persistent only where the queues exist");
        if (p.form == RasterForm::Split) {
            expect(p.lds_s <= 150 * KiB, "split: lds_s <= 150 KiB");
            expect(p.lw == 2 || p.lw == 4, "split: lw 2 or 4");
            expect(p.caps >= 128 && p.caps <= 8192 && p.caps % 4 == 0 && p.caps == p.ws.caps, "split: 128 <= caps <= 8192, a multiple of 4");
            expect(p.ws.counts >= 4 * (n + 1), "split: counts >= 4 (n_img + 1)");
            expect(p.ws.lists >= p.ws.counts + 4 * n, "split: lists >= counts + 4 n_img");
            expect(p.ws.lists3 == p.ws.lists + 16 * n * p.caps, "split: lists3 == lists + 16 n_img caps");
            expect(p.ws.lists3 + 4 * n * p.caps <= room, "split: lists3 + 4 n_img caps <= room");
            expect(p.ws.lists % 16 == 0 && p.ws.lists3 % 16 == 0, "split: lists and lists3 16-aligned");
            expect(p.persist, "split: persistent");
        }
        return;
    case RasterForm::Binned:
        expect(p.ws.lists >= 4 * p.grid, "binned: lists >= 4 grid");
        expect(p.ws.lists + 16 * p.grid * p.caps <= room, "binned: lists + 16 grid caps <= room");
        expect(p.caps >= 1, "binned: caps >= 1");
        expect(p.strips <= MAX_STRIPS, "binned: strips <= MAX_STRIPS");
        [[fallthrough]];
    case RasterForm::Fused:
        expect(p.tw == 0 || lds_bytes(p.tw, in.res) <= 160 * KiB, "packed keys: the tile fits 160 KiB");
        return;
    }
}

}  // namespace

int main() {
    const RasterKnobs k = DEFAULT_KNOBS;
    const int modes[4] = {TDS_OUT_F32, TDS_OUT_U8, TDS_OUT_MASK_U8, TDS_OUT_MASK_BITS};
    const int64_t cameras[5] = {1, 3, 64, 65536, ((int64_t)1 << 31) - 1};
    const int cu_counts[3] = {32, 224, 256};
    long per_form[5] = {0, 0, 0, 0, 0};
    for (int r = 1; r <= 523; ++r) {
        const int res = r <= 520 ? r : 1024 << (r - 521);
        for (int n_keys = -1; n_keys <= MAX_KEYS; ++n_keys)
            for (int out_mode : modes)
                for (int64_t n_img : cameras) {
                    const bool masks = is_mask_mode(out_mode);
                    const int64_t recommended = workspace_bytes_for(n_img, res, out_mode, n_keys, k);
                    // no workspace, a small one, the recommended one, a generous one
                    const int64_t sizes[4] = {0, 4096, recommended, 4 * recommended + 4096};
                    for (int size = 0; size < 4; ++size) {
                        const int64_t bytes = sizes[size], q = queue_offset(bytes), room = lists_room(bytes, masks);
                        for (int listed = 0; listed < 2; ++listed)
                            for (int slices = 0; slices < (out_mode == TDS_OUT_F32 ? 2 : 1); ++slices)       // index slices: of the float32 image only
                                for (int cus : cu_counts) {
                                    const PlanInput in = {n_img, res, out_mode, n_keys, listed != 0, true, false, slices != 0, room, cus};
                                    g_in = &in; g_bytes = bytes;
                                    if (bytes > 0) {
                                        expect(q >= 0 && q % 64 == 0 && q + QUEUE_BYTES <= bytes, "workspace: queue_offset 64-aligned, queue_offset + 64 <= bytes");
                                        if (masks) expect(room + MASK_TABLE_BYTES <= q, "workspace: masks, lists_room + MASK_TABLE_BYTES <= queue_offset");
                                        else expect(room <= q, "workspace: lists_room <= queue_offset");
                                    }
                                    const RasterPlan p = plan_raster_scene(in, k);
                                    ++per_form[(int)p.form];
                                    check_plan(in, p, q);
                                }
                    }
                    // the recommended sizes leave the queues behind the lists they were sized for
                    const PlanInput in = {n_img, res, out_mode, n_keys, true, true, false, false, 0, 256};
                    g_in = &in; g_bytes = recommended;
                    const int64_t split_end = split_layout(n_img, LIST_CAPS).lists3, tw = strip_width(res, k);
                    const int64_t binned_end = tw ? n_img * ((res + tw - 1) / tw) * (DEFAULT_CAPS * 16 + 4) : 0;
                    for (int64_t lists : {split_end, binned_end, (int64_t)0})
                        expect(queue_offset(with_queue_tail(lists)) >= lists, "workspace: the recommended size puts the queues behind the lists");
                    expect(camera_prep_bytes(n_img, res, out_mode, n_keys, k) % PREP_RECORD_BYTES == 0, "camera prep: whole records");
                }
    }
    const char *names[5] = {"bits", "split", "binned", "fused", "error"};
    for (int f = 0; f < 5; ++f) printf("plans %s %ld\n", names[f], per_form[f]);
    for (const auto &f : failures) printf("FAILED %s: %ld plans, first %s\n", f.first.c_str(), f.second.count, f.second.first.c_str());
    // one camera of one pixel, unlisted keys, a workspace of 4096 bytes: the counts' alignment takes 252 of the 4032 bytes the 250 records of
    // caps = (4032 - 4) / 16 would need
    const PlanInput tiny = {1, 1, TDS_OUT_F32, -1, false, true, false, false, lists_room(4096, false), 256};
    const RasterPlan p = plan_raster_scene(tiny, k);
    printf("smallest form %s room %lld lists %lld caps %lld end %lld\n", names[(int)p.form], (long long)tiny.workspace_bytes, (long long)p.ws.lists,
           (long long)p.caps, (long long)(p.ws.lists + 16 * p.grid * p.caps));
    return failures.empty() ? 0 : 1;
}

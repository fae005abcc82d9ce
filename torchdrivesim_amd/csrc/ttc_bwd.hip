// K9b: the backward of time to collision (_ops.time_to_collision_grad; include/tdship.h "K9b"): the gradients of the slots' times
// to x, y, length, width, [sin, cos] and speed of every entity, one launch.  Yardstick: the float64 torch-autograd model tests/ttc_grad_model.py;
// the pair gradient is stated once, in tds_ttc_grad.h.
// The gather form, so that nothing is added to memory: the launch of tds_observers.h over the RECEIVING entities of a scene -- a slice of them per
// workgroup, one wave per receiving entity j, the scene's E entities staged in LDS as ttc.hip stages them, no key rows.  The lanes stride over
// the scene's A * K slots; a lane whose slot has j as its observer or as its entity computes the pair gradient and adds its side of it, times
// the slot's incoming gradient, to seven binary64 sums.  The wave adds the lanes' sums by xor-shuffles in a fixed order, so a result does not
// change from run to run; lane 0 rounds to binary32 and writes the whole row of j.
#include "tds_observers.h"
#include "tds_ttc_grad.h"

namespace {

struct TtcBwdArgs {
    const float *boxes, *sc, *speed, *g_ttc;
    const int32_t *index;
    float *g_boxes, *g_sc, *g_speed;
    int A, E, K;
    double margin;
};

// entity e as staged -- x, y, length, width, sin, cos, speed, finite (0 / 1) --: its box, grown by `margin` on every side; false if one of the seven is no number
__device__ __forceinline__ bool staged_box(const float *bx, int e, double margin, tds::TtcBox &q) {
    const float4 p = *(const float4 *)(bx + tds::OBS_WORDS * e);
    const float4 p2 = *(const float4 *)(bx + tds::OBS_WORDS * e + 4);
    q = tds::ttc_box(p.x, p.y, p.z, p.w, p2.x, p2.y, p2.z, margin);
    return p2.w != 0.0f;
}

// the launch of tds_observers.h: grid = (B, ceil(E / OBS_SLICE)), dynamic LDS = lds_bytes(E, false)
__global__ void __launch_bounds__(tds::OBS_BLOCK) time_to_collision_bwd_kernel(TtcBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const tds::SliceThread t;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    t.stage_items(bx, E, [&](int j) {
        tds::Item it = tds::entity_item(g.boxes, g.sc, g.speed, b * E + j);
        it.hi.w = tds::ttc_finite(it.lo.x, it.lo.y, it.lo.z, it.lo.w, it.hi.x, it.hi.y, it.hi.z) ? 1.0f : 0.0f;
        return it;
    });
    const int slots = A * K;                                                 // at most 1024 * 32
    const int32_t *index = g.index + b * slots;
    const float *g_ttc = g.g_ttc + b * slots;
    t.for_slice(E, [&](int j) {                                              // wave-uniform: all 64 lanes meet at the shuffles below
        double sum[tds::TTC_GRADS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (bx[tds::OBS_WORDS * j + 7] != 0.0f) {                           // an entity that is not finite is in no pair that contributes
            for (int s = t.lane; s < slots; s += 64) {
                const int e = index[s];
                const int a = s / K;
                if ((a != j && e != j) || e < 0 || e >= E || e == a) continue;      // not j's slot, an empty slot, garbage: never dereferenced
                tds::TtcBox me, other;
                if (!staged_box(bx, a, g.margin, me) || !staged_box(bx, e, 0.0, other)) continue;
                double ga[tds::TTC_GRADS], ge[tds::TTC_GRADS];
                if (!tds::ttc_pair_grad(me, other, ga, ge)) continue;
                const double gin = (double)g_ttc[s];
                const bool mine = a == j;
#pragma unroll
                for (int i = 0; i < tds::TTC_GRADS; ++i) sum[i] = sum[i] + gin * (mine ? ga[i] : ge[i]);
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                   // a butterfly: the same order of additions every run
#pragma unroll
            for (int i = 0; i < tds::TTC_GRADS; ++i) sum[i] = sum[i] + __shfl_xor(sum[i], s);
        }
        if (t.lane == 0) {                                                   // the whole row of j, zeros included
            float *gb = g.g_boxes + (b * E + j) * 5;
            gb[0] = (float)sum[tds::TTC_GX], gb[1] = (float)sum[tds::TTC_GY], gb[2] = (float)sum[tds::TTC_GLENGTH], gb[3] = (float)sum[tds::TTC_GWIDTH];
            gb[4] = 0.0f;                                                    // psi is not read: it gets its gradient through [sin, cos]
            *(float2 *)(g.g_sc + (b * E + j) * 2) = make_float2((float)sum[tds::TTC_GSIN], (float)sum[tds::TTC_GCOS]);
            g.g_speed[b * E + j] = (float)sum[tds::TTC_GSPEED];
        }
    });
}

}  // namespace

TDS_EXPORT int tds_time_to_collision_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_ttc,
                                             float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, float margin,
                                             void *stream) {
    const char *what = "tds_time_to_collision_bwd_f32";
    TDS_CHECK_ARG(tds::ttc_finite(margin), "%s: margin must be finite (got %g)", what, (double)margin);
    if (int rc = tds::check_frame(what, B, A, E, K, TDS_TTC_MAX_K, tds::frame_entities(TDS_TTC_MAX_ENTITIES), E); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(boxes && sc && speed && g_boxes && g_sc && g_speed && (A == 0 || (index && g_ttc)), "%s: null pointer", what);
    TtcBwdArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.g_ttc = g_ttc; g.index = index;
    g.g_boxes = g_boxes; g.g_sc = g_sc; g.g_speed = g_speed;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.margin = (double)margin;
    hipLaunchKernelGGL(time_to_collision_bwd_kernel, tds::slice_grid(B, E), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, false), (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("time_to_collision_bwd_kernel");
    return TDS_OK;
}

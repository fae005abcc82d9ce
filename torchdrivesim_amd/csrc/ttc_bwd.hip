// K9b: the backward of time to collision (_ops.time_to_collision_grad; include/tdship.h "K9b"): the gradients of the slots' times
// to x, y, length, width, [sin, cos] and speed of every entity, one launch.  Yardstick: the float64 torch-autograd model tests/ttc_grad_model.py;
// the pair gradient is stated once, in tds_ttc_grad.h.
// The gather form, so that nothing is added to memory: one workgroup = a slice of TTCB_ENTITIES RECEIVING entities of one scene; the scene's E
// entities are staged in LDS once, 32 bytes each, as ttc.hip stages them; one wave per receiving entity j, the waves of a workgroup taking the
// entities of the slice in turn.  The lanes stride over the scene's A * K slots; a lane whose slot has j as its observer or as its entity computes
// the pair gradient and adds its side of it, times the slot's incoming gradient, to seven binary64 sums.  The wave adds the lanes' sums by
// xor-shuffles in a fixed order, so a result does not change from run to run; lane 0 rounds to binary32 and writes the whole row of j.
#include "tds_common.h"
#include "tds_ttc_grad.h"

namespace {

constexpr int TTCB_BLOCK = 256;         // 4 waves
constexpr int TTCB_WAVES = TTCB_BLOCK / 64;
constexpr int TTCB_ENTITIES = 16;       // receiving entities per workgroup: four per wave
constexpr int TTCB_WORDS = 8;           // LDS words per entity: x, y, length, width, sin, cos, speed, finite (0 / 1: all seven are numbers)

struct TtcBwdArgs {
    const float *boxes, *sc, *speed, *g_ttc;
    const int32_t *index;
    float *g_boxes, *g_sc, *g_speed;
    int A, E, K;
    double margin;
};

// entity e as staged: its box, grown by `margin` on every side; false if one of its seven values is no number
__device__ __forceinline__ bool staged_box(const float *bx, int e, double margin, tds::TtcBox &q) {
    const float4 p = *(const float4 *)(bx + TTCB_WORDS * e);
    const float4 p2 = *(const float4 *)(bx + TTCB_WORDS * e + 4);
    q = tds::ttc_box(p.x, p.y, p.z, p.w, p2.x, p2.y, p2.z, margin);
    return p2.w != 0.0f;
}

// grid = (B, ceil(E / TTCB_ENTITIES)); dynamic LDS = E * TTCB_WORDS floats
__global__ void __launch_bounds__(TTCB_BLOCK) time_to_collision_bwd_kernel(TtcBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    for (int j = tid; j < E; j += TTCB_BLOCK) {
        const float *p = g.boxes + (b * E + j) * 5;
        const float2 sc = *(const float2 *)(g.sc + (b * E + j) * 2);
        const float v = g.speed[b * E + j];
        const float x = p[0], y = p[1], l = p[2], w = p[3];
        const bool ok = tds::ttc_finite(x) && tds::ttc_finite(y) && tds::ttc_finite(l) && tds::ttc_finite(w) && tds::ttc_finite(sc.x) &&
                        tds::ttc_finite(sc.y) && tds::ttc_finite(v);
        *(float4 *)(bx + TTCB_WORDS * j) = make_float4(x, y, l, w);
        *(float4 *)(bx + TTCB_WORDS * j + 4) = make_float4(sc.x, sc.y, v, ok ? 1.0f : 0.0f);
    }
    __syncthreads();
    const int slots = A * K;                                                 // at most 1024 * 32
    const int32_t *index = g.index + b * slots;
    const float *g_ttc = g.g_ttc + b * slots;
    const int j0 = blockIdx.y * TTCB_ENTITIES, j1 = min(j0 + TTCB_ENTITIES, E);
    for (int j = j0 + wave; j < j1; j += TTCB_WAVES) {                       // wave-uniform: all 64 lanes meet at the shuffles below
        double sum[tds::TTC_GRADS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (bx[TTCB_WORDS * j + 7] != 0.0f) {                                // an entity that is not finite is in no pair that contributes
            for (int s = lane; s < slots; s += 64) {
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
        if (lane == 0) {                                                     // the whole row of j, zeros included
            float *gb = g.g_boxes + (b * E + j) * 5;
            gb[0] = (float)sum[tds::TTC_GX], gb[1] = (float)sum[tds::TTC_GY], gb[2] = (float)sum[tds::TTC_GLENGTH], gb[3] = (float)sum[tds::TTC_GWIDTH];
            gb[4] = 0.0f;                                                    // psi is not read: it gets its gradient through [sin, cos]
            *(float2 *)(g.g_sc + (b * E + j) * 2) = make_float2((float)sum[tds::TTC_GSIN], (float)sum[tds::TTC_GCOS]);
            g.g_speed[b * E + j] = (float)sum[tds::TTC_GSPEED];
        }
    }
}

}  // namespace

TDS_EXPORT int tds_time_to_collision_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_ttc,
                                             float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, float margin,
                                             void *stream) {
    const char *what = "tds_time_to_collision_bwd_f32";
    TDS_CHECK_ARG(B >= 0 && A >= 0 && E >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld E=%lld", what, (long long)B, (long long)A, (long long)E);
    TDS_CHECK_ARG(K >= 1 && K <= TDS_TTC_MAX_K, "%s: K must be 1 .. %d (got %d)", what, TDS_TTC_MAX_K, K);
    TDS_CHECK_ARG(tds::ttc_finite(margin), "%s: margin must be finite (got %g)", what, (double)margin);
    TDS_CHECK_ARG(A <= E, "%s: %lld exposed agents but only %lld entities", what, (long long)A, (long long)E);
    if (E > TDS_TTC_MAX_ENTITIES) {
        tds::set_error("%s: %lld entities per scene (the entities of a scene live in LDS: at most %d)", what, (long long)E, TDS_TTC_MAX_ENTITIES);
        return TDS_ELIMIT;
    }
    if (B == 0 || E == 0) return TDS_OK;
    TDS_CHECK_ARG(boxes && sc && speed && g_boxes && g_sc && g_speed && (A == 0 || (index && g_ttc)), "%s: null pointer", what);
    TtcBwdArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.g_ttc = g_ttc; g.index = index;
    g.g_boxes = g_boxes; g.g_sc = g_sc; g.g_speed = g_speed;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.margin = (double)margin;
    const size_t lds = (size_t)E * TTCB_WORDS * sizeof(float);
    hipLaunchKernelGGL(time_to_collision_bwd_kernel, dim3((unsigned)B, (unsigned)((E + TTCB_ENTITIES - 1) / TTCB_ENTITIES)), dim3(TTCB_BLOCK), lds,
                       (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("time_to_collision_bwd_kernel");
    return TDS_OK;
}

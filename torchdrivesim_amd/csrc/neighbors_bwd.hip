// K6b: the backward of the neighbour observations (_ops.neighbors_grad; include/tdship.h "K6b"): the gradients of the slots' eight
// features to x, y, length, width, [sin, cos] and speed of every entity, one launch.  Yardstick: the float64 torch-autograd model
// tests/neighbors_grad_model.py; the slot gradient is stated once, in tds_neighbors_grad.h.
// The gather form of ttc_bwd.hip, so that nothing is added to memory: the launch of tds_observers.h over the RECEIVING entities of a scene -- a
// slice of 16 of them per workgroup, the scene's E entities staged in LDS as neighbors.hip stages them, no key rows.  The work per receiving entity
// j is small and bound by instruction issue, so a wave takes FOUR of them at once, NB_ROW_LANES = 16 lanes each: a workgroup's four waves have
// the slice's 16 rows in one pass.  The 16 lanes of j stride over the scene's A * K slots and read the index alone, NB_AHEAD words in flight per
// lane; a lane whose slot names j computes the slot gradient and adds the entity's side of it to seven binary64 sums.  The observer's side needs
// no search: j's own K slots are consecutive.  The 16 lanes' sums are added by xor-shuffles in a fixed order, so a result does not change from
// run to run; the first lane of j rounds to binary32 and writes the whole row of j.
#include "tds_observers.h"
#include "tds_neighbors_grad.h"

namespace {

constexpr int NB_ROW_LANES = 16;        // lanes per receiving entity: four entities per wave
constexpr int NB_AHEAD = 16;            // index words a lane has in flight while it looks for j: 256 slots a turn
static_assert(tds::OBS_SLICE == tds::OBS_WAVES * (64 / NB_ROW_LANES), "the waves of a workgroup have its slice of rows in one pass");

struct NeighborsBwdArgs {
    const float *boxes, *sc, *speed, *g_features;
    const int32_t *index;
    float *g_boxes, *g_sc, *g_speed;
    int A, E, K;
};

// entity e as staged: x, y, length, width, sin, cos, speed, 0
__device__ __forceinline__ tds::NbPose staged_pose(const float *bx, int e) {
    const float4 p = *(const float4 *)(bx + tds::OBS_WORDS * e);
    const float4 p2 = *(const float4 *)(bx + tds::OBS_WORDS * e + 4);
    return tds::nb_pose(p.x, p.y, p2.x, p2.y, p2.z);
}

// the slot gradient of slot s of the scene, observer a and entity e both in [0, E): its eight incoming gradients are read here and nowhere else
__device__ __forceinline__ void slot_grad(const float *bx, const float *g_features, int s, int a, int e, double *ga, double *ge) {
    const float *gp = g_features + (int64_t)s * 8;
    const double g[8] = {(double)gp[0], (double)gp[1], (double)gp[2], (double)gp[3], (double)gp[4], (double)gp[5], (double)gp[6], (double)gp[7]};
    tds::neighbors_slot_grad(staged_pose(bx, a), staged_pose(bx, e), g, ga, ge);
}

// the launch of tds_observers.h: grid = (B, ceil(E / OBS_SLICE)), dynamic LDS = lds_bytes(E, false)
__global__ void __launch_bounds__(tds::OBS_BLOCK) neighbors_bwd_kernel(NeighborsBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const tds::SliceThread t;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    t.stage_items(bx, E, [&](int j) { return tds::entity_item(g.boxes, g.sc, g.speed, b * E + j); });
    const int slots = A * K;                                                 // at most 1024 * 32
    const int32_t *index = g.index + b * slots;
    const float *g_features = g.g_features + b * slots * 8;
    const int sub = t.lane & (NB_ROW_LANES - 1);
    const int j = blockIdx.y * tds::OBS_SLICE + t.wave * (64 / NB_ROW_LANES) + t.lane / NB_ROW_LANES;
    const bool row = j < E;                                                  // (the last slice of a scene may be short)
    double sum[tds::NB_GRADS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double ga[tds::NB_GRADS], ge[tds::NB_GRADS];
    for (int s0 = sub; s0 < slots; s0 += NB_ROW_LANES * NB_AHEAD) {          // j as the entity of somebody's slot
        uint32_t mine = 0;                                                   // bit u: slot s0 + 16 u names j
#pragma unroll
        for (int u = 0; u < NB_AHEAD; ++u) {
            const int s = s0 + NB_ROW_LANES * u;
            const int e = s < slots ? index[s] : -1;
            mine |= (uint32_t)(row && e == j) << u;                          // j is in [0, E): an empty slot and garbage never match
        }                                                                    // (these loads do not wait for each other: one latency per turn)
        for (; mine != 0; mine &= mine - 1) {                                // in slot order
            const int s = s0 + NB_ROW_LANES * (__ffs(mine) - 1);
            const int a = s / K;
            if (a == j) continue;                                            // the observer's own: garbage, treated as empty
            slot_grad(bx, g_features, s, a, j, ga, ge);
#pragma unroll
            for (int i = 0; i < tds::NB_GRADS; ++i) sum[i] = sum[i] + ge[i];
        }
    }
    if (row && j < A) {                                                      // j as the observer of its own row
        for (int k = sub; k < K; k += NB_ROW_LANES) {
            const int s = j * K + k;
            const int e = index[s];
            if (e < 0 || e >= E || e == j) continue;                         // an empty slot or garbage: never dereferenced
            slot_grad(bx, g_features, s, j, e, ga, ge);
            sum[tds::NB_GX] = sum[tds::NB_GX] + ga[tds::NB_GX], sum[tds::NB_GY] = sum[tds::NB_GY] + ga[tds::NB_GY];
            sum[tds::NB_GSIN] = sum[tds::NB_GSIN] + ga[tds::NB_GSIN], sum[tds::NB_GCOS] = sum[tds::NB_GCOS] + ga[tds::NB_GCOS];
            sum[tds::NB_GSPEED] = sum[tds::NB_GSPEED] + ga[tds::NB_GSPEED];
        }
    }
#pragma unroll
    for (int s = NB_ROW_LANES / 2; s > 0; s >>= 1) {                         // a butterfly over the 16 lanes of j: the same order of additions every run
#pragma unroll
        for (int i = 0; i < tds::NB_GRADS; ++i) sum[i] = sum[i] + __shfl_xor(sum[i], s);
    }
    if (row && sub == 0) {                                                   // the whole row of j, zeros included
        float *gb = g.g_boxes + (b * E + j) * 5;
        gb[0] = (float)sum[tds::NB_GX], gb[1] = (float)sum[tds::NB_GY], gb[2] = (float)sum[tds::NB_GLENGTH], gb[3] = (float)sum[tds::NB_GWIDTH];
        gb[4] = 0.0f;                                                        // psi is not read: it gets its gradient through [sin, cos]
        *(float2 *)(g.g_sc + (b * E + j) * 2) = make_float2((float)sum[tds::NB_GSIN], (float)sum[tds::NB_GCOS]);
        g.g_speed[b * E + j] = (float)sum[tds::NB_GSPEED];
    }
}

}  // namespace

TDS_EXPORT int tds_neighbors_bwd_f32(const float *boxes, const float *sc, const float *speed, const int32_t *index, const float *g_features,
                                     float *g_boxes, float *g_sc, float *g_speed, int64_t B, int64_t A, int64_t E, int K, void *stream) {
    const char *what = "tds_neighbors_bwd_f32";
    if (int rc = tds::check_frame(what, B, A, E, K, TDS_NEIGHBORS_MAX_K, tds::frame_entities(TDS_NEIGHBORS_MAX_ENTITIES), E); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(boxes && sc && speed && g_boxes && g_sc && g_speed && (A == 0 || (index && g_features)), "%s: null pointer", what);
    NeighborsBwdArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.g_features = g_features; g.index = index;
    g.g_boxes = g_boxes; g.g_sc = g_sc; g.g_speed = g_speed;
    g.A = (int)A; g.E = (int)E; g.K = K;
    hipLaunchKernelGGL(neighbors_bwd_kernel, tds::slice_grid(B, E), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, false), (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("neighbors_bwd_kernel");
    return TDS_OK;
}

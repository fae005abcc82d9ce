// K6: neighbour observations (Simulator.compute_neighbors).  For every exposed agent the K nearest OTHER entities within max_distance, nearest
// first, in the observer's frame, with relative velocity and size.  No reference counterpart: the definition is this project's own
// (include/tdship.h "K6"; binary32 model, bit for bit: tests/neighbors_model.py).
// One workgroup = a slice of NB_AGENTS observers of one scene; the scene's E entities are staged in LDS once, 32 bytes each; one wave per
// observer, the waves of a workgroup taking the observers of the slice in turn.  The wave selects the K smallest keys (bits of d2) << 32 | e of the
// candidates (tds_select.h, shared with the stop lines of lights.hip): by rank among the candidate lanes up to 64 entities, in K rounds of a wave-wide
// minimum over keys in LDS above.
// All arithmetic is binary32 + - *, rounded once each (-ffp-contract=off).
#include "tds_common.h"
#include "tds_select.h"
#include <algorithm>

namespace {

constexpr int NB_BLOCK = 256;           // 4 waves
constexpr int NB_WAVES = NB_BLOCK / 64;
constexpr int NB_AGENTS = 16;           // observers per workgroup: four per wave
constexpr int NB_WORDS = 8;             // LDS words per entity: x, y, length, width, sin, cos, speed, present (0 / 1)
using tds::NO_KEY;                      // the d2 bits of an entity that is no candidate

struct NeighborArgs {
    const float *boxes, *sc, *speed;
    const uint8_t *present, *visible;
    float *features;
    int32_t *index;
    int A, E, K;
    float r2;
};

// the d2 bits of entity e as observer a (at ax, ay) sees it, NO_KEY if it is no candidate
__device__ __forceinline__ uint32_t key_of(const float *bx, const uint8_t *vis, int a, int e, float ax, float ay, float r2) {
    const float4 q = *(const float4 *)(bx + NB_WORDS * e);
    const float dx = q.x - ax, dy = q.y - ay;
    const float d2 = dx * dx + dy * dy;
    bool ok = e != a && bx[NB_WORDS * e + 7] != 0.0f && d2 <= r2;        // (a NaN d2 fails the comparison)
    if (vis != nullptr) ok = ok && vis[e] != 0;
    return ok ? __float_as_uint(d2) : NO_KEY;
}

// slot k of the row that starts at `row` (in slots): entity e (-1: an empty slot) seen from the observer me / me2
__device__ __forceinline__ void store_slot(const NeighborArgs &g, const float *bx, int64_t row, int k, int e, const float4 me, const float4 me2) {
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
    if (e >= 0) {
        const float4 q = *(const float4 *)(bx + NB_WORDS * e);
        const float4 q2 = *(const float4 *)(bx + NB_WORDS * e + 4);
        const float s = me2.x, c = me2.y, se = q2.x, ce = q2.y;
        const float dx = q.x - me.x, dy = q.y - me.y;
        const float sin_rel = se * c - ce * s, cos_rel = ce * c + se * s;
        lo = make_float4(dx * c + dy * s, dy * c - dx * s, sin_rel, cos_rel);
        hi = make_float4(q2.z * cos_rel - me2.z, q2.z * sin_rel, q.z, q.w);
    }
    float4 *out = (float4 *)(g.features + (row + k) * 8);
    out[0] = lo;
    out[1] = hi;
    g.index[row + k] = e;
}

// grid = (B, ceil(A / NB_AGENTS)); dynamic LDS = E * NB_WORDS floats, and for E > 64 another NB_WAVES * E words of keys
__global__ void __launch_bounds__(NB_BLOCK) neighbors_kernel(NeighborArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    for (int j = tid; j < E; j += NB_BLOCK) {
        const float *p = g.boxes + (b * E + j) * 5;
        const float2 sc = *(const float2 *)(g.sc + (b * E + j) * 2);
        *(float4 *)(bx + NB_WORDS * j) = make_float4(p[0], p[1], p[2], p[3]);
        *(float4 *)(bx + NB_WORDS * j + 4) = make_float4(sc.x, sc.y, g.speed[b * E + j], g.present[b * E + j] ? 1.0f : 0.0f);
    }
    __syncthreads();
    uint32_t *wk = (uint32_t *)(bx + NB_WORDS * E) + wave * E;           // (E > 64 only) this wave's row of d2 bits
    const int a0 = blockIdx.y * NB_AGENTS, a1 = min(a0 + NB_AGENTS, A);
    for (int a = a0 + wave; a < a1; a += NB_WAVES) {                     // wave-uniform: all 64 lanes stay together below
        const int64_t row = (b * A + a) * K;
        const float4 me = *(const float4 *)(bx + NB_WORDS * a);
        const float4 me2 = *(const float4 *)(bx + NB_WORDS * a + 4);
        if (me2.w == 0.0f) {                                             // an observer that is not present: an empty row
            if (lane < K) store_slot(g, bx, row, lane, -1, me, me2);
            continue;
        }
        const uint8_t *vis = g.visible ? g.visible + (b * A + a) * E : nullptr;
        const auto store = [&](int k, int e) { store_slot(g, bx, row, k, e, me, me2); };
        if (E <= 64)
            tds::select_by_rank(lane < E ? key_of(bx, vis, a, lane, me.x, me.y, g.r2) : NO_KEY, lane, K, store);
        else
            tds::select_by_rounds(wk, E, lane, K, [&](int e) { return key_of(bx, vis, a, e, me.x, me.y, g.r2); }, store);
    }
}

}  // namespace

TDS_EXPORT int tds_neighbors_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                                 float *features, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float max_distance, void *stream) {
    const char *what = "tds_neighbors_f32";
    TDS_CHECK_ARG(B >= 0 && A >= 0 && E >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld E=%lld", what, (long long)B, (long long)A, (long long)E);
    TDS_CHECK_ARG(K >= 1 && K <= TDS_NEIGHBORS_MAX_K, "%s: K must be 1 .. %d (got %d)", what, TDS_NEIGHBORS_MAX_K, K);
    TDS_CHECK_ARG(A <= E, "%s: %lld exposed agents but only %lld entities", what, (long long)A, (long long)E);
    TDS_CHECK_ARG(max_distance >= 0.0f, "%s: max_distance must not be negative or NaN (got %g)", what, (double)max_distance);
    if (E > TDS_NEIGHBORS_MAX_ENTITIES) {
        tds::set_error("%s: %lld entities per scene (the entities of a scene live in LDS: at most %d)", what, (long long)E, TDS_NEIGHBORS_MAX_ENTITIES);
        return TDS_ELIMIT;
    }
    if (B == 0 || A == 0) return TDS_OK;
    TDS_CHECK_ARG(boxes && sc && speed && present && features && index, "%s: null pointer", what);
    NeighborArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.present = present; g.visible = visible;
    g.features = features; g.index = index;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.r2 = max_distance * max_distance;
    const size_t lds = (size_t)E * NB_WORDS * sizeof(float) + (E > 64 ? (size_t)NB_WAVES * E * sizeof(uint32_t) : 0);
    hipLaunchKernelGGL(neighbors_kernel, dim3((unsigned)B, (unsigned)((A + NB_AGENTS - 1) / NB_AGENTS)), dim3(NB_BLOCK), lds, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("neighbors_kernel");
    return TDS_OK;
}

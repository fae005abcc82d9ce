// K9: time to collision (Simulator.compute_time_to_collision).  For every exposed agent the K OTHER entities it would touch first within the
// horizon if everybody kept velocity and heading, soonest first, and when.  No reference counterpart: the definition is this project's own
// (include/tdship.h "K9"; float64 model, bit for bit: tests/ttc_model.py); the pair test is stated once, in tds_ttc.h.
// The launch is that of neighbors.hip: one workgroup = a slice of TTC_AGENTS observers of one scene; the scene's E entities are staged in LDS
// once, 32 bytes each; one wave per observer, the waves of a workgroup taking the observers of the slice in turn.  The wave selects the K smallest
// keys (bits of the float32 time) << 32 | e of the candidates (tds_select.h): by rank up to 64 entities, in K rounds of a wave-wide minimum above.
#include "tds_common.h"
#include "tds_select.h"
#include "tds_ttc.h"
#include <algorithm>

namespace {

constexpr int TTC_BLOCK = 256;          // 4 waves
constexpr int TTC_WAVES = TTC_BLOCK / 64;
constexpr int TTC_AGENTS = 16;          // observers per workgroup: four per wave
constexpr int TTC_WORDS = 8;            // LDS words per entity: x, y, length, width, sin, cos, speed, usable (0 / 1: present and all seven finite)
using tds::NO_KEY;                      // the time bits of an entity that is no candidate

struct TtcArgs {
    const float *boxes, *sc, *speed;
    const uint8_t *present, *visible;
    float *ttc;
    int32_t *index;
    int A, E, K;
    double horizon, margin;
};

// the time bits of entity e against the observer a (its box `me`, grown by the margin), NO_KEY if it is no candidate
__device__ __forceinline__ uint32_t key_of(const float *bx, const uint8_t *vis, int a, int e, const tds::TtcBox &me, double horizon) {
    const float4 q = *(const float4 *)(bx + TTC_WORDS * e);
    const float4 q2 = *(const float4 *)(bx + TTC_WORDS * e + 4);
    bool ok = e != a && q2.w != 0.0f;
    if (vis != nullptr) ok = ok && vis[e] != 0;
    if (!ok) return NO_KEY;
    float t;
    if (!tds::ttc_pair(me, tds::ttc_box(q.x, q.y, q.z, q.w, q2.x, q2.y, q2.z, 0.0), horizon, &t)) return NO_KEY;
    return __float_as_uint(t);
}

// slot k of the row that starts at `row` (in slots): entity e with the time bits `key`; e = -1: an empty slot
__device__ __forceinline__ void store_slot(const TtcArgs &g, int64_t row, int k, int e, uint32_t key) {
    g.ttc[row + k] = e >= 0 ? __uint_as_float(key) : INFINITY;
    g.index[row + k] = e;
}

// grid = (B, ceil(A / TTC_AGENTS)); dynamic LDS = E * TTC_WORDS floats, and for E > 64 another TTC_WAVES * E words of keys
__global__ void __launch_bounds__(TTC_BLOCK) time_to_collision_kernel(TtcArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    for (int j = tid; j < E; j += TTC_BLOCK) {
        const float *p = g.boxes + (b * E + j) * 5;
        const float2 sc = *(const float2 *)(g.sc + (b * E + j) * 2);
        const float v = g.speed[b * E + j];
        const float x = p[0], y = p[1], l = p[2], w = p[3];
        const bool ok = g.present[b * E + j] && tds::ttc_finite(x) && tds::ttc_finite(y) && tds::ttc_finite(l) && tds::ttc_finite(w) &&
                        tds::ttc_finite(sc.x) && tds::ttc_finite(sc.y) && tds::ttc_finite(v);
        *(float4 *)(bx + TTC_WORDS * j) = make_float4(x, y, l, w);
        *(float4 *)(bx + TTC_WORDS * j + 4) = make_float4(sc.x, sc.y, v, ok ? 1.0f : 0.0f);
    }
    __syncthreads();
    uint32_t *wk = (uint32_t *)(bx + TTC_WORDS * E) + wave * E;          // (E > 64 only) this wave's row of time bits
    const int a0 = blockIdx.y * TTC_AGENTS, a1 = min(a0 + TTC_AGENTS, A);
    for (int a = a0 + wave; a < a1; a += TTC_WAVES) {                    // wave-uniform: all 64 lanes stay together below
        const int64_t row = (b * A + a) * K;
        const float4 q = *(const float4 *)(bx + TTC_WORDS * a);
        const float4 q2 = *(const float4 *)(bx + TTC_WORDS * a + 4);
        if (q2.w == 0.0f) {                                              // an observer that is absent or not finite: an empty row
            if (lane < K) store_slot(g, row, lane, -1, NO_KEY);
            continue;
        }
        const tds::TtcBox me = tds::ttc_box(q.x, q.y, q.z, q.w, q2.x, q2.y, q2.z, g.margin);
        const uint8_t *vis = g.visible ? g.visible + (b * A + a) * E : nullptr;
        if (E <= 64) {
            const uint32_t key = lane < E ? key_of(bx, vis, a, lane, me, g.horizon) : NO_KEY;
            tds::select_by_rank(key, lane, K, [&](int k, int e) { store_slot(g, row, k, e, key); });      // a filled slot is stored by its own lane
        } else {
            const auto key = [&](int e) { return key_of(bx, vis, a, e, me, g.horizon); };
            // the lane that stores slot k is not the one that computed the winner's key: it computes it again, the same bits
            tds::select_by_rounds(wk, E, lane, K, key, [&](int k, int e) { store_slot(g, row, k, e, e >= 0 ? key(e) : NO_KEY); });
        }
    }
}

}  // namespace

TDS_EXPORT int tds_time_to_collision_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                                         float *ttc, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float horizon, float margin, void *stream) {
    const char *what = "tds_time_to_collision_f32";
    TDS_CHECK_ARG(B >= 0 && A >= 0 && E >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld E=%lld", what, (long long)B, (long long)A, (long long)E);
    TDS_CHECK_ARG(K >= 1 && K <= TDS_TTC_MAX_K, "%s: K must be 1 .. %d (got %d)", what, TDS_TTC_MAX_K, K);
    TDS_CHECK_ARG(horizon >= 0.0f, "%s: horizon must not be negative or NaN (got %g)", what, (double)horizon);
    TDS_CHECK_ARG(tds::ttc_finite(margin), "%s: margin must be finite (got %g)", what, (double)margin);
    TDS_CHECK_ARG(A <= E, "%s: %lld exposed agents but only %lld entities", what, (long long)A, (long long)E);
    if (E > TDS_TTC_MAX_ENTITIES) {
        tds::set_error("%s: %lld entities per scene (the entities of a scene live in LDS: at most %d)", what, (long long)E, TDS_TTC_MAX_ENTITIES);
        return TDS_ELIMIT;
    }
    if (B == 0 || A == 0) return TDS_OK;
    TDS_CHECK_ARG(boxes && sc && speed && present && ttc && index, "%s: null pointer", what);
    TtcArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.present = present; g.visible = visible;
    g.ttc = ttc; g.index = index;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.horizon = (double)horizon; g.margin = (double)margin;
    const size_t lds = (size_t)E * TTC_WORDS * sizeof(float) + (E > 64 ? (size_t)TTC_WAVES * E * sizeof(uint32_t) : 0);
    hipLaunchKernelGGL(time_to_collision_kernel, dim3((unsigned)B, (unsigned)((A + TTC_AGENTS - 1) / TTC_AGENTS)), dim3(TTC_BLOCK), lds, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("time_to_collision_kernel");
    return TDS_OK;
}

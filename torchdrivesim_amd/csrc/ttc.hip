// K9: time to collision (Simulator.compute_time_to_collision).  For every exposed agent the K OTHER entities it would touch first within the
// horizon if everybody kept velocity and heading, soonest first, and when.  No reference counterpart: the definition is this project's own
// (include/tdship.h "K9"; float64 model, bit for bit: tests/ttc_model.py); the pair test is stated once, in tds_ttc.h.
// The launch, the staging of the scene's E entities in LDS and the selection of the K smallest keys (bits of the float32 time) << 32 | e are the
// frame of tds_observers.h; this file says what a key is and what a slot holds.
#include "tds_observers.h"
#include "tds_ttc.h"

namespace {

constexpr int TTC_WORDS = tds::OBS_WORDS;       // LDS words per entity: x, y, length, width, sin, cos, speed, usable (0 / 1: present and all seven finite)

struct TtcArgs {
    const float *boxes, *sc, *speed;
    const uint8_t *present, *visible;
    float *ttc;
    int32_t *index;
    int A, E, K;
    double horizon, margin;
};

// the time bits of entity e against the observer a (its box `me`, grown by the margin), tds::NO_KEY if it is no candidate
__device__ __forceinline__ uint32_t key_of(const float *bx, const uint8_t *vis, int a, int e, const tds::TtcBox &me, double horizon) {
    const float4 q = *(const float4 *)(bx + TTC_WORDS * e);
    const float4 q2 = *(const float4 *)(bx + TTC_WORDS * e + 4);
    bool ok = e != a && q2.w != 0.0f;
    if (vis != nullptr) ok = ok && vis[e] != 0;
    if (!ok) return tds::NO_KEY;
    float t;
    if (!tds::ttc_pair(me, tds::ttc_box(q.x, q.y, q.z, q.w, q2.x, q2.y, q2.z, 0.0), horizon, &t)) return tds::NO_KEY;
    return __float_as_uint(t);
}

// slot k of the row that starts at `row` (in slots): entity e with the time bits `key`; e = -1: an empty slot
__device__ __forceinline__ void store_slot(const TtcArgs &g, int64_t row, int k, int e, uint32_t key) {
    g.ttc[row + k] = e >= 0 ? __uint_as_float(key) : INFINITY;
    g.index[row + k] = e;
}

// the launch of tds_observers.h: grid = (B, ceil(A / OBS_SLICE)), dynamic LDS = lds_bytes(E, true)
__global__ void __launch_bounds__(tds::OBS_BLOCK) time_to_collision_kernel(TtcArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const tds::SliceThread t;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    t.stage_items(bx, E, [&](int j) {
        tds::Item it = tds::entity_item(g.boxes, g.sc, g.speed, b * E + j);
        it.hi.w = g.present[b * E + j] && tds::ttc_finite(it.lo.x, it.lo.y, it.lo.z, it.lo.w, it.hi.x, it.hi.y, it.hi.z) ? 1.0f : 0.0f;
        return it;
    });
    t.for_slice(A, [&](int a) {
        const int64_t row = (b * A + a) * K;
        const float4 q = *(const float4 *)(bx + TTC_WORDS * a);
        const float4 q2 = *(const float4 *)(bx + TTC_WORDS * a + 4);
        const auto store = [=](int k, int e, uint32_t key) { store_slot(g, row, k, e, key); };
        if (q2.w == 0.0f) return t.empty_row(K, store);                  // an observer that is absent or not finite
        const tds::TtcBox me = tds::ttc_box(q.x, q.y, q.z, q.w, q2.x, q2.y, q2.z, g.margin);
        const uint8_t *vis = g.visible ? g.visible + (b * A + a) * E : nullptr;
        t.select_row(bx, E, K, [&](int e) { return key_of(bx, vis, a, e, me, g.horizon); }, store);
    });
}

}  // namespace

TDS_EXPORT int tds_time_to_collision_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                                         float *ttc, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float horizon, float margin, void *stream) {
    const char *what = "tds_time_to_collision_f32";
    TDS_CHECK_ARG(horizon >= 0.0f, "%s: horizon must not be negative or NaN (got %g)", what, (double)horizon);
    TDS_CHECK_ARG(tds::ttc_finite(margin), "%s: margin must be finite (got %g)", what, (double)margin);
    if (int rc = tds::check_frame(what, B, A, E, K, TDS_TTC_MAX_K, tds::frame_entities(TDS_TTC_MAX_ENTITIES), A); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(boxes && sc && speed && present && ttc && index, "%s: null pointer", what);
    TtcArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.present = present; g.visible = visible;
    g.ttc = ttc; g.index = index;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.horizon = (double)horizon; g.margin = (double)margin;
    hipLaunchKernelGGL(time_to_collision_kernel, tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, true), (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("time_to_collision_kernel");
    return TDS_OK;
}

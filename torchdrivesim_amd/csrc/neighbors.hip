// K6: neighbour observations (Simulator.compute_neighbors).  For every exposed agent the K nearest OTHER entities within max_distance, nearest
// first, in the observer's frame, with relative velocity and size.  No reference counterpart: the definition is this project's own
// (include/tdship.h "K6"; binary32 model, bit for bit: tests/neighbors_model.py).
// The launch, the staging of the scene's E entities in LDS and the selection of the K smallest keys (bits of d2) << 32 | e are the frame of
// tds_observers.h; this file says what a key is and what a slot holds.  All arithmetic is binary32 + - *, rounded once each (-ffp-contract=off).
#include "tds_observers.h"

namespace {

constexpr int NB_WORDS = tds::OBS_WORDS;        // LDS words per entity: x, y, length, width, sin, cos, speed, present (0 / 1)

struct NeighborArgs {
    const float *boxes, *sc, *speed;
    const uint8_t *present, *visible;
    float *features;
    int32_t *index;
    int A, E, K;
    float r2;
};

// the d2 bits of entity e as observer a (at ax, ay) sees it, tds::NO_KEY if it is no candidate
__device__ __forceinline__ uint32_t key_of(const float *bx, const uint8_t *vis, int a, int e, float ax, float ay, float r2) {
    const float4 q = *(const float4 *)(bx + NB_WORDS * e);
    const float dx = q.x - ax, dy = q.y - ay;
    const float d2 = dx * dx + dy * dy;
    bool ok = e != a && bx[NB_WORDS * e + 7] != 0.0f && d2 <= r2;        // (a NaN d2 fails the comparison)
    if (vis != nullptr) ok = ok && vis[e] != 0;
    return ok ? __float_as_uint(d2) : tds::NO_KEY;
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

// the launch of tds_observers.h: grid = (B, ceil(A / OBS_SLICE)), dynamic LDS = lds_bytes(E, true)
__global__ void __launch_bounds__(tds::OBS_BLOCK) neighbors_kernel(NeighborArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    const tds::SliceThread t;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, K = g.K;
    t.stage_items(bx, E, [&](int j) {
        tds::Item it = tds::entity_item(g.boxes, g.sc, g.speed, b * E + j);
        it.hi.w = g.present[b * E + j] ? 1.0f : 0.0f;
        return it;
    });
    t.for_slice(A, [&](int a) {
        const int64_t row = (b * A + a) * K;
        const float4 me = *(const float4 *)(bx + NB_WORDS * a);
        const float4 me2 = *(const float4 *)(bx + NB_WORDS * a + 4);
        const auto store = [&](int k, int e, uint32_t) { store_slot(g, bx, row, k, e, me, me2); };
        if (me2.w == 0.0f) return t.empty_row(K, store);                 // an observer that is not present
        const uint8_t *vis = g.visible ? g.visible + (b * A + a) * E : nullptr;
        t.select_row(bx, E, K, [&](int e) { return key_of(bx, vis, a, e, me.x, me.y, g.r2); }, store);
    });
}

}  // namespace

TDS_EXPORT int tds_neighbors_f32(const float *boxes, const float *sc, const float *speed, const uint8_t *present, const uint8_t *visible,
                                 float *features, int32_t *index, int64_t B, int64_t A, int64_t E, int K, float max_distance, void *stream) {
    const char *what = "tds_neighbors_f32";
    TDS_CHECK_ARG(max_distance >= 0.0f, "%s: max_distance must not be negative or NaN (got %g)", what, (double)max_distance);
    if (int rc = tds::check_frame(what, B, A, E, K, TDS_NEIGHBORS_MAX_K, tds::frame_entities(TDS_NEIGHBORS_MAX_ENTITIES), A); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(boxes && sc && speed && present && features && index, "%s: null pointer", what);
    NeighborArgs g{};
    g.boxes = boxes; g.sc = sc; g.speed = speed; g.present = present; g.visible = visible;
    g.features = features; g.index = index;
    g.A = (int)A; g.E = (int)E; g.K = K;
    g.r2 = max_distance * max_distance;
    hipLaunchKernelGGL(neighbors_kernel, tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(E, true), (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("neighbors_kernel");
    return TDS_OK;
}

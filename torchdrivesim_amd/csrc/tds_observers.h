// The frame of the per-observer top-K kernels: neighbors.hip (K6), the stop lines of lights.hip (K7), ttc.hip (K9) and, for
// its staging and its slice loop, ttc_bwd.hip (K9b).  A workgroup of OBS_BLOCK threads has one scene and a slice of OBS_SLICE of its rows
// (observers; K9b: receiving entities); the scene's n items are staged in LDS once, OBS_WORDS words each; one wave per row, the waves taking the
// rows of the slice in turn; per observer the K smallest keys of tds_select.h, by rank up to 64 items, in rounds over the wave's own key row in
// LDS above.
#pragma once
#include "tds_common.h"
#include "tds_select.h"

namespace tds {

constexpr int OBS_BLOCK = 256;          // 4 waves
constexpr int OBS_WAVES = OBS_BLOCK / 64;
constexpr int OBS_SLICE = 16;           // rows per workgroup: four per wave
constexpr int OBS_WORDS = 8;            // LDS words per item

// dynamic LDS of a launch over n items: the items, and with key rows above 64 items another row of n key words per wave
constexpr size_t lds_bytes(int64_t n, bool with_key_rows) {
    return (size_t)n * OBS_WORDS * sizeof(float) + (with_key_rows && n > 64 ? (size_t)OBS_WAVES * n * sizeof(uint32_t) : 0);
}
static_assert(lds_bytes(TDS_NEIGHBORS_MAX_ENTITIES, true) <= 64 * 1024 && lds_bytes(TDS_TTC_MAX_ENTITIES, true) <= 64 * 1024 &&
              lds_bytes(TDS_LIGHTS_MAX_LIGHTS, true) <= 64 * 1024, "a scene at the limit, with its key rows, fits the 64 KiB a launch gets without asking for more");

inline dim3 slice_grid(int64_t B, int64_t rows) { return dim3((unsigned)B, (unsigned)((rows + OBS_SLICE - 1) / OBS_SLICE)); }

// the items of a frame in the messages (the letter of their number, "<noun> per scene", "the <of> of a scene"), how many a scene may have, and
// whether the observers are the first A of them (A <= n)
struct FrameItems { char letter; const char *noun, *of; int limit; bool observers_among; };
constexpr FrameItems frame_entities(int limit) { return {'E', "entities", "entities", limit, true}; }
constexpr FrameItems frame_stop_lines(int limit) { return {'N', "stop lines", "lines", limit, false}; }

// The rules the entry points share, checked after an entry point's own: the sizes, K in 1 .. max_k, A <= n, the LDS limit, and whether B scenes
// of `rows` rows leave anything to do -> FRAME_LAUNCH, or what the entry point returns: TDS_EINVAL, TDS_ELIMIT, TDS_OK for an empty batch
constexpr int FRAME_LAUNCH = 1;
inline int check_frame(const char *what, int64_t B, int64_t A, int64_t n, int K, int max_k, const FrameItems &items, int64_t rows) {
    TDS_CHECK_ARG(B >= 0 && A >= 0 && n >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld %c=%lld", what, (long long)B, (long long)A, items.letter,
                  (long long)n);
    TDS_CHECK_ARG(K >= 1 && K <= max_k, "%s: K must be 1 .. %d (got %d)", what, max_k, K);
    TDS_CHECK_ARG(!items.observers_among || A <= n, "%s: %lld exposed agents but only %lld %s", what, (long long)A, (long long)n, items.noun);
    if (n > items.limit) {
        tds::set_error("%s: %lld %s per scene (the %s of a scene live in LDS: at most %d)", what, (long long)n, items.noun, items.of, items.limit);
        return TDS_ELIMIT;
    }
    return B > 0 && rows > 0 ? FRAME_LAUNCH : TDS_OK;
}

struct Item { float4 lo, hi; };         // the OBS_WORDS words of an item

// entity i of (boxes, sc, speed) as K6, K9 and K9b stage it: x, y, length, width | sin, cos, speed, and a flag the kernel sets
__device__ __forceinline__ Item entity_item(const float *boxes, const float *sc, const float *speed, int64_t i) {
    const float *p = boxes + i * 5;
    const float2 h = *(const float2 *)(sc + i * 2);
    return {make_float4(p[0], p[1], p[2], p[3]), make_float4(h.x, h.y, speed[i], 0.0f)};
}

// A thread's place in the frame -- its lane and its wave, derived once at the top of the kernel -- and what the frame does from there.  The
// kernel says what differs: how an item is loaded, whether an observer is usable, the key bits of an item (NO_KEY: no candidate) and what
// store(k, item, key) writes to slot k (item -1: an empty slot).
struct SliceThread {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // the whole workgroup: load(j) -> the Item j of the scene, j < n; ends in the barrier
    template <class Load>
    __device__ __forceinline__ void stage_items(float *items, int n, Load load) const {
        for (int j = threadIdx.x; j < n; j += OBS_BLOCK) {
            const Item it = load(j);
            *(float4 *)(items + OBS_WORDS * j) = it.lo;
            *(float4 *)(items + OBS_WORDS * j + 4) = it.hi;
        }
        __syncthreads();
    }

    // the rows of this workgroup's slice, a wave each: body(row).  Wave-uniform: all 64 lanes stay together in the body
    template <class Body>
    __device__ __forceinline__ void for_slice(int rows, Body body) const {
        const int r0 = blockIdx.y * OBS_SLICE, r1 = min(r0 + OBS_SLICE, rows);
        for (int r = r0 + wave; r < r1; r += OBS_WAVES) body(r);
    }

    // the row of an observer that is not usable
    template <class Store>
    __device__ __forceinline__ void empty_row(int K, Store store) const {
        if (lane < K) store(lane, -1, NO_KEY);
    }

    // the row of a usable observer over the n staged items, behind which the waves' key rows lie
    template <class KeyOf, class Store>
    __device__ __forceinline__ void select_row(float *items, int n, int K, KeyOf key_of, Store store) const {
        if (n <= 64) {
            const uint32_t key = lane < n ? key_of(lane) : NO_KEY;
            select_by_rank(key, lane, K, [&](int k, int item) { store(k, item, key); });            // a filled slot is stored by its own lane
        } else {
            uint32_t *wk = (uint32_t *)(items + OBS_WORDS * n) + wave * n;                          // this wave's row of key bits
            // the lane that stores slot k is not the one that computed the winner's key: it computes it again, the same bits
            select_by_rounds(wk, n, lane, K, key_of, [&](int k, int item) { store(k, item, item >= 0 ? key_of(item) : NO_KEY); });
        }
    }
};

}  // namespace tds

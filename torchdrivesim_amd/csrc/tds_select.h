// The K nearest of a scene's items, selected by ONE WAVE: what neighbors.hip (K6), lights.hip (K7, stop lines) and ttc.hip (K9, whose "d2" is a
// time) share, called from the frame of tds_observers.h.  Every candidate has the
// 64-bit key (bits of d2) << 32 | item -- d2 >= +0, so its bits order as an unsigned integer; the keys are unique -- and the K smallest keys are the
// answer, slot 0 the nearest.  An item that is no candidate carries the d2 bits NO_KEY.  Two forms, by the number of items:
//   up to 64    a lane per item; a lane's slot is its RANK, the number of smaller keys, counted over the CANDIDATE lanes' d2 read as wave-uniform
//               values (v_readlane: no LDS traffic, one step per candidate whatever K is); the lane whose rank is below K stores its own slot;
//   above 64    the d2 bits go to the wave's own LDS row, then K rounds of a wave-wide minimum over the keys above the last winner.
// All 64 lanes of the wave must call together.  store(k, item) writes slot k; item -1: an empty slot.  Every slot below K is stored exactly once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tds {

constexpr uint32_t NO_KEY = 0xffffffffu; // the d2 bits of an item that is no candidate (a NaN pattern: no candidate's d2 is a NaN)

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// at most 64 items: `key` is the d2 bits of item `lane` (NO_KEY in the lanes beyond the items)
template <class Store>
__device__ __forceinline__ void select_by_rank(uint32_t key, int lane, int K, Store store) {
    const uint64_t cand = __ballot(key != NO_KEY);
    int rank = 0;
    for (uint64_t m = cand; m != 0; m &= m - 1) {                    // one step per candidate (wave-uniform): only they can be smaller
        const int i = __builtin_ctzll(m);
        const uint32_t ki = __builtin_amdgcn_readlane(key, i);
        rank += (ki < key || (ki == key && i < lane)) ? 1 : 0;
    }
    const int found = __popcll(cand);
    if (key != NO_KEY && rank < K) store(rank, lane);
    if (lane >= found && lane < K) store(lane, -1);
}

// n items, any number: wk is this wave's own row of n LDS words, key_of(item) the d2 bits of an item
template <class KeyOf, class Store>
__device__ __forceinline__ void select_by_rounds(uint32_t *wk, int n, int lane, int K, KeyOf key_of, Store store) {
    for (int e = lane; e < n; e += 64) wk[e] = key_of(e);            // read back by the same lane only
    int mine = -1;
    uint64_t above = 0;                                              // the keys still to be dealt: those >= above
    for (int k = 0; k < K; ++k) {
        uint64_t best = ~(uint64_t)0;
        for (int e = lane; e < n; e += 64) {
            const uint64_t key = ((uint64_t)wk[e] << 32) | (uint32_t)e;
            if (key >= above && key < best) best = key;
        }
        best = wave_min(best);
        if ((uint32_t)(best >> 32) == NO_KEY) break;                 // no candidate is left (wave-uniform)
        if (lane == k) mine = (int)(uint32_t)best;
        above = best + 1;
    }
    if (lane < K) store(lane, mine);
}

}  // namespace tds

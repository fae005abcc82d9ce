// How the actor wave of the persistent scene rasteriser (raster.hip: scan_step, ACTW) deals a round's visible agents to its lanes.  A round is
// 64 consecutive agents: lane j culls agent 64 r + j and a ballot gives `vis`, the set of the visible ones.  Producer step k = 0, 1, ... of the
// round serves the members 21 k .. 21 k + 20 of the set in ascending order, three lanes (one per face) each:
//   lane j, whose bit is set with rank 21 k <= actor_rank(vis, j) < 21 (k + 1), drops j at position rank - 21 k of a 64-word array (the
//   wave's LDS slots);  lane L < 63 serves position L / 3, face L % 3, if the set has a member 21 k + L / 3;  lane 63 serves nothing.
// The round takes another step while the set has members beyond.
// Plain integer arithmetic that a host compiler takes as it is (tests/actor_lanes_host.cpp holds it to a brute-force restatement on the CPU).
// Nothing else belongs here: bench.py's source stamp hashes raster.hip, not this header.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TDS_AL_HD __host__ __device__
#else
#define TDS_AL_HD
#endif

#define TDS_ACTOR_FACES 3               /* faces per agent: [0,1,3], [1,3,2] (body), [4,5,6] (direction) */
#define TDS_ACTOR_STEP_AGENTS 21        /* agents a face step serves: 63 lanes */
#define TDS_ACTOR_ROUND 64              /* agents a cull step looks at */

TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_popcount(uint64_t v) {
    return __builtin_popcountll(v);
}
// members of the set below j
TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_rank(uint64_t vis, int j) {
#ifdef __HIP_DEVICE_COMPILE__
    (void)j;                            // (the calling lane's own index: v_mbcnt)
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(vis >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)vis, 0u));
#else
    return actor_popcount(vis & (((uint64_t)1 << j) - 1u));
#endif
}
// agents of round r among N: lane j of the cull step has an agent iff j < actor_round_agents(N, r)
TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_round_agents(int N, int r) {
    const int left = N - TDS_ACTOR_ROUND * r;
    return left < 0 ? 0 : (left > TDS_ACTOR_ROUND ? TDS_ACTOR_ROUND : left);
}
// where lane j drops its index in step `step` of the round (-1: nowhere -- not in the set, or served by another step)
TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_drop_position(uint64_t vis, int j, int step) {
    const int rel = actor_rank(vis, j) - TDS_ACTOR_STEP_AGENTS * step;
    return ((vis >> j) & 1u) && rel >= 0 && rel < TDS_ACTOR_STEP_AGENTS ? rel : -1;
}
// the position lane `lane` serves in that step (-1: none) and its face
TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_lane_position(uint64_t vis, int lane, int step) {
    const int slot = lane / TDS_ACTOR_FACES;
    return lane < TDS_ACTOR_FACES * TDS_ACTOR_STEP_AGENTS && TDS_ACTOR_STEP_AGENTS * step + slot < actor_popcount(vis) ? slot : -1;
}
TDS_AL_HD __inline__ __attribute__((always_inline)) int actor_lane_face(int lane) { return lane - TDS_ACTOR_FACES * (lane / TDS_ACTOR_FACES); }
// does the round need a step after `step`?
TDS_AL_HD __inline__ __attribute__((always_inline)) bool actor_more_steps(uint64_t vis, int step) {
    return actor_popcount(vis) > TDS_ACTOR_STEP_AGENTS * (step + 1);
}

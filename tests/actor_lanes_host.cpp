// The lane assignment of the rasteriser's actor wave (torchdrivesim_amd/csrc/tds_actor_lanes.h) on the host, against a brute-force restatement:
// the visible agents of a round in ascending order, 21 per producer step, three lanes each.  The steps of a round are run as the kernel runs
// them -- every lane drops, then every lane reads, through an array of 64 words that starts out holding garbage -- and over all of them every
// (visible agent, face) pair must come up on exactly one lane and nothing else on any.
//   actor_lanes_host SAMPLES [BREAK]     BREAK = 1: the restatement deals 20 agents per step, so the comparison must fail (tests the test)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "tds_actor_lanes.h"

static int per_step = TDS_ACTOR_STEP_AGENTS;
static long long n_sets = 0, n_bad = 0;

// one round: `vis` among `lanes` agents (bits at and above `lanes` are never set by the cull: those lanes have no agent)
static void check_round(uint64_t vis, int lanes, int base) {
    if (lanes < 64) vis &= ((uint64_t)1 << lanes) - 1u;
    ++n_sets;
    std::vector<int> members;
    for (int j = 0; j < 64; ++j) if ((vis >> j) & 1u) members.push_back(j);
    int seen[64][3] = {};
    bool bad = false;
    uint32_t slots[64];
    int step = 0;
    for (;; ++step) {
        for (int j = 0; j < 64; ++j) slots[j] = 0xdead0000u + (uint32_t)j;              // what the rasteriser left there
        for (int j = 0; j < 64; ++j) {
            const int d = actor_drop_position(vis, j, step);
            if (d >= TDS_ACTOR_STEP_AGENTS || d < -1) { bad = true; continue; }
            if (d >= 0) {
                if (slots[d] < 64u) bad = true;                                          // two lanes on one position
                slots[d] = (uint32_t)j;
            }
        }
        for (int lane = 0; lane < 64; ++lane) {
            const int p = actor_lane_position(vis, lane, step), f = actor_lane_face(lane);
            const int want = lane < 63 && per_step * step + lane / 3 < (int)members.size() && lane / 3 < per_step ? members[per_step * step + lane / 3] : -1;
            if (p < 0) { if (want >= 0) bad = true; continue; }
            if (p >= TDS_ACTOR_STEP_AGENTS || slots[p] >= 64u || lane == 63) { bad = true; continue; }
            const int ag = (int)slots[p];
            if (ag != want || f != lane % 3 || ag >= lanes || !((vis >> ag) & 1u)) bad = true;
            else ++seen[ag][f];
        }
        const bool more = actor_more_steps(vis, step);
        if (more != ((int)members.size() > per_step * (step + 1))) bad = true;
        if (!more || step > 8) break;
    }
    for (int j = 0; j < 64; ++j)
        for (int f = 0; f < 3; ++f)
            if (seen[j][f] != (((vis >> j) & 1u) ? 1 : 0)) bad = true;
    if (bad) {
        if (n_bad < 5) fprintf(stderr, "lane assignment differs: set %016llx, %d lanes, first agent %d\n", (unsigned long long)vis, lanes, base);
        ++n_bad;
    }
}

static uint64_t low_bits(int n) { return n >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << n) - 1u; }

int main(int argc, char **argv) {
    const long long samples = argc > 1 ? atoll(argv[1]) : 300000;
    if (argc > 2 && atoi(argv[2]) == 1) per_step = 20;
    const int counts[] = {1, 3, 63, 64, 65, 128, 130};
    const int bits[] = {0, 1, 2, 20, 21, 22, 42, 43, 63, 64};
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int N : counts) {
        for (int r = 0; TDS_ACTOR_ROUND * r < N; ++r) {
            const int lanes = actor_round_agents(N, r), base = TDS_ACTOR_ROUND * r;
            if (lanes != (N - base < 64 ? N - base : 64)) { fprintf(stderr, "round size differs: N %d round %d\n", N, r); ++n_bad; }
            for (int n : bits) {
                // n members: the lowest, the highest, spread evenly, every other one from the bottom, and around bit 21 / 42 / 63
                const uint64_t low = low_bits(n), high = n == 0 ? 0 : ~low_bits(64 - n);
                uint64_t spread = 0, alt = 0;
                for (int i = 0; i < n; ++i) spread |= (uint64_t)1 << (n <= 1 ? 63 * i : (63 * i) / (n - 1));
                for (int i = 0; i < n && 2 * i < 64; ++i) alt |= (uint64_t)1 << (2 * i);
                const uint64_t pats[] = {low, high, spread, alt, (low << 1) | (n ? 1u : 0u), low << (n <= 43 ? 21 : 0), high >> 1};
                for (uint64_t p : pats) check_round(p, lanes, base);
            }
            for (long long i = 0; i < samples / 8; ++i) {
                uint64_t v = next();
                const int thin = (int)(i & 3);                                           // dense, and thinned to a half, a quarter, an eighth
                for (int t = 0; t < thin; ++t) v &= next();
                check_round(v, lanes, base);
            }
        }
    }
    if (actor_round_agents(64, 1) != 0 || actor_round_agents(130, 2) != 2 || actor_round_agents(130, 3) != 0) { fprintf(stderr, "round size differs\n"); ++n_bad; }
    printf("actor lanes %lld sets, %lld differ\n", n_sets, n_bad);
    return n_bad ? 1 : 0;
}

// The arithmetic of a traffic-light programme's clock (lights.hip; include/tdship.h "K7"): TrafficLightStateMachine.tick of traffic_lights.py
// over the device tables, operation for operation -- float64 + - and comparisons only, so the host class reproduces it bit for bit.  Nothing of
// HIP in here: a host compiler takes this file as it is, and tests/lights_host.cpp replays the reference's recorded trace through it.
#pragma once
#include <stdint.h>

#include "tds_lane_math.h"

#define TDS_LIGHTS_MAX_SKIPS_ 1024     // TDS_LIGHTS_MAX_SKIPS of include/tdship.h (lights.hip holds the two equal)

namespace tds {

struct LightClock {
    int phase;          // LIST POSITION of the current phase in its machine
    double remaining;   // seconds left in it
};

TDS_HD inline int lights_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// One machine advanced by dt.  duration / next_phase: the machine's rows of the tables (n phases, 1 <= n); every index read from them is
// clamped to the machine, and the walk ends after TDS_LIGHTS_MAX_SKIPS phases whatever the tables hold.
TDS_HD inline LightClock lights_tick(const double *duration, const int32_t *next_phase, int n, LightClock s, double dt) {
    double left = s.remaining - dt;
    if (left > 0) {
        s.remaining = left;
        return s;
    }
    int p = lights_clamp(s.phase, n), nxt = p;
    double span = 0.0;
    for (int i = 0; i < TDS_LIGHTS_MAX_SKIPS_; ++i) {
        nxt = lights_clamp(next_phase[p], n);
        span = duration[nxt];
        if (left == 0) return LightClock{nxt, span};            // the phase ended exactly now: the next one starts in full
        left += span;
        if (left > 0) return LightClock{nxt, left <= span ? left : span};   // the overshoot ends inside the next phase
        p = nxt;                                                // the overshoot swallows the whole next phase
    }
    return LightClock{nxt, span};
}

// the phase a reset deals machine m of the scene with this id: the first word of Philox4x32-10 scaled to the machine's n phases
TDS_HD inline int lights_reset_phase(uint64_t seed, uint64_t scene_id, int m, int n) {
    const U4 r = philox4x32_10(U4{(uint32_t)scene_id, (uint32_t)(scene_id >> 32), (uint32_t)m, 0u},
                               (uint32_t)seed ^ 0x4C494748u, (uint32_t)(seed >> 32) ^ 0x54535452u);
    return pick_of(r.x, n);
}

}  // namespace tds

// The 5-disc overlap of two oriented boxes, shared by K2a (collision.hip) and the on-lane spawn kernel (spawn.hip): ONE definition of the
// arithmetic that is held bit-exact against the reference's recorded values (tests/golden G2, G13).
#pragma once
#include "tds_common.h"

namespace tds {

struct Box { float x, y, l, w; float s, c; };

// bbox2discs + cdist + relu, infractions.py:378-426,503-545.  b.s/b.c are of yaw + pi/2*(wid>len).
__device__ inline float discs_pair(const Box &b1, const Box &b2) {
    float ra = fminf(b1.l, b1.w) / 2.0f, rb = fminf(b2.l, b2.w) / 2.0f;
    float ha = fmaxf(b1.l, b1.w) / 2.0f - ra, hb = fmaxf(b2.l, b2.w) / 2.0f - rb;
    float d = __builtin_inff();
    bool any_nan = false;
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
        float da = ((float)i * ha) / 2.0f;
        float ax = (da * b1.c - 0.0f * b1.s) + b1.x, ay = (da * b1.s + 0.0f * b1.c) + b1.y;
#pragma unroll
        for (int j = -2; j <= 2; ++j) {
            float db = ((float)j * hb) / 2.0f;
            float bx = (db * b2.c - 0.0f * b2.s) + b2.x, by = (db * b2.s + 0.0f * b2.c) + b2.y;
            float ex = ax - bx, ey = ay - by;
            float dd = sqrtf(__fmaf_rn(ey, ey, ex * ex));    // torch.cdist accumulates with an FMA (probed)
            any_nan |= (dd != dd);
            d = fminf(d, dd);
        }
    }
    if (any_nan) d = __builtin_nanf("");
    float l = 1.0f - d / (ra + rb);
    return (l != l) ? l : fmaxf(l, 0.0f);
}

}  // namespace tds

// The gradient of the stop-line observations (stop_lines_bwd.hip; include/tdship.h "K7b"): what the incoming gradients of one
// filled slot contribute to x, y, sin, cos of its observer, and the order in which an observer's K slots are added.
// Nothing of HIP in here: a host compiler takes this file as it is, and tests/stop_lines_grad_host.cpp holds both functions to their numpy
// restatement (tests/test_stop_lines_grad_host.py) bit for bit.  Float64, + - * / sqrt only, every operation rounded once, in the order written
// here.  Which line is in the slot is a constant of differentiation; [sin, cos] are independent inputs; the line gets nothing.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef TDS_HD
#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif
#endif

namespace tds {

// the order of an observer's four gradients
enum { SLG_X = 0, SLG_Y, SLG_SIN, SLG_COS, SLG_GRADS };

// lanes that share an observer's K slots: lane l has the slots l, l + SLG_ROW_LANES, ... of the row, in that order
constexpr int SLG_ROW_LANES = 4;

// observer (xa, ya, s, c), line (xn, yn, sl, cl), the float32 values widened exactly; g0 .. g3 and g7 the incoming gradient of the slot's x, y,
// sin_rel, cos_rel and distance (K7's order; length, width and time_to_change are copies of constants: g4 .. g6 are not read) -> out[4]
TDS_HD inline void stop_lines_slot_grad(double xa, double ya, double s, double c, double xn, double yn, double sl, double cl, double g0, double g1,
                                        double g2, double g3, double g7, double *out) {
    const double dx = xn - xa, dy = yn - ya;
    const double r = sqrt(dx * dx + dy * dy);                  // recomputed in binary64: not the forward's rounded distance
    const double q = r == 0.0 ? 0.0 : g7 / r;                  // an observer exactly on the line's centre: the distance contributes 0, not NaN
    out[SLG_X] = -(g0 * c - g1 * s) - q * dx;
    out[SLG_Y] = -(g0 * s + g1 * c) - q * dy;
    out[SLG_SIN] = ((g0 * dy - g1 * dx) - g2 * cl) + g3 * sl;
    out[SLG_COS] = ((g0 * dx + g1 * dy) + g2 * sl) + g3 * cl;
}

// Slot k of a row is FILLED iff 0 <= index[k] < N; nothing is read at any other index, and what comes in at such a slot is not read either.
TDS_HD inline bool stop_lines_slot_filled(int32_t n, int N) { return n >= 0 && n < N; }

// The sum of a row as the kernel forms it, on one thread: lane l starts from +0 and adds its filled slots l, l + LANES, ... in that order; then
// log2(LANES) rounds m = LANES / 2, ..., 1 in which lane l takes (its sum) + (the sum of lane l ^ m); lane 0 holds the result.  lines: the
// scene's N x 5 rows, line_sc its N x 2; index and g_features the row's K and K x 8.
template <int LANES = SLG_ROW_LANES>
inline void stop_lines_row_grad(const float *agent_xy, const float *agent_sc, const float *lines, const float *line_sc, const int32_t *index,
                                const float *g_features, int N, int K, double *out) {
    double sum[LANES][SLG_GRADS];
    for (int l = 0; l < LANES; ++l) {
        for (int i = 0; i < SLG_GRADS; ++i) sum[l][i] = 0.0;
        for (int k = l; k < K; k += LANES) {
            const int32_t n = index[k];
            if (!stop_lines_slot_filled(n, N)) continue;
            const float *g = g_features + 8 * k;
            double d[SLG_GRADS];
            stop_lines_slot_grad(agent_xy[0], agent_xy[1], agent_sc[0], agent_sc[1], lines[5 * n], lines[5 * n + 1], line_sc[2 * n], line_sc[2 * n + 1],
                                 g[0], g[1], g[2], g[3], g[7], d);
            for (int i = 0; i < SLG_GRADS; ++i) sum[l][i] = sum[l][i] + d[i];
        }
    }
    for (int m = LANES / 2; m > 0; m >>= 1) {
        double next[LANES][SLG_GRADS];
        for (int l = 0; l < LANES; ++l)
            for (int i = 0; i < SLG_GRADS; ++i) next[l][i] = sum[l][i] + sum[l ^ m][i];
        for (int l = 0; l < LANES; ++l)
            for (int i = 0; i < SLG_GRADS; ++i) sum[l][i] = next[l][i];
    }
    for (int i = 0; i < SLG_GRADS; ++i) out[i] = sum[0][i];
}

}  // namespace tds

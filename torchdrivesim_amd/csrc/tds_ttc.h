// The pair test of time to collision (ttc.hip; include/tdship.h "K9"): the first time at which two rectangles that keep their
// velocity and heading touch, by the separating axes of the two boxes, each axis giving the interval of times in which the projections overlap.
// Nothing of HIP in here: a host compiler takes this file as it is, and tests/ttc_host.cpp holds this function to the float64 model
// (tests/ttc_model.py) on the CPU.  Float64, + - * / fabs and comparisons only, every operation rounded once, one rounding to float32 at the end.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif

namespace tds {

// one rectangle: centre, HALF extents along and across its heading (the observer's already hold the margin), [sin, cos] of the heading, speed
struct TtcBox { double x, y, hl, hw, s, c, v; };

// a float32 input that is a number: neither a NaN nor an infinity
TDS_HD inline bool ttc_finite(float v) { return fabsf(v) <= 3.40282346638528859812e38f; }
// ... all seven values of an entity: only such an entity observes, is a candidate (K9) or takes part in a pair's gradient (K9b)
TDS_HD inline bool ttc_finite(float x, float y, float length, float width, float s, float c, float v) {
    return ttc_finite(x) && ttc_finite(y) && ttc_finite(length) && ttc_finite(width) && ttc_finite(s) && ttc_finite(c) && ttc_finite(v);
}

// the seven float32 values of an entity, widened exactly; margin grows the box on every side (the observer's; 0 for the other entity)
TDS_HD inline TtcBox ttc_box(float x, float y, float length, float width, float s, float c, float v, double margin) {
    TtcBox q;
    q.x = (double)x; q.y = (double)y;
    q.hl = 0.5 * (double)length + margin; q.hw = 0.5 * (double)width + margin;
    q.s = (double)s; q.c = (double)c; q.v = (double)v;
    return q;
}

// one axis (nx, ny): narrows [lo, hi] to the times at which the projections overlap; false: they never do
TDS_HD inline bool ttc_axis(const TtcBox &a, const TtcBox &e, double dx, double dy, double rvx, double rvy, double nx, double ny, double &lo, double &hi) {
    const double p = dx * nx + dy * ny;
    const double w = rvx * nx + rvy * ny;
    const double R = a.hl * fabs(a.c * nx + a.s * ny) + a.hw * fabs(a.c * ny - a.s * nx) + e.hl * fabs(e.c * nx + e.s * ny) + e.hw * fabs(e.c * ny - e.s * nx);
    if (w == 0.0) return !(fabs(p) > R);
    double t0 = (-R - p) / w, t1 = (R - p) / w;
    if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
    if (t0 > lo) lo = t0;
    if (t1 < hi) hi = t1;
    return true;
}

// observer a against entity e, all values finite: whether they touch within the horizon, and when (never -0.0, never a NaN)
TDS_HD inline bool ttc_pair(const TtcBox &a, const TtcBox &e, double horizon, float *ttc) {
    const double dx = e.x - a.x, dy = e.y - a.y;
    const double rvx = e.v * e.c - a.v * a.c, rvy = e.v * e.s - a.v * a.s;
    double lo = -INFINITY, hi = INFINITY;
    if (!ttc_axis(a, e, dx, dy, rvx, rvy, a.c, a.s, lo, hi)) return false;
    if (!ttc_axis(a, e, dx, dy, rvx, rvy, -a.s, a.c, lo, hi)) return false;
    if (!ttc_axis(a, e, dx, dy, rvx, rvy, e.c, e.s, lo, hi)) return false;
    if (!ttc_axis(a, e, dx, dy, rvx, rvy, -e.s, e.c, lo, hi)) return false;
    if (!(lo <= hi && hi >= 0.0 && lo <= horizon)) return false;
    *ttc = (float)(lo > 0.0 ? lo : 0.0);
    return true;
}

}  // namespace tds

// The lane-graph arithmetic every lane kernel shares (lanes.hip, spawn.hip, follow.hip, route.hip, lane_obs.hip): the random stream, the search
// on a centre line's cumulative lengths, the foot of a pose on a segment, the point at an arc length.  Nothing of HIP in here: a host compiler
// takes this file as it is, and tests/lane_math_host.cpp and tests/lane_foot_host.cpp hold these functions to the float64 models on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif

namespace tds {

struct U4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's known answers: tests/test_spawn_model.py)
TDS_HD inline U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        U4 n;
        n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
        n.y = (uint32_t)p1;
        n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
        n.w = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// a 32-bit random word scaled to [0, n): floor(word * n / 2^32)
TDS_HD inline int pick_of(uint32_t word, int n) { return (int)(((uint64_t)word * (uint64_t)(uint32_t)n) >> 32); }

// the segment of a centre line of n points that holds arc length s: clip(searchsorted(cum, s, 'right') - 1, 0, n - 2); segment 0 for a NaN
TDS_HD inline int segment_of(const double *cum, int n, double s) {
    int lo = 0, hi = n;                                  // first index with cum > s
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (cum[mid] <= s) lo = mid + 1; else hi = mid;
    }
    int k = lo - 1;
    if (k < 0) k = 0;
    if (k > n - 2) k = n - 2;
    return k;
}

// the foot of (x, y) on segment i of a centre line in 2-D, what tds_lane_snap and K8 (lane_obs.hip) rank a lanelet's segments by: u = the
// foot's parameter clamped to [0, 1] (0 on a segment without length, and for a NaN), (fx, fy) = foot - pose, d2 = its squared length.  (ax, ay) is
// the segment's first point, (dx, dy) the segment, l2 = dx*dx + dy*dy.  tests/lane_foot_host.cpp holds it to tests/lane_obs_model.py bit for bit.
struct SegmentFoot { double ax, ay, dx, dy, l2, u, fx, fy, d2; };
TDS_HD inline SegmentFoot segment_foot(const double *cl, int i, double x, double y) {
    SegmentFoot f;
    f.ax = cl[3 * i], f.ay = cl[3 * i + 1], f.dx = cl[3 * i + 3] - f.ax, f.dy = cl[3 * i + 4] - f.ay;
    f.l2 = f.dx * f.dx + f.dy * f.dy;
    double u = f.l2 > 0 ? ((x - f.ax) * f.dx + (y - f.ay) * f.dy) / f.l2 : 0.0;
    f.u = fmin(fmax(u, 0.0), 1.0);
    f.fx = f.ax + f.u * f.dx - x, f.fy = f.ay + f.u * f.dy - y;
    f.d2 = f.fx * f.fx + f.fy * f.fy;
    return f;
}

// what a foot says of the pose against its lanelet: the segment's unit vector ((0, 0) without length), the foot's arc length on `cum` (the
// lanelet's own cumulative lengths, cum[i] at the segment's first point), the pose's signed offset from the segment, left positive
struct Unit2 { double x, y; };
TDS_HD inline Unit2 segment_unit(const SegmentFoot &f) {
    const double len = sqrt(f.l2);
    Unit2 t;
    t.x = len > 0 ? f.dx / len : 0.0, t.y = len > 0 ? f.dy / len : 0.0;
    return t;
}
TDS_HD inline double foot_arc(const SegmentFoot &f, const double *cum, int i) { return cum[i] + f.u * (cum[i + 1] - cum[i]); }
TDS_HD inline double foot_lateral(const SegmentFoot &f, Unit2 t, double x, double y) { return t.x * (y - f.ay) - t.y * (x - f.ax); }

// the point at arc length s on segment k of a centre line (lanelet2.py:183-208 as torchdrivesim_amd/lanelet2.py restates it
// [UNVERIFIED-UPSTREAM]): t = (s - cum[k]) / seg (0 on a segment of length 0), p = c[k] + t (c[k + 1] - c[k]), with (dx, dy) = the segment in 2-D.
// seg is the segment's own 3-D length as the host summed it, sqrt((dx*dx + dy*dy) + dz*dz): cum[k + 1] - cum[k] is NOT that number bit for bit.
struct ArcPoint { double x, y, dx, dy, t; };
TDS_HD inline ArcPoint point_at_arc(const double *cl, const double *cum, int k, double s) {
    const double *a = cl + 3 * k;
    ArcPoint p;
    p.dx = a[3] - a[0], p.dy = a[4] - a[1];
    const double dz = a[5] - a[2];
    const double seg = sqrt((p.dx * p.dx + p.dy * p.dy) + dz * dz);
    p.t = seg > 0.0 ? (s - cum[k]) / seg : 0.0;
    p.x = a[0] + p.t * p.dx, p.y = a[1] + p.t * p.dy;
    return p;
}

}  // namespace tds

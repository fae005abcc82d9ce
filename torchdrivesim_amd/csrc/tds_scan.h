// The per-ray arithmetic of the range scans that the forward (scan.hip, K5) and the backward (scan_bwd.hip, K5b) must do alike, bit for bit: where
// a line meets a triangle, the slab test of a ray against a rectangle, which grid cells a stretch of a ray can touch, which faces count as road.
// Nothing of HIP in here: a host compiler takes this file as it is (tests/scan_grad_host.cpp).  Binary32 + - * / in the order written here, every
// operation rounded once (-ffp-contract=off); only the "positive area" test is float64.
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

// The parameter interval in which the line o + t d (|d| = 1) meets the closed triangle, from the vertices RELATIVE to o:
// u = p . d (along the ray), w = d x p (signed distance from the line).  An edge whose end points lie on different sides (or on the line)
// crosses at u_i + (u_j - u_i) * w_i / (w_i - w_j).  false: the line misses the triangle.
TDS_HD inline bool edge_crossing(float wi, float wj, float ui, float uj, float &u) {
    if (wi != wj && fminf(wi, wj) <= 0.0f && fmaxf(wi, wj) >= 0.0f) {
        u = ui + (uj - ui) * (wi / (wi - wj));
        return true;
    }
    return false;
}

TDS_HD inline bool line_triangle(float dx, float dy, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y, float &lo, float &hi) {
    const float w0 = dx * p0y - dy * p0x, w1 = dx * p1y - dy * p1x, w2 = dx * p2y - dy * p2x;
    if ((w0 > 0.0f && w1 > 0.0f && w2 > 0.0f) || (w0 < 0.0f && w1 < 0.0f && w2 < 0.0f)) return false;
    const float u0 = dx * p0x + dy * p0y, u1 = dx * p1x + dy * p1y, u2 = dx * p2x + dy * p2y;
    lo = __builtin_inff(); hi = -__builtin_inff();
    float u;
    if (edge_crossing(w0, w1, u0, u1, u)) { lo = fminf(lo, u); hi = fmaxf(hi, u); }
    if (edge_crossing(w1, w2, u1, u2, u)) { lo = fminf(lo, u); hi = fmaxf(hi, u); }
    if (edge_crossing(w2, w0, u2, u0, u)) { lo = fminf(lo, u); hi = fmaxf(hi, u); }
    return lo <= hi;
}

// faces without area are no road (padding faces [0,0,0], slivers): float64 on the float32 vertices, as the model evaluates it
TDS_HD inline bool positive_area(float x0, float y0, float x1, float y1, float x2, float y2) {
    const double area2 = ((double)x1 - (double)x0) * ((double)y2 - (double)y0) - ((double)x2 - (double)x0) * ((double)y1 - (double)y0);
    return area2 != 0.0;
}

// The slab test of a ray against a rectangle, in the rectangle's frame: origin (lx, ly) relative to its centre, direction (ex, ey), half sizes
// (hl, hw).  true: the ray's line meets the rectangle at t0 <= t1 with t0 >= 0 where it enters (0 from inside).  `slab` says which term of
// t0 = max(0, x entry, y entry) binds, in that order: 0 nothing (t0 = 0), 1 the x slab, 2 the y slab (it must EXCEED max(0, x entry));
// a parallel slab (e == 0) never binds.
TDS_HD inline bool slab_test(float lx, float ly, float ex, float ey, float hl, float hw, float &t0, int &slab) {
    t0 = 0.0f;
    float t1 = __builtin_inff();
    bool ok = true;
    slab = 0;
    if (ex == 0.0f) ok = ok && fabsf(lx) <= hl;
    else {
        const float u = (-hl - lx) / ex, v = (hl - lx) / ex;
        const float in = fminf(u, v);
        if (in > 0.0f) slab = 1;
        t0 = fmaxf(t0, in); t1 = fminf(t1, fmaxf(u, v));
    }
    if (ey == 0.0f) ok = ok && fabsf(ly) <= hw;
    else {
        const float u = (-hw - ly) / ey, v = (hw - ly) / ey;
        const float in = fminf(u, v);
        if (in > t0) slab = 2;
        t0 = fmaxf(t0, in); t1 = fminf(t1, fmaxf(u, v));
    }
    return ok && t0 <= t1;
}

// the ONE definition of "which cell does this coordinate fall in" is tds::cell_coord (tds_common.h); a file that stands alone restates it
TDS_HD inline int scan_cell_coord(float v, float origin, float inv_cell) { return (int)floorf((v - origin) * inv_cell); }

// which cells of one axis can hold a face that meets the ray between two of its points v0, v1 (coordinates on that axis): the cells of the two,
// widened by `marg` metres (binary32 rounding of the points; a point on a cell border is looked up in both neighbours).  The cell rule is
// monotone, so a face whose bounding box holds a point of that stretch is listed in one of these cells.  Coordinates are clamped to one cell
// around the grid first (non-finite values included) and the cells to the grid: a superset of lists is harmless, every face is tested exactly.
TDS_HD inline void cells_of(float cell, float inv_cell, float v0, float v1, float marg, float origin, int n, int &c0, int &c1) {
    const float lo_lim = origin - cell, hi_lim = origin + (float)(n + 1) * cell;
    const float lo = fminf(fmaxf(fminf(v0, v1) - marg, lo_lim), hi_lim), hi = fminf(fmaxf(fmaxf(v0, v1) + marg, lo_lim), hi_lim);
    const int a = scan_cell_coord(lo, origin, inv_cell), b = scan_cell_coord(hi, origin, inv_cell);
    c0 = a < 0 ? 0 : (a > n - 1 ? n - 1 : a);
    c1 = b < c0 ? c0 : (b > n - 1 ? n - 1 : b);
}

// the margin of cells_of for a ray from (ox, oy) of at most max_range metres
TDS_HD inline float scan_margin(float ox, float oy, float max_range) { return 0.004f + 1e-6f * (fabsf(ox) + fabsf(oy) + max_range); }

}  // namespace tds

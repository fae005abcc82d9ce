// The per-ray derivatives of the range scans (scan_bwd.hip; include/tdship.h "K5b"): d agent_range of the slab that binds and
// d road_range of the edge the road stretch ends on, and the rule that names that edge.  Nothing of HIP in here: a host compiler takes this file
// as it is, and tests/scan_grad_host.cpp holds it to its numpy restatement (tests/test_scan_grad_host.py) bit for bit.
// The choices (which edge) are binary32, made with the forward's own functions (tds_scan.h); the derivatives are binary64 on the widened float32
// inputs, + - * / only, every operation rounded once, in the order written here.
#pragma once
#include "tds_scan.h"

namespace tds {

// ---- agent part: t = (sigma h - l) / e of the binding slab ----------------------------------------------------------------------------------
// the order of the ten derivatives: the observer's x, y; the entity's x, y, length, width, sin, cos; the ray's dx, dy
enum { SG_OX = 0, SG_OY, SG_EX, SG_EY, SG_LENGTH, SG_WIDTH, SG_SIN, SG_COS, SG_DX, SG_DY, SG_AGENT };

// slab 1 (x: l = rx c + ry s, e = dx c + dy s, h = hl) or 2 (y: l = ry c - rx s, e = dy c - dx s, h = hw); (ox, oy) the ray's origin, (cx, cy)
// the rectangle's centre, hl / hw its HALF sizes as the forward staged them, (s, c) its [sin, cos], (dx, dy) the ray.  e != 0 in a binding slab.
TDS_HD inline void scan_agent_grad(int slab, float ox, float oy, float cx, float cy, float hl, float hw, float s_, float c_, float dx_, float dy_,
                                   double *g) {
    const double rx = (double)ox - (double)cx, ry = (double)oy - (double)cy;
    const double s = (double)s_, c = (double)c_, dx = (double)dx_, dy = (double)dy_;
    const bool xs = slab == 1;
    const double l = xs ? rx * c + ry * s : ry * c - rx * s;
    const double e = xs ? dx * c + dy * s : dy * c - dx * s;
    const double h = xs ? (double)hl : (double)hw;
    const float e32 = xs ? dx_ * c_ + dy_ * s_ : dy_ * c_ - dx_ * s_;        // the forward's e: the entry side is a choice, made in binary32
    const double sigma = e32 > 0.0f ? -1.0 : 1.0;                            // -sign(e)
    const double t = (sigma * h - l) / e;
    const double tl = -1.0 / e, th = sigma / e, te = -t / e;                 // d t / d l, / d h, / d e
    // d l / d (rx, ry, s, c) and d e / d (dx, dy, s, c)
    const double l_rx = xs ? c : -s, l_ry = xs ? s : c, l_s = xs ? ry : -rx, l_c = xs ? rx : ry;
    const double e_dx = xs ? c : -s, e_dy = xs ? s : c, e_s = xs ? dy : -dx, e_c = xs ? dx : dy;
    g[SG_OX] = tl * l_rx, g[SG_OY] = tl * l_ry;
    g[SG_EX] = -(tl * l_rx), g[SG_EY] = -(tl * l_ry);
    g[SG_LENGTH] = xs ? th * 0.5 : 0.0, g[SG_WIDTH] = xs ? 0.0 : th * 0.5;
    g[SG_SIN] = tl * l_s + te * e_s, g[SG_COS] = tl * l_c + te * e_c;
    g[SG_DX] = te * e_dx, g[SG_DY] = te * e_dy;
}

// ---- road part: t = u_i + (u_j - u_i) w_i / (w_i - w_j) of the edge i -> j ------------------------------------------------------------------
// the edge a road stretch of length F ends on: the smallest (x_i, y_i, x_j, y_j), every edge oriented so that (x_i, y_i) <= (x_j, y_j)
// lexicographically, among the edges whose crossing equals F of the positive-area faces whose far end equals F -- an order that does not depend
// on the grid or on the order of its lists
struct RoadEdge {
    float xi, yi, xj, yj;
    bool found;
};

TDS_HD inline void road_edge_offer(RoadEdge &best, float ax, float ay, float bx, float by) {
    if (bx < ax || (bx == ax && by < ay)) { const float tx = ax, ty = ay; ax = bx; ay = by; bx = tx; by = ty; }
    const bool less = !best.found || ax < best.xi || (ax == best.xi && (ay < best.yi || (ay == best.yi && (bx < best.xj || (bx == best.xj && by < best.yj)))));
    if (less) { best.xi = ax; best.yi = ay; best.xj = bx; best.yj = by; best.found = true; }
}

// one face (world coordinates) of the lists around the end of the stretch, weighed with the forward's own arithmetic
TDS_HD inline void road_edge_of_face(RoadEdge &best, float ox, float oy, float dx, float dy, float F, float x0, float y0, float x1, float y1, float x2,
                                     float y2) {
    const float p0x = x0 - ox, p0y = y0 - oy, p1x = x1 - ox, p1y = y1 - oy, p2x = x2 - ox, p2y = y2 - oy;
    float lo, hi;
    if (!line_triangle(dx, dy, p0x, p0y, p1x, p1y, p2x, p2y, lo, hi)) return;
    if (!(hi == F) || !positive_area(x0, y0, x1, y1, x2, y2)) return;
    const float w0 = dx * p0y - dy * p0x, w1 = dx * p1y - dy * p1x, w2 = dx * p2y - dy * p2x;
    const float u0 = dx * p0x + dy * p0y, u1 = dx * p1x + dy * p1y, u2 = dx * p2x + dy * p2y;
    float u;
    if (edge_crossing(w0, w1, u0, u1, u) && u == F) road_edge_offer(best, x0, y0, x1, y1);
    if (edge_crossing(w1, w2, u1, u2, u) && u == F) road_edge_offer(best, x1, y1, x2, y2);
    if (edge_crossing(w2, w0, u2, u0, u) && u == F) road_edge_offer(best, x2, y2, x0, y0);
}

// the order of the four derivatives of the road part: the observer's x, y, the ray's dx, dy
enum { SR_OX = 0, SR_OY, SR_DX, SR_DY, SR_ROAD };

TDS_HD inline void scan_road_grad(float ox, float oy, float dx_, float dy_, const RoadEdge &ed, double *g) {
    const double dx = (double)dx_, dy = (double)dy_;
    const double pix = (double)ed.xi - (double)ox, piy = (double)ed.yi - (double)oy, pjx = (double)ed.xj - (double)ox, pjy = (double)ed.yj - (double)oy;
    const double ui = dx * pix + dy * piy, uj = dx * pjx + dy * pjy;
    const double wi = dx * piy - dy * pix, wj = dx * pjy - dy * pjx;
    const double D = wi - wj, du = uj - ui;
    const double lam = wi / D, q = du / D;                                   // q = d t / d w_i + d t / d w_j
    const double twi = -(q * wj) / D, twj = (q * wi) / D;                    // d t / d w_i, d t / d w_j
    g[SR_OX] = dy * q - dx;
    g[SR_OY] = -(dx * q) - dy;
    g[SR_DX] = ((pix + lam * (pjx - pix)) + twi * piy) + twj * pjy;
    g[SR_DY] = ((piy + lam * (pjy - piy)) - twi * pix) - twj * pjx;
}

}  // namespace tds

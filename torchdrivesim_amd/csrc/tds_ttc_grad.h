// The pair gradient of time to collision (ttc_bwd.hip; include/tdship.h "K9b"): whether a pair contributes, and the 14 partial
// derivatives of its time -- x, y, length, width, sin, cos, speed of the observer and of the other entity.  Nothing of HIP in here: a host compiler
// takes this file as it is, and tests/ttc_grad_host.cpp holds this function to its numpy restatement (tests/ttc_grad_model.py) bit for bit.
// Float64, + - * / fabs and comparisons only, every operation rounded once, in the order written here.  The discrete choices of the forward --
// the binding axis, the sign of w on it, the signs of the four fabs arguments of R -- are constants of differentiation.
#pragma once
#include "tds_ttc.h"

namespace tds {

// the order of the seven partials of a box
enum { TTC_GX = 0, TTC_GY, TTC_GLENGTH, TTC_GWIDTH, TTC_GSIN, TTC_GCOS, TTC_GSPEED, TTC_GRADS };

// -1, 0 or 1; sign(0) = 0
TDS_HD inline double ttc_sign(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// axis i of the pair, in K9's order
TDS_HD inline void ttc_axis_of(const TtcBox &a, const TtcBox &e, int i, double &nx, double &ny) {
    nx = i == 0 ? a.c : i == 1 ? -a.s : i == 2 ? e.c : -e.s;
    ny = i == 0 ? a.s : i == 1 ? a.c : i == 2 ? e.s : e.c;
}

// observer a (its half extents already hold the margin) against entity e, all values finite.  lo is K9's, by ttc_axis's expressions: the largest
// t0 of the axes with w != 0, the FIRST such axis on ties (the forward's strict t0 > lo).  false unless lo > 0: the pair contributes nothing.
// Else ga[7], ge[7] = d lo / d (x, y, length, width, sin, cos, speed) of a and of e.  With n the binding axis, w = rv.n, sigma = sign(w),
// t = lo = (-sigma R - p) / w, so with N = sigma R + p + t w:  d lo = -dN / w at constant t; the partials are those of N times inv = -1 / w.
TDS_HD inline bool ttc_pair_grad(const TtcBox &a, const TtcBox &e, double *ga, double *ge) {
    const double dx = e.x - a.x, dy = e.y - a.y;
    const double rvx = e.v * e.c - a.v * a.c, rvy = e.v * e.s - a.v * a.s;
    double lo = -INFINITY, wb = 0.0;
    int axis = 0;
    for (int i = 0; i < 4; ++i) {
        double nx, ny;
        ttc_axis_of(a, e, i, nx, ny);
        const double p = dx * nx + dy * ny;
        const double w = rvx * nx + rvy * ny;
        const double R = a.hl * fabs(a.c * nx + a.s * ny) + a.hw * fabs(a.c * ny - a.s * nx) + e.hl * fabs(e.c * nx + e.s * ny) + e.hw * fabs(e.c * ny - e.s * nx);
        if (w == 0.0) continue;
        double t0 = (-R - p) / w;
        const double t1 = (R - p) / w;
        if (t0 > t1) t0 = t1;
        if (t0 > lo) lo = t0, wb = w, axis = i;
    }
    if (!(lo > 0.0)) return false;
    double nx, ny;
    ttc_axis_of(a, e, axis, nx, ny);
    const double t = lo, sigma = ttc_sign(wb), inv = -1.0 / wb;
    const double a1 = a.c * nx + a.s * ny, a2 = a.c * ny - a.s * nx;          // the four fabs arguments of R
    const double e1 = e.c * nx + e.s * ny, e2 = e.c * ny - e.s * nx;
    const double ka1 = sigma * (a.hl * ttc_sign(a1)), ka2 = sigma * (a.hw * ttc_sign(a2));
    const double ke1 = sigma * (e.hl * ttc_sign(e1)), ke2 = sigma * (e.hw * ttc_sign(e2));
    const double qx = dx + t * rvx, qy = dy + t * rvy;                        // the relative position at contact
    const double gnx = ((ka1 * a.c - ka2 * a.s) + (ke1 * e.c - ke2 * e.s)) + qx;      // dN / d(nx, ny)
    const double gny = ((ka1 * a.s + ka2 * a.c) + (ke1 * e.s + ke2 * e.c)) + qy;
    double nca = (ka1 * nx + ka2 * ny) - t * (a.v * nx);                      // dN / d(cos, sin) of a and of e at a constant axis
    double nsa = (ka1 * ny - ka2 * nx) - t * (a.v * ny);
    double nce = (ke1 * nx + ke2 * ny) + t * (e.v * nx);
    double nse = (ke1 * ny - ke2 * nx) + t * (e.v * ny);
    if (axis == 0) nca = nca + gnx, nsa = nsa + gny;                          // n = (c_a, s_a)
    else if (axis == 1) nsa = nsa - gnx, nca = nca + gny;                     // n = (-s_a, c_a)
    else if (axis == 2) nce = nce + gnx, nse = nse + gny;                     // n = (c_e, s_e)
    else nse = nse - gnx, nce = nce + gny;                                    // n = (-s_e, c_e)
    ge[TTC_GX] = nx * inv, ge[TTC_GY] = ny * inv;
    ga[TTC_GX] = -ge[TTC_GX], ga[TTC_GY] = -ge[TTC_GY];
    ga[TTC_GLENGTH] = (sigma * (0.5 * fabs(a1))) * inv, ga[TTC_GWIDTH] = (sigma * (0.5 * fabs(a2))) * inv;
    ge[TTC_GLENGTH] = (sigma * (0.5 * fabs(e1))) * inv, ge[TTC_GWIDTH] = (sigma * (0.5 * fabs(e2))) * inv;
    ga[TTC_GSIN] = nsa * inv, ga[TTC_GCOS] = nca * inv;
    ge[TTC_GSIN] = nse * inv, ge[TTC_GCOS] = nce * inv;
    ga[TTC_GSPEED] = -((t * a1) * inv), ge[TTC_GSPEED] = (t * e1) * inv;
    return true;
}

}  // namespace tds

// The per-row arithmetic of the route step's backward (route_bwd.hip; DESIGN.md 5.5f, include/tdship.h "Differentiable route progress"), and the
// one piece of the forward it has to repeat to the bit: the clip of a segment to its piece.  Nothing of HIP in here: a host compiler takes this
// file as it is, and tests/route_grad_host.cpp holds these functions to the float64 autograd model tests/route_grad_model.py on the CPU.
//
// Float64, + - * / and the forward's one sqrt (the segment's length, for its tangent).  The discrete choices of the forward -- the piece, the
// segment, which clamp is active, the lookahead's pieces and segments -- are constants of differentiation.
#pragma once
#include "tds_lane_math.h"

namespace tds {

// segment [c0, c1] of a centre line's cumulative lengths clipped to the arc interval [a, b] of its piece: w = its length on `cum`, [ulo, uhi] =
// what of it lies inside, as parameters on the whole segment; false for a segment that is skipped
TDS_HD inline bool route_clip(double c0, double c1, double a, double b, double &w, double &ulo, double &uhi) {
    w = c1 - c0;
    if (!(w > 0.0)) return false;
    ulo = a > c0 ? (a - c0) / w : 0.0, uhi = b < c1 ? (b - c0) / w : 1.0;
    return uhi > ulo;
}

// what a row's backward sums: the gradient to [x, y] and to [sin psi, cos psi]
struct RouteGrad { double x, y, sn, cs; };

// the foot on the winning segment (p0, p1) -> (p3, p4), which starts at c0 = cum[i], is w long on `cum` and clipped to [ulo, uhi]; base =
// offsets[j] and a = a_j of its piece
struct RouteFoot {
    double progress;     // as the forward computed it
    double dx, dy;       // d progress / d[x, y]: w [dx, dy] / l2 where the foot moves with the pose, else 0
    RouteGrad g;         // what progress, advance, remaining, lateral and heading hand to the pose
};

TDS_HD inline RouteFoot route_foot_grad(double p0, double p1, double p3, double p4, double c0, double w, double ulo, double uhi, double base, double a,
                                        double x, double y, double g_progress, double g_advance, double g_remaining, double g_lateral, double g_hs,
                                        double g_hc) {
    RouteFoot f;
    const double dx = p3 - p0, dy = p4 - p1;
    const double l2 = dx * dx + dy * dy;
    const double u_raw = ((x - p0) * dx + (y - p1) * dy) / l2;
    const bool moves = ulo <= u_raw && u_raw <= uhi;                         // torch.clamp's rule: equality counts as interior
    const double u = fmin(fmax(u_raw, ulo), uhi);
    f.progress = base + ((c0 + u * w) - a);
    f.dx = moves ? (w * dx) / l2 : 0.0, f.dy = moves ? (w * dy) / l2 : 0.0;
    const double l = sqrt(l2);
    const double tx = dx / l, ty = dy / l;
    const double gp = (g_progress + g_advance) - g_remaining;               // advance differentiates as progress (stored is a constant), remaining as its negative
    f.g.x = gp * f.dx - g_lateral * ty, f.g.y = gp * f.dy + g_lateral * tx;  // lateral = tx (y - p1) - ty (x - p0), against the segment's LINE: clamped or not
    f.g.sn = g_hs * tx + g_hc * ty, f.g.cs = g_hc * tx - g_hs * ty;          // heading = [sn tx - cs ty, cs tx + sn ty]
    return f;
}

// one lookahead point: (px, py) = the route point at q = progress + (m + 1) spacing as the forward computed it, inside a segment (sx, sy) =
// P_(k+1) - P_k that is sw long on `cum`; (gox, goy) = the incoming gradient of [ox, oy] = [(px-x) cs + (py-y) sn, (py-y) cs - (px-x) sn].
// (fdx, fdy) = d progress / d[x, y] of the row's foot.  q moves with progress iff 0 < q <= length, the complement of route_point's two clamps.
TDS_HD inline RouteGrad route_look_grad(double px, double py, double sx, double sy, double sw, double q, double length, double x, double y, double sn,
                                        double cs, double fdx, double fdy, double gox, double goy) {
    RouteGrad g;
    const double ex = px - x, ey = py - y;
    const bool moves = q > 0.0 && q <= length && sw > 0.0;
    const double qx = moves ? sx / sw : 0.0, qy = moves ? sy / sw : 0.0;     // d[px, py] / dq
    const double gq = gox * (qx * cs + qy * sn) + goy * (qy * cs - qx * sn); // through the point, to progress
    g.x = (goy * sn - gox * cs) + gq * fdx, g.y = gq * fdy - (gox * sn + goy * cs);
    g.sn = gox * ey - goy * ex, g.cs = gox * ex + goy * ey;
    return g;
}

}  // namespace tds

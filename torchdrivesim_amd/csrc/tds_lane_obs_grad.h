// The gradients of the lane observations (lane_obs_bwd.hip; include/tdship.h "K8b"): what the eight incoming gradients of one
// filled slot, and the two of one valid polyline point, contribute to x, y, sin, cos of the observing agent.  The map is constant, so nothing
// goes anywhere else.  Nothing of HIP in here: a host compiler takes this file as it is, and tests/lane_obs_grad_host.cpp holds these functions
// to their numpy restatement (tests/test_lane_obs_grad_host.py) bit for bit.  Float64, every operation rounded once, in the order written here.
// Constants of differentiation: the lanelet of the slot, the foot's segment sb, whether u was clamped, and for every point its validity, the
// lanelet its walk ends on and the segment there.  [sin, cos] are independent inputs.
#pragma once
#include <math.h>
#include <stdint.h>

#include "tds_lane_math.h"

namespace tds {

// the order of the four contributions
enum { LG_X = 0, LG_Y, LG_SIN, LG_COS, LG_GRADS };

// what the points of a slot need of its foot: a = d arc / d(x, y) = m * W * (dx, dy) / l2, (0, 0) where the foot is clamped (m = 0)
struct LaneSlide { double x, y; };

// Slot: f the foot of the pose (x, y) on segment sb (tds::segment_foot), t its unit vector (tds::segment_unit), W = cum[sb + 1] - cum[sb],
// (s, c) the observer's [sin, cos], g[8] the incoming gradient of the slot's features in K8's order -> out[4] (x, y, sin, cos) and the slide.
// m = 1 iff l2 > 0 and the UNCLAMPED u lies strictly inside (0, 1): the expression of tds::segment_foot before its clamp, so a NaN gives 0.
// distance's term m*(f.t)*t / distance is left out: the foot offset is perpendicular to the segment wherever m = 1, so it is zero in exact
// arithmetic.  distance == 0 contributes nothing through feature 7.
TDS_HD inline LaneSlide lane_obs_slot_grad(const SegmentFoot &f, Unit2 t, double W, double x, double y, double s, double c, const double *g,
                                           double *out) {
    const double u = f.l2 > 0 ? ((x - f.ax) * f.dx + (y - f.ay) * f.dy) / f.l2 : 0.0;
    const bool m = f.l2 > 0 && u > 0.0 && u < 1.0;
    LaneSlide a;
    a.x = m ? (W * f.dx) / f.l2 : 0.0, a.y = m ? (W * f.dy) / f.l2 : 0.0;
    const double qx = g[0] * c - g[1] * s, qy = g[0] * s + g[1] * c;          // features 0, 1 turned back into the world frame
    const double tq = t.x * qx + t.y * qy;
    double px = m ? tq * t.x - qx : -qx, py = m ? tq * t.y - qy : -qy;
    const double G = g[4] - g[5];                                              // arc and remaining = cum[last] - arc
    px = px + G * a.x, py = py + G * a.y;
    px = px - g[6] * t.y, py = py + g[6] * t.x;                                // lateral
    const double dist = sqrt(f.d2);
    if (dist > 0.0) px = px - g[7] * (f.fx / dist), py = py - g[7] * (f.fy / dist);
    out[LG_X] = px, out[LG_Y] = py;
    out[LG_SIN] = (g[0] * f.fy - g[1] * f.fx) + (g[3] * t.y - g[2] * t.x);
    out[LG_COS] = (g[0] * f.fx + g[1] * f.fy) + (g[2] * t.y + g[3] * t.x);
    return a;
}

// Valid point: (ex, ey) the point minus the pose in the world frame, (hx, hy) the unit step of its segment per metre of arc ((0, 0) on a segment
// without length), a the slide of its slot, (gx, gy) the incoming gradient of the point -> out[4].  (h.r) * a is the polyline sliding along the
// lane as the agent moves; it vanishes where the foot is clamped.
TDS_HD inline void lane_obs_point_grad(LaneSlide a, double ex, double ey, double hx, double hy, double s, double c, double gx, double gy,
                                       double *out) {
    const double rx = gx * c - gy * s, ry = gx * s + gy * c;
    const double hr = hx * rx + hy * ry;
    out[LG_X] = hr * a.x - rx, out[LG_Y] = hr * a.y - ry;
    out[LG_SIN] = gx * ey - gy * ex, out[LG_COS] = gx * ex + gy * ey;
}

}  // namespace tds

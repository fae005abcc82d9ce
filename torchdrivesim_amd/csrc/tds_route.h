// What the route step (route.hip) and its backward (route_bwd.hip) both do on a lane table: weigh a segment against a pose, and find the point
// at a route arc.  One definition, so that the backward finds the forward's segment again to the bit.
#pragma once
#include "tds_lanes.h"
#include "tds_route_grad.h"

namespace tds {

// what every route kernel reads of a batch: the lane tables and the route tensors (B x A rows)
struct RouteArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    int64_t rows;
    int A;
    const int32_t *route_lanes, *route_n;       // rows x TDS_ROUTE_MAX_LANES, rows
    const double *start_arc, *end_arc, *offsets, *length;
};

// host: the checks every route entry point makes of them
inline int route_args(const char *what, RouteArgs &r, const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, const int32_t *route_lanes,
               const int32_t *route_n, const double *start_arc, const double *end_arc, const double *offsets, const double *length) {
    TDS_CHECK_ARG(set, "%s: the lane-table set is null", what);
    TDS_CHECK_SCENE_MAP(what, set, scene_map);
    TDS_CHECK_ARG(B >= 0 && A >= 0 && A < ((int64_t)1 << 31) && (A == 0 || B <= (((int64_t)1 << 31) - 1) / A), "%s: bad sizes B=%lld A=%lld", what,
                  (long long)B, (long long)A);
    TDS_CHECK_ARG(B * A == 0 || (route_lanes && route_n && start_arc && end_arc && offsets && length), "%s: a route tensor is null", what);
    r.views = set->d_views, r.n_views = set->n, r.scene_map = scene_map, r.rows = B * A, r.A = (int)A;
    r.route_lanes = route_lanes, r.route_n = route_n, r.start_arc = start_arc, r.end_arc = end_arc, r.offsets = offsets, r.length = length;
    return TDS_OK;
}

// segment i of a centre line, clipped to the arc interval [a, b] of its piece, against the pose (x, y): false for a segment that is skipped
// (no length in 2-D or on `cum`, or nothing of it inside [a, b]); else u = the foot's parameter on the whole segment, d2 = its squared distance
__device__ inline bool weigh_segment(const double *cl, const double *cum, int i, double a, double b, double x, double y, double &u, double &d2) {
    const double *p = cl + 3 * (int64_t)i;
    const double dx = p[3] - p[0], dy = p[4] - p[1];
    const double l2 = dx * dx + dy * dy;
    double w, ulo, uhi;
    if (!(l2 > 0.0) || !route_clip(cum[i], cum[i + 1], a, b, w, ulo, uhi)) return false;
    u = ((x - p[0]) * dx + (y - p[1]) * dy) / l2;
    u = fmin(fmax(u, ulo), uhi);
    const double fx = (p[0] + u * dx) - x, fy = (p[1] + u * dy) - y;
    d2 = fx * fx + fy * fy;
    return true;
}

// the point at route arc q, world frame, and the segment it lies in: (sx, sy) = P_(k+1) - P_k, sw = its length on `cum` (all 0 where there is no
// point to give).  Not tds::point_at_arc: a route measures a segment by w = cum[k + 1] - cum[k] (include/tdship.h), the same w its progress is
// computed with, and that is not the segment's own 3-D length bit for bit.
__device__ inline void route_point(const LaneView &v, const int32_t *lanes, const double *offs, int n, double a0, double length, double q,
                                   double &x, double &y, double &sx, double &sy, double &sw) {
    x = 0.0, y = 0.0, sx = 0.0, sy = 0.0, sw = 0.0;
    if (!(q > 0.0)) q = 0.0;
    if (q > length) q = length;
    int j = 0;
    for (int i = 1; i < n; ++i)
        if (offs[i] <= q) j = i;                                             // the last piece that starts at or before q
    const int l = lanes[j];
    if (l < 0 || l >= v.n) return;
    const LaneRec r = v.rec[l];
    if (r.cl_n < 2) return;
    const double *cl = v.cl + 3 * (int64_t)r.cl_start, *cum = v.cum + r.cl_start;
    const double arc = (j == 0 ? a0 : 0.0) + (q - offs[j]);
    const int k = segment_of(cum, r.cl_n, arc);
    const double *p = cl + 3 * (int64_t)k;
    sx = p[3] - p[0], sy = p[4] - p[1], sw = cum[k + 1] - cum[k];
    const double u = sw > 0.0 ? (arc - cum[k]) / sw : 0.0;
    x = p[0] + u * sx, y = p[1] + u * sy;
}

__device__ inline void route_point(const LaneView &v, const int32_t *lanes, const double *offs, int n, double a0, double length, double q,
                                   double &x, double &y) {
    double sx, sy, sw;
    route_point(v, lanes, offs, n, a0, length, q, x, y, sx, sy, sw);
}

}  // namespace tds

// What the lane observations (K8, lane_obs.hip) and their backward (K8b, lane_obs_bwd.hip) both do on a lane table, stated once: which lanelet
// is a candidate, the foot of a pose on a centre line found by a whole wave, and the walk of a polyline point along the lane graph with the
// point it ends at.  The backward REDOES the forward's discrete choices with these, so the arithmetic here is the forward's, operation for
// operation: binary64, every operation rounded once (-ffp-contract=off).  Device code: both kernels run one wave per observer.
#pragma once
#include "tds_lanes.h"

namespace tds {

// a lanelet K8 looks at: drivable and without an excluded tag (the rule of tds_lane_snap)
__device__ __forceinline__ bool usable(const LaneView &v, int l, const LaneRec &r) { return !(r.flags & 1) && drivable(v, l); }

// the foot of (x, y) on the centre line of lanelet record r, found by the WHOLE WAVE (all 64 lanes call together; r, x, y are the same in every
// lane): lane i takes the segments i, i + 64, ... in ascending order, then a wave-wide minimum of (d2, segment) -- the smallest d2, the earliest
// segment on ties, what one pass over the segments in ascending order gives: every d2 is the same number whichever lane computes it.  The result
// is the same in every lane; false if no d2 is below +inf.
__device__ __forceinline__ bool wave_foot(const LaneView &v, const LaneRec &r, double x, double y, int lane, int &sb, double &d2) {
    const double *cl = v.cl + 3 * (int64_t)r.cl_start;
    d2 = INFINITY, sb = 0x7fffffff;
    for (int i = lane; i + 1 < r.cl_n; i += 64) {
        const double d = segment_foot(cl, i, x, y).d2;
        if (d < d2) d2 = d, sb = i;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const double od = __shfl_xor(d2, m, 64);
        const int oi = __shfl_xor(sb, m, 64);
        if (od < d2 || (od == d2 && oi < sb)) d2 = od, sb = oi;
    }
    return sb != 0x7fffffff;
}

// Point j of a slot: the walk from lanelet `cur` (a candidate, in [0, v.n)) to arc length q measured from its start, over at most
// TDS_LANE_OBS_MAX_HOPS unique successors that are candidates, and the centre-line point it ends at.  False for an invalid point; else (ex, ey)
// is the point minus the pose (x, y), in the world frame, and (hx, hy) the segment it lies on divided by w, the segment's length on `cum`
// ((0, 0) where w <= 0): what the point moves by per metre of q.
struct LanePoint { double ex, ey, hx, hy; };
__device__ __forceinline__ bool lane_point(const LaneView &v, int cur, double q, double x, double y, LanePoint &p) {
    LaneRec r = v.rec[cur];
    double base = 0.0, len = v.cum[r.cl_start + r.cl_n - 1];
    for (int hops = 0; q - base > len; ++hops) {         // at most TDS_LANE_OBS_MAX_HOPS hops
        int nxt = -1;
        if (hops < TDS_LANE_OBS_MAX_HOPS && v.succ_start) {
            const int s0 = v.succ_start[cur];
            if (v.succ_start[cur + 1] - s0 == 1) nxt = v.succ_items[s0];
        }
        if (nxt < 0 || nxt >= v.n) return false;
        const LaneRec rn = v.rec[nxt];
        if (!usable(v, nxt, rn)) return false;
        base += len, cur = nxt, r = rn, len = v.cum[r.cl_start + r.cl_n - 1];
    }
    const double *cum = v.cum + r.cl_start, *cl = v.cl + 3 * (int64_t)r.cl_start;
    const double pos = q - base;
    const int sg = segment_of(cum, r.cl_n, pos);
    const double *a = cl + 3 * sg;
    const double w = cum[sg + 1] - cum[sg];
    const double t = w > 0.0 ? (pos - cum[sg]) / w : 0.0;
    const double sx = a[3] - a[0], sy = a[4] - a[1];
    const double wx = a[0] + t * sx, wy = a[1] + t * sy;
    p.ex = wx - x, p.ey = wy - y;
    p.hx = w > 0.0 ? sx / w : 0.0, p.hy = w > 0.0 ? sy / w : 0.0;
    return true;
}

}  // namespace tds

// Lane tables as the kernels see them (lanes.hip builds and queries them; spawn.hip, follow.hip and route.hip move on their centre lines and
// their graph) and what those kernels ask of a table; the arithmetic on one centre line is in tds_lane_math.h.
#pragma once
#include "tds_common.h"
#include "tds_lane_math.h"

namespace tds {

struct LaneRec {
    int32_t poly_start, poly_n;     // outline ring: left bound, then the right bound reversed (implicitly closed)
    int32_t cl_start, cl_n;         // centre line points
    int32_t flags;                  // bit 0: tagged with an excluded attribute ('parking', infractions.py:21)
    float bx0, by0, bx1, by1;       // bounding box of the outline, rounded outwards
};

struct LaneView {
    const double *poly;             // 2 doubles per point
    const double *cl;               // 3 doubles per point
    const LaneRec *rec;
    const int32_t *cell_start;      // nx*ny + 1
    const int32_t *cell_items;      // lanelet indices
    double ox, oy, inv_cell;
    int nx, ny, n;
    float max_tol;
    const double *cum;              // per centre-line point: the 3-D length of its centre line up to it (0 at a lanelet's first point)
    const int32_t *eligible;        // the lanelets a point can be drawn on (>= 2 centre-line points, finite positive length), ascending
    int n_eligible;
    const int32_t *succ_start;      // the lane graph (tds_lanes_set_successors): lanelet l is followed by succ_items[succ_start[l] .. succ_start[l + 1]),
    const int32_t *succ_items;      // ascending; both null until the graph is set
};

// the table of a scene, or false: a scene without a lane map.  `single` is for the kernels that also serve a single-table entry point, and they
// always pass it: without a set (views == null) it is the table of every scene.  Every other caller has a set; views == null without `single`
// is not a case this function handles.
__device__ inline bool view_of(const LaneView *views, int n_views, const int32_t *scene_map, int64_t scene, LaneView &out,
                               const LaneView *single = nullptr) {
    if (single && !views) {
        out = *single;
        return true;
    }
    const int m = scene_map ? scene_map[scene] : 0;
    if (m < 0 || m >= n_views) return false;
    out = views[m];
    return true;
}

// a lanelet one can drive on: one of `eligible` (>= 2 centre-line points, finite positive length)
__device__ inline bool drivable(const LaneView &v, int l) {
    if (l < 0 || l >= v.n) return false;
    const LaneRec r = v.rec[l];
    if (r.cl_n < 2) return false;
    const double len = v.cum[r.cl_start + r.cl_n - 1];
    return len > 0.0 && len < INFINITY;
}

// the successor lanelet `l` takes at hop `hop`, -1 when it has none: one Philox word keyed by (scene id, who, hop), scaled to the number of ALL
// successors and not drawn when there is one.  Whether the drawn lanelet will do is the caller's matter: one that will not is a dead end, not
// a reason to draw again.
__device__ inline int successor_draw(const LaneView &v, int l, uint64_t sid, int who, int hop, uint32_t key0, uint32_t key1) {
    if (!v.succ_start) return -1;
    const int s0 = v.succ_start[l], ns = v.succ_start[l + 1] - s0;
    if (ns <= 0) return -1;
    int pick = 0;
    if (ns > 1) {
        U4 ctr = {(uint32_t)sid, (uint32_t)(sid >> 32), (uint32_t)who, (uint32_t)hop};
        pick = pick_of(philox4x32_10(ctr, key0, key1).x, ns);
    }
    return v.succ_items[s0 + pick];
}

// Between an LDS write of one lane and the reads of the other lanes of the SAME wave: LDS operations of a wave complete in issue order, so
// all that is needed is that the compiler keeps that order.
__device__ inline void order_lds() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// host: what the entry points refuse
inline bool ok_param(double x) { return x >= 0.0 && x < INFINITY; }

}  // namespace tds

struct tds_lanes {
    tds::LaneView view;
    void *d_poly, *d_cl, *d_rec, *d_cell_start, *d_cell_items, *d_cum, *d_eligible, *d_succ_start, *d_succ_items;
    int device;
    int64_t bytes;
};

struct tds_laneset {
    tds::LaneView *d_views;
    int n, device;
    float max_tol;
    int max_lanelets;               // the lanelets of the largest table: what a launch sizes per-table LDS by (lane_obs.hip)
};

#define TDS_CHECK_SCENE_MAP(what, set, scene_map) \
    TDS_CHECK_ARG((scene_map) || (set)->n == 1, "%s: a set of %d lane tables needs scene_map", what, (set)->n)

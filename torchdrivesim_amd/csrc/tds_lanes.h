// Lane tables as the kernels see them (lanes.hip builds and queries them; spawn.hip draws points on their centre lines).
#pragma once
#include "tds_common.h"

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
};

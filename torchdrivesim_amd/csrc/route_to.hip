// Routes to a destination: shortest paths on the lane graph.
//
// No reference counterpart.  The definition is this library's own (include/tdship.h "Routes to a destination"); its yardstick is the float64
// model tests/route_to_model.py, which restates every expression below in the same order.
//
// tds_lane_distances_f64 builds, once per lane table, the L x L table to_go[t][l] = distance from the START of lanelet l to the START of
// lanelet t: one workgroup per destination t, its field in LDS, Jacobi sweeps to the fixed point.  The field is the least fixed point of a
// monotone operator (rounded addition is monotone), so it does not depend on the order of relaxation: sweeps, Gauss-Seidel and Dijkstra give
// the same bits.  tds_route_to_multi deals the routes at a reset: a thread per row, at most TDS_ROUTE_MAX_LANES hops of steepest descent on
// row t of the table.  What it writes is a route like any other: progress, lookahead and points are route.hip's.
//
// Arithmetic: float64, + and compares only (-ffp-contract=off).
#include <math.h>

#include "tds_common.h"
#include "tds_lanes.h"

using tds::LaneRec;
using tds::LaneView;
using tds::drivable;
using tds::view_of;

namespace {

constexpr int DBLOCK = 256;                      // the distance kernel's workgroup: four waves over the lanelets of one destination
constexpr int GRAPH_MAX = TDS_ROUTE_MAX_GRAPH;
constexpr int PER_THREAD = GRAPH_MAX / DBLOCK;   // lanelets a thread relaxes: l = tid, tid + DBLOCK, ...
constexpr int TBLOCK = 256;
constexpr int ROUTE_LANES = TDS_ROUTE_MAX_LANES;
static_assert(GRAPH_MAX % DBLOCK == 0, "the lanelets are dealt to the threads in whole rounds");

struct RouteToArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const int64_t *tables;                       // per view: the address of its L x L to_go table, 0 without one
    int64_t rows;
    int A;
    const int32_t *lane, *dest_lane;
    const double *arc, *dest_arc;
    const uint8_t *present, *mask;
    int32_t *route_lanes, *route_n, *cursor;
    double *start_arc, *end_arc, *offsets, *length, *stored, *rest;
    uint8_t *completed;
};

// a lanelet a route may use: one that can be driven on and carries no excluded tag
__device__ inline bool usable(const LaneView &v, int l) { return drivable(v, l) && !(v.rec[l].flags & 1); }

__device__ inline double length_of(const LaneView &v, int l) { return v.cum[v.rec[l].cl_start + v.rec[l].cl_n - 1]; }

// ---- distance fields: a workgroup per destination ---------------------------------------------------------------------------------------
// Sweep: every thread reads the field for its lanelets (read phase), barrier, writes what got smaller (write phase), barrier, and all read
// the flag.  A field changes in at most L - 1 sweeps (a shortest path has at most L lanelets), so the loop ends after L sweeps whatever the
// table holds.  An unusable lanelet is never written, so it stays +inf and nothing is relaxed through it: len + inf = inf.
__global__ void __launch_bounds__(DBLOCK) lane_distances_kernel(LaneView v, double *to_go) {
    __shared__ double field[GRAPH_MAX];
    __shared__ int changed;
    const int t = blockIdx.x, tid = threadIdx.x, L = v.n;
    double len[PER_THREAD];
    int s0[PER_THREAD], s1[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int l = tid + k * DBLOCK;
        len[k] = 0.0, s0[k] = 0, s1[k] = 0;                                  // no successors: never relaxed
        if (l < L) {
            const bool ok = usable(v, l);
            field[l] = ok && l == t ? 0.0 : INFINITY;
            if (ok && l != t) len[k] = length_of(v, l), s0[k] = v.succ_start[l], s1[k] = v.succ_start[l + 1];
        }
    }
    __syncthreads();
    for (int sweep = 0; sweep < L; ++sweep) {
        if (tid == 0) changed = 0;
        double next[PER_THREAD];
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            double m = INFINITY;
            for (int i = s0[k]; i < s1[k]; ++i) {
                const int s = v.succ_items[i];
                if ((unsigned)s < (unsigned)L && field[s] < m) m = field[s];
            }
            next[k] = len[k] + m;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            const int l = tid + k * DBLOCK;
            if (s1[k] > s0[k] && next[k] < field[l]) field[l] = next[k], changed = 1;
        }
        __syncthreads();
        const int again = changed;
        __syncthreads();                                                     // everyone has read the flag before thread 0 clears it
        if (!again) break;
    }
    for (int l = tid; l < L; l += DBLOCK) to_go[(int64_t)t * L + l] = field[l];
}

// ---- dealing the routes: a thread per row --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TBLOCK) route_to_kernel(RouteToArgs g) {
    const int64_t row = (int64_t)blockIdx.x * TBLOCK + threadIdx.x;
    if (row >= g.rows) return;
    if (g.mask && !g.mask[row]) return;                                      // rows outside the mask keep everything
    const int64_t scene = row / g.A;
    int32_t *lanes = g.route_lanes + row * ROUTE_LANES;
    double *offs = g.offsets + row * ROUTE_LANES;
    int n = 0;
    double a0 = 0.0, bend = 0.0, off = 0.0, rest = INFINITY;
    LaneView v;
    const int l0 = g.lane[row], t = g.dest_lane[row];
    const int m = g.scene_map ? g.scene_map[scene] : 0;
    const double *table = m >= 0 && m < g.n_views ? (const double *)(uintptr_t)g.tables[m] : nullptr;
    if (table && view_of(g.views, g.n_views, g.scene_map, scene, v) && v.succ_start && (!g.present || g.present[row]) && usable(v, l0) && usable(v, t)) {
        const double *to_go = table + (int64_t)t * v.n;
        const double len0 = length_of(v, l0), lent = length_of(v, t);
        double a = g.arc[row], b = g.dest_arc[row];
        if (!(a > 0.0)) a = 0.0;
        if (a > len0) a = len0;
        if (!(b > 0.0)) b = 0.0;
        if (b > lent) b = lent;
        a0 = a;
        if (t == l0 && b >= a0) {                                            // the destination is ahead on the agent's own lanelet
            lanes[0] = l0, offs[0] = off, n = 1;
            bend = b;
            off = off + (bend - a);
            rest = 0.0;
        } else {
            int l = l0;
            for (int j = 0; j < ROUTE_LANES; ++j) {
                const double len = length_of(v, l);
                lanes[j] = l, offs[j] = off, n = j + 1;
                bend = len;
                off = off + (len - a);
                int nxt = -1;                                                // the usable successor nearest to t, the first of equals
                double best = INFINITY;
                for (int i = v.succ_start[l]; i < v.succ_start[l + 1]; ++i) {
                    const int s = v.succ_items[i];
                    if (usable(v, s) && to_go[s] < best) best = to_go[s], nxt = s;
                }
                if (nxt < 0) {                                               // t cannot be reached from here
                    n = 0;
                    break;
                }
                if (nxt == t && !(b > 0.0)) {                                // the destination is this lanelet's end
                    rest = 0.0;
                    break;
                }
                if (j == ROUTE_LANES - 1) {                                  // the cap: the route is short by what is left
                    rest = best + b;
                    break;
                }
                if (nxt == t) {
                    lanes[j + 1] = t, offs[j + 1] = off, n = j + 2;
                    bend = b;
                    off = off + (bend - 0.0);
                    rest = 0.0;
                    break;
                }
                l = nxt, a = 0.0;
            }
        }
        if (n > 0 && !(off > 0.0)) n = 0;                                    // nothing to drive: the agent stands at its destination (rest = 0)
    }
    if (n == 0) a0 = 0.0, bend = 0.0, off = 0.0;
    for (int j = n; j < ROUTE_LANES; ++j) lanes[j] = -1, offs[j] = 0.0;
    g.route_n[row] = n, g.start_arc[row] = a0, g.end_arc[row] = bend, g.length[row] = off, g.rest[row] = rest;
    g.cursor[row] = 0, g.stored[row] = 0.0, g.completed[row] = 0;
}

}  // namespace

TDS_EXPORT int tds_lane_distances_f64(const tds_lanes_t *lanes, double *to_go, void *stream) {
    TDS_CHECK_ARG(lanes, "tds_lane_distances_f64: the lane table is null");
    const int L = lanes->view.n;
    if (L > TDS_ROUTE_MAX_GRAPH) {
        tds::set_error("tds_lane_distances_f64: %d lanelets exceed the %d a destination's distance field holds in LDS", L, TDS_ROUTE_MAX_GRAPH);
        return TDS_ELIMIT;
    }
    TDS_CHECK_ARG(lanes->view.succ_start, "tds_lane_distances_f64: the lane table has no successor graph (tds_lanes_set_successors)");
    if (L == 0) return TDS_OK;
    TDS_CHECK_ARG(to_go, "tds_lane_distances_f64: to_go is null");
    hipLaunchKernelGGL(lane_distances_kernel, dim3((unsigned)L), dim3(DBLOCK), 0, (hipStream_t)stream, lanes->view, to_go);
    TDS_LAUNCH_CHECK("lane_distances_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_route_to_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *tables, int64_t B, int64_t A, const int32_t *lane,
                                  const double *arc, const int32_t *dest_lane, const double *dest_arc, const uint8_t *present, const uint8_t *mask,
                                  int32_t *route_lanes, int32_t *route_n, double *start_arc, double *end_arc, double *offsets, double *length,
                                  int32_t *cursor, double *stored, uint8_t *completed, double *rest, void *stream) {
    const char *what = "tds_route_to_multi";
    TDS_CHECK_ARG(set, "%s: the lane-table set is null", what);
    TDS_CHECK_SCENE_MAP(what, set, scene_map);
    TDS_CHECK_ARG(B >= 0 && A >= 0 && A < ((int64_t)1 << 31) && (A == 0 || B <= (((int64_t)1 << 31) - 1) / A), "%s: bad sizes B=%lld A=%lld", what,
                  (long long)B, (long long)A);
    if (B * A == 0) return TDS_OK;
    TDS_CHECK_ARG(tables && lane && arc && dest_lane && dest_arc && route_lanes && route_n && start_arc && end_arc && offsets && length && cursor &&
                      stored && completed && rest,
                  "%s: null argument", what);
    RouteToArgs g = {};
    g.views = set->d_views, g.n_views = set->n, g.scene_map = scene_map, g.tables = tables, g.rows = B * A, g.A = (int)A;
    g.lane = lane, g.arc = arc, g.dest_lane = dest_lane, g.dest_arc = dest_arc, g.present = present, g.mask = mask;
    g.route_lanes = route_lanes, g.route_n = route_n, g.cursor = cursor;
    g.start_arc = start_arc, g.end_arc = end_arc, g.offsets = offsets, g.length = length, g.stored = stored, g.rest = rest, g.completed = completed;
    hipLaunchKernelGGL(route_to_kernel, dim3((unsigned)((g.rows + TBLOCK - 1) / TBLOCK)), dim3(TBLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("route_to_kernel");
    return TDS_OK;
}

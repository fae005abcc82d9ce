// Route goals: routes sampled on the lane graph, progress and lookahead per step, one launch each.
//
// No reference counterpart: the reference's only goal object is a list of recorded waypoints.  The definition is this library's own; its
// yardstick is the float64 model tests/route_model.py, which restates every expression below in the same order.
//
// tds_route_progress_multi is the per-step path: one wavefront per row (agent), four rows per workgroup, no LDS and no workgroup barrier.  The
// lanes of a wave split the segments of the window's lanelets (at most three), reduce (squared distance, piece, segment) with shuffles, all
// redo the winning segment from a wave-uniform index, lane 0 writes the scalars and lanes 0 .. K-1 a lookahead point each.  Sampling and the
// points query are a thread per row / per point: they run at a reset, and their walks are sequential by definition.
//
// Arithmetic: float64 on the float64 lane table, + - * / sqrt only (-ffp-contract=off); poses are widened from float32, float outputs are
// rounded to binary32 once, at the end.
#include <math.h>

#include "tds_common.h"
#include "tds_lanes.h"
#include "tds_route.h"

using tds::LaneRec;
using tds::LaneView;
using tds::RouteArgs;
using tds::route_args;
using tds::drivable;
using tds::route_point;
using tds::segment_of;
using tds::view_of;
using tds::weigh_segment;

namespace {

constexpr int RBLOCK = 256;                      // four waves = four rows of the progress kernel
constexpr int ROUTE_LANES = TDS_ROUTE_MAX_LANES;
constexpr int SEG_BITS = 28;                     // (piece of the window, segment) packed into one int for the arg-min's tie rule

struct SampleArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const int64_t *scene_ids;
    int64_t rows;
    int A;
    const int32_t *lane;
    const double *arc, *distance;
    const uint8_t *present, *mask;
    uint32_t key0, key1;
    int32_t *route_lanes, *route_n, *cursor;
    double *start_arc, *end_arc, *offsets, *length, *stored;
    uint8_t *completed;
};

struct ProgressArgs {
    RouteArgs r;
    const float *xy, *sc;
    int64_t xy_stride;
    const uint8_t *present;
    int32_t *cursor;
    double *stored;
    uint8_t *completed;
    double goal_tolerance, off_route_distance, spacing;
    int K;
    float *progress, *advance, *lateral, *heading, *remaining, *lookahead;
    uint8_t *reached, *off_route;
};

// ---- sampling: a thread per row ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RBLOCK) route_sample_kernel(SampleArgs g) {
    const int64_t row = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (row >= g.rows) return;
    if (g.mask && !g.mask[row]) return;                                      // rows outside the mask keep their routes
    const int64_t scene = row / g.A;
    const int agent = (int)(row - scene * g.A);
    int32_t *lanes = g.route_lanes + row * ROUTE_LANES;
    double *offs = g.offsets + row * ROUTE_LANES;
    int n = 0;
    double a0 = 0.0, bend = 0.0, off = 0.0;
    LaneView v;
    int l = g.lane[row];
    double rem = g.distance[row];
    if (view_of(g.views, g.n_views, g.scene_map, scene, v) && (!g.present || g.present[row]) && rem > 0.0 && rem < INFINITY && drivable(v, l)) {
        const uint64_t sid = g.scene_ids ? (uint64_t)g.scene_ids[scene] : (uint64_t)scene;
        double a = g.arc[row];
        const double len0 = v.cum[v.rec[l].cl_start + v.rec[l].cl_n - 1];
        if (!(a > 0.0)) a = 0.0;
        if (a > len0) a = len0;
        a0 = a;
        for (int j = 0; j < ROUTE_LANES; ++j) {
            const LaneRec r = v.rec[l];
            const double len = v.cum[r.cl_start + r.cl_n - 1];
            lanes[j] = l, offs[j] = off, n = j + 1;
            if (rem <= len - a) {                                            // the rest fits on this lanelet
                bend = a + rem;
                off = off + (bend - a);
                break;
            }
            bend = len;
            off = off + (len - a), rem = rem - (len - a);
            if (j == ROUTE_LANES - 1) break;                                 // the cap: the route is short by what is left
            // the successor for hop j: one that cannot be driven on or carries an excluded tag is a dead end, the route ends at this lanelet's end
            const int nxt = tds::successor_draw(v, l, sid, agent, j, g.key0, g.key1);
            if (!drivable(v, nxt) || (v.rec[nxt].flags & 1)) break;
            l = nxt, a = 0.0;
        }
        if (!(off > 0.0)) n = 0;                                             // nothing to drive: a start at the very end of a dead end
    }
    if (n == 0) a0 = 0.0, bend = 0.0, off = 0.0;
    for (int j = n; j < ROUTE_LANES; ++j) lanes[j] = -1, offs[j] = 0.0;
    g.route_n[row] = n, g.start_arc[row] = a0, g.end_arc[row] = bend, g.length[row] = off;
    g.cursor[row] = 0, g.stored[row] = 0.0, g.completed[row] = 0;
}

// ---- progress: a wavefront per row --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RBLOCK) route_progress_kernel(ProgressArgs g) {
    const int lane_id = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (RBLOCK / 64) + (threadIdx.x >> 6);
    if (row >= g.r.rows) return;
    const int64_t scene = row / g.r.A;
    const int K = g.K;
    int n = min(g.r.route_n[row], ROUTE_LANES);
    LaneView v;
    if (!view_of(g.r.views, g.r.n_views, g.r.scene_map, scene, v) || (g.present && !g.present[row])) n = 0;
    const int32_t *lanes = g.r.route_lanes + row * ROUTE_LANES;
    const double *offs = g.r.offsets + row * ROUTE_LANES;
    const double x = (double)g.xy[row * g.xy_stride], y = (double)g.xy[row * g.xy_stride + 1];
    const double sn = (double)g.sc[row * 2], cs = (double)g.sc[row * 2 + 1];
    double a0 = 0.0, bend = 0.0;
    int k = 0;
    double best_d2 = INFINITY;
    int best = 0x7fffffff;
    if (n > 0) {
        a0 = g.r.start_arc[row], bend = g.r.end_arc[row];
        k = min(max(g.cursor[row], 0), n - 1);
        for (int w = 0; w < 3 && k + w < n; ++w) {                           // the window: the cursor's piece and the two after it
            const int j = k + w, l = lanes[j];
            if (l < 0 || l >= v.n) continue;
            const LaneRec r = v.rec[l];
            if (r.cl_n < 2) continue;
            const double *cl = v.cl + 3 * (int64_t)r.cl_start, *cum = v.cum + r.cl_start;
            const double a = j == 0 ? a0 : 0.0, b = j == n - 1 ? bend : cum[r.cl_n - 1];
            const int n_seg = min(r.cl_n - 1, 1 << SEG_BITS);
            for (int i = lane_id; i < n_seg; i += 64) {
                double u, d2;
                if (weigh_segment(cl, cum, i, a, b, x, y, u, d2) && d2 < best_d2) best_d2 = d2, best = (w << SEG_BITS) | i;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                   // the smallest distance, the earliest (piece, segment) on ties
            const double od = __shfl_xor(best_d2, s);
            const int ob = __shfl_xor(best, s);
            if (od < best_d2 || (od == best_d2 && ob < best)) best_d2 = od, best = ob;
        }
        best = __builtin_amdgcn_readfirstlane(best);                         // every lane holds the same winner: say so
    }
    float f_progress = 0.f, f_advance = 0.f, f_lateral = 0.f, f_hs = 0.f, f_hc = 1.f, f_remaining = 0.f;
    uint8_t reached = 0, off_route = 0, completed = 0;
    double progress = 0.0, length = 0.0;
    const bool found = best != 0x7fffffff;
    bool keep_completed = !found && n > 0;                                   // a pose no segment can be weighed against (NaN): the route stays as it is
    int piece = 0;
    if (found) {                                                            // every lane redoes the winning segment: the same numbers
        const int j = k + (best >> SEG_BITS), i = best & ((1 << SEG_BITS) - 1);
        const LaneRec r = v.rec[lanes[j]];
        const double *cl = v.cl + 3 * (int64_t)r.cl_start, *cum = v.cum + r.cl_start;
        const double a = j == 0 ? a0 : 0.0, b = j == n - 1 ? bend : cum[r.cl_n - 1];
        double u = 0.0, d2 = 0.0;
        weigh_segment(cl, cum, i, a, b, x, y, u, d2);
        const double *p = cl + 3 * (int64_t)i;
        const double dx = p[3] - p[0], dy = p[4] - p[1];
        const double l2 = sqrt(dx * dx + dy * dy);
        const double tx = dx / l2, ty = dy / l2;
        const double arc = cum[i] + u * (cum[i + 1] - cum[i]);
        length = g.r.length[row];
        progress = offs[j] + (arc - a);
        const double remaining = length - progress;
        reached = remaining <= g.goal_tolerance;
        off_route = sqrt(d2) > g.off_route_distance;
        f_progress = (float)progress, f_remaining = (float)remaining;
        f_lateral = (float)(tx * (y - p[1]) - ty * (x - p[0]));
        f_hs = (float)(sn * tx - cs * ty), f_hc = (float)(cs * tx + sn * ty);
        piece = j;
    }
    if (lane_id == 0) {                                                      // the state a call reads and writes is lane 0's alone: load, then store
        if (found) {
            f_advance = (float)(progress - g.stored[row]);
            completed = (g.completed[row] != 0) | reached;
            g.cursor[row] = piece, g.stored[row] = progress;
        } else if (keep_completed) {
            completed = g.completed[row] != 0;
        }
        g.progress[row] = f_progress, g.advance[row] = f_advance, g.lateral[row] = f_lateral, g.remaining[row] = f_remaining;
        g.heading[row * 2] = f_hs, g.heading[row * 2 + 1] = f_hc;
        g.reached[row] = reached, g.off_route[row] = off_route, g.completed[row] = completed;
    }
    for (int m = lane_id; m < K; m += 64) {                                  // the lookahead: a point per lane, in the agent's frame
        float ox = 0.f, oy = 0.f;
        if (found) {
            double px, py;
            route_point(v, lanes, offs, n, a0, length, progress + (double)(m + 1) * g.spacing, px, py);
            const double dx = px - x, dy = py - y;
            ox = (float)(dx * cs + dy * sn), oy = (float)(dy * cs - dx * sn);
        }
        float *o = g.lookahead + (row * K + m) * 2;
        o[0] = ox, o[1] = oy;
    }
}

// ---- points at given route arcs: a thread per point -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RBLOCK) route_points_kernel(RouteArgs g, int Q, const double *q, float *out) {
    const int64_t idx = (int64_t)blockIdx.x * RBLOCK + threadIdx.x;
    if (idx >= g.rows * Q) return;
    const int64_t row = idx / Q;
    const int n = min(g.route_n[row], ROUTE_LANES);
    LaneView v;
    double px = 0.0, py = 0.0;
    if (n > 0 && view_of(g.views, g.n_views, g.scene_map, row / g.A, v))
        route_point(v, g.route_lanes + row * ROUTE_LANES, g.offsets + row * ROUTE_LANES, n, g.start_arc[row], g.length[row], q[idx], px, py);
    out[idx * 2] = (float)px, out[idx * 2 + 1] = (float)py;
}

}  // namespace

TDS_EXPORT int tds_route_sample_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t A,
                                      const int32_t *lane, const double *arc, const double *distance, const uint8_t *present, const uint8_t *mask,
                                      uint64_t seed, int32_t *route_lanes, int32_t *route_n, double *start_arc, double *end_arc, double *offsets,
                                      double *length, int32_t *cursor, double *stored, uint8_t *completed, void *stream) {
    RouteArgs r = {};
    const int rc = route_args("tds_route_sample_multi", r, set, scene_map, B, A, route_lanes, route_n, start_arc, end_arc, offsets, length);
    if (rc != TDS_OK) return rc;
    if (r.rows == 0) return TDS_OK;
    TDS_CHECK_ARG(lane && arc && distance && cursor && stored && completed, "tds_route_sample_multi: null argument");
    SampleArgs g = {};
    g.views = r.views, g.n_views = r.n_views, g.scene_map = scene_map, g.scene_ids = scene_ids, g.rows = r.rows, g.A = r.A;
    g.lane = lane, g.arc = arc, g.distance = distance, g.present = present, g.mask = mask;
    // the route stream: spawn's key for the same seed with two words folded in ("ROUT", "GOAL"), so it coincides with neither spawn's nor the NPCs'
    g.key0 = (uint32_t)seed ^ 0x524F5554u, g.key1 = (uint32_t)(seed >> 32) ^ 0x474F414Cu;
    g.route_lanes = route_lanes, g.route_n = route_n, g.cursor = cursor;
    g.start_arc = start_arc, g.end_arc = end_arc, g.offsets = offsets, g.length = length, g.stored = stored, g.completed = completed;
    hipLaunchKernelGGL(route_sample_kernel, dim3((unsigned)((r.rows + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("route_sample_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_route_progress_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, const float *xy, int64_t xy_stride,
                                        const float *sc, const uint8_t *present, const int32_t *route_lanes, const int32_t *route_n,
                                        const double *start_arc, const double *end_arc, const double *offsets, const double *length, int32_t *cursor,
                                        double *stored, uint8_t *completed, float goal_tolerance, float off_route_distance, int n_lookahead,
                                        float spacing, float *progress, float *advance, float *lateral, float *heading, float *remaining,
                                        uint8_t *reached, uint8_t *off_route, float *lookahead, void *stream) {
    ProgressArgs g = {};
    const int rc = route_args("tds_route_progress_multi", g.r, set, scene_map, B, A, route_lanes, route_n, start_arc, end_arc, offsets, length);
    if (rc != TDS_OK) return rc;
    TDS_CHECK_ARG(n_lookahead >= 0 && n_lookahead <= TDS_ROUTE_MAX_LOOKAHEAD, "tds_route_progress_multi: %d lookahead points, at most %d", n_lookahead,
                  TDS_ROUTE_MAX_LOOKAHEAD);
    TDS_CHECK_ARG(tds::ok_param(goal_tolerance) && tds::ok_param(off_route_distance) && tds::ok_param(spacing),
                  "tds_route_progress_multi: goal_tolerance, off_route_distance and spacing must be finite and not negative");
    TDS_CHECK_ARG(xy_stride >= 2, "tds_route_progress_multi: xy_stride %lld is less than 2", (long long)xy_stride);
    if (g.r.rows == 0) return TDS_OK;
    TDS_CHECK_ARG(xy && sc && cursor && stored && completed && progress && advance && lateral && heading && remaining && reached && off_route &&
                      (lookahead || n_lookahead == 0),
                  "tds_route_progress_multi: null argument");
    g.xy = xy, g.sc = sc, g.xy_stride = xy_stride, g.present = present, g.cursor = cursor, g.stored = stored, g.completed = completed;
    g.goal_tolerance = goal_tolerance, g.off_route_distance = off_route_distance, g.spacing = spacing, g.K = n_lookahead;
    g.progress = progress, g.advance = advance, g.lateral = lateral, g.heading = heading, g.remaining = remaining, g.lookahead = lookahead;
    g.reached = reached, g.off_route = off_route;
    const int per = RBLOCK / 64;
    hipLaunchKernelGGL(route_progress_kernel, dim3((unsigned)((g.r.rows + per - 1) / per)), dim3(RBLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("route_progress_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_route_points_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, int64_t Q, const int32_t *route_lanes,
                                      const int32_t *route_n, const double *start_arc, const double *end_arc, const double *offsets,
                                      const double *length, const double *q, float *points, void *stream) {
    RouteArgs r = {};
    const int rc = route_args("tds_route_points_multi", r, set, scene_map, B, A, route_lanes, route_n, start_arc, end_arc, offsets, length);
    if (rc != TDS_OK) return rc;
    TDS_CHECK_ARG(Q >= 0 && Q < ((int64_t)1 << 31) && (r.rows == 0 || Q <= (((int64_t)1 << 38)) / r.rows), "tds_route_points_multi: bad size Q=%lld",
                  (long long)Q);
    if (r.rows * Q == 0) return TDS_OK;
    TDS_CHECK_ARG(q && points, "tds_route_points_multi: null argument");
    hipLaunchKernelGGL(route_points_kernel, dim3((unsigned)((r.rows * Q + RBLOCK - 1) / RBLOCK)), dim3(RBLOCK), 0, (hipStream_t)stream, r, (int)Q, q, points);
    TDS_LAUNCH_CHECK("route_points_kernel");
    return TDS_OK;
}

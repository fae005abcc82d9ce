// Differentiable route progress: the gradients of the route step's float outputs to the pose, one launch for all rows (DESIGN.md 5.5f,
// include/tdship.h "Differentiable route progress").  Yardstick: the float64 torch-autograd model tests/route_grad_model.py.
//
// The shape of route_progress_kernel: one wavefront per row, four rows per workgroup, no LDS and no workgroup barrier.  No segment is saved by the
// forward: the lanes of a wave split the segments of piece `piece` (the cursor as the forward left it) alone, with the forward's own
// weigh_segment and its tie rule, which finds the forward's winner again -- that winner lay in this piece, and a row that found nothing in the
// window finds nothing in a part of it.  All lanes redo the winning segment from a wave-uniform index; lanes 0 .. K-1 take a lookahead point each;
// the four partial sums are reduced over the lanes by xor-shuffles in a fixed order, so a result does not change from run to run; lane 0 writes.
//
// Arithmetic (tds_route_grad.h): float64, each of the four outputs of a row rounded to binary32 once.
#include <math.h>

#include "tds_common.h"
#include "tds_route.h"

using tds::LaneRec;
using tds::LaneView;
using tds::RouteArgs;
using tds::RouteFoot;
using tds::RouteGrad;

namespace {

constexpr int RBLOCK = 256;                      // four waves = four rows
constexpr int ROUTE_LANES = TDS_ROUTE_MAX_LANES;
constexpr int MAX_SEGMENTS = 1 << 28;            // the forward's bound on the segments of one piece

struct BwdArgs {
    RouteArgs r;
    const float *xy, *sc;
    int64_t xy_stride;
    const uint8_t *present;
    const int32_t *piece;
    const float *g_progress, *g_advance, *g_lateral, *g_heading, *g_remaining, *g_lookahead;      // each may be null: zero
    double spacing;
    int K;
    float *g_xy, *g_sc;
};

__device__ inline double incoming(const float *g, int64_t at) { return g ? (double)g[at] : 0.0; }

__global__ void __launch_bounds__(RBLOCK) route_progress_bwd_kernel(BwdArgs g) {
    const int lane_id = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (RBLOCK / 64) + (threadIdx.x >> 6);
    if (row >= g.r.rows) return;
    const int64_t scene = row / g.r.A;
    int n = min(g.r.route_n[row], ROUTE_LANES);
    LaneView v;
    if (!tds::view_of(g.r.views, g.r.n_views, g.r.scene_map, scene, v) || (g.present && !g.present[row])) n = 0;
    const int32_t *lanes = g.r.route_lanes + row * ROUTE_LANES;
    const double *offs = g.r.offsets + row * ROUTE_LANES;
    const double x = (double)g.xy[row * g.xy_stride], y = (double)g.xy[row * g.xy_stride + 1];
    const double sn = (double)g.sc[row * 2], cs = (double)g.sc[row * 2 + 1];
    double a0 = 0.0, a = 0.0, b = 0.0;
    int j = 0;
    const double *cl = nullptr, *cum = nullptr;
    double best_d2 = INFINITY;
    int best = 0x7fffffff;
    if (n > 0) {
        a0 = g.r.start_arc[row];
        j = min(max(g.piece[row], 0), n - 1);                                // the forward's clamp of its cursor
        const int l = lanes[j];
        if (l >= 0 && l < v.n) {
            const LaneRec r = v.rec[l];
            if (r.cl_n >= 2) {
                cl = v.cl + 3 * (int64_t)r.cl_start, cum = v.cum + r.cl_start;
                a = j == 0 ? a0 : 0.0, b = j == n - 1 ? g.r.end_arc[row] : cum[r.cl_n - 1];
                const int n_seg = min(r.cl_n - 1, MAX_SEGMENTS);
                for (int i = lane_id; i < n_seg; i += 64) {
                    double u, d2;
                    if (tds::weigh_segment(cl, cum, i, a, b, x, y, u, d2) && d2 < best_d2) best_d2 = d2, best = i;
                }
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                   // the smallest distance, the earliest segment on ties
            const double od = __shfl_xor(best_d2, s);
            const int ob = __shfl_xor(best, s);
            if (od < best_d2 || (od == best_d2 && ob < best)) best_d2 = od, best = ob;
        }
        best = __builtin_amdgcn_readfirstlane(best);                         // every lane holds the same winner: say so
    }
    RouteGrad sum = {0.0, 0.0, 0.0, 0.0};
    if (best != 0x7fffffff) {                                               // every lane redoes the winning segment: the same numbers
        const double *p = cl + 3 * (int64_t)best;
        double w, ulo, uhi;
        tds::route_clip(cum[best], cum[best + 1], a, b, w, ulo, uhi);
        const RouteFoot f = tds::route_foot_grad(p[0], p[1], p[3], p[4], cum[best], w, ulo, uhi, offs[j], a, x, y, incoming(g.g_progress, row),
                                                 incoming(g.g_advance, row), incoming(g.g_remaining, row), incoming(g.g_lateral, row),
                                                 incoming(g.g_heading, row * 2), incoming(g.g_heading, row * 2 + 1));
        if (lane_id == 0) sum = f.g;
        if (lane_id < g.K && g.g_lookahead) {                                // a lookahead point per lane
            const double length = g.r.length[row];
            const double q = f.progress + (double)(lane_id + 1) * g.spacing;
            double px, py, sx, sy, sw;
            tds::route_point(v, lanes, offs, n, a0, length, q, px, py, sx, sy, sw);
            const float *go = g.g_lookahead + (row * g.K + lane_id) * 2;
            const RouteGrad c = tds::route_look_grad(px, py, sx, sy, sw, q, length, x, y, sn, cs, f.dx, f.dy, (double)go[0], (double)go[1]);
            sum.x = sum.x + c.x, sum.y = sum.y + c.y, sum.sn = sum.sn + c.sn, sum.cs = sum.cs + c.cs;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {                                   // a butterfly: the same order of additions every run
            sum.x = sum.x + __shfl_xor(sum.x, s), sum.y = sum.y + __shfl_xor(sum.y, s);
            sum.sn = sum.sn + __shfl_xor(sum.sn, s), sum.cs = sum.cs + __shfl_xor(sum.cs, s);
        }
    }
    if (lane_id == 0) {                                                      // rows without a foot: exact zeros
        g.g_xy[row * 2] = (float)sum.x, g.g_xy[row * 2 + 1] = (float)sum.y;
        g.g_sc[row * 2] = (float)sum.sn, g.g_sc[row * 2 + 1] = (float)sum.cs;
    }
}

}  // namespace

TDS_EXPORT int tds_route_progress_bwd_multi(const tds_laneset_t *set, const int32_t *scene_map, int64_t B, int64_t A, const float *xy, int64_t xy_stride,
                                            const float *sc, const uint8_t *present, const int32_t *route_lanes, const int32_t *route_n,
                                            const double *start_arc, const double *end_arc, const double *offsets, const double *length,
                                            const int32_t *piece, const float *g_progress, const float *g_advance, const float *g_lateral,
                                            const float *g_heading, const float *g_remaining, const float *g_lookahead, int n_lookahead, float spacing,
                                            float *g_xy, float *g_sc, void *stream) {
    BwdArgs g = {};
    const int rc = tds::route_args("tds_route_progress_bwd_multi", g.r, set, scene_map, B, A, route_lanes, route_n, start_arc, end_arc, offsets, length);
    if (rc != TDS_OK) return rc;
    TDS_CHECK_ARG(n_lookahead >= 0 && n_lookahead <= TDS_ROUTE_MAX_LOOKAHEAD, "tds_route_progress_bwd_multi: %d lookahead points, at most %d", n_lookahead,
                  TDS_ROUTE_MAX_LOOKAHEAD);
    TDS_CHECK_ARG(tds::ok_param(spacing), "tds_route_progress_bwd_multi: spacing must be finite and not negative");
    TDS_CHECK_ARG(xy_stride >= 2, "tds_route_progress_bwd_multi: xy_stride %lld is less than 2", (long long)xy_stride);
    if (g.r.rows == 0) return TDS_OK;
    TDS_CHECK_ARG(xy && sc && piece && g_xy && g_sc, "tds_route_progress_bwd_multi: null argument");
    g.xy = xy, g.sc = sc, g.xy_stride = xy_stride, g.present = present, g.piece = piece;
    g.g_progress = g_progress, g.g_advance = g_advance, g.g_lateral = g_lateral, g.g_heading = g_heading, g.g_remaining = g_remaining;
    g.g_lookahead = n_lookahead > 0 ? g_lookahead : nullptr;
    g.spacing = spacing, g.K = n_lookahead, g.g_xy = g_xy, g.g_sc = g_sc;
    const int per = RBLOCK / 64;
    hipLaunchKernelGGL(route_progress_bwd_kernel, dim3((unsigned)((g.r.rows + per - 1) / per)), dim3(RBLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("route_progress_bwd_kernel");
    return TDS_OK;
}

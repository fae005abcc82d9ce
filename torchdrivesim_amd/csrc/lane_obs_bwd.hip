// K8b: the backward of the lane observations (_ops.lane_observations_grad; include/tdship.h "K8b"): the gradients of the slots'
// features and polyline points to x, y and [sin, cos] of the observing agent, one launch.  The map is constant, so there is no gather across
// entities.  Yardstick: the float64 torch-autograd model tests/lane_obs_grad_model.py; the contributions of a slot and of a point are stated
// once, in tds_lane_obs_grad.h.
// K8's own shape: one wave per observer, four per workgroup; no workgroup barrier, no LDS -- the waves share nothing, and what the pairs of a
// slot need of its foot they fetch from lane k by a shuffle.  There is no key phase: the selection is given by `index`.  Two phases per wave:
//   slots    for each filled slot the wave finds the foot again with tds::wave_foot -- K8's arithmetic, K8's sb -- and lane k keeps slot k's
//            lanelet and sb; then the K lanes work side by side, each on its own slot: the foot on sb, the arc, the slide a and the
//            contributions of the eight features (in the loop they would take turns, and their registers would cost a wave of occupancy);
//   points   the K x P (slot, point) pairs spread over the lanes exactly as in K8, each redoing the walk (tds::lane_point) and adding its
//            contribution to the lane's four binary64 sums.
// Then a butterfly over the 64 lanes in a fixed order, and lane 0 rounds to binary32 and stores the two float2s.  No atomics.
#include "tds_lane_obs.h"
#include "tds_lane_obs_grad.h"

namespace {

using tds::LaneRec;
using tds::LaneView;

constexpr int LB_BLOCK = 256;           // 4 waves = 4 observers
constexpr int LB_WAVES = LB_BLOCK / 64;

struct LaneObsBwdArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const float *xy, *sc;
    const int32_t *index;
    const float *g_features, *g_points;     // either may be null: all zero
    float *g_xy, *g_sc;
    int64_t n_obs;
    int A, K, P;
    double spacing;
};

// grid = ceil(n_obs / LB_WAVES)
__global__ void __launch_bounds__(LB_BLOCK) lane_obs_bwd_kernel(LaneObsBwdArgs g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t o = (int64_t)blockIdx.x * LB_WAVES + wave;
    if (o >= g.n_obs) return;                                       // whole waves leave; nothing below waits for another wave
    const int K = g.K, P = g.P;
    const int64_t row = o * K;
    const double x = (double)g.xy[2 * o], y = (double)g.xy[2 * o + 1];
    const double s = (double)g.sc[2 * o], c = (double)g.sc[2 * o + 1];
    LaneView v{};
    bool live = x == x && y == y && s == s && c == c;               // K8's rule: a NaN pose has an empty row
    live = live && tds::view_of(g.views, g.n_views, g.scene_map, o / g.A, v);       // wave-uniform: all 64 lanes stay together below
    double sum[tds::LG_GRADS] = {0.0, 0.0, 0.0, 0.0};
    double part[tds::LG_GRADS];

    // ---- slots: the wave finds the foot of every filled slot again, lane k keeps slot k
    int mine = -1, seg = 0;                                         // (lanes below K) the lanelet of slot `lane`, -1 for one that is not filled, and sb
    double arc = 0.0;
    tds::LaneSlide slide = {0.0, 0.0};
    if (live) {
        for (int k = 0; k < K; ++k) {                               // wave-uniform
            const int l = __builtin_amdgcn_readfirstlane(g.index[row + k]);
            if (l < 0 || l >= v.n) continue;                        // empty, or garbage: nothing is read at it
            const LaneRec r = v.rec[l];
            if (!tds::usable(v, l, r)) continue;
            int sb;
            double d2;
            if (!tds::wave_foot(v, r, x, y, lane, sb, d2) || lane != k) continue;
            mine = l, seg = sb;
        }
    }
    if (mine >= 0) {                                                // lane k on its own: slot k's features
        const LaneRec r = v.rec[mine];
        const double *cum = v.cum + r.cl_start;
        const tds::SegmentFoot f = tds::segment_foot(v.cl + 3 * (int64_t)r.cl_start, seg, x, y);
        const tds::Unit2 t = tds::segment_unit(f);
        arc = tds::foot_arc(f, cum, seg);
        double gin[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (g.g_features) {
            const float4 lo = *(const float4 *)(g.g_features + (row + lane) * 8), hi = *(const float4 *)(g.g_features + (row + lane) * 8 + 4);
            gin[0] = (double)lo.x, gin[1] = (double)lo.y, gin[2] = (double)lo.z, gin[3] = (double)lo.w;
            gin[4] = (double)hi.x, gin[5] = (double)hi.y, gin[6] = (double)hi.z, gin[7] = (double)hi.w;
        }
        slide = tds::lane_obs_slot_grad(f, t, cum[seg + 1] - cum[seg], x, y, s, c, gin, part);
        if (g.g_features) {
#pragma unroll
            for (int i = 0; i < tds::LG_GRADS; ++i) sum[i] = sum[i] + part[i];
        }
    }

    // ---- points: pair = slot * P + point, 64 pairs at a time; every lane takes part in the shuffles
    const int pairs = K * P;
    if (g.g_points) {
        for (int p0 = 0; p0 < pairs; p0 += 64) {                    // wave-uniform
            const int pair = p0 + lane;
            const bool has = pair < pairs;
            const int k = has ? pair / P : 0, j = pair - k * P;     // (k < K <= 32: a lane of this wave)
            const int cur = __shfl(mine, k, 64);
            const double from = __shfl(arc, k, 64);
            tds::LaneSlide a;
            a.x = __shfl(slide.x, k, 64), a.y = __shfl(slide.y, k, 64);
            tds::LanePoint p;
            if (has && cur >= 0 && tds::lane_point(v, cur, from + (double)j * g.spacing, x, y, p)) {     // (an invalid point: its gradient is not read)
                const float2 gp = *(const float2 *)(g.g_points + (row * P + pair) * 2);
                tds::lane_obs_point_grad(a, p.ex, p.ey, p.hx, p.hy, s, c, (double)gp.x, (double)gp.y, part);
#pragma unroll
                for (int i = 0; i < tds::LG_GRADS; ++i) sum[i] = sum[i] + part[i];
            }
        }
    }

#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {                              // a butterfly over the 64 lanes: the same order of additions every run
#pragma unroll
        for (int i = 0; i < tds::LG_GRADS; ++i) sum[i] = sum[i] + __shfl_xor(sum[i], m, 64);
    }
    if (lane == 0) {                                                // the whole row, zeros included
        *(float2 *)(g.g_xy + 2 * o) = make_float2((float)sum[tds::LG_X], (float)sum[tds::LG_Y]);
        *(float2 *)(g.g_sc + 2 * o) = make_float2((float)sum[tds::LG_SIN], (float)sum[tds::LG_COS]);
    }
}

}  // namespace

TDS_EXPORT int tds_lane_observations_bwd_multi(const tds_laneset_t *set, const int32_t *scene_map, const float *agent_xy, const float *agent_sc,
                                               const int32_t *index, const float *g_features, const float *g_points, float *g_xy, float *g_sc,
                                               int64_t B, int64_t A, int K, int P, float spacing, void *stream) {
    const char *what = "tds_lane_observations_bwd_multi";
    TDS_CHECK_ARG(set, "%s: the lane-table set is null", what);
    TDS_CHECK_ARG(B >= 0 && A >= 0 && A < ((int64_t)1 << 31) && (A == 0 || B <= (((int64_t)1 << 31) - 1) / A), "%s: bad sizes B=%lld A=%lld", what,
                  (long long)B, (long long)A);
    TDS_CHECK_ARG(K >= 1 && K <= TDS_LANE_OBS_MAX_K, "%s: K must be 1 .. %d (got %d)", what, TDS_LANE_OBS_MAX_K, K);
    TDS_CHECK_ARG(P >= 1 && P <= TDS_LANE_OBS_MAX_POINTS, "%s: P must be 1 .. %d (got %d)", what, TDS_LANE_OBS_MAX_POINTS, P);
    TDS_CHECK_ARG(spacing > 0.0f && spacing < INFINITY, "%s: spacing must be finite and positive (got %g)", what, (double)spacing);
    TDS_CHECK_SCENE_MAP(what, set, scene_map);
    if (set->max_lanelets > TDS_LANE_OBS_MAX_LANELETS) {
        tds::set_error("%s: a lane table of %d lanelets (K8 takes at most %d)", what, set->max_lanelets, TDS_LANE_OBS_MAX_LANELETS);
        return TDS_ELIMIT;
    }
    if (B * A == 0) return TDS_OK;
    TDS_CHECK_ARG(agent_xy && agent_sc && index && g_xy && g_sc, "%s: null pointer", what);
    LaneObsBwdArgs g{};
    g.views = set->d_views, g.n_views = set->n, g.scene_map = scene_map;
    g.xy = agent_xy, g.sc = agent_sc, g.index = index;
    g.g_features = g_features, g.g_points = g_points, g.g_xy = g_xy, g.g_sc = g_sc;
    g.n_obs = B * A, g.A = (int)A, g.K = K, g.P = P;
    g.spacing = (double)spacing;
    hipLaunchKernelGGL(lane_obs_bwd_kernel, dim3((unsigned)((g.n_obs + LB_WAVES - 1) / LB_WAVES)), dim3(LB_BLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("lane_obs_bwd_kernel");
    return TDS_OK;
}

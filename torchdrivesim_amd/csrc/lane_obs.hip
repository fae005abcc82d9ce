// K8: lane observations (Simulator.compute_lanes).  For every exposed agent the K nearest lanelets of its scene's lane table within
// max_distance of their centre lines, nearest first, each as the foot point in the observer's frame plus a polyline of P points ahead that
// follows the lane graph while the way is unambiguous.  No reference counterpart: the definition is this project's own (include/tdship.h
// "K8"; float64 model, bit for bit: tests/lane_obs_model.py).
// One wave per observer, four per workgroup; no workgroup barrier anywhere, the waves do not share anything.  Three phases per wave:
//   keys     64 lanelets at a time, a lane each: rejected by the record's box grown by max_distance or for not being usable; the ballot of those
//            left is walked by the WHOLE wave, which splits the segments of one centre line between its lanes (tds::segment_foot, the one
//            tds_lane_snap uses) and takes the wave-wide minimum of (d2, segment): centre lines are long (Town01: 51 points on average, up to 123)
//            and few lanelets pass the box, so a lane per lanelet would leave most lanes idle behind the longest line.  The key is the bits of (float)d2;
//   select   the K smallest (key, lanelet) by tds_select.h: by rank among the candidate lanes up to 64 lanelets, in K rounds of a wave-wide
//            minimum over the keys in the wave's LDS row above.  The winners go to the wave's LDS slots; the wave then finds the foot of every
//            filled slot AGAIN (the same arithmetic: the same bits) -- no (segment, u) per candidate is kept anywhere -- and lane k writes slot k;
//   points   the K x P (slot, point) pairs spread over the lanes, each pair walking from its slot's lanelet over at most TDS_LANE_OBS_MAX_HOPS
//            unique successors to its own arc length; n_valid is counted from the wave's ballots of the valid pairs.
// Lane-table arithmetic is binary64, every operation rounded once (-ffp-contract=off); every output float is the double rounded once.
#include "tds_lane_obs.h"
#include "tds_select.h"

namespace {

using tds::LaneRec;
using tds::LaneView;
using tds::NO_KEY;
using tds::usable;       // (tds_lane_obs.h: what K8 shares with its backward)
using tds::wave_foot;

constexpr int LO_BLOCK = 256;           // 4 waves = 4 observers
constexpr int LO_WAVES = LO_BLOCK / 64;
constexpr int LO_MAX_K = TDS_LANE_OBS_MAX_K;
constexpr double LO_BOX_MARGIN = 1e-3;  // metres the box test is generous by: a centre line is made of midpoints of the outline's points, so it lies
                                        // in the outline's box but for a rounding, and so does a foot on it; the test must never drop a candidate

struct LaneObsArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const float *xy, *sc;
    const uint8_t *present;
    float *features, *points;
    int32_t *n_valid, *index;
    int64_t n_obs;
    int A, K, P, key_stride;
    double spacing, reach, r2;          // reach = max_distance + LO_BOX_MARGIN, r2 = max_distance^2
};

// whether lanelet l can be a candidate in range at all, before its centre line is touched: inside the record's box grown by `reach`, and usable
__device__ __forceinline__ bool worth_a_look(const LaneView &v, int l, double x, double y, double reach) {
    const LaneRec r = v.rec[l];
    if (x < (double)r.bx0 - reach || x > (double)r.bx1 + reach || y < (double)r.by0 - reach || y > (double)r.by1 + reach) return false;
    return usable(v, l, r);
}

// grid = ceil(n_obs / LO_WAVES); dynamic LDS = LO_WAVES * key_stride words of keys when a table has more than 64 lanelets, else none
__global__ void __launch_bounds__(LO_BLOCK) lane_obs_kernel(LaneObsArgs g) {
    extern __shared__ uint32_t lo_keys[];
    __shared__ int32_t s_item[LO_WAVES][LO_MAX_K];                  // per wave: the lanelet of slot k, -1 for an empty slot
    __shared__ double s_arc[LO_WAVES][LO_MAX_K];                    // ... and the arc length of its foot
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t o = (int64_t)blockIdx.x * LO_WAVES + wave;
    if (o >= g.n_obs) return;                                       // whole waves leave; nothing below waits for another wave
    const int K = g.K, P = g.P;
    const int64_t row = o * K;
    const double x = (double)g.xy[2 * o], y = (double)g.xy[2 * o + 1];
    const double s = (double)g.sc[2 * o], c = (double)g.sc[2 * o + 1];
    LaneView v{};
    bool live = g.present[o] != 0 && x == x && y == y && s == s && c == c;
    live = live && tds::view_of(g.views, g.n_views, g.scene_map, o / g.A, v);   // wave-uniform: all 64 lanes stay together below
    int32_t *item = s_item[wave];
    double *arcs = s_arc[wave];

    // ---- keys and selection
    if (live) {
        const int L = v.n;
        uint32_t *wk = lo_keys + (size_t)wave * g.key_stride;       // (L > 64 only) this wave's row of d2 bits
        uint32_t key = NO_KEY;                                      // (L <= 64 only) the d2 bits of lanelet `lane`
        for (int l0 = 0; l0 < L; l0 += 64) {                        // 64 lanelets at a time: a lane each for the box, then the wave for each one left
            const int mine = l0 + lane;
            uint64_t look = __ballot(mine < L && worth_a_look(v, mine, x, y, g.reach));
            if (L > 64 && mine < L) wk[mine] = NO_KEY;
            for (; look != 0; look &= look - 1) {                   // wave-uniform
                const int l = l0 + __builtin_ctzll(look);
                const LaneRec r = v.rec[l];
                int sb;
                double d2;
                if (!wave_foot(v, r, x, y, lane, sb, d2) || !(d2 <= g.r2)) continue;
                if (mine == l) {
                    key = __float_as_uint((float)d2);
                    if (L > 64) wk[l] = key;
                }
            }
        }
        const auto store = [&](int k, int l) { item[k] = l; };
        if (L <= 64) {
            tds::select_by_rank(key, lane, K, store);
        } else {
            tds::order_lds();
            tds::select_by_rounds(wk, L, lane, K, [&](int l) { return wk[l]; }, store);
        }
    } else if (lane < K) {
        item[lane] = -1;
    }
    tds::order_lds();

    // ---- features: the wave finds the foot of every filled slot again, lane k writes slot k
    {
        float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
        double arc = 0.0;
        int mine = -1;
        for (int k = 0; k < K; ++k) {                               // wave-uniform
            const int l = item[k];
            if (l < 0) continue;
            const LaneRec r = v.rec[l];
            int sb;
            double d2;
            if (!wave_foot(v, r, x, y, lane, sb, d2) || lane != k) continue;    // (a winner has a foot: the same arithmetic found it before)
            const double *cum = v.cum + r.cl_start;
            const tds::SegmentFoot f = tds::segment_foot(v.cl + 3 * (int64_t)r.cl_start, sb, x, y);
            const tds::Unit2 t = tds::segment_unit(f);
            arc = tds::foot_arc(f, cum, sb);
            lo = make_float4((float)(f.fx * c + f.fy * s), (float)(f.fy * c - f.fx * s), (float)(t.y * c - t.x * s), (float)(t.x * c + t.y * s));
            hi = make_float4((float)arc, (float)(cum[r.cl_n - 1] - arc), (float)tds::foot_lateral(f, t, x, y), (float)sqrt(f.d2));
            mine = l;
        }
        tds::order_lds();
        if (lane < K) {
            float4 *out = (float4 *)(g.features + (row + lane) * 8);
            out[0] = lo;
            out[1] = hi;
            g.index[row + lane] = mine;
            item[lane] = mine;
            arcs[lane] = arc;
        }
    }
    tds::order_lds();

    // ---- points: pair = slot * P + point, 64 pairs at a time; every lane takes part in the ballot
    const int pairs = K * P;
    int nv = 0;                                                      // (lanes below K) the valid points of slot `lane`
    for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int pair = p0 + lane;
        bool valid = false;
        float2 pt = make_float2(0.0f, 0.0f);
        if (pair < pairs) {
            const int k = pair / P, j = pair - k * P;
            const int cur = item[k];
            if (cur >= 0) {
                tds::LanePoint p;
                valid = tds::lane_point(v, cur, arcs[k] + (double)j * g.spacing, x, y, p);       // at most TDS_LANE_OBS_MAX_HOPS hops
                if (valid) pt = make_float2((float)(p.ex * c + p.ey * s), (float)(p.ey * c - p.ex * s));
            }
            *(float2 *)(g.points + ((row * P) + pair) * 2) = pt;
        }
        const uint64_t mask = __ballot(valid);
        if (lane < K) {                                              // the pairs of slot `lane` in this round: [lane * P, lane * P + P) - p0
            const int b0 = max(lane * P - p0, 0), b1 = min(lane * P + P - p0, 64);
            if (b1 > b0) nv += __popcll((mask >> b0) & (b1 - b0 == 64 ? ~(uint64_t)0 : (((uint64_t)1 << (b1 - b0)) - 1)));
        }
    }
    if (lane < K) g.n_valid[row + lane] = nv;
}

}  // namespace

TDS_EXPORT int tds_lane_observations_multi(const tds_laneset_t *set, const int32_t *scene_map, const float *agent_xy, const float *agent_sc,
                                           const uint8_t *present, float *features, float *points, int32_t *n_valid, int32_t *index, int64_t B,
                                           int64_t A, int K, int P, float spacing, float max_distance, void *stream) {
    const char *what = "tds_lane_observations_multi";
    TDS_CHECK_ARG(set, "%s: the lane-table set is null", what);
    TDS_CHECK_ARG(B >= 0 && A >= 0 && A < ((int64_t)1 << 31) && (A == 0 || B <= (((int64_t)1 << 31) - 1) / A), "%s: bad sizes B=%lld A=%lld", what,
                  (long long)B, (long long)A);
    TDS_CHECK_ARG(K >= 1 && K <= TDS_LANE_OBS_MAX_K, "%s: K must be 1 .. %d (got %d)", what, TDS_LANE_OBS_MAX_K, K);
    TDS_CHECK_ARG(P >= 1 && P <= TDS_LANE_OBS_MAX_POINTS, "%s: P must be 1 .. %d (got %d)", what, TDS_LANE_OBS_MAX_POINTS, P);
    TDS_CHECK_ARG(spacing > 0.0f && spacing < INFINITY, "%s: spacing must be finite and positive (got %g)", what, (double)spacing);
    TDS_CHECK_ARG(max_distance >= 0.0f, "%s: max_distance must not be negative or NaN (got %g)", what, (double)max_distance);
    TDS_CHECK_SCENE_MAP(what, set, scene_map);
    if (set->max_lanelets > TDS_LANE_OBS_MAX_LANELETS) {
        tds::set_error("%s: a lane table of %d lanelets (the keys of a table live in LDS, a row per wave: at most %d)", what, set->max_lanelets,
                       TDS_LANE_OBS_MAX_LANELETS);
        return TDS_ELIMIT;
    }
    if (B * A == 0) return TDS_OK;
    TDS_CHECK_ARG(agent_xy && agent_sc && present && features && points && n_valid && index, "%s: null pointer", what);
    LaneObsArgs g{};
    g.views = set->d_views, g.n_views = set->n, g.scene_map = scene_map;
    g.xy = agent_xy, g.sc = agent_sc, g.present = present;
    g.features = features, g.points = points, g.n_valid = n_valid, g.index = index;
    g.n_obs = B * A, g.A = (int)A, g.K = K, g.P = P;
    g.key_stride = set->max_lanelets > 64 ? set->max_lanelets : 0;
    g.spacing = (double)spacing;
    g.reach = (double)max_distance + LO_BOX_MARGIN;
    g.r2 = (double)max_distance * (double)max_distance;
    const size_t lds = (size_t)LO_WAVES * g.key_stride * sizeof(uint32_t);
    hipLaunchKernelGGL(lane_obs_kernel, dim3((unsigned)((g.n_obs + LO_WAVES - 1) / LO_WAVES)), dim3(LO_BLOCK), lds, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("lane_obs_kernel");
    return TDS_OK;
}

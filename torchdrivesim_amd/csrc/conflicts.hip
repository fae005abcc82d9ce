// Giving way at junctions: the per-map conflict table and the per-step yield pass.
//
// No reference counterpart.  The definition is this library's own (include/tdship.h "Giving way at junctions"); its yardstick is the float64
// model tests/give_way_model.py, which restates every expression in the same order.  The expressions themselves are in tds_conflicts.h.
//
// tds_lane_conflicts_f64 builds, once per lane table, for every ordered pair of lanelets (a, b) the last arc of a's centre line that lies
// within the clearance of b's: one workgroup per lanelet a, the lanelets excluded for it (itself, successors, predecessors, siblings) as
// bytes in LDS, a wave per candidate b, the lanes of the wave over a's samples.  tds_lane_give_way_multi decides per step who stops before which
// junction: one workgroup per scene, a thread per NPC, the NPCs' summaries in LDS, one barrier, no atomics.
//
// Arithmetic: float64, + - * / sqrt only (-ffp-contract=off).
#include <math.h>

#include "tds_common.h"
#include "tds_conflicts.h"
#include "tds_lanes.h"

using tds::LaneRec;
using tds::LaneView;
using tds::drivable;

namespace {

constexpr int CBLOCK = 256;                      // the table kernel's workgroup: four waves, each on a lanelet b of its own
constexpr int CWAVES = CBLOCK / 64;
constexpr int CONFLICT_LANELETS = TDS_CONFLICT_MAX_LANELETS;
constexpr int GIVE_WAY_NPCS = TDS_GIVE_WAY_MAX_NPCS;
constexpr int SUMMARY_BYTES = 3 * 8 + 4 + 1;     // LDS per NPC of the yield pass: start, t, half length (doubles), junction (int), flags (byte)

__device__ inline double length_of(const LaneView &v, int l) { return v.cum[v.rec[l].cl_start + v.rec[l].cl_n - 1]; }

// nothing of b can lie within the clearance of anything of a: the outlines' boxes (rounded outwards, and a centre line lies inside its
// outline) are further apart than the clearance and a millimetre.  A box that is no number rejects nothing.
__device__ inline bool boxes_apart(const LaneRec &a, const LaneRec &b, double clearance) {
    const double far = clearance + 1e-3;
    return (double)a.bx0 - (double)b.bx1 > far || (double)b.bx0 - (double)a.bx1 > far || (double)a.by0 - (double)b.by1 > far ||
           (double)b.by0 - (double)a.by1 > far;
}

// ---- the table: a workgroup per lanelet a -------------------------------------------------------------------------------------------------
// table = exit (L x L), zone_in (L), zone_out (L).  Loops: L / CBLOCK lanelets per thread and their successor lists (marking), L / CWAVES lanelets
// per wave, (last_sample + 1) / 64 samples per lane, the segments of b per sample.
__global__ void __launch_bounds__(CBLOCK) lane_conflicts_kernel(LaneView v, double *table, double clearance, double step) {
    __shared__ uint8_t excluded[CONFLICT_LANELETS];
    __shared__ double wave_in[CWAVES], wave_out[CWAVES];
    const int a = blockIdx.x, tid = threadIdx.x, lane_id = tid & 63, wave = tid >> 6, L = v.n;
    const bool a_ok = drivable(v, a);
    for (int l = tid; l < L; l += CBLOCK) excluded[l] = 0;
    __syncthreads();
    if (a_ok) {                                                              // every store writes a 1: the order does not matter
        for (int p = tid; p < L; p += CBLOCK) {
            const int s0 = v.succ_start[p], s1 = v.succ_start[p + 1];
            bool parent = false;
            for (int i = s0; i < s1; ++i) parent |= v.succ_items[i] == a;
            if (parent) excluded[p] = 1;                                     // a is a successor of p
            if (parent || p == a)                                            // a's siblings (a among them), a's successors
                for (int i = s0; i < s1; ++i) {
                    const int s = v.succ_items[i];
                    if ((unsigned)s < (unsigned)L) excluded[s] = 1;
                }
            if (p == a) excluded[p] = 1;
        }
    }
    __syncthreads();
    const LaneRec ra = v.rec[a];
    const double *cl_a = v.cl + 3 * (int64_t)ra.cl_start, *cum_a = v.cum + ra.cl_start;
    const int last = a_ok ? tds::last_sample(cum_a[ra.cl_n - 1], step) : -1;
    const double c2 = clearance * clearance;
    double zin = INFINITY, zout = -1.0;
    for (int b = wave; b < L; b += CWAVES) {                                 // wave-uniform
        double exit_ab = -1.0;
        if (a_ok && !excluded[b] && drivable(v, b)) {
            const LaneRec rb = v.rec[b];
            if (!boxes_apart(ra, rb, clearance)) {
                const double *cl_b = v.cl + 3 * (int64_t)rb.cl_start;
                int first = 0x7fffffff, last_hit = -1;
                for (int k = lane_id; k <= last; k += 64)
                    if (tds::sample_hit(cl_a, cum_a, ra.cl_n, k, step, cl_b, rb.cl_n, c2)) {
                        if (k < first) first = k;
                        last_hit = k;
                    }
#pragma unroll
                for (int m = 32; m > 0; m >>= 1) {
                    first = min(first, __shfl_xor(first, m));
                    last_hit = max(last_hit, __shfl_xor(last_hit, m));
                }
                if (last_hit >= 0) {
                    exit_ab = tds::sample_arc(last_hit, step);
                    zin = fmin(zin, tds::sample_arc(first, step)), zout = fmax(zout, exit_ab);
                }
            }
        }
        if (lane_id == 0) table[(int64_t)a * L + b] = exit_ab;
    }
    if (lane_id == 0) wave_in[wave] = zin, wave_out[wave] = zout;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < CWAVES; ++w) zin = fmin(zin, wave_in[w]), zout = fmax(zout, wave_out[w]);
        table[(int64_t)L * L + a] = zin;
        table[(int64_t)L * L + L + a] = zout;
    }
}

// ---- the yield pass: a workgroup per scene, a thread per NPC ---------------------------------------------------------------------------------
struct GiveWayArgs {
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const int64_t *scene_ids;
    const int64_t *tables;                       // per view: the address of its conflict table, 0 without one
    int N, S;
    const int32_t *lane, *hops;
    const double *arc;
    const float *state, *npc_size;
    const uint8_t *present;
    const int32_t *line_lane;
    const double *line_arc;
    const uint8_t *line_red;
    double *stop_at;
    int32_t *yield_to;
    uint32_t key0, key1;
    double horizon, b_max, creep_speed;
};

// blockDim.x = N rounded up to whole waves; dynamic LDS = blockDim.x * SUMMARY_BYTES.  Loops: at most TDS_FOLLOW_MAX_HOPS + 1 lanelets of the
// path with S stop lines each (phase 1), N contenders (phase 2).
__global__ void __launch_bounds__(GIVE_WAY_NPCS) lane_give_way_kernel(GiveWayArgs g) {
    extern __shared__ __attribute__((aligned(16))) double summary[];
    const int i = threadIdx.x, n_pad = blockDim.x, N = g.N;
    double *s_start = summary, *s_t = summary + n_pad, *s_half = summary + 2 * n_pad;
    int *s_junction = (int *)(summary + 3 * n_pad);
    uint8_t *s_flags = (uint8_t *)(s_junction + n_pad);                      // bit 0: committed, bit 1: held
    const int64_t scene = blockIdx.x, row = scene * N + i;
    const int m = g.scene_map ? g.scene_map[scene] : 0;
    const bool mapped = m >= 0 && m < g.n_views;
    const double *table = mapped ? (const double *)g.tables[m] : nullptr;
    LaneView v = {};
    if (mapped) v = g.views[m];
    const int64_t L = v.n;

    // ---- phase 1: the junction on this NPC's path -----------------------------------------------------------------------------------------
    int junction = -1;
    double start_j = 0.0, half = 0.0;
    tds::Approach ap = {INFINITY, INFINITY, INFINITY, false};
    bool held = false;
    if (i < N && table && g.present[row] && drivable(v, g.lane[row])) {
        const uint64_t sid = g.scene_ids ? (uint64_t)g.scene_ids[scene] : (uint64_t)scene;
        const double *zone_in = table + L * L, *zone_out = zone_in + L;
        const double vel = (double)g.state[row * 4 + 3];
        const int hops0 = g.hops[row];
        half = (double)g.npc_size[row * 2] / 2.0;
        int l = g.lane[row];
        double start = -g.arc[row], red = INFINITY;
        for (int k = 0; k <= TDS_FOLLOW_MAX_HOPS; ++k) {
            for (int s = 0; s < g.S; ++s) {
                const int64_t e = scene * g.S + s;
                if (g.line_red[e] && g.line_lane[e] == l) red = tds::nearest_red_line(start + g.line_arc[e], red);
            }
            const double zi = zone_in[l], zo = zone_out[l];
            if (tds::is_junction(start, zi, zo, half, g.horizon)) {
                junction = l, start_j = start;
                ap = tds::approach(start, zi, half, vel, g.b_max, g.creep_speed);
                held = tds::is_held(ap.committed, red, start, zo);
                break;
            }
            const double next_start = start + length_of(v, l);
            if (next_start >= g.horizon || k == TDS_FOLLOW_MAX_HOPS) break;
            const int nxt = tds::successor_draw(v, l, sid, i, hops0 + k, g.key0, g.key1);
            if (!drivable(v, nxt)) break;
            l = nxt, start = next_start;
        }
    }
    s_start[i] = start_j, s_t[i] = ap.t, s_half[i] = half, s_junction[i] = junction;
    s_flags[i] = (uint8_t)((ap.committed ? 1 : 0) | (held ? 2 : 0));
    __syncthreads();
    if (i >= N) return;

    // ---- phase 2: the first contender this NPC gives way to ---------------------------------------------------------------------------------
    double stop = INFINITY;
    int who = -1;
    if (junction >= 0 && !ap.committed) {
        for (int j = 0; j < N; ++j) {
            const int q = s_junction[j];
            const int f = s_flags[j];
            if (j == i || q < 0 || (f & 2)) continue;
            if (tds::gives_way(table[q * L + junction], table[junction * L + q], s_start[j], s_half[j], f & 1, false, s_t[j], j, ap.t, i)) {
                stop = ap.D, who = j;
                break;
            }
        }
    }
    g.stop_at[row] = stop, g.yield_to[row] = who;
}

}  // namespace

TDS_EXPORT int tds_lane_conflicts_f64(const tds_lanes_t *lanes, double *table, float clearance, float step, void *stream) {
    TDS_CHECK_ARG(lanes, "tds_lane_conflicts_f64: the lane table is null");
    TDS_CHECK_ARG(clearance > 0.f && clearance < INFINITY && step > 0.f && step < INFINITY,
                  "tds_lane_conflicts_f64: clearance and step must be finite and greater than 0 (got %g, %g)", (double)clearance, (double)step);
    const int L = lanes->view.n;
    if (L > TDS_CONFLICT_MAX_LANELETS) {
        tds::set_error("tds_lane_conflicts_f64: %d lanelets exceed the %d whose exclusions a workgroup holds in LDS", L, TDS_CONFLICT_MAX_LANELETS);
        return TDS_ELIMIT;
    }
    TDS_CHECK_ARG(lanes->view.succ_start, "tds_lane_conflicts_f64: the lane table has no successor graph (tds_lanes_set_successors)");
    if (L == 0) return TDS_OK;
    TDS_CHECK_ARG(table, "tds_lane_conflicts_f64: table is null");
    hipLaunchKernelGGL(lane_conflicts_kernel, dim3((unsigned)L), dim3(CBLOCK), 0, (hipStream_t)stream, lanes->view, table, (double)clearance, (double)step);
    TDS_LAUNCH_CHECK("lane_conflicts_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_lane_give_way_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, const int64_t *tables, int64_t B,
                                       int64_t N, const int32_t *lane, const double *arc, const int32_t *hops, const float *state, const float *npc_size,
                                       const uint8_t *npc_present, int64_t S, const int32_t *line_lane, const double *line_arc, const uint8_t *line_red,
                                       uint64_t seed, float horizon, float b_max, float creep_speed, double *stop_at, int32_t *yield_to, void *stream) {
    TDS_CHECK_ARG(set, "tds_lane_give_way_multi: the lane-table set is null");
    TDS_CHECK_SCENE_MAP("tds_lane_give_way_multi", set, scene_map);
    TDS_CHECK_ARG(B >= 0 && N >= 0 && S >= 0 && B < ((int64_t)1 << 31) && S < ((int64_t)1 << 31), "tds_lane_give_way_multi: bad sizes B=%lld N=%lld S=%lld",
                  (long long)B, (long long)N, (long long)S);
    if (N > TDS_GIVE_WAY_MAX_NPCS) {
        tds::set_error("tds_lane_give_way_multi: %lld NPCs exceed the %d of a scene's workgroup", (long long)N, TDS_GIVE_WAY_MAX_NPCS);
        return TDS_ELIMIT;
    }
    TDS_CHECK_ARG(tds::ok_param(horizon) && tds::ok_param(b_max), "tds_lane_give_way_multi: horizon and b_max must be finite and not negative");
    TDS_CHECK_ARG(creep_speed > 0.f && creep_speed < INFINITY, "tds_lane_give_way_multi: creep_speed must be finite and greater than 0 (got %g)",
                  (double)creep_speed);
    if (B == 0 || N == 0) return TDS_OK;
    TDS_CHECK_ARG(tables && lane && arc && hops && state && npc_size && npc_present && stop_at && yield_to, "tds_lane_give_way_multi: null argument");
    TDS_CHECK_ARG(S == 0 || (line_lane && line_arc && line_red), "tds_lane_give_way_multi: %lld stop lines without their arrays", (long long)S);
    GiveWayArgs g = {};
    g.views = set->d_views, g.n_views = set->n, g.scene_map = scene_map, g.scene_ids = scene_ids, g.tables = tables;
    g.N = (int)N, g.S = (int)S;
    g.lane = lane, g.hops = hops, g.arc = arc, g.state = state, g.npc_size = npc_size, g.present = npc_present;
    g.line_lane = line_lane, g.line_arc = line_arc, g.line_red = line_red, g.stop_at = stop_at, g.yield_to = yield_to;
    // the follow kernel's route stream, so that the successors drawn here are the ones it will take
    g.key0 = (uint32_t)seed ^ 0x4C414E45u, g.key1 = (uint32_t)(seed >> 32) ^ 0x464F4C57u;
    g.horizon = horizon, g.b_max = b_max, g.creep_speed = creep_speed;
    const unsigned block = (unsigned)((N + 63) / 64 * 64);
    hipLaunchKernelGGL(lane_give_way_kernel, dim3((unsigned)B), dim3(block), (size_t)block * SUMMARY_BYTES, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("lane_give_way_kernel");
    return TDS_OK;
}

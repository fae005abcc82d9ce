// Lane-following NPC traffic: the Intelligent Driver Model on the lane graph, one launch per step.
//
// No reference counterpart: the reference's only reactive NPC controller is an HTTP client.  The definition is this library's own; its
// yardstick is the float64 model tests/lane_follow_model.py, which restates every expression below in the same order.
//
// One wavefront per NPC, four NPCs of ONE scene per workgroup (two when a scene has more than 480 entities: the LDS of a workgroup
// stays within the 64 KiB a launch gets without asking for more).  LDS (dynamic): the scene's entities, eight floats each (x, y, length, width,
// sin, cos, speed, present), loaded once by the workgroup; then per wave up to FOLLOW_MAX_PIECES pieces of the NPC's path, six doubles
// each (start point, unit vector, 2-D length, path distance at its start), and 64 ints for the entities in reach.  The lanes of a wave first split
// the segments of the path's lanelets (stage), then the entities (keep those in reach), then the 5 points of each kept entity (project), and
// reduce (path distance, point index) with shuffles.
//
// Arithmetic: float64 on the float64 lane table, + - * / sqrt only (-ffp-contract=off); entity coordinates are widened from float32.  The
// one exception is the reported psi, atan2 of the segment's direction; [sin, cos] is that direction's unit vector, as on-lane initialisation has it.
#include <math.h>

#include "tds_common.h"
#include "tds_conflicts.h"
#include "tds_lanes.h"

using tds::LaneRec;
using tds::LaneView;
using tds::order_lds;
using tds::segment_of;

namespace {

constexpr int FBLOCK = 256;                      // at most four waves = four NPCs
constexpr int FOLLOW_MAX_PIECES = 256;           // path segments staged per NPC; a path that needs more ends there (no obstacle)
constexpr int ENT_WORDS = 8;                     // LDS floats per entity
constexpr int PIECE_DOUBLES = 6;
constexpr int NEAR_SLOTS = 64;                   // entities in reach kept per wave before their points are weighed

struct FollowArgs {
    LaneView single;                // the single-map form (views == null)
    const LaneView *views;
    int n_views;
    const int32_t *scene_map;
    const int64_t *scene_ids;
    int N, E;
    const float *boxes, *ent_sc, *ent_speed;
    const uint8_t *ent_present;
    const int32_t *self_index;
    const float *npc_size, *desired_speed;
    const uint8_t *npc_present;
    int32_t *lane, *hops, *leader;
    double *arc;
    float *state, *sc;
    uint32_t key0, key1;
    double dt, horizon, margin, T, s0, a, b, b_max;
    const double *stop_at;          // per NPC or null: where the yield pass (conflicts.hip) has it stop, +inf for nowhere
};

// grid = (B, ceil(N / W)), W = blockDim.x / 64 waves; dynamic LDS = E * ENT_WORDS floats + W * FOLLOW_MAX_PIECES * PIECE_DOUBLES doubles + W * NEAR_SLOTS ints
__global__ void __launch_bounds__(FBLOCK) lane_follow_kernel(FollowArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ent[];
    const int tid = threadIdx.x, lane_id = tid & 63, wave = tid >> 6;
    const int64_t scene = blockIdx.x;
    const int E = g.E;
    for (int j = tid; j < E; j += (int)blockDim.x) {
        const float *bx = g.boxes + (scene * E + j) * 5;
        float *d = ent + j * ENT_WORDS;
        d[0] = bx[0], d[1] = bx[1], d[2] = bx[2], d[3] = bx[3];
        d[4] = g.ent_sc[(scene * E + j) * 2], d[5] = g.ent_sc[(scene * E + j) * 2 + 1];
        d[6] = g.ent_speed[scene * E + j];
        d[7] = g.ent_present[scene * E + j] ? 1.f : 0.f;
    }
    __syncthreads();                                                         // the only workgroup barrier: waves are on their own from here
    const int npc = blockIdx.y * (int)(blockDim.x >> 6) + wave;
    if (npc >= g.N) return;
    const int64_t row = scene * g.N + npc;
    double *pieces = (double *)(ent + (size_t)((E * ENT_WORDS + 3) & ~3)) + (size_t)wave * FOLLOW_MAX_PIECES * PIECE_DOUBLES;
    int cur = g.lane[row];
    LaneView v;
    if (!tds::view_of(g.views, g.n_views, g.scene_map, scene, v, &g.single) || cur < 0 || !g.npc_present[row] || !(g.desired_speed[row] > 0.f)) {      // rows that do not move (v0 must be > 0; NaN is not)
        if (lane_id == 0) g.leader[row] = -1;
        return;
    }
    if (cur >= v.n || v.rec[cur].cl_n < 2) {
        if (lane_id == 0) g.leader[row] = -1;
        return;
    }
    const uint64_t sid = g.scene_ids ? (uint64_t)g.scene_ids[scene] : (uint64_t)scene;
    const double arc0 = g.arc[row];
    const int hops0 = g.hops[row];
    const double vel = (double)g.state[row * 4 + 3];
    const double own_len = (double)g.npc_size[row * 2], own_wid = (double)g.npc_size[row * 2 + 1];
    const int self = g.self_index ? g.self_index[row] : -1;

    // ---- stage the path: the lanelet's segments from the one that holds arc0, then the successors' --------------------------------
    int n_piece = 0;
    double off = 0.0, smin = 0.0;
    bool dead_end = false;
    {
        int l = cur, hop = hops0;
        for (int visited = 0; visited <= TDS_FOLLOW_MAX_HOPS; ++visited) {
            const LaneRec r = v.rec[l];
            const double *cl = v.cl + 3 * (int64_t)r.cl_start, *cum = v.cum + r.cl_start;
            const int n_seg = r.cl_n - 1;
            const int k0 = visited == 0 ? segment_of(cum, r.cl_n, arc0) : 0;
            const int take = min(n_seg - k0, FOLLOW_MAX_PIECES - n_piece);
            for (int i = lane_id; i < take; i += 64) {
                const double *p = cl + 3 * (k0 + i);
                const double dx = p[3] - p[0], dy = p[4] - p[1];
                const double l2 = sqrt(dx * dx + dy * dy);
                double *q = pieces + (size_t)(n_piece + i) * PIECE_DOUBLES;
                q[0] = p[0], q[1] = p[1];
                q[2] = l2 > 0.0 ? dx / l2 : 0.0, q[3] = l2 > 0.0 ? dy / l2 : 0.0;
                q[4] = l2;
            }
            order_lds();
            if (visited == 0) {                                              // where on its first segment the NPC stands
                const tds::ArcPoint p = tds::point_at_arc(cl, cum, k0, arc0);
                smin = p.t * sqrt(p.dx * p.dx + p.dy * p.dy);
            }
            bool full = false;
            for (int i = 0; i < take; ++i) {                                 // the running path distance, front to back (every lane the same)
                double *q = pieces + (size_t)n_piece * PIECE_DOUBLES;
                if (lane_id == 0) q[5] = off;
                off = off + (n_piece == 0 ? q[4] - smin : q[4]);
                n_piece++;
                if (off >= g.horizon) {
                    full = true;
                    break;
                }
            }
            order_lds();
            if (full || take < n_seg - k0 || visited == TDS_FOLLOW_MAX_HOPS) break;
            const int nxt = tds::successor_draw(v, l, sid, npc, hop, g.key0, g.key1);
            if (!tds::drivable(v, nxt)) {                                    // no successor, or one without a centre line to drive on
                dead_end = true;
                break;
            }
            l = nxt, hop++;
        }
    }

    // ---- project the entities' points onto the path -----------------------------------------------------------------------------------
    const double reach = own_wid / 2.0 + g.margin;
    const double reach2 = reach * reach;
    double sx0 = 0.0, sy0 = 0.0;                                             // where the path starts
    if (n_piece > 0) sx0 = pieces[0] + smin * pieces[2], sy0 = pieces[1] + smin * pieces[3];
    double best_d = INFINITY, best_cos = 0.0;
    int best_p = 0x7fffffff;
    // Two passes, so that the loop over the path runs for full waves of points: the lanes first take an entity each and keep the few that are in
    // reach (compacted through LDS, ascending), then split the 5 points of each of those.
    int *near = (int *)(pieces + (size_t)((int)(blockDim.x >> 6) - wave) * FOLLOW_MAX_PIECES * PIECE_DOUBLES) + wave * NEAR_SLOTS;
    int n_near = 0;
    auto weigh = [&](int n) {                                                // the 5 n points of the kept entities against the path
        for (int q0 = lane_id; q0 < 5 * n; q0 += 64) {
            const int j = near[q0 / 5], c = q0 % 5, p = 5 * j + c;
            const float *e = ent + j * ENT_WORDS;
            const double ex = (double)e[0], ey = (double)e[1], hl = (double)e[2] / 2.0, hw = (double)e[3] / 2.0, es = (double)e[4], ec = (double)e[5];
            double px = ex, py = ey;
            if (c > 0) {                                                     // corners 1..4: (+,+), (+,-), (-,-), (-,+) in the box frame
                const double fl = (c == 1 || c == 2) ? hl : -hl, fw = (c == 1 || c == 4) ? hw : -hw;
                px = ex + (fl * ec - fw * es), py = ey + (fl * es + fw * ec);
            }
            double bd2 = INFINITY, bs = 0.0;
            int bi = -1;
            for (int i = 0; i < n_piece; ++i) {
                const double *q = pieces + (size_t)i * PIECE_DOUBLES;
                double s = (px - q[0]) * q[2] + (py - q[1]) * q[3];
                s = fmin(fmax(s, i == 0 ? smin : 0.0), q[4]);
                const double fx = px - (q[0] + s * q[2]), fy = py - (q[1] + s * q[3]);
                const double d2 = fx * fx + fy * fy;
                if (d2 < bd2) bd2 = d2, bs = s, bi = i;
            }
            if (bi < 0 || !(bd2 <= reach2)) continue;
            const double *q = pieces + (size_t)bi * PIECE_DOUBLES;
            const double d = q[5] + (bi == 0 ? bs - smin : bs);
            if (!(d > 0.0)) continue;
            if (d < best_d || (d == best_d && p < best_p)) best_d = d, best_p = p, best_cos = ec * q[2] + es * q[3];
        }
    };
    for (int j0 = 0; j0 < E; j0 += 64) {
        const int j = j0 + lane_id;
        bool in_reach = false;
        if (j < E && j != self) {
            const float *e = ent + j * ENT_WORDS;
            if (e[7] != 0.f) {
                // nothing of an entity this far from the path's start can lie within `reach` of the path (1e-6: far above the rounding of these sums)
                const double far = (off + reach + ((double)e[2] / 2.0 + (double)e[3] / 2.0)) * (1.0 + 1e-6) + 1e-6;
                const double cx = (double)e[0] - sx0, cy = (double)e[1] - sy0;
                in_reach = !(cx * cx + cy * cy > far * far);
            }
        }
        const unsigned long long m = __ballot(in_reach);
        const int c = __popcll(m);
        if (c == 0) continue;
        if (n_near + c > NEAR_SLOTS) {                                       // wave-uniform: the list is full, weigh what it holds
            weigh(n_near);
            n_near = 0;
            order_lds();
        }
        if (in_reach) near[n_near + __popcll(m & ((1ull << lane_id) - 1ull))] = j;
        n_near += c;
        order_lds();
    }
    weigh(n_near);
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        const double od = __shfl_xor(best_d, k);
        const int op = __shfl_xor(best_p, k);
        const double oc = __shfl_xor(best_cos, k);
        if (od < best_d || (od == best_d && op < best_p)) best_d = od, best_p = op, best_cos = oc;
    }

    // ---- IDM (every lane the same numbers; lane 0 writes) -----------------------------------------------------------------------------
    int leader = -1;
    double gap = 0.0, v_lead = 0.0;
    if (best_p != 0x7fffffff) {
        leader = best_p / 5;
        gap = best_d - own_len / 2.0;
        v_lead = (double)ent[leader * ENT_WORDS + 6] * fmax(0.0, best_cos);
    }
    if (dead_end) {
        const double end_gap = off - own_len / 2.0;
        if (leader == -1 || end_gap < gap) leader = -2, gap = end_gap, v_lead = 0.0;
    }
    if (g.stop_at) {                                                         // the junction it gives way at: one more standing obstacle
        double gap_s;
        if (tds::stop_is_nearest(g.stop_at[row], own_len / 2.0, leader, gap, &gap_s)) leader = -3, gap = gap_s, v_lead = 0.0;
    }
    const double v0 = (double)g.desired_speed[row];
    const double r1 = vel / v0, r2 = r1 * r1;
    double acc = 1.0 - r2 * r2;
    if (leader != -1) {
        gap = fmax(gap, 0.1);
        const double s_star = g.s0 + fmax(0.0, vel * g.T + vel * (vel - v_lead) / (2.0 * sqrt(g.a * g.b)));
        const double q = s_star / gap;
        acc = acc - q * q;
    }
    acc = fmax(-g.b_max, g.a * acc);
    float v_new = (float)fmax(0.0, vel + acc * g.dt);
    const double ds = (vel + (double)v_new) / 2.0 * g.dt;

    // ---- move along the lane graph --------------------------------------------------------------------------------------------------
    double arc = arc0 + ds;
    int hops = hops0;
    for (int i = 0; i < TDS_FOLLOW_MAX_HOPS; ++i) {
        const LaneRec r = v.rec[cur];
        const double length = v.cum[r.cl_start + r.cl_n - 1];
        if (!(arc >= length)) break;
        const int nxt = tds::successor_draw(v, cur, sid, npc, hops, g.key0, g.key1);
        if (!tds::drivable(v, nxt)) {                                        // a dead end: stand at the lanelet's end
            arc = length, v_new = 0.f;
            break;
        }
        arc = arc - length, cur = nxt, hops++;
    }
    const LaneRec r = v.rec[cur];
    const double *cl = v.cl + 3 * (int64_t)r.cl_start, *cum = v.cum + r.cl_start;
    const double length = cum[r.cl_n - 1];
    if (!(arc <= length)) arc = length;                                     // more hops in one step than the kernel makes: stop at the end of the last
    const tds::ArcPoint p = tds::point_at_arc(cl, cum, segment_of(cum, r.cl_n, arc), arc);
    const double dx = p.dx, dy = p.dy;
    const double l2 = sqrt(dx * dx + dy * dy);
    if (lane_id != 0) return;
    float *st = g.state + row * 4;
    st[0] = (float)p.x, st[1] = (float)p.y;
    st[2] = l2 > 0.0 ? (float)atan2(dy, dx) : 0.f;
    st[3] = v_new;
    g.sc[row * 2] = l2 > 0.0 ? (float)(dy / l2) : 0.f, g.sc[row * 2 + 1] = l2 > 0.0 ? (float)(dx / l2) : 1.f;
    g.lane[row] = cur, g.arc[row] = arc, g.hops[row] = hops, g.leader[row] = leader;
}

int follow_launch(const char *what, FollowArgs &g, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t N, int64_t E,
                  const float *boxes, const float *ent_sc, const float *ent_speed, const uint8_t *ent_present, const int32_t *self_index,
                  const float *npc_size, const float *desired_speed, const uint8_t *npc_present, int32_t *lane, double *arc, int32_t *hops,
                  float *state, float *sc, int32_t *leader, uint64_t seed, float dt, float horizon, float lateral_margin, const float *idm,
                  void *stream, const double *stop_at = nullptr) {
    TDS_CHECK_ARG(B >= 0 && N >= 0 && E >= 0 && B < ((int64_t)1 << 31) && N <= 2 * 65535, "%s: bad sizes B=%lld N=%lld E=%lld", what, (long long)B,
                  (long long)N, (long long)E);
    if (E > TDS_FOLLOW_MAX_ENTITIES) {
        tds::set_error("%s: %lld entities exceed the %d a scene's LDS holds", what, (long long)E, TDS_FOLLOW_MAX_ENTITIES);
        return TDS_ELIMIT;
    }
    TDS_CHECK_ARG(idm, "%s: the IDM parameters are null", what);
    TDS_CHECK_ARG(tds::ok_param(dt) && tds::ok_param(horizon) && tds::ok_param(lateral_margin), "%s: dt, horizon and lateral_margin must be finite and not negative",
                  what);
    for (int i = 0; i < 5; i++) TDS_CHECK_ARG(tds::ok_param(idm[i]), "%s: IDM parameter %d must be finite and not negative (got %g)", what, i, (double)idm[i]);
    TDS_CHECK_ARG(idm[2] > 0.f && idm[3] > 0.f, "%s: the IDM accelerations a and b must be positive", what);
    if (B == 0 || N == 0) return TDS_OK;
    TDS_CHECK_ARG(npc_size && desired_speed && npc_present && lane && arc && hops && state && sc && leader, "%s: null argument", what);
    TDS_CHECK_ARG(E == 0 || (boxes && ent_sc && ent_speed && ent_present), "%s: %lld entities without their arrays", what, (long long)E);
    g.scene_map = scene_map, g.scene_ids = scene_ids, g.N = (int)N, g.E = (int)E;
    g.boxes = boxes, g.ent_sc = ent_sc, g.ent_speed = ent_speed, g.ent_present = ent_present, g.self_index = self_index;
    g.npc_size = npc_size, g.desired_speed = desired_speed, g.npc_present = npc_present;
    g.lane = lane, g.arc = arc, g.hops = hops, g.state = state, g.sc = sc, g.leader = leader, g.stop_at = stop_at;
    // the route stream: spawn's key for the same seed with two words folded in ("LANE", "FOLW"), so the two streams never coincide
    g.key0 = (uint32_t)seed ^ 0x4C414E45u, g.key1 = (uint32_t)(seed >> 32) ^ 0x464F4C57u;
    g.dt = dt, g.horizon = horizon, g.margin = lateral_margin;
    g.T = idm[0], g.s0 = idm[1], g.a = idm[2], g.b = idm[3], g.b_max = idm[4];
    const int waves = E <= 480 ? 4 : 2;                                      // 15 + 48 + 1 KiB, or at most 32 + 24 + 0.5 KiB
    const size_t lds = (size_t)((E * ENT_WORDS + 3) & ~3) * sizeof(float) +
                       (size_t)waves * (FOLLOW_MAX_PIECES * PIECE_DOUBLES * sizeof(double) + NEAR_SLOTS * sizeof(int));
    hipLaunchKernelGGL(lane_follow_kernel, dim3((unsigned)B, (unsigned)((N + waves - 1) / waves)), dim3(64 * waves), lds, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("lane_follow_kernel");
    return TDS_OK;
}

}  // namespace

TDS_EXPORT int tds_lane_follow_step(const tds_lanes_t *lanes, const int64_t *scene_ids, int64_t B, int64_t N, int64_t E, const float *boxes,
                                    const float *ent_sc, const float *ent_speed, const uint8_t *ent_present, const int32_t *self_index,
                                    const float *npc_size, const float *desired_speed, const uint8_t *npc_present, int32_t *lane, double *arc,
                                    int32_t *hops, float *state, float *sc, int32_t *leader, uint64_t seed, float dt, float horizon,
                                    float lateral_margin, const float *idm, void *stream) {
    TDS_CHECK_ARG(lanes, "tds_lane_follow_step: the lane table is null");
    FollowArgs g = {};
    g.single = lanes->view, g.views = nullptr, g.n_views = 0;
    return follow_launch("tds_lane_follow_step", g, nullptr, scene_ids, B, N, E, boxes, ent_sc, ent_speed, ent_present, self_index, npc_size,
                         desired_speed, npc_present, lane, arc, hops, state, sc, leader, seed, dt, horizon, lateral_margin, idm, stream);
}

TDS_EXPORT int tds_lane_follow_step_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t N,
                                          int64_t E, const float *boxes, const float *ent_sc, const float *ent_speed, const uint8_t *ent_present,
                                          const int32_t *self_index, const float *npc_size, const float *desired_speed,
                                          const uint8_t *npc_present, int32_t *lane, double *arc, int32_t *hops, float *state, float *sc,
                                          int32_t *leader, uint64_t seed, float dt, float horizon, float lateral_margin, const float *idm,
                                          void *stream) {
    TDS_CHECK_ARG(set, "tds_lane_follow_step_multi: the lane-table set is null");
    TDS_CHECK_SCENE_MAP("tds_lane_follow_step_multi", set, scene_map);
    FollowArgs g = {};
    g.views = set->d_views, g.n_views = set->n;
    return follow_launch("tds_lane_follow_step_multi", g, scene_map, scene_ids, B, N, E, boxes, ent_sc, ent_speed, ent_present, self_index, npc_size,
                         desired_speed, npc_present, lane, arc, hops, state, sc, leader, seed, dt, horizon, lateral_margin, idm, stream);
}

TDS_EXPORT int tds_lane_follow_step_stops_multi(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t B, int64_t N,
                                                int64_t E, const float *boxes, const float *ent_sc, const float *ent_speed, const uint8_t *ent_present,
                                                const int32_t *self_index, const float *npc_size, const float *desired_speed,
                                                const uint8_t *npc_present, int32_t *lane, double *arc, int32_t *hops, float *state, float *sc,
                                                int32_t *leader, const double *stop_at, uint64_t seed, float dt, float horizon, float lateral_margin,
                                                const float *idm, void *stream) {
    TDS_CHECK_ARG(set, "tds_lane_follow_step_stops_multi: the lane-table set is null");
    TDS_CHECK_SCENE_MAP("tds_lane_follow_step_stops_multi", set, scene_map);
    FollowArgs g = {};
    g.views = set->d_views, g.n_views = set->n;
    return follow_launch("tds_lane_follow_step_stops_multi", g, scene_map, scene_ids, B, N, E, boxes, ent_sc, ent_speed, ent_present, self_index, npc_size,
                         desired_speed, npc_present, lane, arc, hops, state, sc, leader, seed, dt, horizon, lateral_margin, idm, stream, stop_at);
}

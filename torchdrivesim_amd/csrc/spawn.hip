// On-lane scene initialisation, rejection-sampled on the device.
//
//   heuristic_initialize                   reference behavior/heuristic.py:10-53   (one torch call and one Lanelet2 query per ATTEMPT)
//   -> pick_random_point_and_orientation   reference lanelet2.py:183-208           (lanelet2 `length`, `interpolatedPointAtDistance`)
//   -> collision_detection_with_discs      reference infractions.py:503-545
//
// The algorithm is sequential over the agents of a scene and data-parallel over scenes and over the ATTEMPTS of one agent: a candidate
// is a pure function of (seed, scene id, agent, attempt) -- Philox4x32-10 evaluated in the kernel -- so a wavefront evaluates 64 attempts
// of the current agent at once and takes the free one with the lowest attempt index (ballot, lowest set bit).  That is the candidate the
// reference's loop would have stopped at, whatever the number evaluated together.
//
// One wavefront per scene, no workgroup barrier.  LDS (dynamic): the boxes a candidate is tested against -- the occupied boxes, then the
// agents placed so far --, six floats each: x, y, length + gap_long, width + gap_lat, [sin, cos] of the angle the disc metric uses.
//
// Arithmetic ("On-lane initialisation"): the point on the centre line in float64 (Lanelet2 computes in double), rounded once to
// float32; the acceptance test is tds::discs_pair (tds_discs.h) on [sin, cos] taken from the UNIT VECTOR of the local direction, never from
// a device sinf / cosf; only the reported psi goes through atan2.
#include <math.h>

#include "tds_common.h"
#include "tds_discs.h"
#include "tds_lanes.h"

using tds::Box;
using tds::LaneRec;
using tds::LaneView;
using tds::U4;
using tds::order_lds;

namespace {

constexpr int BOX_FLOATS = 6;

__device__ inline Box lds_box(const float *p) {
    Box b;
    b.x = p[0], b.y = p[1], b.l = p[2], b.w = p[3], b.s = p[4], b.c = p[5];
    return b;
}

// A pair whose centres lie further apart than both half-diagonals of the discs' chains (+ a margin far above the rounding of the disc
// centres) has the value 0 exactly: every disc distance exceeds r1 + r2.  NaNs fail the comparison and take the full path.
__device__ inline bool touches(const Box &a, const Box &b) {
    float ex = a.x - b.x, ey = a.y - b.y;
    float reach = 0.5f * (fmaxf(a.l, a.w) + fmaxf(b.l, b.w)) + 0.05f + 1e-5f * fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(b.x), fabsf(b.y)));
    if (ex * ex + ey * ey > reach * reach) return false;
    return tds::discs_pair(a, b) > 0.0f;
}

__global__ __launch_bounds__(64) void spawn_on_lanes_kernel(const LaneView *views, int n_tables, const int32_t *scene_map, const int64_t *scene_ids,
                                                            int A, const float *attributes, const float *occupied, const float *occupied_sc,
                                                            const uint8_t *occupied_mask, int M, uint32_t key0, uint32_t key1, float min_speed,
                                                            float max_speed, float gap_long, float gap_lat, int max_attempts, float *state,
                                                            float *sc, uint8_t *placed, int32_t *attempts) {
    extern __shared__ __attribute__((aligned(16))) float boxes[];        // (M + A) x BOX_FLOATS
    const int lane = threadIdx.x;
    const int64_t scene = blockIdx.x;
    const uint64_t sid = scene_ids ? (uint64_t)scene_ids[scene] : (uint64_t)scene;
    // the occupied boxes, compacted: the absent ones are never tested
    int n_box = 0;
    for (int j0 = 0; j0 < M; j0 += 64) {
        int j = j0 + lane;
        bool on = j < M && (!occupied_mask || occupied_mask[scene * M + j]);
        unsigned long long b = __ballot(on);
        if (on) {
            const float *o = occupied + (scene * M + j) * 5;
            float *d = boxes + (n_box + __popcll(b & ((1ull << lane) - 1ull))) * BOX_FLOATS;
            d[0] = o[0], d[1] = o[1], d[2] = o[2] + gap_long, d[3] = o[3] + gap_lat;
            d[4] = occupied_sc[(scene * M + j) * 2], d[5] = occupied_sc[(scene * M + j) * 2 + 1];
        }
        n_box += __popcll(b);
    }
    order_lds();                                                           // one wave per workgroup: no barrier needed
    int n_placed = 0;
    LaneView v;
    const bool has_lanes = tds::view_of(views, n_tables, scene_map, scene, v) && v.n_eligible > 0;
    if (has_lanes) {
        const float dv = max_speed - min_speed;
        for (; n_placed < A; ++n_placed) {
            const int i = n_placed;
            const float *at = attributes + (scene * A + i) * 3;
            const float len = at[0], wid = at[1];
            int won = -1;                                                  // wave-uniform
            float wx = 0.f, wy = 0.f, wpsi = 0.f, wv = 0.f, ws = 0.f, wc = 1.f;
            for (int a0 = 0; a0 < max_attempts && won < 0; a0 += 64) {
                const int a = a0 + lane;
                bool free_ = false;
                float x = 0.f, y = 0.f, psi = 0.f, speed = 0.f, s = 0.f, c = 1.f;
                if (a < max_attempts) {
                    U4 ctr = {(uint32_t)sid, (uint32_t)(sid >> 32), (uint32_t)i, (uint32_t)a};
                    U4 r = tds::philox4x32_10(ctr, key0, key1);
                    const int k = tds::pick_of(r.x, v.n_eligible);
                    const LaneRec rec = v.rec[v.eligible[k]];
                    const double *cl = v.cl + 3 * (int64_t)rec.cl_start, *cum = v.cum + rec.cl_start;
                    const double length = cum[rec.cl_n - 1];
                    const double dist = (length * ((double)r.y + 0.5)) * 0x1p-32;
                    speed = min_speed + dv * ((float)(r.z >> 8) * 0x1p-24f);
                    const double ahead = fmin(dist + 1.0, length);
                    const tds::ArcPoint p = tds::point_at_arc(cl, cum, tds::segment_of(cum, rec.cl_n, dist), dist);
                    const tds::ArcPoint q = tds::point_at_arc(cl, cum, tds::segment_of(cum, rec.cl_n, ahead), ahead);
                    const double ddx = q.x - p.x, ddy = q.y - p.y;
                    const double norm = sqrt(ddx * ddx + ddy * ddy);
                    x = (float)p.x, y = (float)p.y;
                    if (norm > 0.0) {
                        psi = (float)atan2(ddy, ddx);
                        s = (float)(ddy / norm), c = (float)(ddx / norm);
                    }
                    Box me;
                    me.x = x, me.y = y, me.l = len, me.w = wid;
                    if (wid > len) me.s = c, me.c = -s; else me.s = s, me.c = c;      // a quarter turn on: the disc chain runs along the longer side
                    free_ = true;
                    for (int j = 0; j < n_box; ++j) {
                        if (touches(me, lds_box(boxes + j * BOX_FLOATS))) {
                            free_ = false;
                            break;
                        }
                    }
                }
                const unsigned long long ok = __ballot(free_);
                if (ok) {
                    const int l = (int)__ffsll((long long)ok) - 1;
                    won = a0 + l;
                    wx = __shfl(x, l), wy = __shfl(y, l), wpsi = __shfl(psi, l), wv = __shfl(speed, l), ws = __shfl(s, l), wc = __shfl(c, l);
                }
            }
            if (lane == 0) attempts[scene * A + i] = won >= 0 ? won + 1 : max_attempts;
            if (won < 0) break;
            if (lane == 0) {
                float *st = state + (scene * A + i) * 4;
                st[0] = wx, st[1] = wy, st[2] = wpsi, st[3] = wv;
                sc[(scene * A + i) * 2] = ws, sc[(scene * A + i) * 2 + 1] = wc;
                placed[scene * A + i] = 1;
                float *d = boxes + n_box * BOX_FLOATS;
                const float il = len + gap_long, iw = wid + gap_lat;
                d[0] = wx, d[1] = wy, d[2] = il, d[3] = iw;
                if (iw > il) d[4] = wc, d[5] = -ws; else d[4] = ws, d[5] = wc;
            }
            n_box++;
            order_lds();
        }
    }
    // what was not placed: zero rows; the agent that found no place keeps its attempt count, those behind it were never reached
    for (int i = n_placed + lane; i < A; i += 64) {
        float *st = state + (scene * A + i) * 4;
        st[0] = st[1] = st[2] = st[3] = 0.f;
        sc[(scene * A + i) * 2] = sc[(scene * A + i) * 2 + 1] = 0.f;
        placed[scene * A + i] = 0;
        if (i > n_placed || !has_lanes) attempts[scene * A + i] = 0;
    }
}

}  // namespace

TDS_EXPORT int tds_spawn_on_lanes_f32(const tds_laneset_t *set, const int32_t *scene_map, const int64_t *scene_ids, int64_t n_scenes,
                                      int agents_per_scene, const float *attributes, const float *occupied, const float *occupied_sc,
                                      const uint8_t *occupied_mask, int n_occupied, uint64_t seed, float min_speed, float max_speed,
                                      float gap_long, float gap_lat, int max_attempts, float *state, float *sc, uint8_t *placed,
                                      int32_t *attempts, void *stream) {
    TDS_CHECK_ARG(n_scenes >= 0 && n_scenes <= 0x7fffffff, "tds_spawn_on_lanes_f32: n_scenes %lld out of range", (long long)n_scenes);
    TDS_CHECK_ARG(agents_per_scene >= 0, "tds_spawn_on_lanes_f32: agents_per_scene %d out of range", agents_per_scene);
    TDS_CHECK_ARG(max_attempts >= 1, "tds_spawn_on_lanes_f32: max_attempts must be >= 1, got %d", max_attempts);
    TDS_CHECK_ARG(n_occupied >= 0, "tds_spawn_on_lanes_f32: n_occupied %d out of range", n_occupied);
    TDS_CHECK_ARG((int64_t)agents_per_scene + n_occupied <= TDS_SPAWN_MAX_BOXES,
                  "tds_spawn_on_lanes_f32: agents_per_scene + n_occupied = %lld exceeds the %d boxes a scene's LDS holds",
                  (long long)agents_per_scene + n_occupied, TDS_SPAWN_MAX_BOXES);
    TDS_CHECK_ARG(isfinite(min_speed) && isfinite(max_speed) && isfinite(gap_long) && isfinite(gap_lat),
                  "tds_spawn_on_lanes_f32: speeds and gaps must be finite");
    TDS_CHECK_ARG(set, "tds_spawn_on_lanes_f32: the lane-table set is null");
    TDS_CHECK_SCENE_MAP("tds_spawn_on_lanes_f32", set, scene_map);
    if (n_scenes == 0 || agents_per_scene == 0) return TDS_OK;
    TDS_CHECK_ARG(attributes && state && sc && placed && attempts, "tds_spawn_on_lanes_f32: null argument");
    TDS_CHECK_ARG(n_occupied == 0 || (occupied && occupied_sc), "tds_spawn_on_lanes_f32: n_occupied = %d without occupied / occupied_sc", n_occupied);
    const size_t lds = (size_t)(agents_per_scene + n_occupied) * BOX_FLOATS * sizeof(float);
    hipLaunchKernelGGL(spawn_on_lanes_kernel, dim3((unsigned)n_scenes), dim3(64), lds, (hipStream_t)stream, set->d_views, set->n, scene_map,
                       scene_ids, agents_per_scene, attributes, occupied, occupied_sc, occupied_mask, n_occupied, (uint32_t)seed,
                       (uint32_t)(seed >> 32), min_speed, max_speed, gap_long, gap_lat, max_attempts, state, sc, placed, attempts);
    TDS_LAUNCH_CHECK("spawn_on_lanes_kernel");
    return TDS_OK;
}

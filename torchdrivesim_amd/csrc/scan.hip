// K5: range-scan observations (Simulator.compute_range_scan).  R rays per exposed agent; every ray reports the distance to the nearest OTHER
// entity's rectangle and the length of its initial stretch that lies on the road mesh.  No reference counterpart: the definition is this
// project's own (DESIGN.md "K5", float64 model in tests/range_scan_model.py).
// One workgroup = one scene, or a slice of its exposed agents; the scene's E boxes are staged in LDS once; one lane per ray.  With R a multiple
// of 64 a wave holds rays of ONE agent: they share the origin, so the first look at the map grid is wave-uniform (scalar loads).
// All arithmetic of the ranges is binary32 + - * / relative to the ray's origin; only the "positive area" test of a face is float64.
#include "tds_common.h"
#include "tds_scan.h"
#include <algorithm>

namespace {

using tds::GridEntry;
using tds::MapView;
using tds::line_triangle;

constexpr int SBLOCK = 256;             // 4 waves
constexpr int SCAN_MAX_PASSES = 16384;  // hard cap of the fixed-point iteration (a pass that continues has retired at least one face)
constexpr int PEND = 8;                // road faces a lane keeps waiting per pass (LDS: PEND x 256 x 8 bytes)
constexpr int BOX_WORDS = 8;            // LDS words per entity: cx, cy, half length, half width, sin, cos, present (0 / 1), unused

struct ScanArgs {
    MapView one;                        // the map of every scene (views == null)
    const MapView *views;               // ... or one map per scene: views[scene_map[b]]
    const int32_t *scene_map;
    int n_maps;
    int has_map;                        // 0: no road part (every road range is max_range)
    const float *boxes, *sc;
    const uint8_t *present;
    const float2 *ray_sc;
    float *agent_range, *road_range;
    int32_t *hit;
    int A, E, R, agents_per_block;
    float max_range, gap;
};

// The faces of a pass that lie AHEAD of F + gap wait in a per-lane list in LDS (the PEND nearest ones, entry k of lane t at pend[k * SBLOCK + t]:
// consecutive lanes, consecutive words), so that a pass can chain through the faces of its cells instead of scanning them once per face.
struct Pending {
    float2 *slot;                       // this lane's entry 0
    int n, imax;                        // entries in use; the one with the largest a (valid when n == PEND)
    float amax, dropped;                // its a; the smallest a of an interval that found no room (inf: none)
};

__device__ __forceinline__ void pending_add(Pending &q, float a, float b) {
    if (q.n < PEND) {
        q.slot[q.n * SBLOCK] = make_float2(a, b);
        if (q.n == 0 || a > q.amax) { q.amax = a; q.imax = q.n; }
        ++q.n;
    } else if (a < q.amax) {            // takes the place of the farthest one
        q.dropped = fminf(q.dropped, q.amax);
        q.slot[q.imax * SBLOCK] = make_float2(a, b);
        q.amax = -__builtin_inff();
        for (int k = 0; k < PEND; ++k) {
            const float ak = q.slot[k * SBLOCK].x;
            if (ak > q.amax) { q.amax = ak; q.imax = k; }
        }
    } else {
        q.dropped = fminf(q.dropped, a);
    }
}

// One pass of the fixed point over the lists of the cells [cx0, cx1] x [cy0, cy1]: F grows to b_f whenever a face of positive area has
// a_f <= F + gap and b_f > F; faces further ahead go to the pending list.  Updating F inside the pass is sound: F never exceeds the least
// fixed point (a_f <= F + gap <= F* + gap gives b_f <= F*).  UNIFORM: the cells are the same for every lane of the wave; the list is then
// read with scalar loads.
template <bool UNIFORM>
__device__ __forceinline__ float road_pass(const MapView &m, float ox, float oy, float dx, float dy, float F, float gap, float max_range, int cx0,
                                           int cx1, int cy0, int cy1, Pending &pq) {
    for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
            int s = m.cell_start[cy * m.nx + cx], e = m.cell_start[cy * m.nx + cx + 1];
            if (UNIFORM) { s = __builtin_amdgcn_readfirstlane(s); e = __builtin_amdgcn_readfirstlane(e); }
            for (int i = s; i < e; ++i) {
                const float4 *q = (const float4 *)(m.entries + i);
                const float4 v01 = q[0];
                const float2 v2 = *(const float2 *)(q + 1);
                float lo, hi;
                if (!line_triangle(dx, dy, v01.x - ox, v01.y - oy, v01.z - ox, v01.w - oy, v2.x - ox, v2.y - oy, lo, hi)) continue;
                const float a = fmaxf(lo, 0.0f), b = fminf(hi, max_range);
                if (!(a <= b) || !(b > F)) continue;
                // faces without area are no road (padding faces [0,0,0], slivers): float64 on the float32 vertices, as the model evaluates it
                if (!tds::positive_area(v01.x, v01.y, v01.z, v01.w, v2.x, v2.y)) continue;
                if (a <= F + gap) F = b;
                else pending_add(pq, a, b);
            }
        }
    // chain through the waiting faces: a round that raises F retires at least one of them
    bool grew = pq.n > 0;
    for (int round = 0; round <= PEND && grew; ++round) {
        grew = false;
        for (int k = 0; k < pq.n; ++k) {
            const float2 ab = pq.slot[k * SBLOCK];
            if (ab.x <= F + gap && ab.y > F) { F = ab.y; grew = true; }
        }
    }
    return F;
}

// which cells can hold a face that meets the ray between the parameters F and F + gap: tds::cells_of (tds_scan.h) on the map's grid
__device__ __forceinline__ void cells_of(const MapView &m, float v0, float v1, float marg, float origin, int n, int &c0, int &c1) {
    tds::cells_of(m.cell, m.inv_cell, v0, v1, marg, origin, n, c0, c1);
}

__device__ float road_range_of(const MapView &m, float ox, float oy, float dx, float dy, float gap, float max_range, bool uniform_origin, float2 *slot) {
    if (m.nx <= 0 || m.ny <= 0) return 0.0f;
    const float marg = tds::scan_margin(ox, oy, max_range);
    float F = 0.0f;
    int moves = m.nx + m.ny + 2;                                 // the cell walk: a straight line changes its first cell at most nx + ny times
    int pcx0 = -1, pcx1 = -1, pcy0 = -1, pcy1 = -1;              // the cells of the last pass ...
    bool settled = false;                                        // ... and whether it weighed EVERY face of them against the F it ended at
    for (int pass = 0; pass < SCAN_MAX_PASSES; ++pass) {
        const float G = F + gap;
        int cx0, cx1, cy0, cy1;
        cells_of(m, ox + dx * F, ox + dx * G, marg, m.ox, m.nx, cx0, cx1);
        cells_of(m, oy + dy * F, oy + dy * G, marg, m.oy, m.ny, cy0, cy1);
        if (settled && cx0 >= pcx0 && cx1 <= pcx1 && cy0 >= pcy0 && cy1 <= pcy1) break;       // nothing in these cells can raise this F
        if (cx0 != pcx0 || cy0 != pcy0) {
            if (--moves < 0) break;
        }
        Pending pq;
        pq.slot = slot; pq.n = 0; pq.imax = 0; pq.amax = -__builtin_inff(); pq.dropped = __builtin_inff();
        float Fn;
        // F == 0: r(F) is the agent's centre and r(G) within `gap` of it -- the same cells for all rays of the agent unless the gap crosses a border
        bool uni = false;
        if (pass == 0 && uniform_origin) {
            const bool same = __builtin_amdgcn_readfirstlane(cx0) == cx0 && __builtin_amdgcn_readfirstlane(cx1) == cx1 &&
                              __builtin_amdgcn_readfirstlane(cy0) == cy0 && __builtin_amdgcn_readfirstlane(cy1) == cy1;
            uni = __all(same) && __ballot(1) == ~0ull;
        }
        if (uni) {
            Fn = road_pass<true>(m, ox, oy, dx, dy, F, gap, max_range, __builtin_amdgcn_readfirstlane(cx0), __builtin_amdgcn_readfirstlane(cx1),
                                 __builtin_amdgcn_readfirstlane(cy0), __builtin_amdgcn_readfirstlane(cy1), pq);
        } else {
            Fn = road_pass<false>(m, ox, oy, dx, dy, F, gap, max_range, cx0, cx1, cy0, cy1, pq);
        }
        // every face of the cells was used, was behind F, or waited in the list and was weighed against the final F -- unless one found no
        // room there and starts within reach
        settled = Fn + gap < pq.dropped;
        pcx0 = cx0; pcx1 = cx1; pcy0 = cy0; pcy1 = cy1;
        if (!(Fn > F)) break;
        F = Fn;
        if (F >= max_range) break;
    }
    return fminf(F, max_range);
}

// grid = (B, ceil(A / agents_per_block)); dynamic LDS = E * BOX_WORDS floats + PEND * SBLOCK float2
__global__ void __launch_bounds__(SBLOCK) range_scan_kernel(ScanArgs g) {
    extern __shared__ __attribute__((aligned(16))) float bx[];
    __shared__ int any_present;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, R = g.R;
    const bool want_agents = g.agent_range != nullptr;
    if (tid == 0) any_present = 0;
    __syncthreads();
    for (int j = tid; j < E; j += SBLOCK) {
        const float *p = g.boxes + (b * E + j) * 5;
        const int pr = g.present[b * E + j] ? 1 : 0;
        float4 lo = make_float4(p[0], p[1], p[2] / 2.0f, p[3] / 2.0f);
        float4 hi = make_float4(g.sc[(b * E + j) * 2], g.sc[(b * E + j) * 2 + 1], pr ? 1.0f : 0.0f, 0.0f);
        *(float4 *)(bx + BOX_WORDS * j) = lo;
        *(float4 *)(bx + BOX_WORDS * j + 4) = hi;
        if (pr) any_present = 1;
    }
    __syncthreads();
    MapView m = g.one;
    bool has_map = g.has_map != 0;
    if (g.views != nullptr) {
        const int im = g.scene_map[b];
        if (im >= 0 && im < g.n_maps) m = g.views[im]; else has_map = false;      // (an index outside the set: as without a road mesh)
    }
    const int a0 = blockIdx.y * g.agents_per_block;
    const int a1 = min(a0 + g.agents_per_block, A);
    const int n_rays = (a1 - a0) * R;
    const bool wave_per_agent = (R & 63) == 0;              // every wave holds rays of one agent
    const int n_iter = (n_rays + SBLOCK - 1) / SBLOCK;
    for (int it = 0; it < n_iter; ++it) {
        const int i = it * SBLOCK + tid;
        if (i >= n_rays) continue;                           // (no barrier below)
        const int a = a0 + i / R, k = i - (i / R) * R;
        const int64_t o = (b * A + a) * R + k;
        const float4 me = *(const float4 *)(bx + BOX_WORDS * a);
        const float4 me2 = *(const float4 *)(bx + BOX_WORDS * a + 4);
        float ta = g.max_range, tr = g.max_range;
        int who = -1;
        if (me2.z != 0.0f) {
            const float2 rsc = g.ray_sc[o];
            const float dx = rsc.y, dy = rsc.x;
            if (want_agents && any_present) {
                for (int j = 0; j < E; ++j) {
                    const float4 q = *(const float4 *)(bx + BOX_WORDS * j);
                    const float4 q2 = *(const float4 *)(bx + BOX_WORDS * j + 4);
                    if (j == a || q2.z == 0.0f) continue;
                    // the ray in the rectangle's frame (origin relative to its centre), slab test
                    const float rx = me.x - q.x, ry = me.y - q.y;
                    const float lx = rx * q2.y + ry * q2.x, ly = ry * q2.y - rx * q2.x;
                    const float ex = dx * q2.y + dy * q2.x, ey = dy * q2.y - dx * q2.x;
                    float t0;
                    int slab;
                    if (tds::slab_test(lx, ly, ex, ey, q.z, q.w, t0, slab) && t0 < ta) { ta = t0; who = j; }
                }
            }
            if (has_map) tr = road_range_of(m, me.x, me.y, dx, dy, g.gap, g.max_range, wave_per_agent, (float2 *)(bx + BOX_WORDS * E) + tid);
        }
        if (g.agent_range) g.agent_range[o] = ta;
        if (g.road_range) g.road_range[o] = tr;
        if (g.hit) g.hit[o] = (ta < g.max_range && ta <= tr) ? who : ((tr < g.max_range && tr < ta) ? -2 : -1);
    }
}

int launch(const ScanArgs &g0, int64_t B, void *stream, const char *what) {
    ScanArgs g = g0;
    // about one ray per lane of the workgroup: whole agents per workgroup, at least one
    g.agents_per_block = (int)std::min<int64_t>(std::max<int64_t>(SBLOCK / g.R, 1), g.A);
    const unsigned gy = (unsigned)((g.A + g.agents_per_block - 1) / g.agents_per_block);
    if (gy > 65535u) { tds::set_error("%s: %d exposed agents per scene are too many for %d rays each", what, g.A, g.R); return TDS_ELIMIT; }
    const size_t lds = (size_t)g.E * BOX_WORDS * sizeof(float) + (g.has_map ? (size_t)PEND * SBLOCK * sizeof(float2) : 0);
    hipLaunchKernelGGL(range_scan_kernel, dim3((unsigned)B, gy), dim3(SBLOCK), lds, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("range_scan_kernel");
    return TDS_OK;
}

int check_and_fill(const char *what, ScanArgs &g, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc, float *agent_range,
                   float *road_range, int32_t *hit, int64_t B, int64_t A, int64_t E, int R, float max_range, float gap_tolerance, bool &nothing) {
    nothing = false;
    TDS_CHECK_ARG(B >= 0 && A >= 0 && E >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld E=%lld", what, (long long)B, (long long)A, (long long)E);
    TDS_CHECK_ARG(R > 0 && R <= (1 << 16), "%s: the number of rays must be 1 .. 65536 (got %d)", what, R);
    TDS_CHECK_ARG(A <= E, "%s: %lld exposed agents but only %lld entities", what, (long long)A, (long long)E);
    TDS_CHECK_ARG(max_range >= 0.0f && max_range <= 3.0e38f, "%s: max_range must be finite and not negative (got %g)", what, (double)max_range);
    TDS_CHECK_ARG(gap_tolerance >= 0.0f && gap_tolerance <= 3.0e38f, "%s: gap_tolerance must be finite and not negative (got %g)", what, (double)gap_tolerance);
    if (E > TDS_SCAN_MAX_ENTITIES) { tds::set_error("%s: %lld entities per scene (the boxes of a scene live in LDS: at most %d)", what, (long long)E, TDS_SCAN_MAX_ENTITIES); return TDS_ELIMIT; }
    if (B == 0 || A == 0 || (!agent_range && !road_range && !hit)) { nothing = true; return TDS_OK; }
    TDS_CHECK_ARG(boxes && sc && present && ray_sc, "%s: null pointer", what);
    g.views = nullptr; g.scene_map = nullptr; g.n_maps = 0; g.has_map = 0;
    g.boxes = boxes; g.sc = sc; g.present = present; g.ray_sc = (const float2 *)ray_sc;
    g.agent_range = agent_range; g.road_range = road_range; g.hit = hit;
    g.A = (int)A; g.E = (int)E; g.R = R; g.agents_per_block = 1;
    g.max_range = max_range; g.gap = gap_tolerance;
    return TDS_OK;
}

}  // namespace

TDS_EXPORT int tds_range_scan_f32(const tds_map_t *map, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,
                                  float *agent_range, float *road_range, int32_t *hit, int64_t B, int64_t A, int64_t E, int R, float max_range,
                                  float gap_tolerance, void *stream) {
    ScanArgs g{};
    bool nothing;
    const int rc = check_and_fill("tds_range_scan_f32", g, boxes, sc, present, ray_sc, agent_range, road_range, hit, B, A, E, R, max_range, gap_tolerance, nothing);
    if (rc != TDS_OK || nothing) return rc;
    if (map) { g.one = map->view; g.has_map = 1; }
    return launch(g, B, stream, "tds_range_scan_f32");
}

TDS_EXPORT int tds_range_scan_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, const float *boxes, const float *sc, const uint8_t *present,
                                        const float *ray_sc, float *agent_range, float *road_range, int32_t *hit, int64_t B, int64_t A, int64_t E, int R,
                                        float max_range, float gap_tolerance, void *stream) {
    TDS_CHECK_ARG(set && set->n > 0 && scene_map, "tds_range_scan_multi_f32: null map set or scene index array");
    ScanArgs g{};
    bool nothing;
    const int rc = check_and_fill("tds_range_scan_multi_f32", g, boxes, sc, present, ray_sc, agent_range, road_range, hit, B, A, E, R, max_range, gap_tolerance, nothing);
    if (rc != TDS_OK || nothing) return rc;
    g.views = set->d_views; g.scene_map = scene_map; g.n_maps = set->n; g.has_map = 1;
    return launch(g, B, stream, "tds_range_scan_multi_f32");
}

// K5b: the backward of the range scans (_ops.range_scan_grad; include/tdship.h "K5b"): the gradients of agent_range and
// road_range to x, y, length, width and [sin, cos] of every entity and to [sin, cos] of every ray, one launch.  Yardstick: the float64
// torch-autograd model tests/range_scan_grad_model.py; the per-ray derivatives are stated once, in tds_scan_grad.h.
// One workgroup = one scene.  The scene's E boxes are staged in LDS as scan.hip stages them.  The scene's A * R rays are taken in chunks of
// SGBLOCK, one ray per lane: a lane makes the forward's choices again with the forward's own code (tds_scan.h) -- the entity and the slab that
// define agent_range, and ONE look at the map's lists around the end of the road stretch for the edge that ends it --, writes the ray's own
// gradient and its witness, and leaves a record (entity, the entity's six terms, the observer's two) in LDS.  After a barrier the lanes act as
// RECEIVING entities: lane j, strided over E, walks the chunk's records in ray order and adds those that name j, then the observer terms of
// agent j's own rays, into binary64 accumulators in LDS that only it touches.  So every sum has one fixed order, nothing is added to memory, and
// two runs give the same bits.  The accumulators are rounded to binary32 and stored once, at the end.
#include "tds_common.h"
#include "tds_scan_grad.h"

namespace {

using tds::MapView;

constexpr int SGBLOCK = 256;            // 4 waves; rays per chunk
constexpr int SG_BOX_WORDS = 8;         // LDS words per entity, as scan.hip: cx, cy, half length, half width, sin, cos, present (0 / 1), unused
constexpr int SG_ACC = 6;               // binary64 accumulators per entity: x, y, length, width, sin, cos
constexpr int SG_REC = 8;               // binary64 terms per ray record: the entity's six, the observer's x, y

struct ScanBwdArgs {
    MapView one;                        // the map of every scene (views == null)
    const MapView *views;               // ... or one map per scene: views[scene_map[b]]
    const int32_t *scene_map;
    int n_maps;
    int has_map;
    const float *boxes, *sc;
    const uint8_t *present;
    const float2 *ray_sc;
    const float *road_range, *g_agent, *g_road;
    float *g_boxes, *g_sc;
    float2 *g_ray_sc;
    int32_t *choice;
    float *road_edge;
    int A, E, R;
    int do_agents, do_road;             // whether a part is computed at all
    float max_range;
};

// A kernel argument that is read once per ray, or once at the end, is kept in vector registers: the scalar file cannot hold all of them next to
// the map's grid, and the compiler would park them in a vector register's lanes instead.  Asked for again inside the loop over the chunks, it
// also keeps a test of such an argument where it is written: hoisted out of the loop, every one of them would hold a pair of scalar registers
template <class T>
__device__ __forceinline__ T in_vgpr(T p) {
    asm volatile("" : "+v"(p));
    return p;
}

// dynamic LDS: SG_ACC * E + SG_REC * SGBLOCK doubles, SG_BOX_WORDS * E floats, SGBLOCK ints
size_t lds_bytes(int64_t E) {
    return ((size_t)SG_ACC * E + (size_t)SG_REC * SGBLOCK) * sizeof(double) + (size_t)SG_BOX_WORDS * E * sizeof(float) + (size_t)SGBLOCK * sizeof(int32_t);
}

// the edge the road stretch of length F ends on: one pass over the lists of the cells around r(F), every face weighed by tds::road_edge_of_face
__device__ __forceinline__ tds::RoadEdge road_edge_at(const MapView &m, float ox, float oy, float dx, float dy, float F, float max_range) {
    tds::RoadEdge best;
    best.xi = best.yi = best.xj = best.yj = 0.0f;
    best.found = false;
    if (m.nx <= 0 || m.ny <= 0) return best;
    const float marg = tds::scan_margin(ox, oy, max_range);
    const float px = ox + dx * F, py = oy + dy * F;
    int cx0, cx1, cy0, cy1;
    tds::cells_of(m.cell, m.inv_cell, px, px, marg, m.ox, m.nx, cx0, cx1);
    tds::cells_of(m.cell, m.inv_cell, py, py, marg, m.oy, m.ny, cy0, cy1);
    for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) {
            const int s = m.cell_start[cy * m.nx + cx], e = m.cell_start[cy * m.nx + cx + 1];
            for (int i = s; i < e; ++i) {
                const float4 *q = (const float4 *)(m.entries + i);
                const float4 v01 = q[0];
                const float2 v2 = *(const float2 *)(q + 1);
                tds::road_edge_of_face(best, ox, oy, dx, dy, F, v01.x, v01.y, v01.z, v01.w, v2.x, v2.y);
            }
        }
    return best;
}

// grid = B; dynamic LDS = lds_bytes(E).  MULTI: one map per scene (g.views), else the map of every scene (g.one)
template <bool MULTI>
__global__ void __launch_bounds__(SGBLOCK) range_scan_bwd_kernel(ScanBwdArgs g) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int A = g.A, E = g.E, R = g.R;
    const float *road_range = in_vgpr(g.road_range), *g_agent = in_vgpr(g.g_agent), *g_road = in_vgpr(g.g_road);
    float *g_boxes = in_vgpr(g.g_boxes), *g_sc = in_vgpr(g.g_sc), *road_edge = in_vgpr(g.road_edge);
    float2 *g_ray_sc = in_vgpr(g.g_ray_sc);
    int32_t *choice = in_vgpr(g.choice);
    double *acc = lds;                                           // [SG_ACC][E]
    double *rec = lds + (size_t)SG_ACC * E;                      // [SG_REC][SGBLOCK]
    float *bx = (float *)(rec + SG_REC * SGBLOCK);               // [E][SG_BOX_WORDS]
    int32_t *rec_who = (int32_t *)(bx + (size_t)SG_BOX_WORDS * E);
    for (int j = tid; j < E; j += SGBLOCK) {
        const float *p = g.boxes + (b * E + j) * 5;
        const int pr = g.present[b * E + j] ? 1 : 0;
        *(float4 *)(bx + SG_BOX_WORDS * j) = make_float4(p[0], p[1], p[2] / 2.0f, p[3] / 2.0f);
        *(float4 *)(bx + SG_BOX_WORDS * j + 4) = make_float4(g.sc[(b * E + j) * 2], g.sc[(b * E + j) * 2 + 1], pr ? 1.0f : 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < SG_ACC; ++k) acc[k * E + j] = 0.0;
    }
    __syncthreads();
    int do_road = g.do_road, do_agents = g.do_agents;
    int im = 0;
    if (MULTI) {
        im = g.scene_map[b];
        if (im < 0 || im >= g.n_maps) { im = 0; do_road = 0; }               // (an index outside the set: as without a road mesh)
    }
    MapView m = MULTI ? g.views[im] : g.one;                     // (the grid alone is read)
    m.entries = in_vgpr(m.entries), m.cell_start = in_vgpr(m.cell_start);
    m.ox = in_vgpr(m.ox), m.oy = in_vgpr(m.oy), m.inv_cell = in_vgpr(m.inv_cell), m.cell = in_vgpr(m.cell);
    m.nx = in_vgpr(m.nx), m.ny = in_vgpr(m.ny);
    const int n_rays = A * R;                                    // at most 2^26
    const int n_chunks = (n_rays + SGBLOCK - 1) / SGBLOCK;
    for (int chunk = 0; chunk < n_chunks; ++chunk) {
        const int base = chunk * SGBLOCK;
        const int i = base + tid;
        int who = -1, wslab = 0;
        double r8[SG_REC] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool live = false;
        if (i < n_rays) {
            const int a = i / R;
            const int64_t o = b * n_rays + i;
            const float4 me = *(const float4 *)(bx + SG_BOX_WORDS * a);
            const float4 me2 = *(const float4 *)(bx + SG_BOX_WORDS * a + 4);
            double gdx = 0.0, gdy = 0.0;
            tds::RoadEdge ed;
            ed.found = false;
            if (me2.z != 0.0f) {
                const float2 rsc = g.ray_sc[o];
                const float dx = rsc.y, dy = rsc.x;
                if (in_vgpr(do_agents)) {
                    float ta = g.max_range;
                    for (int j = 0; j < E; ++j) {
                        const float4 q = *(const float4 *)(bx + SG_BOX_WORDS * j);
                        const float4 q2 = *(const float4 *)(bx + SG_BOX_WORDS * j + 4);
                        if (j == a || q2.z == 0.0f) continue;
                        // the forward's lines: the ray in the rectangle's frame (origin relative to its centre), slab test
                        const float rx = me.x - q.x, ry = me.y - q.y;
                        const float lx = rx * q2.y + ry * q2.x, ly = ry * q2.y - rx * q2.x;
                        const float ex = dx * q2.y + dy * q2.x, ey = dy * q2.y - dx * q2.x;
                        float t0;
                        int slab;
                        if (tds::slab_test(lx, ly, ex, ey, q.z, q.w, t0, slab) && t0 < ta) { ta = t0; who = j; wslab = slab; }
                    }
                    const float *gap = in_vgpr(g_agent);
                    if (who >= 0 && wslab != 0 && gap != nullptr) {
                        const double ga = (double)gap[o];
                        const float4 q = *(const float4 *)(bx + SG_BOX_WORDS * who);
                        const float4 q2 = *(const float4 *)(bx + SG_BOX_WORDS * who + 4);
                        double d[tds::SG_AGENT];
                        tds::scan_agent_grad(wslab, me.x, me.y, q.x, q.y, q.z, q.w, q2.x, q2.y, dx, dy, d);
                        r8[0] = ga * d[tds::SG_EX], r8[1] = ga * d[tds::SG_EY], r8[2] = ga * d[tds::SG_LENGTH], r8[3] = ga * d[tds::SG_WIDTH];
                        r8[4] = ga * d[tds::SG_SIN], r8[5] = ga * d[tds::SG_COS];
                        r8[6] = ga * d[tds::SG_OX], r8[7] = ga * d[tds::SG_OY];
                        gdx = ga * d[tds::SG_DX], gdy = ga * d[tds::SG_DY];
                        live = true;
                    }
                }
                if (in_vgpr(do_road)) {
                    const float F = road_range[o];
                    if (F > 0.0f && F < g.max_range) {
                        ed = road_edge_at(m, me.x, me.y, dx, dy, F, g.max_range);
                        const float *grp = in_vgpr(g_road);
                        if (ed.found && grp != nullptr) {
                            const double gr = (double)grp[o];
                            double d[tds::SR_ROAD];
                            tds::scan_road_grad(me.x, me.y, dx, dy, ed, d);
                            r8[6] = r8[6] + gr * d[tds::SR_OX], r8[7] = r8[7] + gr * d[tds::SR_OY];
                            gdx = gdx + gr * d[tds::SR_DX], gdy = gdy + gr * d[tds::SR_DY];
                            live = true;
                        }
                    }
                }
            }
            if (float2 *out = in_vgpr(g_ray_sc)) out[o] = make_float2((float)gdy, (float)gdx);     // [sin, cos]
            if (int32_t *out = in_vgpr(choice)) *(int2 *)(out + o * 2) = make_int2(who, wslab);
            if (float *out = in_vgpr(road_edge)) {
                const float nan = __builtin_nanf("");
                *(float4 *)(out + o * 4) = ed.found ? make_float4(ed.xi, ed.yi, ed.xj, ed.yj) : make_float4(nan, nan, nan, nan);
            }
        }
        // nothing to gather from a chunk without a contributing ray (uniform: every lane has the same answer)
        if (!__syncthreads_or(live ? 1 : 0)) continue;
        rec_who[tid] = (wslab != 0 && in_vgpr(g_agent) != nullptr) ? who : -1;
#pragma unroll
        for (int k = 0; k < SG_REC; ++k) rec[k * SGBLOCK + tid] = r8[k];
        __syncthreads();
        const int cnt = min(SGBLOCK, n_rays - base);
        for (int j = tid; j < E; j += SGBLOCK) {
            double s[SG_ACC];
#pragma unroll
            for (int k = 0; k < SG_ACC; ++k) s[k] = acc[k * E + j];
            for (int r = 0; r < cnt; ++r) {                      // j as the entity a ray ends on, in ray order
                if (rec_who[r] != j) continue;
#pragma unroll
                for (int k = 0; k < SG_ACC; ++k) s[k] = s[k] + rec[k * SGBLOCK + r];
            }
            if (j < A) {                                         // j as the observer of its own rays, in ray order
                const int r0 = max(j * R, base) - base, r1 = min((j + 1) * R, base + cnt) - base;
                for (int r = r0; r < r1; ++r) s[0] = s[0] + rec[6 * SGBLOCK + r], s[1] = s[1] + rec[7 * SGBLOCK + r];
            }
#pragma unroll
            for (int k = 0; k < SG_ACC; ++k) acc[k * E + j] = s[k];
        }
        __syncthreads();
    }
    for (int j = tid; j < E; j += SGBLOCK) {                     // every row in full, zeros included
        if (g_boxes) {
            float *gb = g_boxes + (b * E + j) * 5;
            gb[0] = (float)acc[0 * E + j], gb[1] = (float)acc[1 * E + j], gb[2] = (float)acc[2 * E + j], gb[3] = (float)acc[3 * E + j];
            gb[4] = 0.0f;                                        // psi is not read: it gets its gradient through [sin, cos]
        }
        if (g_sc) *(float2 *)(g_sc + (b * E + j) * 2) = make_float2((float)acc[4 * E + j], (float)acc[5 * E + j]);
    }
}

int check_and_fill(const char *what, ScanBwdArgs &g, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,
                   const float *road_range, const float *g_agent, const float *g_road, float *g_boxes, float *g_sc, float *g_ray_sc, int32_t *choice,
                   float *road_edge, int64_t B, int64_t A, int64_t E, int R, float max_range, float gap_tolerance, bool &nothing) {
    nothing = false;
    TDS_CHECK_ARG(B >= 0 && A >= 0 && E >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld A=%lld E=%lld", what, (long long)B, (long long)A, (long long)E);
    TDS_CHECK_ARG(R > 0 && R <= (1 << 16), "%s: the number of rays must be 1 .. 65536 (got %d)", what, R);
    TDS_CHECK_ARG(A <= E, "%s: %lld exposed agents but only %lld entities", what, (long long)A, (long long)E);
    TDS_CHECK_ARG(max_range >= 0.0f && max_range <= 3.0e38f, "%s: max_range must be finite and not negative (got %g)", what, (double)max_range);
    TDS_CHECK_ARG(gap_tolerance >= 0.0f && gap_tolerance <= 3.0e38f, "%s: gap_tolerance must be finite and not negative (got %g)", what, (double)gap_tolerance);
    if (E > TDS_SCAN_MAX_ENTITIES) { tds::set_error("%s: %lld entities per scene (the boxes of a scene live in LDS: at most %d)", what, (long long)E, TDS_SCAN_MAX_ENTITIES); return TDS_ELIMIT; }
    if (B == 0 || E == 0 || (!g_boxes && !g_sc && !g_ray_sc && !choice && !road_edge)) { nothing = true; return TDS_OK; }
    TDS_CHECK_ARG(boxes && sc && present && (A == 0 || ray_sc), "%s: null pointer", what);
    g.views = nullptr; g.scene_map = nullptr; g.n_maps = 0; g.has_map = 0;
    g.boxes = boxes; g.sc = sc; g.present = present; g.ray_sc = (const float2 *)ray_sc;
    g.road_range = road_range; g.g_agent = g_agent; g.g_road = g_road;
    g.g_boxes = g_boxes; g.g_sc = g_sc; g.g_ray_sc = (float2 *)g_ray_sc; g.choice = choice; g.road_edge = road_edge;
    g.A = (int)A; g.E = (int)E; g.R = R;
    g.max_range = max_range;
    return TDS_OK;
}

int launch(ScanBwdArgs &g, int64_t B, void *stream) {
    const bool grads = g.g_boxes || g.g_sc || g.g_ray_sc;
    g.do_agents = ((g.g_agent && grads) || g.choice) ? 1 : 0;
    g.do_road = (g.has_map && g.road_range && ((g.g_road && (g.g_boxes || g.g_ray_sc)) || g.road_edge)) ? 1 : 0;
    const size_t lds = lds_bytes(g.E);
    auto go = [&](auto kern) {
        if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(SGBLOCK), lds, (hipStream_t)stream, g);
    };
    if (g.views != nullptr) go(range_scan_bwd_kernel<true>); else go(range_scan_bwd_kernel<false>);
    TDS_LAUNCH_CHECK("range_scan_bwd_kernel");
    return TDS_OK;
}

}  // namespace

TDS_EXPORT int tds_range_scan_bwd_f32(const tds_map_t *map, const float *boxes, const float *sc, const uint8_t *present, const float *ray_sc,
                                      const float *road_range, const float *g_agent, const float *g_road, float *g_boxes, float *g_sc, float *g_ray_sc,
                                      int32_t *choice, float *road_edge, int64_t B, int64_t A, int64_t E, int R, float max_range, float gap_tolerance,
                                      void *stream) {
    ScanBwdArgs g{};
    bool nothing;
    const int rc = check_and_fill("tds_range_scan_bwd_f32", g, boxes, sc, present, ray_sc, road_range, g_agent, g_road, g_boxes, g_sc, g_ray_sc, choice,
                                  road_edge, B, A, E, R, max_range, gap_tolerance, nothing);
    if (rc != TDS_OK || nothing) return rc;
    if (map) { g.one = map->view; g.has_map = 1; }
    TDS_CHECK_ARG(!(g.has_map && (g_road || road_edge)) || road_range || A == 0, "tds_range_scan_bwd_f32: the road part needs road_range");
    return launch(g, B, stream);
}

TDS_EXPORT int tds_range_scan_bwd_multi_f32(const tds_mapset_t *set, const int32_t *scene_map, const float *boxes, const float *sc, const uint8_t *present,
                                            const float *ray_sc, const float *road_range, const float *g_agent, const float *g_road, float *g_boxes,
                                            float *g_sc, float *g_ray_sc, int32_t *choice, float *road_edge, int64_t B, int64_t A, int64_t E, int R,
                                            float max_range, float gap_tolerance, void *stream) {
    TDS_CHECK_ARG(set && set->n > 0 && scene_map, "tds_range_scan_bwd_multi_f32: null map set or scene index array");
    ScanBwdArgs g{};
    bool nothing;
    const int rc = check_and_fill("tds_range_scan_bwd_multi_f32", g, boxes, sc, present, ray_sc, road_range, g_agent, g_road, g_boxes, g_sc, g_ray_sc,
                                  choice, road_edge, B, A, E, R, max_range, gap_tolerance, nothing);
    if (rc != TDS_OK || nothing) return rc;
    g.views = set->d_views; g.scene_map = scene_map; g.n_maps = set->n; g.has_map = 1;
    TDS_CHECK_ARG(!(g_road || road_edge) || road_range || A == 0, "tds_range_scan_bwd_multi_f32: the road part needs road_range");
    return launch(g, B, stream);
}

// The nearest mesh face of a point, for K2b off-road and its gradient (map.hip: offroad_kernel, backward.hip: offroad_bwd_kernel): the
// reference's point-to-triangle distance and its gradient, the conservative box bound every walk prunes with, and ONE traversal of each map
// structure -- candidate lists, hierarchy, grid rings -- that either kernel instantiates.  The first part is plain arithmetic that a host
// compiler takes as it is (tests/nearest_face_host.cpp holds it to the oracle on the CPU); the traversals below it are HIP.
// Reference: infractions.py:86-229 (pure-torch path).  -ffp-contract=off: every operation rounds once, in the reference's order.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif

namespace tds {

TDS_HD inline float dot2(float ax, float ay, float bx, float by) { return (ax * bx + ay * by) + 0.0f; }

// point_line_distance, infractions.py:147-159: the edge a -> b, its squared length, the UNCLAMPED parameter of the foot point, and the vector
// from the clamped foot point to p
struct SegFoot { float ex, ey, l2, t, rx, ry; };
TDS_HD inline SegFoot seg_foot(float px, float py, float ax, float ay, float bx, float by) {
    SegFoot s;
    s.ex = bx - ax; s.ey = by - ay;
    s.l2 = dot2(s.ex, s.ey, s.ex, s.ey);
    s.t = dot2(s.ex, s.ey, px - ax, py - ay) / (s.l2 + (float)1e-8);
    float tt = fminf(fmaxf(s.t, 0.0f), 1.0f);
    tt = (s.t != s.t) ? s.t : tt;                            // torch.clamp propagates NaN
    const float qx = ax + tt * s.ex, qy = ay + tt * s.ey;
    s.rx = px - qx; s.ry = py - qy;
    return s;
}
// squared distance from p to the segment a - b
TDS_HD inline float seg_d2(float px, float py, float ax, float ay, float bx, float by) {
    const SegFoot s = seg_foot(px, py, ax, ay, bx, by);
    float d = dot2(s.rx, s.ry, s.rx, s.ry);
    if (s.l2 <= (float)1e-8) d = dot2(px - bx, py - by, px - bx, py - by);
    return d;
}
// ... and its gradient w.r.t. p, as autograd takes it
TDS_HD inline void seg_d2_grad(float px, float py, float ax, float ay, float bx, float by, float &gx, float &gy) {
    const SegFoot s = seg_foot(px, py, ax, ay, bx, by);
    gx = 2.0f * s.rx; gy = 2.0f * s.ry;
    if (s.t >= 0.0f && s.t <= 1.0f) {                        // clamp passes the gradient on [0, 1]
        const float k = 2.0f * (s.rx * s.ex + s.ry * s.ey) / (s.l2 + (float)1e-8);
        gx -= k * s.ex; gy -= k * s.ey;
    }
    if (s.l2 <= (float)1e-8) { gx = 2.0f * (px - bx); gy = 2.0f * (py - by); }
}

// point_to_mesh_distance_pt for one (point, triangle) in the z = 0 plane, infractions.py:100-170.  Face: anything with the vertices x0, y0 ..
// x2, y2 (tds::GridEntry).  Inside the triangle (barycentric test; slivers never hold a point) the distance is 0 ...
template <class Face>
TDS_HD inline bool tri_inside(float px, float py, const Face &e) {
    float cz = (e.x2 - e.x0) * (e.y1 - e.y0) - (e.y2 - e.y0) * (e.x1 - e.x0);
    float norm_normal = sqrtf(cz * cz);
    float p0x = e.x1 - e.x0, p0y = e.y1 - e.y0, p1x = e.x2 - e.x0, p1y = e.y2 - e.y0;
    float p2x = px - e.x0, p2y = py - e.y0;
    float d00 = dot2(p0x, p0y, p0x, p0y), d01 = dot2(p0x, p0y, p1x, p1y), d11 = dot2(p1x, p1y, p1x, p1y);
    float d20 = dot2(p2x, p2y, p0x, p0y), d21 = dot2(p2x, p2y, p1x, p1y);
    float denom = d00 * d11 - d01 * d01 + (float)1e-8;
    float w1 = (d11 * d20 - d01 * d21) / denom;
    float w2 = (d00 * d21 - d01 * d20) / denom;
    float w0 = 1.0f - w1 - w2;
    bool inside = (0.0f <= w0) && (w0 <= 1.0f) && (0.0f <= w1) && (w1 <= 1.0f) && (0.0f <= w2) && (w2 <= 1.0f);
    float area = fabsf(p0x * p1y - p0y * p1x) / 2.0f;
    return inside && !(area < (float)5e-3) && (norm_normal > (float)1e-8);
}
// ... else the least of the distances to the three edges
template <class Face>
TDS_HD inline float tri_d2(float px, float py, const Face &e) {
    const bool inside = tri_inside(px, py, e);
    float e01 = seg_d2(px, py, e.x0, e.y0, e.x1, e.y1);
    float e02 = seg_d2(px, py, e.x0, e.y0, e.x2, e.y2);
    float e12 = seg_d2(px, py, e.x1, e.y1, e.x2, e.y2);
    float dist = fminf(fminf(e01, e02), e12);
    return inside ? 0.0f : dist;
}
// The gradient of tri_d2 w.r.t. p: zero inside, else that of the nearest edge (the first of v0-v1, v0-v2, v1-v2 among equals).  Only ever
// needed for one face, the nearest.
template <class Face>
TDS_HD inline void tri_d2_grad(float px, float py, const Face &e, float &gx, float &gy) {
    gx = gy = 0.0f;
    if (tri_inside(px, py, e)) return;
    float e01 = seg_d2(px, py, e.x0, e.y0, e.x1, e.y1);
    float e02 = seg_d2(px, py, e.x0, e.y0, e.x2, e.y2);
    float e12 = seg_d2(px, py, e.x1, e.y1, e.x2, e.y2);
    if (e12 < fminf(e01, e02)) seg_d2_grad(px, py, e.x1, e.y1, e.x2, e.y2, gx, gy);
    else if (e02 < e01) seg_d2_grad(px, py, e.x0, e.y0, e.x2, e.y2, gx, gy);
    else seg_d2_grad(px, py, e.x0, e.y0, e.x1, e.y1, gx, gy);
}

// Lower bound of the squared distance from p to anything inside the box, shrunk a little so that rounding can only make a walk look at
// more: a cell, a subtree or a face is left out only if it is certainly farther than the minimum so far, so every walk returns the minimum
// over ALL faces, bit for bit.
TDS_HD inline float box_lb(float px, float py, float x0, float y0, float x1, float y1) {
    const float ex = fmaxf(fmaxf(x0 - px, px - x1), 0.0f), ey = fmaxf(fmaxf(y0 - py, py - y1), 0.0f);
    return (ex * ex + ey * ey) * 0.998f - 1e-3f;
}
// ... to the bounding box of a face
template <class Face>
TDS_HD inline float face_lb(float px, float py, const Face &e) {
    const float x0 = fminf(e.x0, fminf(e.x1, e.x2)), x1 = fmaxf(e.x0, fmaxf(e.x1, e.x2));
    const float y0 = fminf(e.y0, fminf(e.y1, e.y2)), y1 = fmaxf(e.y0, fmaxf(e.y1, e.y2));
    return box_lb(px, py, x0, y0, x1, y1);
}

TDS_HD inline bool finite_point(float px, float py) { return px == px && py == py && !__builtin_isinf(px) && !__builtin_isinf(py); }

// corner k of an agent's box (box2corners_th :285-288): centre (x, y), length, width, [sin, cos] of the heading
struct BoxCorner { float sx, sy, x4, y4, px, py; };
TDS_HD inline BoxCorner box_corner(int k, float x, float y, float length, float width, float sn, float cs) {
    BoxCorner c;
    c.sx = (k == 0 || k == 3) ? 0.5f : -0.5f; c.sy = (k < 2) ? 0.5f : -0.5f;
    c.x4 = c.sx * length; c.y4 = c.sy * width;
    c.px = (c.x4 * cs + c.y4 * (-sn)) + x;
    c.py = (c.x4 * sn + c.y4 * cs) + y;
    return c;
}
// what a corner at squared distance d adds to the agent's value: nan_to_num :171, F.threshold(d, thr, 0) :172
TDS_HD inline float offroad_corner_value(float d, float threshold) {
    d = (d != d) ? 0.0f : d;
    if (__builtin_isinf(d)) d = 3.4028234663852886e38f;
    return (d > threshold) ? d : 0.0f;
}

}  // namespace tds

#ifdef __HIPCC__
#include "tds_common.h"

namespace tds {

// A point is served by a GROUP of NF_LANES consecutive lanes that all hold it; `sub` is the lane's place in its group.  4 consecutive groups
// are the corners of one agent, so a wavefront holds whole agents.  Eight: a lane per child of a hierarchy node (BvhNode).
constexpr int NF_LANES = 8;
constexpr int NF_NONE = 0x7fffffff;

__device__ __forceinline__ float group_min(float v) {
#pragma unroll
    for (int k = 1; k < NF_LANES; k <<= 1) v = fminf(v, __shfl_xor(v, k));
    return v;
}

// What a traversal minimises, and so how it treats ties -- the ONLY difference between the forward's walks and the backward's:
//   ARGMIN = false (offroad_kernel): the distance alone.  Comparisons are strict: a box or candidate whose bound is AT the minimum cannot
//            lower it and stays shut.
//   ARGMIN = true (offroad_bwd_kernel): (distance, lowest face index), torch.min's choice among faces at the same distance.  Bounds AT the
//            minimum are opened: a face behind them may tie it with a lower index.  The gradient is taken once, from the winner.
// The state is the same in all lanes of a group.
template <bool ARGMIN>
struct Nearest {
    float d = __builtin_inff();
    int f = NF_NONE;
    // can something behind this bound still change the result?  (An infinite bound stands for nothing at all: an empty child of a node, a
    // lane beyond the end of a list.)
    __device__ __forceinline__ bool open(float lb) const { return ARGMIN ? lb <= d && lb < __builtin_inff() : lb < d; }
    __device__ __forceinline__ bool shut(float lb) const { return ARGMIN ? lb > d : lb >= d; }
    // every lane of the group brings the face it looked at (inf, NF_NONE: none); the group's best of them against the state
    __device__ __forceinline__ void take(float cd, int cf) {
        if (ARGMIN) {
#pragma unroll
            for (int k = 1; k < NF_LANES; k <<= 1) {
                const float od = __shfl_xor(cd, k);
                const int of = __shfl_xor(cf, k);
                if (od < cd || (od == cd && of < cf)) { cd = od; cf = of; }
            }
            if (cd < d || (cd == d && cf < f)) { d = cd; f = cf; }
        } else {
            d = fminf(d, group_min(cd));
        }
    }
    // the lane looked at face `face` (index fi): a NaN distance never becomes the minimum
    __device__ __forceinline__ void weigh(float px, float py, const GridEntry &face, int fi, float &cd, int &cf) const {
        if (!shut(face_lb(px, py, face))) {
            const float t = tri_d2(px, py, face);
            if (t < __builtin_inff()) { cd = t; cf = fi; }
        }
    }
};

// `stop` (all walks): the caller needs the exact minimum only if it exceeds `stop` (F.threshold zeroes everything else), so a walk ends as
// soon as the running minimum is <= stop.

// The candidate list of the point's cell (NearView; cell (cx, cy) of the lists' grid), walked by the group together: candidate i + sub of
// every round, ended by the first round whose first candidate's bound is shut (the list is sorted by bound).  The minimum over faces does not
// depend on the order in which they are looked at, so the result is a sequential walk's, bit for bit.  (One lane per point was a chain of
// dependent loads, candidate -> face -> next candidates, a few dozen rounds long: 0.148 ms at B = 1024 x 64 forward, 0.09 with eight.)
template <bool ARGMIN>
__device__ __forceinline__ Nearest<ARGMIN> nearest_in_lists(const NearView &nv, int cx, int cy, float px, float py, float stop, int sub) {
    const int s = nv.cand_start[cy * nv.nx + cx], e = nv.cand_start[cy * nv.nx + cx + 1];
    Nearest<ARGMIN> n;
    for (int i = s; i < e && n.d > stop; i += NF_LANES) {
        const int j = i + sub;
        NearCand c;
        c.face = 0; c.lb = __builtin_inff();
        if (j < e) c = nv.cand[j];
        const float lb0 = __shfl(c.lb, (threadIdx.x & 63 & ~(NF_LANES - 1)));         // the round's first candidate
        if (n.shut(lb0)) break;
        float d = __builtin_inff();
        int f = NF_NONE;
        if (n.open(c.lb)) {
            const GridEntry ge = nv.faces[c.face];
            n.weigh(px, py, ge, c.face, d, f);
        }
        n.take(d, f);
    }
    return n;
}

// An ordered descent of the hierarchy over the faces (BvhNode), for the points the lists do not cover.  At an inner node every lane weighs
// ONE of the eight children (a 16-byte box each: one 128-byte line for the group); the open children go onto the group's stack (in LDS)
// farthest first -- a lane finds its place by comparing its bound with the other seven -- and the nearest is taken up at once; at a leaf a
// face per lane.  BLOCK: the including kernel's workgroup size.  (The forward has the same walk in a text of its own: see nearest_face.)  tds_map_create refuses to attach a hierarchy BVH_STACK cannot hold.
// (Two children per node, both weighed by every lane, was three times the depth: 0.60 ms for 65 536 strayed agents.)
template <bool ARGMIN, int BLOCK>
__device__ Nearest<ARGMIN> nearest_in_bvh(const NearView &nv, float px, float py, float stop, int sub) {
    static_assert(NF_LANES == 8, "nearest_in_bvh: a lane per child of a node");
    __shared__ int2 stacks[BLOCK / NF_LANES][BVH_STACK];
    int2 *st = stacks[threadIdx.x / NF_LANES];
    const float inf = __builtin_inff();
    const int shift = (int)(threadIdx.x & 63 & ~(NF_LANES - 1));                      // the group's first lane within the wavefront
    Nearest<ARGMIN> n;
    int sp = 0, cur = 0;
    for (;;) {
        if (cur >= 0) {
            const float4 bx = nv.bvh[cur].box[sub];
            const int ch = nv.bvh[cur].child[sub];
            const float lb = box_lb(px, py, bx.x, bx.y, bx.z, bx.w);
            const bool open = n.open(lb);
            const float key = open ? lb : inf;
            int above = 0;                                                             // open children that will lie above this lane's on the stack
#pragma unroll
            for (int k = 1; k < NF_LANES; ++k) {
                const float o = __shfl_xor(key, k);
                above += (o < key || (o == key && (sub ^ k) < sub)) ? 1 : 0;
            }
            const int nopen = __popc((unsigned)(__ballot(open) >> shift) & 0xffu);
            const int slot = sp + nopen - 1 - above;
            if (open && slot < BVH_STACK) st[slot] = make_int2(ch, __float_as_int(lb));
            sp = min(sp + nopen, BVH_STACK);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else {
            const int code = -1 - cur, first = code >> 4, cnt = code & 15;
            float d = inf;
            int f = NF_NONE;
            if (sub < cnt) {
                const int fi = nv.bvh_idx[first + sub];
                n.weigh(px, py, nv.faces[fi], fi, d, f);
            }
            n.take(d, f);
        }
        // the next subtree that is still open
        float lb;
        do {
            if (sp == 0 || n.d <= stop) return n;
            --sp;
            cur = st[sp].x; lb = __int_as_float(st[sp].y);
        } while (n.shut(lb));
    }
}

// The map's own grid (MapView), walked in rings outwards from the point's cell: for maps without lists, and beyond the lists where there is
// no hierarchy.  A face is listed in every cell its bounding box touches, so its closest point lies in a listed cell whose box is at least as
// close as the face: a cell whose bound is not below the minimum so far is skipped, and the walk ends once the minimum is <= stop, once a
// whole ring is farther than it, or once the rings have covered the grid.  Comparisons are strict for both kernels; what a cell's visit does
// is the kernels' third difference:
//   ARGMIN = false: the group shares the cell's entries (entry i + sub of every round, faces whose box bound is shut left out) and agrees on
//            the minimum after every cell;
//   ARGMIN = true:  every lane walks alone over every entry, the same point and so the same answer in all of them, and the FIRST face met
//            wins a tie (the hierarchy and the lists take the lowest index).  Nearest::f is an index into m.entries here.
template <bool ARGMIN>
__device__ __forceinline__ Nearest<ARGMIN> nearest_in_rings(const MapView &m, float px, float py, float stop, int sub) {
    Nearest<ARGMIN> n;
    if (m.nx <= 0 || !finite_point(px, py)) return n;
    // unclamped cell of the point (float -> int conversion saturates, keep it in a sane range first)
    float fx = fminf(fmaxf((px - m.ox) * m.inv_cell, -1.0e6f), 1.0e6f), fy = fminf(fmaxf((py - m.oy) * m.inv_cell, -1.0e6f), 1.0e6f);
    int cx = (int)floorf(fx), cy = (int)floorf(fy);
    auto visit = [&](int x, int y) {
        float bx0 = m.ox + (float)x * m.cell, by0 = m.oy + (float)y * m.cell;
        if (box_lb(px, py, bx0, by0, bx0 + m.cell, by0 + m.cell) >= n.d || n.d <= stop) return;
        const int s = m.cell_start[y * m.nx + x], e = m.cell_start[y * m.nx + x + 1];
        if (ARGMIN) {
            for (int i = s; i < e && n.d > stop; ++i) {
                const float d = tri_d2(px, py, m.entries[i]);
                if (d < n.d) { n.d = d; n.f = i; }
            }
        } else {
            float mine = n.d;
            for (int i = s + sub; i < e; i += NF_LANES) {
                const GridEntry ge = m.entries[i];
                if (face_lb(px, py, ge) >= mine) continue;
                float d = tri_d2(px, py, ge);
                mine = (d < mine) ? d : mine;                // a NaN distance never becomes the minimum
            }
            n.d = group_min(mine);
        }
    };
    int k = max(max(0, max(-cx, cx - (m.nx - 1))), max(-cy, cy - (m.ny - 1)));
    for (;; ++k) {
        // cells at Chebyshev distance exactly k from (cx, cy), clipped to the grid
        int y0 = max(cy - k, 0), y1 = min(cy + k, m.ny - 1);
        int x0 = max(cx - k, 0), x1 = min(cx + k, m.nx - 1);
        for (int y = y0; y <= y1; ++y) {
            if (y == cy - k || y == cy + k) {
                for (int x = x0; x <= x1; ++x) visit(x, y);
            } else {
                if (cx - k >= 0 && cx - k < m.nx) visit(cx - k, y);
                if (k > 0 && cx + k >= 0 && cx + k < m.nx) visit(cx + k, y);
            }
        }
        if (n.d <= stop) break;
        float bound = (float)k * m.cell * 0.999f;            // everything unvisited is at least this far away
        if (n.d <= bound * bound) break;
        if (cx - k <= 0 && cx + k >= m.nx - 1 && cy - k <= 0 && cy + k >= m.ny - 1) break;
    }
    return n;
}

// The nearest face of p: its squared distance (inf: no face, or p is not finite) and, for ARGMIN, the face itself (null: none).  The lists
// where p lies inside their grid; beyond it the hierarchy where the map has one, else the rings.  (Uniform within the group.)  `in_bvh`: the
// kernel's walk of the hierarchy, (nv, px, py, stop, sub) -> Nearest<ARGMIN>: nearest_in_bvh for the backward; the forward keeps the walk it
// had (map.hip: nearest_face_d2_bvh), because nearest_in_bvh<false> measured 1.4 % slower on agents that strayed from the map.
struct NearestFace { float d2; const GridEntry *face; };
template <bool ARGMIN>
__device__ __forceinline__ NearestFace nearest_face_of(const Nearest<ARGMIN> &n, const GridEntry *faces) {
    return NearestFace{n.d, ARGMIN && n.f != NF_NONE ? faces + n.f : nullptr};
}
template <bool ARGMIN, class Hierarchy>
__device__ __forceinline__ NearestFace nearest_face(const MapView &m, const NearView &nv, float px, float py, float stop, int sub, Hierarchy in_bvh) {
    const bool finite = finite_point(px, py);
    bool beyond = nv.cand == nullptr || m.nx <= 0 || !finite;
    int cx = 0, cy = 0;
    if (!beyond) {                                           // inside the lists' grid?
        const float fx = (px - nv.ox) * m.inv_cell, fy = (py - nv.oy) * m.inv_cell;
        beyond = !(fx >= 0.0f && fy >= 0.0f && fx < (float)nv.nx && fy < (float)nv.ny);
        if (!beyond) {
            cx = cell_coord(px, nv.ox, m.inv_cell); cy = cell_coord(py, nv.oy, m.inv_cell);
            beyond = cx < 0 || cy < 0 || cx >= nv.nx || cy >= nv.ny;
        }
    }
    if (beyond) {
        if (nv.bvh != nullptr && finite) return nearest_face_of<ARGMIN>(in_bvh(nv, px, py, stop, sub), nv.faces);
        return nearest_face_of(nearest_in_rings<ARGMIN>(m, px, py, stop, sub), m.entries);
    }
    return nearest_face_of(nearest_in_lists<ARGMIN>(nv, cx, cy, px, py, stop, sub), nv.faces);
}

// ---- what the two kernels do before and after ---------------------------------------------------------------------------------------------
// a thread of the launch (workgroups of BLOCK threads) -> agent, corner of its box, place in the corner's group
struct NearLane { int64_t a; int k, sub; };
template <int BLOCK>
__device__ __forceinline__ NearLane near_lane() {
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    NearLane l;
    l.a = t / (4 * NF_LANES); l.k = (int)((t / NF_LANES) & 3); l.sub = (int)(t & (NF_LANES - 1));
    return l;
}
inline unsigned near_blocks(int64_t n_agents, int block) { return (unsigned)((n_agents * 4 * NF_LANES + block - 1) / block); }
// one map per scene (the _multi entry points): agent a's scene selects its map from the set
__device__ __forceinline__ void select_scene_map(MapView &m, NearView &nv, const MapView *views, const NearView *nears, const int32_t *scene_map,
                                                 int64_t a, int agents_per_scene) {
    if (views == nullptr) return;
    const int im = scene_map[a / agents_per_scene];
    m = views[im]; nv = nears[im];
}
__device__ __forceinline__ BoxCorner box_corner(int k, float4 state, float2 lenwid, float2 sc) {
    return box_corner(k, state.x, state.y, lenwid.x, lenwid.y, sc.x, sc.y);
}

}  // namespace tds
#endif  // __HIPCC__

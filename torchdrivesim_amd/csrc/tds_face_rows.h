// The row rule of the scene rasteriser (raster.hip): how the outline edges of a triangle that lie inside the image are merged into the rows
// of OpenCV's 16.16 edge chains, and the rows of the three vertices, which process_batch_bits and process_small_bits both paint by these
// functions.  Plain integer arithmetic that a host compiler takes as it is (tests/small_block_model.cpp calls it on the CPU and holds it to
// the oracle's cv::fillConvexPoly).  Nothing else belongs here: bench.py's source stamp hashes raster.hip, not this header -- only per-face
// arithmetic that cannot change what a kernel reads or writes in memory.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "tds_short_slope.h"

#define TDS_HD_INLINE TDS_HD __inline__ __attribute__((always_inline))

TDS_HD_INLINE int tds_min(int a, int b) { return a < b ? a : b; }
TDS_HD_INLINE int tds_max(int a, int b) { return a > b ? a : b; }

TDS_HD inline uint32_t pack_xy(int x, int y) { return ((uint32_t)x & 0xffffu) | ((uint32_t)y << 16); }
TDS_HD inline int unpack_x(uint32_t p) { return (int)(short)(p & 0xffffu); }
TDS_HD inline int unpack_y(uint32_t p) { return (int)p >> 16; }
// packed vertices (x & 0xffff | y << 16) compare like (y, x): sorted by row with three instructions
TDS_HD_INLINE int top_vertex(uint32_t v0, uint32_t v1, uint32_t v2) { return tds_min((int)v0, tds_min((int)v1, (int)v2)); }
TDS_HD_INLINE int bottom_vertex(uint32_t v0, uint32_t v1, uint32_t v2) { return tds_max((int)v0, tds_max((int)v1, (int)v2)); }
TDS_HD_INLINE int middle_vertex(uint32_t v0, uint32_t v1, uint32_t v2) { return tds_max(tds_min((int)v0, (int)v1), tds_min(tds_max((int)v0, (int)v1), (int)v2)); }

// For an edge that lies inside the image (cv::Line does not clip it) the pixels of the edge in a row and the scan-converted span of that row
// are ONE run of pixels, and its ends follow from the 16.16 edge chain of the scan conversion by an add and a shift -- the edge is never walked:
//   y-major (|dy| > |dx|): cv::Line paints x(tau) = x0 + dx tau / |dy| rounded to nearest, a tie going to the LEFT pixel (either direction
//     of the walk); the span ends at floor(chain + 1/2).  Left end: floor(chain + 1/2 - BIAS), right end unchanged.
//   x-major: row tau holds the pixels x with x(tau - 1/2) < x <= x(tau + 1/2), cut at the edge's end points:
//     floor(chain - slope/2 + BIAS) + 1 .. floor(chain + slope/2 + BIAS), merged with the span by min / max.
// The chain strays from the exact line: OpenCV's slope is trunc(q + 1/2) in units of 2^-16, i.e. within 1/2 unit of q for q >= 0 but
// between 1/2 and 3/2 units ABOVE it for q < 0, per row.  The half-row positions of the exact line are multiples of 1/(2|dy|): BIAS must
// exceed the accumulated error and, with it, stay below 1/(2|dy|) -- 160 units for |dy| <= 100 (3/2 * 100 < 160, 160 + 150 < 32768 / 100).
constexpr int MERGE_BIAS = 160;

// class of an edge: bit 0: the edge is merged into the rows, bit 1: x-major, bit 2: biased (raster.hip: edge_class).  A short edge with
// both end points inside the image (|dy| <= 100: every edge of a small face) is merged and biased:
TDS_HD_INLINE unsigned short_edge_class(int ax, int ay, int bx, int by) { return 5u | ((abs(bx - ax) >= abs(by - ay)) ? 2u : 0u); }

// row ends of a chain that follows an edge of class `cls` with 16.16 slope s: left = (x + offL) >> 16, right = (x + offR) >> 16
TDS_HD_INLINE void edge_offsets(unsigned cls, int s, int &offL, int &offR) {
    // selects, no branches: neighbouring lanes hold edges of every class
    const int bias = (cls & 4u) ? MERGE_BIAS : 0;
    const int h = abs(s) >> 1;
    const bool mx = (cls & 3u) == 3u;
    const int yl = 32768 - ((cls & 1u) ? bias : 0);
    const int xl = tds_min(32768, 65536 - h + bias), xr = tds_max(32768, h + bias);
    offL = mx ? xl : yl;
    offR = mx ? xr : 32768;
}
// the pixels of a merged edge in the row of its end point x0: x0 itself and, x-major, the run from x0 towards x0 + d (d = half a row's
// advance along the edge, 16.16, signed)
TDS_HD_INLINE void edge_reach(unsigned cls, int x0, int d, int &L, int &R) {
    if (cls & 1u) {
        L = tds_min(L, x0); R = tds_max(R, x0);
        if (cls & 2u) {
            const int v = ((x0 << 16) + d + ((cls & 4u) ? MERGE_BIAS : 0)) >> 16;       // a merged edge lies inside the image: x0 >= 0
            if (d >= 0) R = tds_max(R, v); else L = tds_min(L, v + 1);
        }
    }
}
TDS_HD_INLINE int half_slope(int s) { return s >= 0 ? (s >> 1) : -((-s) >> 1); }
// the slope over one row, edge_dx(xs, xe, 1) = trunc((xe - xs) * 65536 + 1/2) with C's truncation: (xe - xs) << 16 for xe >= xs and
// ((xe - xs) << 16) + 1 below
TDS_HD_INLINE int slope_one_row(int xs, int xe) { const int d = xe - xs; return d >= 0 ? d << 16 : (int)(((unsigned)d << 16) + 1u); }

// ---- the rows of the three vertices of a face of at least two rows (yt < yb) ----
// The vertices by row (T, M, B), the classes and the 16.16 slopes of the edges T->M, M->B, T->B (slope 0 for an edge in one row).  These
// rows are painted apart from the rows in between: the runs of the merged edges are cut at their end points there.
struct FaceEdges {
    int xt, yt, xm, ym, xb, yb;
    unsigned cTM, cMB, cTB;
    int sTM, sMB, sTB;
};
// the row of the top vertex (two of them: the span between them): both chains start here
TDS_HD_INLINE void face_row_top(const FaceEdges f, int &L, int &R) {
    L = f.xt; R = f.xt;
    if (f.ym > f.yt) edge_reach(f.cTM, f.xt, half_slope(f.sTM), L, R);
    else { L = tds_min(f.xt, f.xm); R = tds_max(f.xt, f.xm); edge_reach(f.cMB, f.xm, half_slope(f.sMB), L, R); }
    edge_reach(f.cTB, f.xt, half_slope(f.sTB), L, R);
}
// the row of the middle vertex when it lies strictly between the others (yt < ym < yb): T->M ends, M->B starts, T->B passes
// (chain positions in unsigned: a product may wrap, the sums do not)
TDS_HD_INLINE void face_row_middle(const FaceEdges f, int &L, int &R) {
    int oL, oR;
    edge_offsets(f.cTB, f.sTB, oL, oR);
    const int xc = (int)(((unsigned)f.xt << 16) + (unsigned)(f.ym - f.yt) * (unsigned)f.sTB);
    L = tds_min(f.xm, (xc + oL) >> 16); R = tds_max(f.xm, (xc + oR) >> 16);
    edge_reach(f.cTM, f.xm, -half_slope(f.sTM), L, R);
    edge_reach(f.cMB, f.xm, half_slope(f.sMB), L, R);
}
// the row of the bottom vertex is never scan-converted: the last pixels of the merged edges that end there (L > R: none)
TDS_HD_INLINE void face_row_bottom(const FaceEdges f, int &L, int &R) {
    L = 0x7fffffff; R = -0x7fffffff;
    edge_reach(f.cTB, f.xb, -half_slope(f.sTB), L, R);
    if (f.ym < f.yb) edge_reach(f.cMB, f.xb, -half_slope(f.sMB), L, R);
    else {
        edge_reach(f.cTM, f.xm, -half_slope(f.sTM), L, R);
        if (f.cMB & 1u) { L = tds_min(L, tds_min(f.xm, f.xb)); R = tds_max(R, tds_max(f.xm, f.xb)); }      // the horizontal bottom edge
    }
}

/* Test infrastructure: the block that paints a SMALL face on the lane that scanned it (torchdrivesim_amd/csrc/raster.hip:
 * process_small_bits<ROWS>, ROWS > 2) run on the CPU, checked against the oracle's restatement of cv::fillConvexPoly (oracle/tds_oracle.c)
 * triangle by triangle.  The row rule is the kernel's own code, compiled for the host: the sort by row, the classes of the short edges, the
 * rows of the three vertices and the row ends of the chains (tds_face_rows.h), the slopes (tds_short_slope.h: edge_dx_short).  What the
 * model states itself is what the kernel keeps beside its stores: the order of the rows and the loop over the rows that hold no vertex, from
 * row ends set up once relative to the top row (32-bit unsigned arithmetic: a product may wrap, the sums do not).
 * tests/small_rows_model.c is the block's earlier form, written independently, and stays.
 *
 * usage: small_block_model ROWS exhaustive RES OFFSET N | ROWS random RES COUNT SEED | ROWS wide RES
 *        ("oldrows-..." paints the middle vertex's row as a row of part 1, which the check must notice)
 * exit status 0 = no differing pixel, none skipped.  Build + run: tests/test_small_block_model.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tds_face_rows.h"
#include "tds_short_slope.h"

extern "C" void orc_fill_convex_poly(float *img, int W, int H, const int32_t *pts, int npts, const float *col);

static int BROKEN = 0;
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

static uint8_t *g_mask; static int g_W, g_H, ROWS;
static void paint_row(int y, int L, int R) {
    const int s0 = imax(L, 0), s1 = imin(R, g_W - 1);
    if (y < 0 || y >= g_H) { fprintf(stderr, "row %d outside the image\n", y); exit(3); }
    for (int x = s0; x <= s1; ++x) g_mask[y * g_W + x] = 1;
}

/* the dynamic test of drain_bits */
static int is_small(const int32_t *p) {
    for (int i = 0; i < 3; ++i) if (p[2 * i] < 0 || p[2 * i] >= g_W || p[2 * i + 1] < 0 || p[2 * i + 1] >= g_H) return 0;
    const int yt = imin(p[1], imin(p[3], p[5])), yb = imax(p[1], imax(p[3], p[5]));
    return yb - yt <= ROWS - 1;
}

static void model_small(const int32_t *p) {
    const uint32_t v0 = pack_xy(p[0], p[1]), v1 = pack_xy(p[2], p[3]), v2 = pack_xy(p[4], p[5]);
    const int pT = top_vertex(v0, v1, v2), pB = bottom_vertex(v0, v1, v2), pM = middle_vertex(v0, v1, v2);
    const int xt = unpack_x((uint32_t)pT), yt = unpack_y((uint32_t)pT), xm = unpack_x((uint32_t)pM), ym = unpack_y((uint32_t)pM);
    const int xb = unpack_x((uint32_t)pB), yb = unpack_y((uint32_t)pB);
    if (yt == yb) { paint_row(yt, imin(xt, imin(xm, xb)), imax(xt, imax(xm, xb))); return; }
    const unsigned cTM = short_edge_class(xt, yt, xm, ym), cMB = short_edge_class(xm, ym, xb, yb), cTB = short_edge_class(xt, yt, xb, yb);
    const int sTB = edge_dx_short(xt, xb, yb - yt);
    const int sTM = ym > yt ? edge_dx_short(xt, xm, ym - yt) : 0;
    const int sMB = yb > ym ? edge_dx_short(xm, xb, yb - ym) : 0;
    const FaceEdges f{xt, yt, xm, ym, xb, yb, cTM, cMB, cTB, sTM, sMB, sTB};
    int L, R;
    face_row_top(f, L, R);
    paint_row(yt, L, R);
    if (ym > yt && ym < yb && !BROKEN) {
        face_row_middle(f, L, R);
        paint_row(ym, L, R);
    }
    int oLb, oRb, oL1, oR1, oL2, oR2;
    edge_offsets(cTB, sTB, oLb, oRb);
    edge_offsets(cTM, sTM, oL1, oR1);
    edge_offsets(cMB, sMB, oL2, oR2);
    const unsigned xt16 = (unsigned)xt << 16;
    const unsigned x2 = ((unsigned)xm << 16) - (unsigned)(ym - yt) * (unsigned)sMB;
    const unsigned l1 = xt16 + (unsigned)oL1, r1 = xt16 + (unsigned)oR1, l2 = x2 + (unsigned)oL2, r2 = x2 + (unsigned)oR2;
    const unsigned lb = xt16 + (unsigned)oLb, rb = xt16 + (unsigned)oRb;
    for (int j = 1; j <= ROWS - 2; ++j) {
        const int y = yt + j;
        if (y >= yb) break;
        const int second = y > ym;
        const unsigned sA = (unsigned)(second ? sMB : sTM) * (unsigned)j, sB = (unsigned)sTB * (unsigned)j;
        if (y != ym || BROKEN) paint_row(y, imin((int)((second ? l2 : l1) + sA), (int)(lb + sB)) >> 16, imax((int)((second ? r2 : r1) + sA), (int)(rb + sB)) >> 16);
    }
    face_row_bottom(f, L, R);
    paint_row(yb, L, R);
}

static long g_checked, g_bad, g_skipped;
static void check(const int32_t *pts, float *img) {
    const float one[3] = {1, 1, 1};
    if (!is_small(pts)) { ++g_skipped; return; }
    orc_fill_convex_poly(img, g_W, g_H, pts, 3, one);
    model_small(pts);
    ++g_checked;
    /* the whole image for small images, else the rows of the face and two around them (both sides paint only rows yt .. yb; the model
     * refuses any other row) over the full width */
    int y0 = 0, y1 = g_H - 1;
    if (g_H > 32) { y0 = imax(imin(pts[1], imin(pts[3], pts[5])) - 2, 0); y1 = imin(imax(pts[1], imax(pts[3], pts[5])) + 2, g_H - 1); }
    int bad = 0;
    for (int i = y0 * g_W; i < (y1 + 1) * g_W; ++i) {
        const int ref = img[3 * i] != 0.0f, got = g_mask[i];
        if (ref != got && !bad) {
            if (g_bad < 10) fprintf(stderr, "differs at (x %d, y %d): oracle %d model %d for (%d,%d) (%d,%d) (%d,%d) in %dx%d\n", i % g_W, i / g_W, ref, got,
                                    pts[0], pts[1], pts[2], pts[3], pts[4], pts[5], g_W, g_H);
            bad = 1;
        }
    }
    g_bad += bad;
    memset(img + 3 * (size_t)y0 * g_W, 0, sizeof(float) * 3 * (size_t)(y1 - y0 + 1) * g_W);
    memset(g_mask + (size_t)y0 * g_W, 0, (size_t)(y1 - y0 + 1) * g_W);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s ROWS exhaustive RES OFFSET N | ROWS random RES COUNT SEED | ROWS wide RES\n", argv[0]); return 2; }
    ROWS = atoi(argv[1]);
    const char *mode = argv[2];
    if (!strncmp(mode, "oldrows-", 8)) { BROKEN = 1; mode += 8; }
    g_W = g_H = atoi(argv[3]);
    float *img = (float *)calloc((size_t)3 * g_W * g_H, sizeof(float));
    g_mask = (uint8_t *)calloc((size_t)g_W * g_H, 1);
    if (!strcmp(mode, "exhaustive") && argc >= 6) {
        /* every triangle with its vertices on the N x N grid whose corner is (OFFSET, OFFSET) */
        const int lo = atoi(argv[4]), hi = lo + atoi(argv[5]) - 1;
        int32_t p[6];
        for (p[0] = lo; p[0] <= hi; ++p[0]) for (p[1] = lo; p[1] <= hi; ++p[1])
        for (p[2] = lo; p[2] <= hi; ++p[2]) for (p[3] = lo; p[3] <= hi; ++p[3])
        for (p[4] = lo; p[4] <= hi; ++p[4]) for (p[5] = lo; p[5] <= hi; ++p[5]) check(p, img);
    } else if (!strcmp(mode, "wide")) {
        /* flat wide faces: every height of 2 .. ROWS rows, the middle vertex in every row from the top to the bottom, every width from 8 pixels to
         * the image's, the middle vertex left of, between and right of the others, every order of the vertices (both directions of every edge) */
        static const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        for (int h = 1; h <= ROWS - 1; ++h) for (int m = 0; m <= h; ++m) for (int wid = 8; wid <= g_W - 1; ++wid) for (int kind = 0; kind < 6; ++kind) {
            const int x0 = (wid * 7 + h * 13 + m) % (g_W - wid), y0 = (wid + 5 * h) % (g_H - h);
            /* x of (top, middle, bottom): the long edge T->B left to right or right to left, the middle vertex beside, between, beyond */
            const int fwd = kind & 1, pos = kind >> 1;
            const int xT = fwd ? x0 : x0 + wid, xB = fwd ? x0 + wid : x0;
            const int xM = pos == 0 ? x0 + wid / 3 : (pos == 1 ? x0 : x0 + wid);
            const int v[3][2] = {{xT, y0}, {xM, y0 + m}, {xB, y0 + h}};
            for (int o = 0; o < 6; ++o) {
                int32_t p[6];
                for (int i = 0; i < 3; ++i) { p[2 * i] = v[order[o][i]][0]; p[2 * i + 1] = v[order[o][i]][1]; }
                check(p, img);
            }
        }
    } else if (!strcmp(mode, "random") && argc >= 6) {
        /* at most ROWS rows, any width: slivers along a row, faces that touch the border of the image, flat tops and bottoms */
        const long count = atol(argv[4]);
        rng_state ^= (uint64_t)atol(argv[5]) * 0x2545F4914F6CDD1Dull;
        for (long n = 0; n < count; ++n) {
            int32_t p[6];
            const int kind = (int)(rnd() % 3), y0 = rnd_range(0, g_H - ROWS);
            const int wid = kind == 0 ? g_W - 1 : (kind == 1 ? 12 : 3), x0 = rnd_range(0, g_W - 1 - wid);
            for (int i = 0; i < 3; ++i) { p[2 * i] = x0 + rnd_range(0, wid); p[2 * i + 1] = y0 + rnd_range(0, ROWS - 1); }
            if (rnd() % 8 == 0) p[0] = (rnd() & 1) ? 0 : g_W - 1;
            if (rnd() % 8 == 0) p[3] = (rnd() & 1) ? imax(0, imin(p[1], p[5])) : imin(g_H - 1, imax(p[1], p[5]));
            check(p, img);
        }
    } else { fprintf(stderr, "unknown mode %s\n", mode); return 2; }
    free(img); free(g_mask);
    printf("%ld triangles, %ld differ, %ld not small\n", g_checked, g_bad, g_skipped);
    return g_bad || g_skipped ? 1 : 0;
}

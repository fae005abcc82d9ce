// OpenCV's 16.16 edge slope for the scene rasteriser (raster.hip): the general form over two short divisions and the short form for the
// edges of small faces, which needs no division and no correction step.  Plain integer and float arithmetic that a host compiler takes as
// it is (tests/short_slope_host.cpp holds both to the 64-bit statement on the CPU).  Nothing else belongs here: bench.py's source stamp
// hashes raster.hip, not this header.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif

#ifdef __HIP_DEVICE_COMPILE__
#define TDS_SLOPE_RCP(x) __builtin_amdgcn_rcpf(x)          // v_rcp_f32: within one ulp
#define TDS_SLOPE_MUL24(a, b) __umul24(a, b)
#else
#define TDS_SLOPE_RCP(x) (1.0f / (x))
#define TDS_SLOPE_MUL24(a, b) ((unsigned)(a) * (unsigned)(b))
#endif

// n / d for n < 2^31, 1 <= d < 2^16 and a quotient of at most 2^16: the fp32 estimate (24-bit operand, v_rcp_f32, one product: relative
// error below 2^-22) is within 0.02 of the exact quotient, so its floor is off by at most one and one correction step in integers makes
// it exact (q and d fit the 24-bit multiplier, q d < 2^32)
TDS_HD __inline__ __attribute__((always_inline)) unsigned udiv_small(unsigned n, unsigned d) {
    unsigned q = (unsigned)((float)n * TDS_SLOPE_RCP((float)d));
    int r = (int)(n - TDS_SLOPE_MUL24(q, d));
    if (r < 0) --q;
    else if (r >= (int)d) ++q;
    return q;
}

// OpenCV's edge slope ((xe - xs) * 2 + dy) / (2 * dy) in 16.16 fixed point, C truncating division.
// With N = (xe - xs) << 16 this is trunc(N / dy + 1/2):
//   N >= 0: a + (2 r >= dy);   N < 0: -(a - (2 r < dy)),   a, r = divmod(|N|, dy)
// (for N < 0 the case 2|N| <= dy -> 0 of the general formula cannot occur: |N| >= 65536 > dy).  |xe - xs| and dy are below 2^15 (packed
// coordinate range), so divmod(|N|, dy) is two short divisions: |xe - xs| = hi dy + r1, then (r1 << 16) = lo dy + r  ->  a = hi << 16 | lo.
// A 32-bit unsigned division costs the compiler two quarter-rate multiplies and twenty instructions; there are four per face.
TDS_HD inline int edge_dx(int xs, int xe, int dyy) {
    const int dxs = xe - xs;
    const unsigned D = (unsigned)abs(dxs), d = (unsigned)dyy;
    const unsigned hi = udiv_small(D, d), r1 = D - TDS_SLOPE_MUL24(hi, d);
    const unsigned lo = udiv_small(r1 << 16, d), r = (r1 << 16) - TDS_SLOPE_MUL24(lo, d);
    const unsigned a = (hi << 16) + lo;
    if (dxs >= 0) return (int)(a + ((2u * r >= d) ? 1u : 0u));
    return -(int)(a - ((2u * r < d) ? 1u : 0u));
}

// The same value for the edges of SMALL faces: 1 <= dy <= TDS_SHORT_SLOPE_MAX_DY rows, |xe - xs| <= TDS_SHORT_SLOPE_MAX_DX (every
// difference of two packed coordinates the rasteriser accepts: |coordinate| < 16000).  Both halves of the quotient come out of the float
// unit without a correction step, because with so small a divisor the exact quotients keep clear of the integers:
//   hi = floor(D / dy), D = |xe - xs|: D / dy is a multiple of 1 / dy, so its fraction is at most 1 - 1/dy <= 5/6.  D rc + 1/16 with
//     rc = 1 / dy to one ulp is off by less than 2^15 (2^-22 + 2^-24) < 2^-6: it lies in [k + 1/16 - 2^-6, k + 5/6 + 1/16 + 2^-6], inside
//     [k, k + 1), and floor gives hi.
//   r1 = D - hi dy, one fma: exact (the result, below dy, has a handful of bits).
//   lo + round-up = trunc(r1 65536 / dy + 1/2): r1 65536 / dy is an integer or has a fraction of k/3 or k/5 (2^17 r1 = dy (2 k + 1) has no
//     solution: never 1/2), so the exact value + 1/2 stays 1/10 away from every integer unless it is one + 1/2; (r1 rc) 65536 + 1/2 is
//     off by less than 2^16 2^-22 = 2^-6, and the truncation gives lo + (2 r >= dy).
// So A = (hi << 16) + that is a + (2 r >= dy), the slope for xe >= xs; below, -(a - (2 r < dy)) = -(a - 1 + (2 r >= dy)) = 1 - A.
// The fma calls are the operations meant (one rounding), not contractions: -ffp-contract=off stays.  `rc` is a parameter so that the host
// test can hand in the reciprocal an ulp off either way, as v_rcp_f32 may.
#define TDS_SHORT_SLOPE_MAX_DY 6
#define TDS_SHORT_SLOPE_MAX_DX 32767
TDS_HD __inline__ __attribute__((always_inline)) int edge_dx_short_rc(int xs, int xe, int dyy, float rc) {
    const int dxs = xe - xs;
    const float Df = fabsf((float)dxs), df = (float)dyy;
    const float hif = floorf(fmaf(Df, rc, 0.0625f));
    const float r1f = fmaf(-hif, df, Df);
    const float lrf = fmaf(r1f * rc, 65536.0f, 0.5f);
    const int A = ((int)hif << 16) + (int)lrf;
    return dxs >= 0 ? A : 1 - A;
}
TDS_HD __inline__ __attribute__((always_inline)) int edge_dx_short(int xs, int xe, int dyy) {
    return edge_dx_short_rc(xs, xe, dyy, TDS_SLOPE_RCP((float)dyy));
}

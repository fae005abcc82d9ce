/* Test infrastructure: the rasteriser's edge slopes (torchdrivesim_amd/csrc/tds_short_slope.h) compiled for the HOST and held to OpenCV's
 * statement in 64-bit integers, ((xe - xs) << 17) + dy) / (2 dy) with C's truncating division.
 *   short form: every dy in 1 .. TDS_SHORT_SLOPE_MAX_DY and every dx in -TDS_SHORT_SLOPE_MAX_DX .. TDS_SHORT_SLOPE_MAX_DX, with the exactly
 *     rounded reciprocal and with the reciprocal one ulp off either way (what v_rcp_f32 may return), at two positions of the edge;
 *   general form (edge_dx, moved into the header unchanged): a seeded sample over the packed coordinate range with dy up to 255, plus the
 *     short form's whole domain.
 * Prints one line per part; exit status 0 = no differing value.  Build + run: tests/test_short_slope_host.py. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "tds_short_slope.h"

/* (<< 17 written as a product: shifting a negative value left is undefined before C++20) */
static int statement(int xs, int xe, int dy) { return (int)(((int64_t)(xe - xs) * 131072 + dy) / (2 * (int64_t)dy)); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
static int rnd_range(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

int main(int argc, char **argv) {
    const long samples = argc > 1 ? atol(argv[1]) : 200000;
    const int force_bad = argc > 2 && atoi(argv[2]);                /* the check of the check: a reciprocal 64 ulp off must be noticed */
    long n_short = 0, bad_short = 0, n_gen = 0, bad_gen = 0;
    for (int dy = 1; dy <= TDS_SHORT_SLOPE_MAX_DY; ++dy) {
        const float rc = 1.0f / (float)dy;
        float rcs[3] = {rc, nextafterf(rc, 0.0f), nextafterf(rc, 2.0f)};
        if (force_bad) for (int k = 0; k < 64; ++k) rcs[1] = nextafterf(rcs[1], 0.0f);
        for (int dx = -TDS_SHORT_SLOPE_MAX_DX; dx <= TDS_SHORT_SLOPE_MAX_DX; ++dx) {
            const int want = statement(0, dx, dy);
            /* the edge from 0 and, inside the packed range, from a coordinate that puts both ends off zero */
            const int xs = dx >= 0 ? -(dx / 2) : (-dx) / 2;
            int ok = edge_dx_short(0, dx, dy) == want && edge_dx_short(xs, xs + dx, dy) == want;
            for (int k = 0; k < 3; ++k) ok = ok && edge_dx_short_rc(0, dx, dy, rcs[k]) == want;
            ++n_short;
            if (!ok) {
                if (bad_short < 10) fprintf(stderr, "short form differs: dx %d dy %d: want %d got %d / %d / %d\n", dx, dy, want, edge_dx_short_rc(0, dx, dy, rcs[0]),
                                            edge_dx_short_rc(0, dx, dy, rcs[1]), edge_dx_short_rc(0, dx, dy, rcs[2]));
                ++bad_short;
            }
            ++n_gen;
            if (edge_dx(0, dx, dy) != want) ++bad_gen;
        }
    }
    for (long i = 0; i < samples; ++i) {
        /* |dx| and dy below 2^15, dy mostly short; a quarter of the edges a few pixels wide */
        const int dy = (i & 3) == 0 ? rnd_range(1, 32767) : rnd_range(1, 255);
        const int wid = (i & 7) == 1 ? 8 : 32767;
        const int xs = rnd_range(-16383, 16383), dx = rnd_range(-wid, wid);
        int xe = xs + dx;
        if (xe - xs > 32767 || xs - xe > 32767) xe = xs;
        const int want = statement(xs, xe, dy);
        ++n_gen;
        if (edge_dx(xs, xe, dy) != want) {
            if (bad_gen < 10) fprintf(stderr, "edge_dx differs: xs %d xe %d dy %d: want %d got %d\n", xs, xe, dy, want, edge_dx(xs, xe, dy));
            ++bad_gen;
        }
    }
    printf("short %ld cases, %ld differ\n", n_short, bad_short);
    printf("general %ld cases, %ld differ\n", n_gen, bad_gen);
    return bad_short || bad_gen ? 1 : 0;
}

// The lane kernels' shared arithmetic (torchdrivesim_amd/csrc/tds_lane_math.h) compiled by a host compiler and printed for
// tests/test_lane_math_host.py: Philox4x32-10 on Random123's known-answer inputs, the scaled pick, and the segment search and the point at an
// arc length on a small centre line.  Doubles are printed as hexadecimal floats: every bit, the sign of a zero included.
#include <stdio.h>

#include "tds_lane_math.h"

int main() {
    const uint32_t ones = 0xFFFFFFFFu;
    const tds::U4 counters[3] = {{0, 0, 0, 0}, {ones, ones, ones, ones}, {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
    const uint32_t keys[3][2] = {{0, 0}, {ones, ones}, {0xa4093822u, 0x299f31d0u}};
    for (int i = 0; i < 3; ++i) {
        const tds::U4 r = tds::philox4x32_10(counters[i], keys[i][0], keys[i][1]);
        printf("philox %08x %08x %08x %08x\n", r.x, r.y, r.z, r.w);
    }
    const uint32_t words[4] = {0u, 0x7FFFFFFFu, 0x80000000u, ones};
    for (int n = 1; n <= 7; n += 3)
        for (uint32_t w : words) printf("pick %08x %d %d\n", w, n, tds::pick_of(w, n));

    // five points, the third repeats the second: segment 1 has no length.  The line starts at x = -0 and runs towards negative x, so a zero
    // parameter times dx is a negative zero.
    const int n = 5;
    const double cl[3 * n] = {-0.0, 0.0, 0.0, -3.0, 4.0, 0.0, -3.0, 4.0, 0.0, -1.0, 10.0, 1.0, -1.0, 12.0, 1.0};
    double cum[n] = {0.0};
    for (int i = 1; i < n; ++i) {                                            // as tds_lanes_create sums it
        const double dx = cl[3 * i] - cl[3 * i - 3], dy = cl[3 * i + 1] - cl[3 * i - 2], dz = cl[3 * i + 2] - cl[3 * i - 1];
        const double seg = sqrt((dx * dx + dy * dy) + dz * dz);
        cum[i] = i == 1 ? seg : cum[i - 1] + seg;
    }
    for (int i = 0; i < n; ++i) printf("point %a %a %a %a\n", cl[3 * i], cl[3 * i + 1], cl[3 * i + 2], cum[i]);
    // before the line, its start, inside a segment, an interior point, the repeated point, the end, beyond it, not a number
    const double arcs[8] = {-1.5, 0.0, 2.5, cum[3], cum[1], cum[n - 1], cum[n - 1] + 1.0, NAN};
    for (double s : arcs) {
        const int k = tds::segment_of(cum, n, s);
        const tds::ArcPoint p = tds::point_at_arc(cl, cum, k, s);
        printf("arc %a %d %a %a %a %a %a\n", s, k, p.x, p.y, p.dx, p.dy, p.t);
    }
    // the segment without length, which no arc length selects: the parameter is 0, not 0 / 0
    const tds::ArcPoint z = tds::point_at_arc(cl, cum, 1, cum[1]);
    printf("arc %a %d %a %a %a %a %a\n", cum[1], 1, z.x, z.y, z.dx, z.dy, z.t);
    return 0;
}

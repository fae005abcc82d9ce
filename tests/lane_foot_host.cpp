// The foot of a pose on a centre-line segment (tds::segment_foot and what is read off it: segment_unit, foot_arc, foot_lateral of
// torchdrivesim_amd/csrc/tds_lane_math.h, shared by tds_lane_snap and K8) compiled by a host compiler and printed for
// tests/test_lane_foot_host.py, which holds every number to tests/lane_obs_model.py.  Doubles are printed as hexadecimal floats: every bit,
// the sign of a zero included.
#include <stdio.h>

#include "tds_lane_math.h"

int main() {
    // six points: the third repeats the second (a segment without length), the line turns back on itself at the end, and it climbs (cum is 3-D)
    const int n = 6;
    const double cl[3 * n] = {-0.0, 0.0, 0.0, -3.0, 4.0, 0.0, -3.0, 4.0, 0.0, -1.0, 10.0, 1.0, 0.1, 12.3, 1.0, -1.0, 10.0, 1.5};
    double cum[n] = {0.0};
    for (int i = 1; i < n; ++i) {                                            // as tds_lanes_create sums it
        const double dx = cl[3 * i] - cl[3 * i - 3], dy = cl[3 * i + 1] - cl[3 * i - 2], dz = cl[3 * i + 2] - cl[3 * i - 1];
        const double seg = sqrt((dx * dx + dy * dy) + dz * dz);
        cum[i] = i == 1 ? seg : cum[i - 1] + seg;
    }
    for (int i = 0; i < n; ++i) printf("point %a %a %a %a\n", cl[3 * i], cl[3 * i + 1], cl[3 * i + 2], cum[i]);
    // on the line, beside it on either side, before its start, beyond its end, on a vertex, on the repeated point, far away, float32 values as
    // the kernels read them, then infinities and a NaN
    const double poses[][2] = {{-1.5, 2.0}, {0.5, 1.0}, {-4.0, 3.0}, {2.0, -3.0}, {-2.0, 9.0}, {-1.0, 10.0}, {-3.0, 4.0}, {1e6, -3e5},
                               {(double)0.1f, (double)12.3f}, {(double)-2.7182817f, (double)3.1415927f}, {1e-300, 1e-300},
                               {INFINITY, 1.0}, {2.0, -INFINITY}, {INFINITY, INFINITY}, {NAN, 1.0}, {1.0, NAN}};
    for (const double *p : poses) {
        for (int i = 0; i + 1 < n; ++i) {
            const tds::SegmentFoot f = tds::segment_foot(cl, i, p[0], p[1]);
            const tds::Unit2 t = tds::segment_unit(f);
            printf("foot %a %a %d %a %a %a %a %a %a %a %a %a %a %a %a %a\n", p[0], p[1], i, f.ax, f.ay, f.dx, f.dy, f.l2, f.u, f.fx, f.fy, f.d2, t.x, t.y,
                   tds::foot_arc(f, cum, i), tds::foot_lateral(f, t, p[0], p[1]));
        }
    }
    return 0;
}

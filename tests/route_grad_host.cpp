// The per-row arithmetic of the route step's backward (torchdrivesim_amd/csrc/tds_route_grad.h) compiled by a host compiler for
// tests/test_route_grad_host.py.  Standard input holds rows, numbers as hexadecimal floats (every bit):
//   p0 p1 p3 p4 c0 c1 a b base x y sn cs g_progress g_advance g_remaining g_lateral g_hs g_hc length spacing K
// followed by K lines `px py sx sy sw gox goy`, the lookahead points as the forward found them.  Per row one line goes out: the progress the
// header recomputes and the four sums, the foot's terms first and the points' in order; `skip` for a segment the clip refuses.
#include <stdio.h>

#include <vector>

#include "tds_route_grad.h"

int main() {
    double r[21];
    for (;;) {
        for (int i = 0; i < 21; ++i)
            if (scanf("%lf", &r[i]) != 1) return i == 0 ? 0 : 1;
        int K = 0;
        if (scanf("%d", &K) != 1 || K < 0 || K > 64) return 1;
        std::vector<double> look(7 * (size_t)K);
        for (double &v : look)
            if (scanf("%lf", &v) != 1) return 1;
        double w, ulo, uhi;
        if (!tds::route_clip(r[4], r[5], r[6], r[7], w, ulo, uhi)) {
            printf("skip\n");
            continue;
        }
        const tds::RouteFoot f = tds::route_foot_grad(r[0], r[1], r[2], r[3], r[4], w, ulo, uhi, r[8], r[6], r[9], r[10], r[13], r[14], r[15], r[16], r[17], r[18]);
        tds::RouteGrad sum = f.g;
        for (int m = 0; m < K; ++m) {
            const double *p = look.data() + 7 * (size_t)m;
            const double q = f.progress + (double)(m + 1) * r[20];
            const tds::RouteGrad c = tds::route_look_grad(p[0], p[1], p[2], p[3], p[4], q, r[19], r[9], r[10], r[11], r[12], f.dx, f.dy, p[5], p[6]);
            sum.x = sum.x + c.x, sum.y = sum.y + c.y, sum.sn = sum.sn + c.sn, sum.cs = sum.cs + c.cs;
        }
        printf("row %a %a %a %a %a\n", f.progress, sum.x, sum.y, sum.sn, sum.cs);
    }
}

// The host part of torchdrivesim_amd/csrc/tds_nearest_face.h (point-triangle distance and its gradient, the corner of a box, the value of a
// corner) compiled by a host compiler for tests/test_nearest_face_host.py.  Reads the cases the test wrote to argv[1] and prints
//   off  <case> <agent> <bits>                        the off-road value of every agent by brute force over ALL faces: corners, the minimum of
//                                                     tri_d2, NaN / infinity handling, threshold, the sum of the four corners in order
//   grad <agent> <gap> <gx> <gy> <fdx> <fdy> <d2>     (cases marked for it) at the agent's position: how much nearer the nearest face is than the
//                                                     second nearest (metres), tri_d2_grad at the face the brute force picks, the central
//                                                     difference of tri_d2 on that face with a step of 1 mm, and the squared distance
// Floats are printed as their bits or as hexadecimal doubles: nothing is rounded on the way.
// A case: int64 B, A, V, F, mesh_batch, has_present, want_grad; float threshold; float state[B A 4], lenwid[B A 2], sc[B A 2];
// uint8 present[B A] (if has_present); float verts[mesh_batch V 2]; int32 faces[mesh_batch F 3].  The file starts with the int64 number of cases.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tds_nearest_face.h"

struct Face { float x0, y0, x1, y1, x2, y2; };

template <class T>
static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const int64_t n_cases = take<int64_t>(f, 1)[0];
    for (int64_t c = 0; c < n_cases; ++c) {
        const std::vector<int64_t> h = take<int64_t>(f, 7);
        const int64_t B = h[0], A = h[1], V = h[2], F = h[3], mesh_batch = h[4];
        const float threshold = take<float>(f, 1)[0];
        const std::vector<float> state = take<float>(f, B * A * 4), lenwid = take<float>(f, B * A * 2), sc = take<float>(f, B * A * 2);
        const std::vector<uint8_t> present = take<uint8_t>(f, h[5] ? B * A : 0);
        const std::vector<float> verts = take<float>(f, mesh_batch * V * 2);
        const std::vector<int32_t> faces = take<int32_t>(f, mesh_batch * F * 3);
        std::vector<Face> tri(mesh_batch * F);
        for (size_t i = 0; i < tri.size(); ++i) {
            const float *vb = verts.data() + (i / F) * V * 2;
            const float *p0 = vb + 2 * faces[3 * i], *p1 = vb + 2 * faces[3 * i + 1], *p2 = vb + 2 * faces[3 * i + 2];
            tri[i] = Face{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1]};
        }
        for (int64_t a = 0; a < B * A; ++a) {
            const Face *mesh = tri.data() + (mesh_batch > 1 ? a / A : 0) * F;
            float total = 0.0f;
            for (int k = 0; k < 4; ++k) {
                const tds::BoxCorner p = tds::box_corner(k, state[4 * a], state[4 * a + 1], lenwid[2 * a], lenwid[2 * a + 1], sc[2 * a], sc[2 * a + 1]);
                float best = INFINITY;
                for (int64_t i = 0; i < F; ++i) {
                    const float d = tds::tri_d2(p.px, p.py, mesh[i]);
                    best = (d < best) ? d : best;                    // a NaN distance never becomes the minimum
                }
                total = total + tds::offroad_corner_value(best, threshold);
            }
            if (F == 0) total = 0.0f;
            if (!present.empty()) total = total * (present[a] ? 1.0f : 0.0f);
            uint32_t bits;
            memcpy(&bits, &total, 4);
            printf("off %lld %lld %08x\n", (long long)c, (long long)a, bits);
            if (!h[6]) continue;
            const float px = state[4 * a], py = state[4 * a + 1];
            float d1 = INFINITY, d2 = INFINITY;                       // nearest (the first among equals) and second nearest
            int64_t f1 = -1;
            for (int64_t i = 0; i < F; ++i) {
                const float d = tds::tri_d2(px, py, mesh[i]);
                if (d < d1) { d2 = d1; d1 = d; f1 = i; } else if (d < d2) d2 = d;
            }
            if (f1 < 0) continue;
            float gx, gy;
            tds::tri_d2_grad(px, py, mesh[f1], gx, gy);
            const float step = 1e-3f, xp = px + step, xm = px - step, yp = py + step, ym = py - step;     // (the steps really taken: xp - xm, yp - ym)
            const double fdx = ((double)tds::tri_d2(xp, py, mesh[f1]) - (double)tds::tri_d2(xm, py, mesh[f1])) / ((double)xp - (double)xm);
            const double fdy = ((double)tds::tri_d2(px, yp, mesh[f1]) - (double)tds::tri_d2(px, ym, mesh[f1])) / ((double)yp - (double)ym);
            printf("grad %lld %a %a %a %a %a %a\n", (long long)a, sqrt((double)d2) - sqrt((double)d1), (double)gx, (double)gy, fdx, fdy, (double)d1);
        }
    }
    fclose(f);
    return 0;
}

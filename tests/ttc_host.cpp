// The pair test of time to collision (torchdrivesim_amd/csrc/tds_ttc.h) compiled for the HOST: every ordered pair of the entities of a scene, as
// the kernel's lanes take them.  tests/test_ttc_host.py writes the input, reads the output and holds it to tests/ttc_model.py bit for bit.
//
// Input (numbers as C99 hex floats), any number of scenes:
//   scene N horizon margin        then per entity:  x y length width sin cos speed     (float32 values)
// Output per scene:  "scene N", then "finite e flag" per entity, then "pair a e candidate bits" for every a != e with both finite: bits is the
// float32 time as 8 hex digits, ffffffff where the pair is no candidate.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tds_ttc.h"

static FILE *in;

static float number() {
    char word[64];
    if (fscanf(in, "%63s", word) != 1) exit(2);
    return strtof(word, nullptr);
}

struct Entity { float v[7]; };

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 2;
    char word[64];
    while (fscanf(in, "%63s", word) == 1) {
        if (strcmp(word, "scene") != 0) return 2;
        int n;
        if (fscanf(in, "%d", &n) != 1 || n < 0) return 2;
        const float horizon = number(), margin = number();
        std::vector<Entity> ent(n);
        for (Entity &q : ent)
            for (float &v : q.v) v = number();
        printf("scene %d\n", n);
        std::vector<char> finite(n);
        for (int e = 0; e < n; ++e) {
            finite[e] = 1;
            for (float v : ent[e].v) finite[e] = finite[e] && tds::ttc_finite(v);
            printf("finite %d %d\n", e, (int)finite[e]);
        }
        for (int a = 0; a < n; ++a) {
            if (!finite[a]) continue;
            const float *p = ent[a].v;
            const tds::TtcBox me = tds::ttc_box(p[0], p[1], p[2], p[3], p[4], p[5], p[6], (double)margin);
            for (int e = 0; e < n; ++e) {
                if (e == a || !finite[e]) continue;
                const float *q = ent[e].v;
                float t = 0.0f;
                const bool cand = tds::ttc_pair(me, tds::ttc_box(q[0], q[1], q[2], q[3], q[4], q[5], q[6], 0.0), (double)horizon, &t);
                uint32_t bits = 0xffffffffu;
                if (cand) memcpy(&bits, &t, sizeof bits);
                printf("pair %d %d %d %08x\n", a, e, (int)cand, bits);
            }
        }
    }
    fclose(in);
    return 0;
}

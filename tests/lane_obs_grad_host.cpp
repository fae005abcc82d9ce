// The gradients of the lane observations (torchdrivesim_amd/csrc/tds_lane_obs_grad.h) compiled for the HOST.
// tests/test_lane_obs_grad_host.py writes the input, reads the output and holds it to its numpy restatement bit for bit.
//
// Input (numbers as C99 hex floats), any number of lines of two kinds:
//   S  x0 y0 z0 x1 y1 z1  (the two centre-line points of segment sb)   cum0 cum1   x y sin cos  (the observer)   g0 .. g7
//   P  ax ay  (the slot's slide)   ex ey hx hy   sin cos   gx gy
// Output per line:  "slot" and the four contributions and the slide (6 numbers), or "point" and the four contributions, each number as the 16 hex
// digits of its binary64 bits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tds_lane_obs_grad.h"

static FILE *in;

static bool word(char *w) { return fscanf(in, "%63s", w) == 1; }

static bool numbers(double *v, int n) {
    char w[64];
    for (int i = 0; i < n; ++i) {
        if (!word(w)) return false;
        v[i] = strtod(w, nullptr);
    }
    return true;
}

static void print(const char *what, const double *v, int n) {
    printf("%s", what);
    for (int i = 0; i < n; ++i) {
        unsigned long long bits;
        memcpy(&bits, &v[i], sizeof bits);
        printf(" %016llx", bits);
    }
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 2;
    char kind[64];
    while (word(kind)) {
        double v[20], out[tds::LG_GRADS + 2];
        if (kind[0] == 'S') {
            if (!numbers(v, 20)) return 2;
            const tds::SegmentFoot f = tds::segment_foot(v, 0, v[8], v[9]);
            const tds::LaneSlide a = tds::lane_obs_slot_grad(f, tds::segment_unit(f), v[7] - v[6], v[8], v[9], v[10], v[11], v + 12, out);
            out[tds::LG_GRADS] = a.x, out[tds::LG_GRADS + 1] = a.y;
            print("slot", out, tds::LG_GRADS + 2);
        } else if (kind[0] == 'P') {
            if (!numbers(v, 10)) return 2;
            const tds::LaneSlide a = {v[0], v[1]};
            tds::lane_obs_point_grad(a, v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], out);
            print("point", out, tds::LG_GRADS);
        } else {
            return 2;
        }
    }
    fclose(in);
    return 0;
}

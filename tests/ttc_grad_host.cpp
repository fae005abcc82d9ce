// The pair gradient of time to collision (torchdrivesim_amd/csrc/tds_ttc_grad.h) compiled for the HOST.  tests/test_ttc_grad_host.py writes the
// input, reads the output and holds it to the numpy restatement in tests/ttc_grad_model.py bit for bit.
//
// Input (numbers as C99 hex floats), any number of pairs, one per line:
//   margin   x y length width sin cos speed  (the observer)   x y length width sin cos speed  (the other)          (float32 values)
// Output per pair:  "pair finite contributes" and the 14 partials as the 16 hex digits of their binary64 bits, the observer's seven first; finite is
// 0 where one of the 14 values is no number (the function is then not called), and the partials of a pair that does not contribute are printed as 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tds_ttc_grad.h"

static FILE *in;

static bool number(float &v) {
    char word[64];
    if (fscanf(in, "%63s", word) != 1) return false;
    v = strtof(word, nullptr);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 2;
    float margin;
    while (number(margin)) {
        float v[14];
        bool finite = true;
        for (float &q : v) {
            if (!number(q)) return 2;
            finite = finite && tds::ttc_finite(q);
        }
        double g[2 * tds::TTC_GRADS];
        bool contributes = false;
        if (finite)
            contributes = tds::ttc_pair_grad(tds::ttc_box(v[0], v[1], v[2], v[3], v[4], v[5], v[6], (double)margin),
                                             tds::ttc_box(v[7], v[8], v[9], v[10], v[11], v[12], v[13], 0.0), g, g + tds::TTC_GRADS);
        printf("pair %d %d", (int)finite, (int)contributes);
        for (int i = 0; i < 2 * tds::TTC_GRADS; ++i) {
            unsigned long long bits = 0;
            if (contributes) memcpy(&bits, &g[i], sizeof bits);
            printf(" %016llx", bits);
        }
        printf("\n");
    }
    fclose(in);
    return 0;
}

// The slot gradient of the neighbour observations (torchdrivesim_amd/csrc/tds_neighbors_grad.h) compiled for the HOST.
// tests/test_neighbors_grad_host.py writes the input, reads the output and holds it to its numpy restatement bit for bit.
//
// Input (numbers as C99 hex floats), any number of slots, one per line:
//   x y sin cos speed  (the observer)   x y sin cos speed  (the entity)   g0 .. g7  (the incoming gradient)          (float32 values)
// Output per slot:  "slot" and the 14 contributions as the 16 hex digits of their binary64 bits, the observer's seven first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tds_neighbors_grad.h"

static FILE *in;

static bool number(float &v) {
    char word[64];
    if (fscanf(in, "%63s", word) != 1) return false;
    v = strtof(word, nullptr);
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 2;
    float v[18];
    while (number(v[0])) {
        for (int i = 1; i < 18; ++i)
            if (!number(v[i])) return 2;
        double gin[8], g[2 * tds::NB_GRADS];
        for (int i = 0; i < 8; ++i) gin[i] = (double)v[10 + i];
        tds::neighbors_slot_grad(tds::nb_pose(v[0], v[1], v[2], v[3], v[4]), tds::nb_pose(v[5], v[6], v[7], v[8], v[9]), gin, g, g + tds::NB_GRADS);
        printf("slot");
        for (int i = 0; i < 2 * tds::NB_GRADS; ++i) {
            unsigned long long bits;
            memcpy(&bits, &g[i], sizeof bits);
            printf(" %016llx", bits);
        }
        printf("\n");
    }
    fclose(in);
    return 0;
}

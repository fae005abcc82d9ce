// The clock of the device traffic lights (torchdrivesim_amd/csrc/tds_lights.h: the very code lights.hip runs per machine) compiled by a host
// compiler and driven by a script for tests/test_lights_host.py.  Input (argv[1], text; doubles in any form strtod reads):
//   M P                         then per machine: n_phases, P durations, P next_phase entries
//   then until the end of the file one command per line:
//     start p_0 r_0 .. p_M-1 r_M-1      the clocks as they are
//     tick dt
//     set K  i_0 t_0 .. i_K-1 t_K-1     TrafficLightStateMachine.set_to for the first K machines (index and time clamped)
//     pick seed scene_id m n            the phase a reset deals
// After every start / tick / set one line "clock p_0 r_0 ..." with the remaining times as hexadecimal floats: every bit.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tds_lights.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int M = 0, P = 0;
    if (fscanf(f, "%d %d", &M, &P) != 2 || M < 1 || P < 1) return 3;
    std::vector<int32_t> n_phases(M), next_phase((size_t)M * P);
    std::vector<double> duration((size_t)M * P);
    char word[64];
    for (int m = 0; m < M; ++m) {
        if (fscanf(f, "%d", &n_phases[m]) != 1) return 3;
        for (int p = 0; p < P; ++p) {
            if (fscanf(f, "%63s", word) != 1) return 3;
            duration[(size_t)m * P + p] = strtod(word, nullptr);
        }
        for (int p = 0; p < P; ++p)
            if (fscanf(f, "%d", &next_phase[(size_t)m * P + p]) != 1) return 3;
    }
    std::vector<tds::LightClock> clock(M, tds::LightClock{0, 0.0});
    auto number = [&](double *out) {
        if (fscanf(f, "%63s", word) != 1) return false;
        *out = strtod(word, nullptr);
        return true;
    };
    while (fscanf(f, "%63s", word) == 1) {
        if (!strcmp(word, "pick")) {
            unsigned long long seed, scene;
            int m, n;
            if (fscanf(f, "%llu %llu %d %d", &seed, &scene, &m, &n) != 4) return 4;
            printf("pick %d\n", tds::lights_reset_phase(seed, scene, m, n));
            continue;
        }
        if (!strcmp(word, "start")) {
            for (int m = 0; m < M; ++m)
                if (fscanf(f, "%d", &clock[m].phase) != 1 || !number(&clock[m].remaining)) return 4;
        } else if (!strcmp(word, "tick")) {
            double dt;
            if (!number(&dt)) return 4;
            for (int m = 0; m < M; ++m)
                clock[m] = tds::lights_tick(&duration[(size_t)m * P], &next_phase[(size_t)m * P], n_phases[m], clock[m], dt);
        } else if (!strcmp(word, "set")) {
            int K;
            if (fscanf(f, "%d", &K) != 1 || K > M) return 4;
            for (int m = 0; m < K; ++m) {
                int i;
                double t;
                if (fscanf(f, "%d", &i) != 1 || !number(&t)) return 4;
                const int p = tds::lights_clamp(i, n_phases[m]);
                const double span = duration[(size_t)m * P + p];
                clock[m] = tds::LightClock{p, t <= span ? t : span};
            }
        } else {
            return 5;
        }
        printf("clock");
        for (int m = 0; m < M; ++m) printf(" %d %a", clock[m].phase, clock[m].remaining);
        printf("\n");
    }
    fclose(f);
    return 0;
}

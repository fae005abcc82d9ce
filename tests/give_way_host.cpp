// The arithmetic of giving way at junctions (torchdrivesim_amd/csrc/tds_conflicts.h) compiled for the HOST: the conflict table of a map, sample by
// sample as the kernel's lanes take them, and the yield decision for NPCs whose paths are given.  tests/test_give_way_host.py writes the input,
// reads the output and holds it to tests/give_way_model.py bit for bit.
//
// Input (numbers as C99 hex floats):
//   map L                              then per lanelet:  n  x y z (n times)  cum (n times)  n_succ  succ (n_succ times)
//   table clearance step
//   scene N S horizon b_max creep      then per stop line:  lanelet arc red
//                                      then per NPC:  present length speed n_path  lanelet start (n_path times)
// Output:  "exit a b value" for every entry >= 0, "zone a in out" per lanelet, "npc i stop_at yield_to" per NPC.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tds_conflicts.h"

struct Lanelet {
    std::vector<double> cl, cum;
    std::vector<int> succ;
    int n() const { return (int)cum.size(); }
    bool drivable() const { return n() >= 2 && cum.back() > 0.0 && cum.back() < INFINITY; }
};

struct Npc {
    int present, junction = -1;
    double length, speed, start = 0.0, half = 0.0;
    std::vector<int> lane;
    std::vector<double> starts;
    tds::Approach ap = {INFINITY, INFINITY, INFINITY, false};
    bool held = false;
};

static FILE *in;

static double number() {
    char word[64];
    if (fscanf(in, "%63s", word) != 1) exit(2);
    return strtod(word, nullptr);
}

static int integer() {
    int v;
    if (fscanf(in, "%d", &v) != 1) exit(2);
    return v;
}

static void expect(const char *what) {
    char word[64];
    if (fscanf(in, "%63s", word) != 1 || std::string(word) != what) exit(3);
}

int main(int argc, char **argv) {
    if (argc != 2 || !(in = fopen(argv[1], "r"))) return 1;
    expect("map");
    const int L = integer();
    std::vector<Lanelet> lanes(L);
    for (auto &l : lanes) {
        const int n = integer();
        for (int i = 0; i < 3 * n; ++i) l.cl.push_back(number());
        for (int i = 0; i < n; ++i) l.cum.push_back(number());
        const int ns = integer();
        for (int i = 0; i < ns; ++i) l.succ.push_back(integer());
    }
    expect("table");
    const double clearance = number(), step = number(), c2 = clearance * clearance;
    std::vector<double> exits((size_t)L * L, -1.0), zone_in(L, INFINITY), zone_out(L, -1.0);
    for (int a = 0; a < L; ++a) {
        if (!lanes[a].drivable()) continue;
        std::vector<char> excluded(L, 0);
        excluded[a] = 1;
        for (int p = 0; p < L; ++p) {
            bool parent = false;
            for (int s : lanes[p].succ) parent |= s == a;
            if (parent) excluded[p] = 1;
            if (parent || p == a)
                for (int s : lanes[p].succ) excluded[s] = 1;
        }
        const Lanelet &la = lanes[a];
        const int last = tds::last_sample(la.cum.back(), step);
        for (int b = 0; b < L; ++b) {
            if (excluded[b] || !lanes[b].drivable()) continue;
            int first = -1, last_hit = -1;
            for (int k = 0; k <= last; ++k)
                if (tds::sample_hit(la.cl.data(), la.cum.data(), la.n(), k, step, lanes[b].cl.data(), lanes[b].n(), c2)) {
                    if (first < 0) first = k;
                    last_hit = k;
                }
            if (last_hit < 0) continue;
            exits[(size_t)a * L + b] = tds::sample_arc(last_hit, step);
            zone_in[a] = fmin(zone_in[a], tds::sample_arc(first, step)), zone_out[a] = fmax(zone_out[a], tds::sample_arc(last_hit, step));
            printf("exit %d %d %a\n", a, b, exits[(size_t)a * L + b]);
        }
    }
    for (int a = 0; a < L; ++a) printf("zone %d %a %a\n", a, zone_in[a], zone_out[a]);

    expect("scene");
    const int N = integer(), S = integer();
    const double horizon = number(), b_max = number(), creep = number();
    std::vector<int> line_lane(S), line_red(S);
    std::vector<double> line_arc(S);
    for (int s = 0; s < S; ++s) line_lane[s] = integer(), line_arc[s] = number(), line_red[s] = integer();
    std::vector<Npc> npcs(N);
    for (auto &c : npcs) {
        c.present = integer(), c.length = number(), c.speed = number();
        const int n_path = integer();
        for (int k = 0; k < n_path; ++k) c.lane.push_back(integer()), c.starts.push_back(number());
        if (!c.present) continue;
        c.half = c.length / 2.0;
        double red = INFINITY;
        for (size_t k = 0; k < c.lane.size(); ++k) {
            const int l = c.lane[k];
            for (int s = 0; s < S; ++s)
                if (line_red[s] && line_lane[s] == l) red = tds::nearest_red_line(c.starts[k] + line_arc[s], red);
            if (tds::is_junction(c.starts[k], zone_in[l], zone_out[l], c.half, horizon)) {
                c.junction = l, c.start = c.starts[k];
                c.ap = tds::approach(c.start, zone_in[l], c.half, c.speed, b_max, creep);
                c.held = tds::is_held(c.ap.committed, red, c.start, zone_out[l]);
                break;
            }
        }
    }
    for (int i = 0; i < N; ++i) {
        const Npc &me = npcs[i];
        double stop = INFINITY;
        int who = -1;
        if (me.junction >= 0 && !me.ap.committed)
            for (int j = 0; j < N && who < 0; ++j) {
                const Npc &o = npcs[j];
                if (j == i || o.junction < 0) continue;
                if (tds::gives_way(exits[(size_t)o.junction * L + me.junction], exits[(size_t)me.junction * L + o.junction], o.start, o.half, o.ap.committed, o.held,
                                   o.ap.t, j, me.ap.t, i))
                    stop = me.ap.D, who = j;
            }
        printf("npc %d %a %d\n", i, stop, who);
    }
    fclose(in);
    return 0;
}

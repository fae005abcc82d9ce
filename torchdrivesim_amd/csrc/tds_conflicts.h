// The arithmetic of giving way at junctions (conflicts.hip, follow.hip): which samples of a lanelet's centre line lie within the
// clearance of another lanelet, what makes a lanelet an NPC's junction, when an NPC is committed or held, and who gives way to whom.  Nothing of
// HIP in here: a host compiler takes this file as it is, and tests/give_way_host.cpp holds these functions to the float64 model
// (tests/give_way_model.py) on the CPU.  Float64, + - * / sqrt only (floor and casts are exact).
#pragma once
#include "tds_lane_math.h"

namespace tds {

// samples of one lanelet: k = 0 .. last_sample at arcs (double)k * step; a lanelet never has more than CONFLICT_MAX_SAMPLES + 1
constexpr int CONFLICT_MAX_SAMPLES = 1 << 20;

// floor(length / step), capped; -1 when that is no number >= 0
TDS_HD inline int last_sample(double length, double step) {
    const double q = floor(length / step);
    if (!(q >= 0.0)) return -1;
    return q < (double)CONFLICT_MAX_SAMPLES ? (int)q : CONFLICT_MAX_SAMPLES;
}

TDS_HD inline double sample_arc(int k, double step) { return (double)k * step; }

// sample k of lanelet a (n_a centre-line points, cumulative lengths cum_a): the point at its arc, 2-D
TDS_HD inline ArcPoint sample_point(const double *cl_a, const double *cum_a, int n_a, int k, double step) {
    const double s = sample_arc(k, step);
    return point_at_arc(cl_a, cum_a, segment_of(cum_a, n_a, s), s);
}

// whether (x, y) lies within the clearance of lanelet b: the least squared distance to its 2-D centre-line segments against clearance^2
TDS_HD inline bool within_clearance(const double *cl_b, int n_b, double x, double y, double clearance2) {
    double best = INFINITY;
    for (int i = 0; i + 1 < n_b; ++i) {
        const double d2 = segment_foot(cl_b, i, x, y).d2;
        if (d2 < best) best = d2;
    }
    return best <= clearance2;
}

TDS_HD inline bool sample_hit(const double *cl_a, const double *cum_a, int n_a, int k, double step, const double *cl_b, int n_b, double clearance2) {
    const ArcPoint p = sample_point(cl_a, cum_a, n_a, k, step);
    return within_clearance(cl_b, n_b, p.x, p.y, clearance2);
}

// ---- the yield pass -------------------------------------------------------------------------------------------------------------------------
// `start`: the path distance from the NPC's centre to the beginning of a lanelet of its path (negative on its own lanelet); half = length / 2.

// the lanelet is the NPC's junction: it has a conflict zone, the NPC's rear has not cleared it, and it begins within the horizon
TDS_HD inline bool is_junction(double start, double zone_in, double zone_out, double half, double horizon) {
    return zone_out >= 0.0 && start + zone_out + half > 0.0 && start + zone_in <= horizon;
}

struct Approach {
    double D, gap, t;               // path distance to the zone's entry, the same from the NPC's front, the time it needs for that
    bool committed;                 // in the zone already, or unable to stop before it at b_max
};
TDS_HD inline Approach approach(double start, double zone_in, double half, double v, double b_max, double creep_speed) {
    Approach a;
    a.D = start + zone_in;
    a.gap = a.D - half;
    a.committed = a.gap <= 0.0 || v * v >= 2.0 * b_max * a.gap;
    a.t = fmax(a.gap, 0.0) / fmax(v, creep_speed);
    return a;
}

// the nearest red stop line ahead on the path so far: `pos` = start of the line's lanelet + the line's arc
TDS_HD inline double nearest_red_line(double pos, double nearest) { return 0.0 < pos && pos < nearest ? pos : nearest; }

// an NPC that is not committed is held by a red line that stands before the end of its junction's zone
TDS_HD inline bool is_held(bool committed, double nearest_red, double start, double zone_out) { return !committed && nearest_red < start + zone_out; }

// NPC i (time t_i, junction p) gives way to NPC j (junction q): exit_qp = exit[q][p], exit_pq = exit[p][q]
TDS_HD inline bool gives_way(double exit_qp, double exit_pq, double start_j, double half_j, bool committed_j, bool held_j, double t_j, int j, double t_i,
                             int i) {
    if (held_j || !(exit_qp >= 0.0) || !(exit_pq >= 0.0)) return false;
    if (!(start_j + exit_qp + half_j > 0.0)) return false;                  // j's rear has cleared the pair's zone
    return committed_j || t_j < t_i || (t_j == t_i && j < i);
}

// ---- the follow kernel ----------------------------------------------------------------------------------------------------------------------
// a finite stop_at is one more standing obstacle: whether it is the nearest (leader -1: none so far), and its gap
TDS_HD inline bool stop_is_nearest(double stop_at, double half, int leader, double gap, double *gap_s) {
    if (!(stop_at > -INFINITY && stop_at < INFINITY)) return false;
    *gap_s = stop_at - half;
    return leader == -1 || *gap_s < gap;
}

}  // namespace tds

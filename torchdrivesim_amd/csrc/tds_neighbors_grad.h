// The slot gradient of the neighbour observations (neighbors_bwd.hip; include/tdship.h "K6b"): what the eight incoming gradients
// of one filled slot contribute to x, y, length, width, sin, cos, speed of the slot's entity and to x, y, sin, cos, speed of its observer.
// Nothing of HIP in here: a host compiler takes this file as it is, and tests/neighbors_grad_host.cpp holds this function to its numpy
// restatement (tests/test_neighbors_grad_host.py) bit for bit.  Float64, + - * only, every operation rounded once, in the order written here.
// Which entity is in the slot is a constant of differentiation; [sin, cos] are independent inputs.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef TDS_HD
#ifdef __HIPCC__
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif
#endif

namespace tds {

// the order of the seven contributions of a side; the observer's length and width get none (they are written as 0)
enum { NB_GX = 0, NB_GY, NB_GLENGTH, NB_GWIDTH, NB_GSIN, NB_GCOS, NB_GSPEED, NB_GRADS };

// what K6 reads of an entity, the float32 values widened exactly
struct NbPose { double x, y, s, c, v; };
TDS_HD inline NbPose nb_pose(float x, float y, float s, float c, float v) { return {(double)x, (double)y, (double)s, (double)c, (double)v}; }

// observer a, entity e, g[8] the incoming gradient of the slot's features f0 .. f7 (K6's order) -> ga[7], ge[7]
TDS_HD inline void neighbors_slot_grad(const NbPose &a, const NbPose &e, const double *g, double *ga, double *ge) {
    const double dx = e.x - a.x, dy = e.y - a.y;
    const double f2 = e.s * a.c - e.c * a.s, f3 = e.c * a.c + e.s * a.s;      // sin_rel, cos_rel
    const double G2 = g[2] + g[5] * e.v, G3 = g[3] + g[4] * e.v;              // what reaches sin_rel and cos_rel, vy and vx included
    const double px = g[0] * a.c - g[1] * a.s, py = g[0] * a.s + g[1] * a.c;  // the gradient of (x, y) turned back into the world frame
    ge[NB_GX] = px, ge[NB_GY] = py;
    ge[NB_GLENGTH] = g[6], ge[NB_GWIDTH] = g[7];
    ge[NB_GSIN] = G2 * a.c + G3 * a.s;
    ge[NB_GCOS] = G3 * a.c - G2 * a.s;
    ge[NB_GSPEED] = g[4] * f3 + g[5] * f2;
    ga[NB_GX] = -px, ga[NB_GY] = -py;
    ga[NB_GLENGTH] = 0.0, ga[NB_GWIDTH] = 0.0;
    ga[NB_GSIN] = ((g[0] * dy - g[1] * dx) - G2 * e.c) + G3 * e.s;
    ga[NB_GCOS] = ((g[0] * dx + g[1] * dy) + G2 * e.s) + G3 * e.c;
    ga[NB_GSPEED] = -g[4];
}

}  // namespace tds

// K7: traffic lights on the device (traffic_controls.ProgrammedTrafficLightControl, Simulator.compute_stop_lines; include/tdship.h "K7",
// DESIGN.md 5.5h; models, bit for bit: tests/lights_model.py).
//   lights_step_kernel   one workgroup per scene: a thread per machine advances its clock (tds_lights.h: TrafficLightStateMachine.tick in float64),
//                        then, after a barrier, a thread per light takes the colour of the LAST machine whose current phase names it.
//   lights_reset_kernel  a thread per (scene, machine): a Philox-picked phase at its beginning.
//   stop_lines_kernel    the K nearest stop lines of every exposed agent, in K6's layout (neighbors.hip): the frame of tds_observers.h over the
//                        scene's lines.  Binary32 + - * and one correctly rounded square root, every operation rounded once
//                        (-ffp-contract=off).
#include "tds_common.h"
#include "tds_lights.h"
#include "tds_observers.h"
#include <math.h>

static_assert(TDS_LIGHTS_MAX_SKIPS == TDS_LIGHTS_MAX_SKIPS_, "tds_lights.h and tdship.h disagree");

namespace {

constexpr int LT_BLOCK = 256;           // = TDS_LIGHTS_MAX_MACHINES: a thread per machine

struct LightsArgs {
    const double *duration;
    const int32_t *next_phase, *n_phases;
    const uint8_t *colour;
    int32_t *phase;
    double *remaining;
    int64_t *state;
    float *time_to_change;
    const uint8_t *mask;
    int M, P, N, advance;
    double dt;
};

// grid = B
__global__ void __launch_bounds__(LT_BLOCK) lights_step_kernel(LightsArgs g) {
    __shared__ int32_t s_phase[LT_BLOCK];
    __shared__ float s_left[LT_BLOCK];
    const int64_t b = blockIdx.x;
    if (g.mask != nullptr && g.mask[b] == 0) return;                     // the whole workgroup: nobody waits at the barrier
    const int tid = threadIdx.x, M = g.M, P = g.P, N = g.N;
    if (tid < M) {
        int n = g.n_phases[tid];
        n = n < 1 ? 1 : (n > P ? P : n);
        tds::LightClock s{tds::lights_clamp(g.phase[b * M + tid], n), g.remaining[b * M + tid]};
        if (g.advance) {
            s = tds::lights_tick(g.duration + (int64_t)tid * P, g.next_phase + (int64_t)tid * P, n, s, g.dt);
            g.phase[b * M + tid] = s.phase;
            g.remaining[b * M + tid] = s.remaining;
        }
        s_phase[tid] = s.phase;
        s_left[tid] = (float)s.remaining;
    }
    __syncthreads();
    for (int l = tid; l < N; l += LT_BLOCK) {
        for (int m = M - 1; m >= 0; --m) {                              // the later machine wins, as the host's merged.update
            const uint8_t c = g.colour[((int64_t)m * P + s_phase[m]) * N + l];
            if (c != 255) {
                g.state[b * N + l] = (int64_t)c;
                g.time_to_change[b * N + l] = s_left[m];
                break;
            }
        }
    }
}

__global__ void __launch_bounds__(LT_BLOCK) lights_reset_kernel(const int32_t *n_phases, const double *duration, int32_t *phase, double *remaining,
                                                               const uint8_t *mask, const int64_t *scene_ids, int64_t B, int M, int P, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * LT_BLOCK + threadIdx.x;
    if (i >= B * M) return;
    const int64_t b = i / M;
    const int m = (int)(i - b * M);
    if (mask != nullptr && mask[b] == 0) return;
    int n = n_phases[m];
    n = n < 1 ? 1 : (n > P ? P : n);
    const int p = tds::lights_reset_phase(seed, (uint64_t)scene_ids[b], m, n);
    phase[i] = p;
    remaining[i] = duration[(int64_t)m * P + p];
}

// ---------------------------------------------------------------------------------------------------------------- stop lines
constexpr int SL_WORDS = tds::OBS_WORDS;        // LDS words per line: x, y, length, width, sin, cos, time to change, state (int32 bits)

struct StopLineArgs {
    const float *agent_xy, *agent_sc, *lines, *line_sc, *time_to_change;
    const uint8_t *agent_present, *mask;
    const int64_t *state;
    float *features;
    int32_t *index, *slot_state;
    int A, N, K, ahead_only;
    float r2, min_cos;
};

struct Observer { float x, y, s, c; };

// the d2 bits of line n as the observer sees it, tds::NO_KEY if it is no candidate (a NaN fails every comparison)
__device__ __forceinline__ uint32_t key_of(const StopLineArgs &g, const float *ln, const uint8_t *mask, int n, const Observer me) {
    const float4 q = *(const float4 *)(ln + SL_WORDS * n);
    const float2 h = *(const float2 *)(ln + SL_WORDS * n + 4);
    const float dx = q.x - me.x, dy = q.y - me.y;
    const float d2 = dx * dx + dy * dy;
    const float x = dx * me.c + dy * me.s;
    const float cos_rel = h.y * me.c + h.x * me.s;
    bool ok = mask[n] != 0 && d2 <= g.r2 && cos_rel >= g.min_cos;
    if (g.ahead_only) ok = ok && x >= 0.0f;
    return ok ? __float_as_uint(d2) : tds::NO_KEY;
}

// slot k of the row that starts at `row` (in slots): line n (-1: an empty slot)
__device__ __forceinline__ void store_slot(const StopLineArgs &g, const float *ln, int64_t row, int k, int n, const Observer me) {
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
    int st = -1;
    if (n >= 0) {
        const float4 q = *(const float4 *)(ln + SL_WORDS * n);
        const float4 q2 = *(const float4 *)(ln + SL_WORDS * n + 4);
        const float dx = q.x - me.x, dy = q.y - me.y;
        const float d2 = dx * dx + dy * dy;
        lo = make_float4(dx * me.c + dy * me.s, dy * me.c - dx * me.s, q2.x * me.c - q2.y * me.s, q2.y * me.c + q2.x * me.s);
        hi = make_float4(q.z, q.w, q2.z, sqrtf(d2));
        st = __float_as_int(q2.w);
    }
    float4 *out = (float4 *)(g.features + (row + k) * 8);
    out[0] = lo;
    out[1] = hi;
    g.index[row + k] = n;
    g.slot_state[row + k] = st;
}

// the launch of tds_observers.h: grid = (B, ceil(A / OBS_SLICE)), dynamic LDS = lds_bytes(N, true)
__global__ void __launch_bounds__(tds::OBS_BLOCK) stop_lines_kernel(StopLineArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ln[];
    const tds::SliceThread t;
    const int64_t b = blockIdx.x;
    const int A = g.A, N = g.N, K = g.K;
    t.stage_items(ln, N, [&](int j) {
        const float *p = g.lines + (b * N + j) * 5;
        const float2 sc = *(const float2 *)(g.line_sc + (b * N + j) * 2);
        return tds::Item{make_float4(p[0], p[1], p[2], p[3]), make_float4(sc.x, sc.y, g.time_to_change ? g.time_to_change[b * N + j] : 0.0f,
                                                                           __int_as_float((int32_t)g.state[b * N + j]))};
    });
    const uint8_t *mask = g.mask + b * N;
    t.for_slice(A, [&](int a) {
        const int64_t row = (b * A + a) * K;
        const float2 xy = *(const float2 *)(g.agent_xy + (b * A + a) * 2), sc = *(const float2 *)(g.agent_sc + (b * A + a) * 2);
        const Observer me{xy.x, xy.y, sc.x, sc.y};
        const auto store = [&](int k, int n, uint32_t) { store_slot(g, ln, row, k, n, me); };
        if (g.agent_present[b * A + a] == 0) return t.empty_row(K, store);       // an observer that is not present
        t.select_row(ln, N, K, [&](int n) { return key_of(g, ln, mask, n, me); }, store);
    });
}

int check_lights_sizes(const char *what, int64_t B, int64_t M, int64_t P, int64_t N) {
    TDS_CHECK_ARG(B >= 0 && M >= 0 && P >= 0 && N >= 0 && B < ((int64_t)1 << 31), "%s: bad sizes B=%lld M=%lld P=%lld N=%lld", what, (long long)B, (long long)M,
                  (long long)P, (long long)N);
    if (M > TDS_LIGHTS_MAX_MACHINES || P > TDS_LIGHTS_MAX_PHASES || N > TDS_LIGHTS_MAX_LIGHTS) {
        tds::set_error("%s: M=%lld machines, P=%lld phases, N=%lld lights (at most %d, %d and %d)", what, (long long)M, (long long)P, (long long)N,
                       TDS_LIGHTS_MAX_MACHINES, TDS_LIGHTS_MAX_PHASES, TDS_LIGHTS_MAX_LIGHTS);
        return TDS_ELIMIT;
    }
    return TDS_OK;
}

}  // namespace

static_assert(LT_BLOCK == TDS_LIGHTS_MAX_MACHINES, "a thread per machine");

TDS_EXPORT int tds_lights_step(const double *duration, const int32_t *next_phase, const int32_t *n_phases, const uint8_t *colour, int32_t *phase,
                               double *remaining, int64_t *state, float *time_to_change, const uint8_t *mask, int64_t B, int64_t M, int64_t P, int64_t N,
                               const double *dt, int advance, void *stream) {
    const char *what = "tds_lights_step";
    if (int rc = check_lights_sizes(what, B, M, P, N)) return rc;
    TDS_CHECK_ARG(dt != nullptr, "%s: dt is a null pointer", what);
    const double step = *dt;
    TDS_CHECK_ARG(step >= 0.0 && step <= 1.7976931348623157e308, "%s: dt must not be negative or non-finite (got %g)", what, step);
    if (B == 0 || M == 0) return TDS_OK;
    TDS_CHECK_ARG(P >= 1, "%s: %lld machines without a phase", what, (long long)M);
    TDS_CHECK_ARG(duration && next_phase && n_phases && phase && remaining && (N == 0 || (colour && state && time_to_change)), "%s: null pointer", what);
    LightsArgs g{};
    g.duration = duration; g.next_phase = next_phase; g.n_phases = n_phases; g.colour = colour;
    g.phase = phase; g.remaining = remaining; g.state = state; g.time_to_change = time_to_change; g.mask = mask;
    g.M = (int)M; g.P = (int)P; g.N = (int)N; g.advance = advance != 0; g.dt = step;
    hipLaunchKernelGGL(lights_step_kernel, dim3((unsigned)B), dim3(LT_BLOCK), 0, (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("lights_step_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_lights_reset(const int32_t *n_phases, const double *duration, int32_t *phase, double *remaining, const uint8_t *mask,
                                const int64_t *scene_ids, int64_t B, int64_t M, int64_t P, uint64_t seed, void *stream) {
    const char *what = "tds_lights_reset";
    if (int rc = check_lights_sizes(what, B, M, P, 0)) return rc;
    if (B == 0 || M == 0) return TDS_OK;
    TDS_CHECK_ARG(P >= 1, "%s: %lld machines without a phase", what, (long long)M);
    TDS_CHECK_ARG(n_phases && duration && phase && remaining && scene_ids, "%s: null pointer", what);
    const int64_t blocks = (B * M + LT_BLOCK - 1) / LT_BLOCK;
    hipLaunchKernelGGL(lights_reset_kernel, dim3((unsigned)blocks), dim3(LT_BLOCK), 0, (hipStream_t)stream, n_phases, duration, phase, remaining, mask, scene_ids,
                       B, (int)M, (int)P, seed);
    TDS_LAUNCH_CHECK("lights_reset_kernel");
    return TDS_OK;
}

TDS_EXPORT int tds_stop_lines_f32(const float *agent_xy, const float *agent_sc, const uint8_t *agent_present, const float *lines, const float *line_sc,
                                  const uint8_t *mask, const int64_t *state, const float *time_to_change, float *features, int32_t *index,
                                  int32_t *slot_state, int64_t B, int64_t A, int64_t N, int K, float max_distance, int ahead_only, float min_cos,
                                  void *stream) {
    const char *what = "tds_stop_lines_f32";
    TDS_CHECK_ARG(A < ((int64_t)1 << 20), "%s: bad sizes B=%lld A=%lld N=%lld", what, (long long)B, (long long)A, (long long)N);
    TDS_CHECK_ARG(max_distance >= 0.0f, "%s: max_distance must not be negative or NaN (got %g)", what, (double)max_distance);
    TDS_CHECK_ARG(min_cos == min_cos, "%s: min_cos must not be NaN", what);
    if (int rc = tds::check_frame(what, B, A, N, K, TDS_STOP_LINES_MAX_K, tds::frame_stop_lines(TDS_LIGHTS_MAX_LIGHTS), A); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(agent_xy && agent_sc && agent_present && features && index && slot_state, "%s: null pointer", what);
    TDS_CHECK_ARG(N == 0 || (lines && line_sc && mask && state), "%s: null pointer", what);
    StopLineArgs g{};
    g.agent_xy = agent_xy; g.agent_sc = agent_sc; g.agent_present = agent_present; g.lines = lines; g.line_sc = line_sc; g.mask = mask; g.state = state;
    g.time_to_change = time_to_change; g.features = features; g.index = index; g.slot_state = slot_state;
    g.A = (int)A; g.N = (int)N; g.K = K; g.ahead_only = ahead_only != 0;
    g.r2 = max_distance * max_distance;
    g.min_cos = min_cos;
    hipLaunchKernelGGL(stop_lines_kernel, tds::slice_grid(B, A), dim3(tds::OBS_BLOCK), tds::lds_bytes(N, true), (hipStream_t)stream, g);
    TDS_LAUNCH_CHECK("stop_lines_kernel");
    return TDS_OK;
}

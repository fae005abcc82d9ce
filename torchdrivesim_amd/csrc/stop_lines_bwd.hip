// K7b: the backward of the stop-line observations (_ops.stop_lines_grad; include/tdship.h "K7b"): the gradients of the slots'
// features to x, y and [sin, cos] of the observing agent, one launch.  Yardstick: the float64 torch-autograd model tests/stop_lines_grad_model.py;
// the slot gradient and the order of a row's sum are stated once, in tds_stop_lines_grad.h.
// Nothing is gathered across observers -- the lines are constants and get nothing --, so there is no staging and no LDS: SLG_ROW_LANES = 4 lanes
// share an observer, a wave has 16 observers and a workgroup 64 (16 lanes, K6b's shape, and a thread per observer were measured against it and
// lost: DESIGN.md 5.5q).  Lane l of an observer takes the slots l, l + 4, ...
// of its row: the index, then the five incoming gradients that are read (x, y, sin_rel, cos_rel as one 16-byte load, distance as one word) and the
// line's four words from global memory.  The four lanes' sums are added by xor-shuffles in a fixed order, so a result does not change from run to
// run; the first lane rounds to binary32 and writes the observer's two rows, zeros included.
#include "tds_observers.h"
#include "tds_stop_lines_grad.h"

namespace {

struct StopLinesBwdArgs {
    const float *agent_xy, *agent_sc, *lines, *line_sc, *g_features;
    const int32_t *index;
    float *g_xy, *g_sc;
    int A, N, K;
};

// grid = (B, ceil(A / (OBS_BLOCK / LANES))): LANES lanes per observer
template <int LANES>
__global__ void __launch_bounds__(tds::OBS_BLOCK) stop_lines_bwd_kernel(StopLinesBwdArgs g) {
    constexpr int ROWS = tds::OBS_BLOCK / LANES;
    const int64_t b = blockIdx.x;
    const int A = g.A, N = g.N, K = g.K;
    const int sub = threadIdx.x & (LANES - 1);
    const int a = blockIdx.y * ROWS + threadIdx.x / LANES;
    const bool row = a < A;                                                  // (the last workgroup of a scene may be short)
    const int64_t o = b * A + a;
    double sum[tds::SLG_GRADS] = {0.0, 0.0, 0.0, 0.0};
    if (row) {
        const float2 xy = *(const float2 *)(g.agent_xy + o * 2), sc = *(const float2 *)(g.agent_sc + o * 2);
        for (int k = sub; k < K; k += LANES) {
            const int64_t s = o * K + k;
            const int n = g.index[s];
            if (!tds::stop_lines_slot_filled(n, N)) continue;                // an empty slot or garbage: never dereferenced, its gradient never read
            const float4 g03 = *(const float4 *)(g.g_features + s * 8);
            const float g7 = g.g_features[s * 8 + 7];
            const float *p = g.lines + (b * N + n) * 5;
            const float2 h = *(const float2 *)(g.line_sc + (b * N + n) * 2);
            double d[tds::SLG_GRADS];
            tds::stop_lines_slot_grad(xy.x, xy.y, sc.x, sc.y, p[0], p[1], h.x, h.y, g03.x, g03.y, g03.z, g03.w, g7, d);
#pragma unroll
            for (int i = 0; i < tds::SLG_GRADS; ++i) sum[i] = sum[i] + d[i];
        }
    }
#pragma unroll
    for (int m = LANES / 2; m > 0; m >>= 1) {                                // a butterfly over the lanes of the observer: the same additions every run
#pragma unroll
        for (int i = 0; i < tds::SLG_GRADS; ++i) sum[i] = sum[i] + __shfl_xor(sum[i], m);
    }
    if (row && sub == 0) {                                                   // both rows of the observer in full
        *(float2 *)(g.g_xy + o * 2) = make_float2((float)sum[tds::SLG_X], (float)sum[tds::SLG_Y]);
        *(float2 *)(g.g_sc + o * 2) = make_float2((float)sum[tds::SLG_SIN], (float)sum[tds::SLG_COS]);
    }
}

#ifdef TDS_TESTING
int g_row_lanes = tds::SLG_ROW_LANES;       // the other launch shapes exist in the testing build alone (tools/rule_grad_timing.py measures them)
#endif

template <int LANES>
void launch(const StopLinesBwdArgs &g, int64_t B, int64_t A, hipStream_t stream) {
    constexpr int ROWS = tds::OBS_BLOCK / LANES;
    hipLaunchKernelGGL(stop_lines_bwd_kernel<LANES>, dim3((unsigned)B, (unsigned)((A + ROWS - 1) / ROWS)), dim3(tds::OBS_BLOCK), 0, stream, g);
}

}  // namespace

#ifdef TDS_TESTING
// testing build only (include/tdship.h, "testing hooks"): the launch shapes that were measured against each other
TDS_EXPORT int tds_stop_lines_bwd_set_row_lanes(int lanes) {
    TDS_CHECK_ARG(lanes == 1 || lanes == 4 || lanes == 16, "tds_stop_lines_bwd_set_row_lanes: 1, 4 or 16 lanes per observer (got %d)", lanes);
    g_row_lanes = lanes;
    return TDS_OK;
}
#endif

TDS_EXPORT int tds_stop_lines_bwd_f32(const float *agent_xy, const float *agent_sc, const float *lines, const float *line_sc, const int32_t *index,
                                      const float *g_features, float *g_xy, float *g_sc, int64_t B, int64_t A, int64_t N, int K, void *stream) {
    const char *what = "tds_stop_lines_bwd_f32";
    TDS_CHECK_ARG(A < ((int64_t)1 << 20), "%s: bad sizes B=%lld A=%lld N=%lld", what, (long long)B, (long long)A, (long long)N);
    if (int rc = tds::check_frame(what, B, A, N, K, TDS_STOP_LINES_MAX_K, tds::frame_stop_lines(TDS_LIGHTS_MAX_LIGHTS), A); rc != tds::FRAME_LAUNCH) return rc;
    TDS_CHECK_ARG(agent_xy && agent_sc && index && g_features && g_xy && g_sc, "%s: null pointer", what);
    TDS_CHECK_ARG(N == 0 || (lines && line_sc), "%s: null pointer", what);
    TDS_CHECK_ARG((uintptr_t)g_features % 16 == 0, "%s: g_features must start at a multiple of 16 bytes", what);
    StopLinesBwdArgs g{};
    g.agent_xy = agent_xy; g.agent_sc = agent_sc; g.lines = lines; g.line_sc = line_sc; g.g_features = g_features; g.index = index;
    g.g_xy = g_xy; g.g_sc = g_sc;
    g.A = (int)A; g.N = (int)N; g.K = K;
#ifdef TDS_TESTING
    if (g_row_lanes == 1) launch<1>(g, B, A, (hipStream_t)stream);
    else if (g_row_lanes == 16) launch<16>(g, B, A, (hipStream_t)stream);
    else
#endif
    launch<tds::SLG_ROW_LANES>(g, B, A, (hipStream_t)stream);
    TDS_LAUNCH_CHECK("stop_lines_bwd_kernel");
    return TDS_OK;
}

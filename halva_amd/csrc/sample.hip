// Temperature / top-k / top-p token selection for generate (halva_amd/decode.py:sample) on gfx950: one launch, one workgroup of 1024
// lanes per row, the row read from HBM once and held in registers (32 values per lane) for every later pass (sample_row.h).
#include "sample_row.h"

namespace {

__global__ __launch_bounds__(kSmpThreads) void sample_top_k_top_p_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ u,
                                                                         int V, float temperature, int top_k, float top_p,
                                                                         int64_t* __restrict__ token, float* __restrict__ thr_out,
                                                                         int32_t* __restrict__ kept_out) {
    __shared__ SmpShared sh;
    int par = 0;
    const int tid = threadIdx.x;
    const float* row = logits + (int64_t)blockIdx.x * ld;
    float e[4 * kSmpGroups];

    // ---- the one read of the row: x = l / temperature, columns at or beyond V stand as -inf (never loaded)
    float m = -INFINITY;
    unsigned bad = 0;
#pragma unroll
    for (int g = 0; g < kSmpGroups; ++g) {
        float v[4];
        smp_load4(row, g * kSmpSpan + 4 * tid, V, -INFINITY, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) e[4 * g + c] = smp_scale(v[c], temperature, bad, m);
    }
    smp_select_row(e, bad, m, u, V, top_k, top_p, token, thr_out, kept_out, sh, par);
}

}  // namespace

extern "C" int halva_sample_max_vocab(void) { return kSmpMaxV; }

extern "C" int halva_sample_top_k_top_p(const float* logits, int64_t ld, const float* u, int64_t* token, float* thr, int32_t* kept, int B,
                                        int V, float temperature, int top_k, float top_p, void* stream) {
    HALVA_CHECK_ARG(logits && u && token, "sample_top_k_top_p: null pointer");
    HALVA_CHECK_ARG(B >= 1 && V >= 1, "sample_top_k_top_p: bad B=%d / V=%d", B, V);
    HALVA_CHECK_ARG(V <= kSmpMaxV, "sample_top_k_top_p: V=%d exceeds the %d columns a workgroup holds (halva_sample_max_vocab)", V, kSmpMaxV);
    HALVA_CHECK_ARG(ld >= V, "sample_top_k_top_p: row stride %lld < V=%d", (long long)ld, V);
    HALVA_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "sample_top_k_top_p: temperature=%g (needs a finite value > 0)",
                    (double)temperature);
    HALVA_CHECK_ARG(top_k >= 0, "sample_top_k_top_p: top_k=%d (needs >= 0; 0 = off)", top_k);
    HALVA_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "sample_top_k_top_p: top_p=%g (needs 0 < top_p <= 1)", (double)top_p);
    hipLaunchKernelGGL(sample_top_k_top_p_kernel, dim3(B), dim3(kSmpThreads), 0, (hipStream_t)stream, logits, ld, u, V, temperature, top_k,
                       top_p, token, thr, kept);
    HALVA_CHECK_LAUNCH("sample_top_k_top_p");
    return HALVA_OK;
}

// Contrastive token selection for generate (halva_amd/decode.py:contrast) on gfx950: the row of the prompt as given (l) and the row of the
// contrast prompt (lcd) become x = (1 + alpha) * l - alpha * lcd on the columns that are plausible under l, and x goes through the
// temperature / top-k / top-p select of sample_row.h - one launch, one workgroup of 1024 lanes per row pair.
//
// Each row is read from HBM once.  l is loaded into the 32 registers per lane that later hold x; its maximum is reduced (wave butterfly,
// then the 16 waves in wave order - a maximum has no rounding, so any order gives the same bits); then lcd is streamed, 16 bytes per lane
// at a time, and x overwrites l in place.  x is product, product, difference in fp32 with round-to-nearest intrinsics, so no fused
// multiply-add is ever formed and float32 arithmetic on the host reproduces x bit for bit.  A masked column's lcd is loaded but never
// looked at: x = -inf there whatever lcd holds, NaN included.
#include "sample_row.h"

namespace {

__global__ __launch_bounds__(kSmpThreads) void contrast_select_kernel(const float* __restrict__ logits, int64_t ld,
                                                                      const float* __restrict__ logits_cd, int64_t ld_cd,
                                                                      const float* __restrict__ u, int V, float one_plus_alpha, float alpha,
                                                                      float log_beta, float temperature, int top_k, float top_p,
                                                                      int64_t* __restrict__ token, float* __restrict__ thr_out,
                                                                      int32_t* __restrict__ kept_out, int32_t* __restrict__ plausible_out) {
    __shared__ SmpShared sh;
    int par = 0;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (int64_t)b * ld;
    const float* row_cd = logits_cd + (int64_t)b * ld_cd;
    float e[4 * kSmpGroups];

    // ---- the one read of l: columns at or beyond V stand as -inf (never loaded)
    float m = -INFINITY;
    unsigned bad = 0;
#pragma unroll
    for (int g = 0; g < kSmpGroups; ++g) {
        float v[4];
        smp_load4(row, g * kSmpSpan + 4 * tid, V, -INFINITY, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bad |= (v[c] != v[c] || v[c] == INFINITY) ? 1u : 0u;
            m = fmaxf(m, v[c]);
            e[4 * g + c] = v[c];
        }
    }
    bad = smp_red_u<SMP_OR>(bad, sh.red, par);
    const unsigned kmax = smp_red_u<SMP_MAX>(bad ? 0u : smp_key(m), sh.red, par);
    if (bad || kmax < kSmpKeyMinFinite) {                       // (uniform) a NaN / +inf in l, or nothing above -inf: lcd is not read
        if (tid == 0) {
            token[b] = -1;
            if (thr_out) thr_out[b] = __uint_as_float(0x7fc00000u);
            if (kept_out) kept_out[b] = 0;
            if (plausible_out) plausible_out[b] = 0;
        }
        return;
    }
    const float cut = __fadd_rn(smp_unkey(kmax), log_beta);     // log_beta = -inf (beta = 0): cut = -inf, nothing is below it

    // ---- the one read of lcd: x in place of l.  Columns at or beyond V hold l = -inf and lcd = 0 (never loaded): x = -inf there either
    // way, and they pass the cut only when it is -inf, which the count takes back below
    unsigned cnt = 0;
    m = -INFINITY;
#pragma unroll
    for (int g = 0; g < kSmpGroups; ++g) {
        const int i0 = g * kSmpSpan + 4 * tid;
        float v[4];
        smp_load4(row_cd, i0, V, 0.f, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float l = e[4 * g + c];
            const bool in = !(l < cut);
            cnt += (unsigned)__popcll(__ballot(in));
            bad |= (in && (v[c] != v[c] || v[c] == INFINITY)) ? 1u : 0u;
            const float x = in ? __fsub_rn(__fmul_rn(one_plus_alpha, l), __fmul_rn(alpha, v[c])) : -INFINITY;
            e[4 * g + c] = smp_scale(x, temperature, bad, m);
        }
    }
    cnt = smp_red_u<SMP_ADD>(cnt, sh.red, par) - (cut == -INFINITY ? (unsigned)(kSmpMaxV - V) : 0u);
    if (tid == 0 && plausible_out) plausible_out[b] = (int32_t)cnt;      // (a row that x makes unservable still has its cut on l)
    smp_select_row(e, bad, m, u, V, top_k, top_p, token, thr_out, kept_out, sh, par);
}

}  // namespace

extern "C" int halva_contrast_select(const float* logits, int64_t ld, const float* logits_cd, int64_t ld_cd, const float* u, int64_t* token,
                                     float* thr, int32_t* kept, int32_t* plausible, int B, int V, float alpha, float log_beta,
                                     float temperature, int top_k, float top_p, void* stream) {
    HALVA_CHECK_ARG(logits && logits_cd && u && token, "contrast_select: null pointer");
    HALVA_CHECK_ARG(B >= 1 && V >= 1, "contrast_select: bad B=%d / V=%d", B, V);
    HALVA_CHECK_ARG(V <= kSmpMaxV, "contrast_select: V=%d exceeds the %d columns a workgroup holds (halva_sample_max_vocab)", V, kSmpMaxV);
    HALVA_CHECK_ARG(ld >= V, "contrast_select: row stride %lld < V=%d", (long long)ld, V);
    HALVA_CHECK_ARG(ld_cd >= V, "contrast_select: contrast row stride %lld < V=%d", (long long)ld_cd, V);
    HALVA_CHECK_ARG(std::isfinite(alpha) && alpha >= 0.f, "contrast_select: alpha=%g (needs a finite value >= 0)", (double)alpha);
    HALVA_CHECK_ARG(log_beta <= 0.f, "contrast_select: log_beta=%g (needs log(beta) <= 0; -inf for beta = 0)", (double)log_beta);
    HALVA_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "contrast_select: temperature=%g (needs a finite value > 0)",
                    (double)temperature);
    HALVA_CHECK_ARG(top_k >= 0, "contrast_select: top_k=%d (needs >= 0; 0 = off)", top_k);
    HALVA_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "contrast_select: top_p=%g (needs 0 < top_p <= 1)", (double)top_p);
    const float one_plus_alpha = 1.0f + alpha;                  // formed once, here, as a float
    hipLaunchKernelGGL(contrast_select_kernel, dim3(B), dim3(kSmpThreads), 0, (hipStream_t)stream, logits, ld, logits_cd, ld_cd, u, V,
                       one_plus_alpha, alpha, log_beta, temperature, top_k, top_p, token, thr, kept, plausible);
    HALVA_CHECK_LAUNCH("contrast_select");
    return HALVA_OK;
}

// Extending a kept KV cache by a block of rows (halva_amd/decode.py:extend - sessions, chunked prefill, block teacher forcing) on gfx950:
// RoPE + cache append of up to n new rows per sequence, causal attention of those rows over the past + n keys of the cache on MFMA, and the
// launch that advances lens.  Three launches, so that no workgroup ever reads a lens value written by its own launch.  The rotation and the
// cache write of a row are rope_append.h's one routine, the one decode.hip's append calls: the two cannot differ in arithmetic.
//
// Cache layout as decode.hip: K, V bf16 [B, H, Lcap, 128]; lens int32 [B] and n_new int32 [B] on the device (never a launch-time host
// value).  With past = lens[b]: slots at or beyond past + n_new[b] and q rows at or beyond n_new[b] are never read.
#include "common.h"
#include "rope_append.h"
#include <cmath>

namespace {

#include "sdpa_common.h"      // tile_off / mfma32 / frag_rows / frag_cols / Stage / store_rows_T, mask_half / half_max / xhalf_*: the attention kernels' tile pieces
#include "extend_attn.h"      // kExt*, ext_rows, ext_tile, extend_attn_body: the attention's kernel body, shared with fork.hip

static_assert(kExtD == 8 * kRopeChunks, "rope_append_row serves this head_dim");

// ---------------------------------------------------------------------------------------------------
// RoPE + append.  One workgroup per (row i, sequence b): rope_append_row (rope_append.h, the routine decode_rope_append_kernel calls) on
// row i at position lens[b] + i.  lens is only read.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void extend_rope_append_kernel(u32x4* __restrict__ qkv, int64_t ldrow_chunks, int64_t ldseq_chunks,
                                                                 const u32x4* __restrict__ cosb, const u32x4* __restrict__ sinb, int max_pos,
                                                                 u32x4* __restrict__ kc, u32x4* __restrict__ vc, const int32_t* __restrict__ lens,
                                                                 const int32_t* __restrict__ n_new, int n, int H, int Lcap) {
    const int i = blockIdx.x, b = blockIdx.y;
    const int past = lens[b];
    if (past < 0 || i >= min(n_new[b], n)) return;
    const int p = past + i;
    if (p >= Lcap || p >= max_pos) return;      // (the host refuses such calls; never written out of bounds)
    rope_append_row(qkv + (int64_t)b * ldseq_chunks + (int64_t)i * ldrow_chunks, cosb, sinb, kc, vc, b, p, H, Lcap);
}

__global__ void extend_advance_kernel(int32_t* __restrict__ lens, const int32_t* __restrict__ n_new, int B, int Lcap) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) lens[b] = min(max(lens[b], 0) + max(n_new[b], 0), Lcap);
}

// ---------------------------------------------------------------------------------------------------
// Attention of the new rows: workgroup (row block qb, head h, sequence b) runs extend_attn.h's body without a prefix phase.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kExtWaves, 2) void extend_attn_kernel(const bf16_t* __restrict__ q, int64_t ldrow, int64_t ldseq,
                                                                     const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                                                                     const int32_t* __restrict__ lens, const int32_t* __restrict__ n_new,
                                                                     bf16_t* __restrict__ out, int64_t ld_out_row, int64_t ld_out_seq, int n, int H,
                                                                     int Lcap, float sc) {
    const int qb = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int past = lens[b];
    if (past < 0) return;
    const int nn = ext_rows(past, n_new[b], n, Lcap);
    const int64_t bh = ((int64_t)b * H + hd) * Lcap * kExtD;
    extend_attn_body<false>(q + (int64_t)b * ldseq, ldrow, nullptr, nullptr, 0, kc + bh, vc + bh, past, nn, out + (int64_t)b * ld_out_seq,
                            ld_out_row, qb, hd, sc);
}

}  // namespace

extern "C" int64_t halva_extend_attn_ws_bytes(int B, int n, int H, int Lcap) {
    (void)B, (void)n, (void)H, (void)Lcap;
    return 0;      // one workgroup owns a row from its first key to its last: no partials
}

extern "C" int halva_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos, void* kcache,
                                        void* vcache, const int32_t* lens, const int32_t* n_new, int B, int n, int H, int D, int Lcap,
                                        void* stream) {
    HALVA_CHECK_ARG(qkv && cos && sin && kcache && vcache && lens && n_new, "extend_rope_append: null pointer");
    HALVA_CHECK_ARG(D == kExtD, "extend_rope_append: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(B > 0 && n > 0 && H > 0 && Lcap > 0 && max_pos > 0 && B <= 65535,
                    "extend_rope_append: bad B=%d / n=%d / H=%d / Lcap=%d / max_pos=%d", B, n, H, Lcap, max_pos);
    HALVA_CHECK_ARG(ldrow >= 3LL * H * D && ldrow % 8 == 0, "extend_rope_append: row stride %lld (needs >= 3*H*D and a multiple of 8)",
                    (long long)ldrow);
    HALVA_CHECK_ARG(ldseq >= (int64_t)n * ldrow && ldseq % 8 == 0, "extend_rope_append: sequence stride %lld (needs >= n * row stride and a multiple of 8)",
                    (long long)ldseq);
    HALVA_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)kcache | (uintptr_t)vcache) % 16 == 0,
                    "extend_rope_append: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(extend_rope_append_kernel, dim3(n, B), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldrow / 8, ldseq / 8,
                       (const u32x4*)cos, (const u32x4*)sin, max_pos, (u32x4*)kcache, (u32x4*)vcache, lens, n_new, n, H, Lcap);
    HALVA_CHECK_LAUNCH("extend_rope_append");
    return HALVA_OK;
}

extern "C" int halva_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* kcache, const void* vcache, const int32_t* lens,
                                 const int32_t* n_new, void* out, int64_t ld_out_row, int64_t ld_out_seq, void* ws, int64_t ws_bytes, int B, int n,
                                 int H, int D, int Lcap, float scale, void* stream) {
    HALVA_CHECK_ARG(q && kcache && vcache && lens && n_new && out, "extend_attn: null pointer");
    HALVA_CHECK_ARG(D == kExtD, "extend_attn: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(B > 0 && n > 0 && H > 0 && Lcap > 0 && H <= 65535 && B <= 65535, "extend_attn: bad B=%d / n=%d / H=%d / Lcap=%d", B, n, H, Lcap);
    HALVA_CHECK_ARG(ldrow >= (int64_t)H * D && ldrow % 8 == 0, "extend_attn: q row stride %lld (needs >= H*D and a multiple of 8)", (long long)ldrow);
    HALVA_CHECK_ARG(ldseq >= (int64_t)n * ldrow && ldseq % 8 == 0, "extend_attn: q sequence stride %lld (needs >= n * row stride and a multiple of 8)",
                    (long long)ldseq);
    HALVA_CHECK_ARG(ld_out_row >= (int64_t)H * D && ld_out_row % 8 == 0, "extend_attn: out row stride %lld (needs >= H*D and a multiple of 8)",
                    (long long)ld_out_row);
    HALVA_CHECK_ARG(ld_out_seq >= (int64_t)n * ld_out_row && ld_out_seq % 8 == 0,
                    "extend_attn: out sequence stride %lld (needs >= n * row stride and a multiple of 8)", (long long)ld_out_seq);
    HALVA_CHECK_ARG(((uintptr_t)q | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)out | (uintptr_t)ws) % 16 == 0,
                    "extend_attn: q / cache / out / workspace pointers must be 16-byte aligned");
    const int64_t need = halva_extend_attn_ws_bytes(B, n, H, Lcap);
    HALVA_CHECK_ARG(ws_bytes >= need && (need == 0 || ws), "extend_attn: workspace of %lld bytes, %lld needed (halva_extend_attn_ws_bytes)",
                    (long long)ws_bytes, (long long)need);
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    hipLaunchKernelGGL(extend_attn_kernel, dim3((n + kExtBM - 1) / kExtBM, H, B), dim3(64 * kExtWaves), 0, (hipStream_t)stream, (const bf16_t*)q,
                       ldrow, ldseq, (const bf16_t*)kcache, (const bf16_t*)vcache, lens, n_new, (bf16_t*)out, ld_out_row, ld_out_seq, n, H, Lcap,
                       scale * kLog2e);
    HALVA_CHECK_LAUNCH("extend_attn");
    return HALVA_OK;
}

extern "C" int halva_extend_advance(int32_t* lens, const int32_t* n_new, int B, int Lcap, void* stream) {
    HALVA_CHECK_ARG(lens && n_new, "extend_advance: null pointer");
    HALVA_CHECK_ARG(B > 0 && Lcap > 0, "extend_advance: bad B=%d / Lcap=%d", B, Lcap);
    hipLaunchKernelGGL(extend_advance_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lens, n_new, B, Lcap);
    HALVA_CHECK_LAUNCH("extend_advance");
    return HALVA_OK;
}

// Single-token decode over a KV cache (greedy generation, halva_amd/decode.py) on gfx950: RoPE + cache append of the new token, and
// split-KV ("flash-decoding") attention of one query row per (sequence, head).  Both are HBM-bound and use no MFMA: M = 1 per head.
// The rotation and the cache write of a row are rope_append.h's one routine, which extend.hip calls for its rows too.
//
// Cache layout, per layer: K, V bf16 [B, H, Lcap, 128]; lens int32 [B] on the device (never a launch-time host value, so the step can
// be captured in a graph later).  Slots at or beyond lens[b] are never read.
#include "common.h"
#include "decode_partial.h"      // kDecD / kDecChunks / kDecWaves, DecChunkRegs, decode_chunk_partial: one chunk's partial, shared with fork.hip
#include "rope_append.h"
#include <cmath>

namespace {

static_assert(kDecChunks == kRopeChunks, "rope_append_row serves this head_dim");

// ---------------------------------------------------------------------------------------------------
// RoPE of the new token + cache append.  One workgroup per sequence b: every thread reads lens[b] before the barrier, thread 0 advances
// it after, so no other reader of this launch sees the new value.  qkv row b = [3, H, D] goes through rope_append_row (rope_append.h, shared
// with extend.hip) at position lens[b].
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_rope_append_kernel(u32x4* __restrict__ qkv, int64_t ldq_chunks, const u32x4* __restrict__ cosb,
                                                                 const u32x4* __restrict__ sinb, int max_pos, u32x4* __restrict__ kc,
                                                                 u32x4* __restrict__ vc, int32_t* __restrict__ lens, int H, int Lcap) {
    const int b = blockIdx.x;
    const int p = lens[b];
    const bool ok = p >= 0 && p < Lcap && p < max_pos;      // (the host sizes the cache; a full one is left untouched, never overrun)
    if (ok) rope_append_row(qkv + (int64_t)b * ldq_chunks, cosb, sinb, kc, vc, b, p, H, Lcap);
    __syncthreads();
    if (threadIdx.x == 0 && ok) lens[b] = p + 1;
}

// ---------------------------------------------------------------------------------------------------
// Split-KV attention, partial pass.  Workgroup (chunk c, head h, sequence b) covers keys [c KC, (c + 1) KC) ∩ [0, lens[b]); 4 waves of
// KC / 4 keys each.  A wave takes 4 keys per step, 16 lanes per key row (one 16-byte piece of K and V per lane, straight to VGPRs - all
// of the wave's K and V loads are issued before the first dot).  Scores in fp32 in the log2 domain (q pre-scaled by log2(e) / sqrt(D)).
// The 4 waves combine in LDS in a fixed order; the chunk's (m, l, o[128]) go to the fp32 workspace (decode_partial.h holds the routine).
// Nothing here depends on B or on the other rows: row b's result is bitwise the same in any batch.
// ---------------------------------------------------------------------------------------------------
template <int KC>
__global__ __launch_bounds__(256) void decode_attn_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, const u32x4* __restrict__ kc,
                                                                  const u32x4* __restrict__ vc, const int32_t* __restrict__ lens, int H, int Lcap,
                                                                  int nchunk_cap, float qscale, float* __restrict__ ws_o,
                                                                  float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int len = min(lens[b], Lcap);
    const int k0 = c * KC;
    if (k0 >= len) return;                         // (uniform over the workgroup: no barrier is skipped by part of it)
    const int sub = threadIdx.x & 15;
    const int64_t bh = (int64_t)b * H + h;
    const u32x4 q8 = q[(int64_t)b * ldq_chunks + h * kDecChunks + sub];
    DecChunkRegs<KC> ch;
    ch.load(kc + bh * Lcap * kDecChunks + sub, vc + bh * Lcap * kDecChunks + sub, k0, len);
    decode_chunk_partial<KC>(q8, ch, k0, len, qscale, ws_o, ws_ml, bh * nchunk_cap + c);
}

// Combine pass: one workgroup of 128 threads per (head, sequence) reduces the ceil(lens[b] / KC) partials in chunk order.
template <int KC>
__global__ __launch_bounds__(128) void decode_attn_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                                  const int32_t* __restrict__ lens, int H, int Lcap, int nchunk_cap,
                                                                  bf16_t* __restrict__ out, int64_t ld_out) {
    const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
    const int len = min(lens[b], Lcap);
    const int n = len > 0 ? (len + KC - 1) / KC : 0;
    const int64_t slot0 = ((int64_t)b * H + h) * nchunk_cap;
    float M = -INFINITY;
    for (int c = 0; c < n; ++c) M = fmaxf(M, ws_ml[(slot0 + c) * 2]);
    float acc = 0.f, L = 0.f;
    for (int c = 0; c < n; ++c) {
        const float f = exp2f(ws_ml[(slot0 + c) * 2] - M);
        acc = fmaf(f, ws_o[(slot0 + c) * kDecD + d], acc);
        L = fmaf(f, ws_ml[(slot0 + c) * 2 + 1], L);
    }
    out[(int64_t)b * ld_out + h * kDecD + d] = f32_to_bf16(n > 0 ? acc / L : 0.f);
}

constexpr int kDecodeKC = 256;      // keys per split-KV chunk (tools/bench_decode.py: 4.85 TB/s at 256, 4.73 at 128, 4.54 at 64)

int64_t decode_ws_bytes(int B, int H, int Lcap, int kc) {
    if (B <= 0 || H <= 0 || Lcap <= 0) return 0;
    return (int64_t)B * H * ((Lcap + kc - 1) / kc) * (kDecD + 2) * (int64_t)sizeof(float);
}

template <int KC>
void launch_decode_attn(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out, int64_t ld_out,
                        float* ws, int B, int H, int Lcap, float scale, hipStream_t stream) {
    const int nchunk_cap = (Lcap + KC - 1) / KC;
    float* ws_o = ws;
    float* ws_ml = ws + (int64_t)B * H * nchunk_cap * kDecD;
    hipLaunchKernelGGL(decode_attn_partial_kernel<KC>, dim3(nchunk_cap, H, B), dim3(64 * kDecWaves), 0, stream, (const u32x4*)q, ldq / 8,
                       (const u32x4*)kcache, (const u32x4*)vcache, lens, H, Lcap, nchunk_cap, scale * 1.4426950408889634f, ws_o, ws_ml);
    hipLaunchKernelGGL(decode_attn_combine_kernel<KC>, dim3(H, B), dim3(kDecD), 0, stream, ws_o, ws_ml, lens, H, Lcap, nchunk_cap,
                       (bf16_t*)out, ld_out);
}

}  // namespace

extern "C" int halva_decode_attn_kc(void) { return kDecodeKC; }

extern "C" int64_t halva_decode_attn_ws_bytes(int B, int H, int Lcap) { return decode_ws_bytes(B, H, Lcap, kDecodeKC); }

extern "C" int halva_decode_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, void* kcache, void* vcache,
                                        int32_t* lens, int B, int H, int D, int Lcap, void* stream) {
    HALVA_CHECK_ARG(qkv && cos && sin && kcache && vcache && lens, "decode_rope_append: null pointer");
    HALVA_CHECK_ARG(D == kDecD, "decode_rope_append: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(B > 0 && H > 0 && Lcap > 0 && max_pos > 0, "decode_rope_append: bad B=%d / H=%d / Lcap=%d / max_pos=%d", B, H, Lcap, max_pos);
    HALVA_CHECK_ARG(ldqkv >= 3LL * H * D && ldqkv % 8 == 0, "decode_rope_append: row stride %lld (needs >= 3*H*D and a multiple of 8)",
                    (long long)ldqkv);
    HALVA_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)kcache | (uintptr_t)vcache) % 16 == 0,
                    "decode_rope_append: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(decode_rope_append_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldqkv / 8, (const u32x4*)cos,
                       (const u32x4*)sin, max_pos, (u32x4*)kcache, (u32x4*)vcache, lens, H, Lcap);
    HALVA_CHECK_LAUNCH("decode_rope_append");
    return HALVA_OK;
}

static int decode_attn(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out, int64_t ld_out,
                       void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, int kc, void* stream) {
    HALVA_CHECK_ARG(q && kcache && vcache && lens && out && ws, "decode_attn: null pointer");
    HALVA_CHECK_ARG(D == kDecD, "decode_attn: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(B > 0 && H > 0 && Lcap > 0 && H <= 65535 && B <= 65535, "decode_attn: bad B=%d / H=%d / Lcap=%d", B, H, Lcap);
    HALVA_CHECK_ARG(kc == 64 || kc == 128 || kc == 256, "decode_attn: chunk of %d keys (64, 128 or 256)", kc);
    HALVA_CHECK_ARG(ldq >= (int64_t)H * D && ldq % 8 == 0, "decode_attn: q row stride %lld (needs >= H*D and a multiple of 8)", (long long)ldq);
    HALVA_CHECK_ARG(ld_out >= (int64_t)H * D, "decode_attn: out row stride %lld < H*D", (long long)ld_out);
    HALVA_CHECK_ARG(((uintptr_t)q | (uintptr_t)kcache | (uintptr_t)vcache | (uintptr_t)ws) % 16 == 0,
                    "decode_attn: q / cache / workspace pointers must be 16-byte aligned");
    const int64_t need = decode_ws_bytes(B, H, Lcap, kc);
    HALVA_CHECK_ARG(ws_bytes >= need, "decode_attn: workspace of %lld bytes, %lld needed (halva_decode_attn_ws_bytes)", (long long)ws_bytes,
                    (long long)need);
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    switch (kc) {
        case 64: launch_decode_attn<64>(q, ldq, kcache, vcache, lens, out, ld_out, (float*)ws, B, H, Lcap, scale, (hipStream_t)stream); break;
        case 128: launch_decode_attn<128>(q, ldq, kcache, vcache, lens, out, ld_out, (float*)ws, B, H, Lcap, scale, (hipStream_t)stream); break;
        default: launch_decode_attn<256>(q, ldq, kcache, vcache, lens, out, ld_out, (float*)ws, B, H, Lcap, scale, (hipStream_t)stream); break;
    }
    HALVA_CHECK_LAUNCH("decode_attn");
    return HALVA_OK;
}

extern "C" int halva_decode_attn(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out,
                                 int64_t ld_out, void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, void* stream) {
    return decode_attn(q, ldq, kcache, vcache, lens, out, ld_out, ws, ws_bytes, B, H, D, Lcap, scale, kDecodeKC, stream);
}

extern "C" int halva_decode_attn_chunked(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out,
                                         int64_t ld_out, void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, int kc,
                                         void* stream) {
    return decode_attn(q, ldq, kcache, vcache, lens, out, ld_out, ws, ws_bytes, B, H, D, Lcap, scale, kc, stream);
}

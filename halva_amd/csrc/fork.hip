// Forks of a kept KV cache (halva_amd/decode.py:ForkCache - n sampled continuations of one prompt, many questions about one image) on
// gfx950.  M members share P prefix rows of a parent cache and own only the rows behind them:
//   parent  K, V bf16 [Bp, H, Lpre, 128], read only, row p = prefix_of[m] up to prefix_lens[p] (recorded at fork time: slots at or beyond it
//           are never read, so the parent may go on appending);
//   own     K, V bf16 [M, H, Lown, 128], own_lens int32 [M]; own row t of member m sits at position prefix_lens[prefix_of[m]] + t.
// prefix_of int32 [M] is non-decreasing (members of one prefix row are contiguous), prefix_lens int32 [P]; every length lives on the
// device.  Nothing is copied from the parent.
//
// Decode step: fork_rope_append_kernel (rope_append.h's routine at the member's absolute position), then split-KV attention with KC = 256
// in two partial passes and one combine.  The prefix pass loads a chunk of a prefix row ONCE per workgroup - into the registers
// decode_attn_partial_kernel keeps its chunk in - and serves up to 16 members from that load, one after the other, each through
// decode_partial.h's routine: the VALU path (see DESIGN.md section 11 for why not MFMA).  The own pass is decode.hip's partial pass over
// the member's own rows.  A member's partials, and the order in which the combine pass merges them, are fixed by (prefix_lens[p],
// own_lens[m]) alone: its bits do not depend on M, on the other members, on its place in a block of 16 or on other prefix rows.
//
// Pushing n rows per member: extend.hip's two kernels with the prefix in front (extend_attn.h's body with its prefix phase on).
//
// Beam search (halva_amd/decode.py:BeamCache): the members are B prompts x K beams, and a beam that continues another beam's history moves
// no K / V row - an ancestry table anc int32 [M, Lown] names, per member and own row, the member whose slot holds it.  halva_fork_decode_attn
// and halva_beam_decode_attn are one launcher (fork_decode_attn: the checks and the three launches); given a table, its own pass reads
// through it (beam_own_partial_kernel).  halva_beam_advance derives the next step's table from this step's parents.
#include "common.h"
#include "decode_partial.h"
#include "rope_append.h"
#include <cmath>

namespace {

#include "sdpa_common.h"
#include "extend_attn.h"

static_assert(kDecChunks == kRopeChunks && kExtD == kDecD, "one head_dim");
constexpr int kForkKC = 256;        // keys per split-KV chunk, as halva_decode_attn
constexpr int kForkBlock = 16;      // members served from one load of a prefix chunk

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------------
// RoPE + append of one new row per member.  One workgroup per member, as decode_rope_append_kernel: every thread reads own_lens[m]
// before the barrier, thread 0 advances it after.  rope_append_row takes one index for the cos / sin row and the cache slot; the tables
// are handed over shifted by the prefix length, so that slot t reads the row of position prefix_lens[p] + t.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fork_rope_append_kernel(u32x4* __restrict__ qkv, int64_t ldq_chunks, const u32x4* __restrict__ cosb,
                                                               const u32x4* __restrict__ sinb, int max_pos, const int32_t* __restrict__ prefix_lens,
                                                               const int32_t* __restrict__ prefix_of, u32x4* __restrict__ kc, u32x4* __restrict__ vc,
                                                               int32_t* __restrict__ own_lens, int P, int H, int Lown) {
    const int m = blockIdx.x;
    const int p = prefix_of[m];
    const int t = own_lens[m];
    const int plen = (p >= 0 && p < P) ? prefix_lens[p] : -1;
    const bool ok = plen >= 0 && t >= 0 && t < Lown && (int64_t)plen + t < max_pos;      // a full own cache is left untouched, never overrun
    if (ok) {
        const int64_t shift = (int64_t)plen * (kRopeChunks / 2);
        rope_append_row(qkv + (int64_t)m * ldq_chunks, cosb + shift, sinb + shift, kc, vc, m, t, H, Lown);
    }
    __syncthreads();
    if (threadIdx.x == 0 && ok) own_lens[m] = t + 1;
}

// rows i < min(n_new[m], n) of member m at own slot own_lens[m] + i; own_lens is only read (halva_extend_advance moves it)
__global__ __launch_bounds__(256) void fork_extend_rope_append_kernel(u32x4* __restrict__ qkv, int64_t ldrow_chunks, int64_t ldseq_chunks,
                                                                      const u32x4* __restrict__ cosb, const u32x4* __restrict__ sinb, int max_pos,
                                                                      const int32_t* __restrict__ prefix_lens, const int32_t* __restrict__ prefix_of,
                                                                      u32x4* __restrict__ kc, u32x4* __restrict__ vc,
                                                                      const int32_t* __restrict__ own_lens, const int32_t* __restrict__ n_new, int n,
                                                                      int P, int H, int Lown) {
    const int i = blockIdx.x, m = blockIdx.y;
    const int p = prefix_of[m];
    const int past = own_lens[m];
    if (p < 0 || p >= P || past < 0 || i >= min(n_new[m], n)) return;
    const int plen = prefix_lens[p];
    const int t = past + i;
    if (plen < 0 || t >= Lown || (int64_t)plen + t >= max_pos) return;      // (the host refuses such calls; never written out of bounds)
    const int64_t shift = (int64_t)plen * (kRopeChunks / 2);
    rope_append_row(qkv + (int64_t)m * ldseq_chunks + (int64_t)i * ldrow_chunks, cosb + shift, sinb + shift, kc, vc, m, t, H, Lown);
}

// ---------------------------------------------------------------------------------------------------
// Prefix pass.  Grid (chunk c, head h, member m0); the workgroup works only when m0 opens a block of 16 among the members of its prefix
// row p (they are contiguous: the row's first member is found by bisection of prefix_of), and then serves members m0 .. m0 + cnt - 1 from
// one load of keys [c KC, (c + 1) KC) ∩ [0, prefix_lens[p]) of row p.  Every other workgroup leaves at once.  Record c of member m.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fork_prefix_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, const u32x4* __restrict__ pk,
                                                                  const u32x4* __restrict__ pv, const int32_t* __restrict__ prefix_lens,
                                                                  const int32_t* __restrict__ prefix_of, int M, int P, int H, int Lpre, int nrec,
                                                                  float qscale, float* __restrict__ ws_o, float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, m0 = blockIdx.z;
    const int p = prefix_of[m0];
    if (p < 0 || p >= P) return;                   // (every exit is uniform over the workgroup: no barrier is skipped by part of it)
    const int plen = clampi(prefix_lens[p], 0, Lpre);
    const int k0 = c * kForkKC;
    if (k0 >= plen) return;
    int lo = 0, hi = m0;                           // first member of row p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix_of[mid] < p) lo = mid + 1; else hi = mid;
    }
    if ((m0 - lo) % kForkBlock != 0) return;
    int cnt = 1;
    while (cnt < kForkBlock && m0 + cnt < M && prefix_of[m0 + cnt] == p) ++cnt;
    const int sub = threadIdx.x & 15;
    const int64_t ph = ((int64_t)p * H + h) * Lpre * kDecChunks + sub;
    DecChunkRegs<kForkKC> ch;
    ch.load(pk + ph, pv + ph, k0, plen);
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
        const int64_t m = m0 + j;
        // keep the chunk packed (128 VGPRs) across members: left alone, the compiler unpacks it to fp32 once in front of the loop, which
        // takes every register of the wave (256 VGPRs + AGPRs, one wave per SIMD) to save two VALU operations per element
#pragma unroll
        for (int i = 0; i < DecChunkRegs<kForkKC>::NI; ++i) asm volatile("" : "+v"(ch.kr[i]), "+v"(ch.vr[i]));
        const u32x4 q8 = q[m * ldq_chunks + h * kDecChunks + sub];
        decode_chunk_partial<kForkKC>(q8, ch, k0, plen, qscale, ws_o, ws_ml, (m * H + h) * nrec + c);
        __syncthreads();                           // the routine's LDS is free again
    }
}

// Own pass: decode_attn_partial_kernel over the member's own rows, chunked from own key 0.  Record npre_cap + c of member m.
__global__ __launch_bounds__(256) void fork_own_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, const u32x4* __restrict__ kc,
                                                               const u32x4* __restrict__ vc, const int32_t* __restrict__ own_lens, int H, int Lown,
                                                               int npre_cap, int nrec, float qscale, float* __restrict__ ws_o,
                                                               float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, m = blockIdx.z;
    const int len = clampi(own_lens[m], 0, Lown);
    const int k0 = c * kForkKC;
    if (k0 >= len) return;
    const int sub = threadIdx.x & 15;
    const int64_t mh = (int64_t)m * H + h;
    const u32x4 q8 = q[(int64_t)m * ldq_chunks + h * kDecChunks + sub];
    DecChunkRegs<kForkKC> ch;
    ch.load(kc + mh * Lown * kDecChunks + sub, vc + mh * Lown * kDecChunks + sub, k0, len);
    decode_chunk_partial<kForkKC>(q8, ch, k0, len, qscale, ws_o, ws_ml, mh * nrec + npre_cap + c);
}

// Beam search's own pass (halva_amd/decode.py:BeamCache): fork_own_partial_kernel with key t of member m fetched from own slot
// (anc[m][t], h, t) - the ancestry table says whose slot holds row t of m's history; no K / V row is ever copied when a beam continues
// another beam.  Slots at or beyond own_lens[m] are never read, and neither is any slot (m', t) with m' != anc[m][t] on behalf of m.
__global__ __launch_bounds__(256) void beam_own_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, const u32x4* __restrict__ kc,
                                                               const u32x4* __restrict__ vc, const int32_t* __restrict__ own_lens,
                                                               const int32_t* __restrict__ anc, int M, int H, int Lown, int npre_cap, int nrec,
                                                               float qscale, float* __restrict__ ws_o, float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, m = blockIdx.z;
    const int len = clampi(own_lens[m], 0, Lown);
    const int k0 = c * kForkKC;
    if (k0 >= len) return;
    const int sub = threadIdx.x & 15;
    const int64_t mh = (int64_t)m * H + h;
    const u32x4 q8 = q[(int64_t)m * ldq_chunks + h * kDecChunks + sub];
    DecChunkRegs<kForkKC> ch;
    ch.load_via(kc + sub, vc + sub, anc + (int64_t)m * Lown, h, H, Lown, M, k0, len);
    decode_chunk_partial<kForkKC>(q8, ch, k0, len, qscale, ws_o, ws_ml, mh * nrec + npre_cap + c);
}

// The ancestry table of the next step from this step's parents, one workgroup per member: with t = own_lens[m] (before this step's
// append), dst[m][j] = src[parent[m]][j] for j < t and dst[m][t] = m, the slot halva_fork_rope_append is about to write.  dst[m][j] for
// j > t is not written; a parent outside [0, M) or t outside [0, Lown) leaves row m untouched.
__global__ __launch_bounds__(256) void beam_advance_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                           const int32_t* __restrict__ parent, const int32_t* __restrict__ own_lens, int M, int Lown) {
    const int m = blockIdx.x;
    const int p = parent[m], t = own_lens[m];
    if (p < 0 || p >= M || t < 0 || t >= Lown) return;
    const int32_t* s = src + (int64_t)p * Lown;
    int32_t* d = dst + (int64_t)m * Lown;
    for (int j = threadIdx.x; j < t; j += blockDim.x) d[j] = s[j];
    if (threadIdx.x == 0) d[t] = m;
}

// Combine: one workgroup of 128 threads per (head, member) merges the ceil(prefix_lens[p] / KC) prefix records and then the
// ceil(own_lens[m] / KC) own records, in that order, in the log2 domain as decode_attn_combine_kernel does.
__global__ __launch_bounds__(128) void fork_combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
                                                           const int32_t* __restrict__ prefix_lens, const int32_t* __restrict__ prefix_of,
                                                           const int32_t* __restrict__ own_lens, int P, int H, int Lpre, int Lown, int npre_cap,
                                                           int nrec, bf16_t* __restrict__ out, int64_t ld_out) {
    const int h = blockIdx.x, m = blockIdx.y, d = threadIdx.x;
    const int p = prefix_of[m];
    const int plen = (p >= 0 && p < P) ? clampi(prefix_lens[p], 0, Lpre) : 0;
    const int olen = clampi(own_lens[m], 0, Lown);
    const int npre = (plen + kForkKC - 1) / kForkKC, nown = (olen + kForkKC - 1) / kForkKC;
    const int64_t slot0 = ((int64_t)m * H + h) * nrec;
    float Mx = -INFINITY;
    for (int c = 0; c < npre; ++c) Mx = fmaxf(Mx, ws_ml[(slot0 + c) * 2]);
    for (int c = 0; c < nown; ++c) Mx = fmaxf(Mx, ws_ml[(slot0 + npre_cap + c) * 2]);
    float acc = 0.f, L = 0.f;
    for (int c = 0; c < npre; ++c) {
        const float f = exp2f(ws_ml[(slot0 + c) * 2] - Mx);
        acc = fmaf(f, ws_o[(slot0 + c) * kDecD + d], acc);
        L = fmaf(f, ws_ml[(slot0 + c) * 2 + 1], L);
    }
    for (int c = 0; c < nown; ++c) {
        const int64_t s = slot0 + npre_cap + c;
        const float f = exp2f(ws_ml[s * 2] - Mx);
        acc = fmaf(f, ws_o[s * kDecD + d], acc);
        L = fmaf(f, ws_ml[s * 2 + 1], L);
    }
    out[(int64_t)m * ld_out + h * kDecD + d] = f32_to_bf16(npre + nown > 0 ? acc / L : 0.f);
}

// ---------------------------------------------------------------------------------------------------
// Attention of n new rows per member: extend_attn_kernel with the prefix row's tiles in front (extend_attn.h).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kExtWaves, 2) void fork_extend_attn_kernel(const bf16_t* __restrict__ q, int64_t ldrow, int64_t ldseq,
                                                                          const bf16_t* __restrict__ pk, const bf16_t* __restrict__ pv,
                                                                          const int32_t* __restrict__ prefix_lens,
                                                                          const int32_t* __restrict__ prefix_of, const bf16_t* __restrict__ kc,
                                                                          const bf16_t* __restrict__ vc, const int32_t* __restrict__ own_lens,
                                                                          const int32_t* __restrict__ n_new, bf16_t* __restrict__ out,
                                                                          int64_t ld_out_row, int64_t ld_out_seq, int n, int P, int H, int Lpre,
                                                                          int Lown, float sc) {
    const int qb = blockIdx.x, hd = blockIdx.y, m = blockIdx.z;
    const int p = prefix_of[m];
    const int past = own_lens[m];
    if (p < 0 || p >= P || past < 0) return;
    const int plen = clampi(prefix_lens[p], 0, Lpre);
    const int nn = ext_rows(past, n_new[m], n, Lown);
    const int64_t ph = ((int64_t)p * H + hd) * Lpre * kExtD, mh = ((int64_t)m * H + hd) * Lown * kExtD;
    extend_attn_body<true>(q + (int64_t)m * ldseq, ldrow, pk + ph, pv + ph, plen, kc + mh, vc + mh, past, nn, out + (int64_t)m * ld_out_seq,
                           ld_out_row, qb, hd, sc);
}

int64_t fork_ws_bytes(int M, int H, int Lpre, int Lown) {
    if (M <= 0 || H <= 0 || Lpre <= 0 || Lown <= 0) return 0;
    const int64_t nrec = (int64_t)(Lpre + kForkKC - 1) / kForkKC + (Lown + kForkKC - 1) / kForkKC;
    return (int64_t)M * H * nrec * (kDecD + 2) * (int64_t)sizeof(float);
}

}  // namespace

extern "C" int64_t halva_fork_decode_attn_ws_bytes(int M, int H, int Lpre, int Lown) { return fork_ws_bytes(M, H, Lpre, Lown); }

extern "C" int halva_fork_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, void* kown, void* vown, int32_t* own_lens, int M, int P, int H, int D, int Lown,
                                      void* stream) {
    HALVA_CHECK_ARG(qkv && cos && sin && prefix_lens && prefix_of && kown && vown && own_lens, "fork_rope_append: null pointer");
    HALVA_CHECK_ARG(D == kDecD, "fork_rope_append: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(M > 0 && P > 0 && H > 0 && Lown > 0 && max_pos > 0, "fork_rope_append: bad M=%d / P=%d / H=%d / Lown=%d / max_pos=%d", M, P, H,
                    Lown, max_pos);
    HALVA_CHECK_ARG(ldqkv >= 3LL * H * D && ldqkv % 8 == 0, "fork_rope_append: row stride %lld (needs >= 3*H*D and a multiple of 8)",
                    (long long)ldqkv);
    HALVA_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)kown | (uintptr_t)vown) % 16 == 0,
                    "fork_rope_append: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(fork_rope_append_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldqkv / 8, (const u32x4*)cos,
                       (const u32x4*)sin, max_pos, prefix_lens, prefix_of, (u32x4*)kown, (u32x4*)vown, own_lens, P, H, Lown);
    HALVA_CHECK_LAUNCH("fork_rope_append");
    return HALVA_OK;
}

// The decode attention of forks and beams: every check, then the prefix pass, the own pass - through the ancestry table anc when one is
// given, plain when anc is null - and the combine.  name: the entry's, for its error messages.
static int fork_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens, const int32_t* prefix_of,
                            const void* kown, const void* vown, const int32_t* own_lens, void* out, int64_t ld_out, void* ws, int64_t ws_bytes,
                            int M, int P, int H, int D, int Lpre, int Lown, float scale, void* stream, const int32_t* anc, const char* name) {
    HALVA_CHECK_ARG(q && pk && pv && prefix_lens && prefix_of && kown && vown && own_lens && out && ws, "%s: null pointer", name);
    HALVA_CHECK_ARG(D == kDecD, "%s: head_dim=%d (only 128)", name, D);
    HALVA_CHECK_ARG(M > 0 && P > 0 && H > 0 && Lpre > 0 && Lown > 0 && H <= 65535 && M <= 65535, "%s: bad M=%d / P=%d / H=%d / Lpre=%d / Lown=%d",
                    name, M, P, H, Lpre, Lown);
    HALVA_CHECK_ARG(ldq >= (int64_t)H * D && ldq % 8 == 0, "%s: q row stride %lld (needs >= H*D and a multiple of 8)", name, (long long)ldq);
    HALVA_CHECK_ARG(ld_out >= (int64_t)H * D, "%s: out row stride %lld < H*D", name, (long long)ld_out);
    HALVA_CHECK_ARG(((uintptr_t)q | (uintptr_t)pk | (uintptr_t)pv | (uintptr_t)kown | (uintptr_t)vown | (uintptr_t)ws) % 16 == 0,
                    "%s: q / cache / workspace pointers must be 16-byte aligned", name);
    const int64_t need = fork_ws_bytes(M, H, Lpre, Lown);
    HALVA_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (halva_fork_decode_attn_ws_bytes)", name, (long long)ws_bytes,
                    (long long)need);
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    const int npre_cap = (Lpre + kForkKC - 1) / kForkKC, nown_cap = (Lown + kForkKC - 1) / kForkKC, nrec = npre_cap + nown_cap;
    float* ws_o = (float*)ws;
    float* ws_ml = ws_o + (int64_t)M * H * nrec * kDecD;
    const float qscale = scale * 1.4426950408889634f;
    hipLaunchKernelGGL(fork_prefix_partial_kernel, dim3(npre_cap, H, M), dim3(64 * kDecWaves), 0, (hipStream_t)stream, (const u32x4*)q, ldq / 8,
                       (const u32x4*)pk, (const u32x4*)pv, prefix_lens, prefix_of, M, P, H, Lpre, nrec, qscale, ws_o, ws_ml);
    if (anc)
        hipLaunchKernelGGL(beam_own_partial_kernel, dim3(nown_cap, H, M), dim3(64 * kDecWaves), 0, (hipStream_t)stream, (const u32x4*)q, ldq / 8,
                           (const u32x4*)kown, (const u32x4*)vown, own_lens, anc, M, H, Lown, npre_cap, nrec, qscale, ws_o, ws_ml);
    else
        hipLaunchKernelGGL(fork_own_partial_kernel, dim3(nown_cap, H, M), dim3(64 * kDecWaves), 0, (hipStream_t)stream, (const u32x4*)q, ldq / 8,
                           (const u32x4*)kown, (const u32x4*)vown, own_lens, H, Lown, npre_cap, nrec, qscale, ws_o, ws_ml);
    hipLaunchKernelGGL(fork_combine_kernel, dim3(H, M), dim3(kDecD), 0, (hipStream_t)stream, ws_o, ws_ml, prefix_lens, prefix_of, own_lens, P, H,
                       Lpre, Lown, npre_cap, nrec, (bf16_t*)out, ld_out);
    HALVA_CHECK_LAUNCH(name);
    return HALVA_OK;
}

extern "C" int halva_fork_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens, void* out,
                                      int64_t ld_out, void* ws, int64_t ws_bytes, int M, int P, int H, int D, int Lpre, int Lown, float scale,
                                      void* stream) {
    return fork_decode_attn(q, ldq, pk, pv, prefix_lens, prefix_of, kown, vown, own_lens, out, ld_out, ws, ws_bytes, M, P, H, D, Lpre, Lown, scale,
                            stream, nullptr, "fork_decode_attn");
}

extern "C" int halva_beam_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens, const int32_t* anc,
                                      void* out, int64_t ld_out, void* ws, int64_t ws_bytes, int M, int P, int H, int D, int Lpre, int Lown,
                                      float scale, void* stream) {
    HALVA_CHECK_ARG(anc, "beam_decode_attn: null pointer");
    HALVA_CHECK_ARG((uintptr_t)anc % 4 == 0, "beam_decode_attn: the ancestry table must be 4-byte aligned");
    return fork_decode_attn(q, ldq, pk, pv, prefix_lens, prefix_of, kown, vown, own_lens, out, ld_out, ws, ws_bytes, M, P, H, D, Lpre, Lown, scale,
                            stream, anc, "beam_decode_attn");
}

extern "C" int halva_beam_advance(const int32_t* anc_src, int32_t* anc_dst, const int32_t* parent, const int32_t* own_lens, int M, int Lown,
                                  void* stream) {
    HALVA_CHECK_ARG(anc_src && anc_dst && parent && own_lens, "beam_advance: null pointer");
    HALVA_CHECK_ARG(M > 0 && Lown > 0 && M <= 65535, "beam_advance: bad M=%d / Lown=%d", M, Lown);
    HALVA_CHECK_ARG(((uintptr_t)anc_src | (uintptr_t)anc_dst | (uintptr_t)parent | (uintptr_t)own_lens) % 4 == 0,
                    "beam_advance: pointers must be 4-byte aligned");
    const int64_t bytes = (int64_t)M * Lown * (int64_t)sizeof(int32_t);
    const intptr_t gap = (intptr_t)((uintptr_t)anc_dst - (uintptr_t)anc_src);
    HALVA_CHECK_ARG(gap >= bytes || gap <= -bytes, "beam_advance: source and destination tables overlap (they are the two halves of one pair)");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, anc_src, anc_dst, parent, own_lens, M, Lown);
    HALVA_CHECK_LAUNCH("beam_advance");
    return HALVA_OK;
}

extern "C" int halva_fork_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos,
                                             const int32_t* prefix_lens, const int32_t* prefix_of, void* kown, void* vown,
                                             const int32_t* own_lens, const int32_t* n_new, int M, int n, int P, int H, int D, int Lown,
                                             void* stream) {
    HALVA_CHECK_ARG(qkv && cos && sin && prefix_lens && prefix_of && kown && vown && own_lens && n_new, "fork_extend_rope_append: null pointer");
    HALVA_CHECK_ARG(D == kDecD, "fork_extend_rope_append: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(M > 0 && n > 0 && P > 0 && H > 0 && Lown > 0 && max_pos > 0 && M <= 65535,
                    "fork_extend_rope_append: bad M=%d / n=%d / P=%d / H=%d / Lown=%d / max_pos=%d", M, n, P, H, Lown, max_pos);
    HALVA_CHECK_ARG(ldrow >= 3LL * H * D && ldrow % 8 == 0, "fork_extend_rope_append: row stride %lld (needs >= 3*H*D and a multiple of 8)",
                    (long long)ldrow);
    HALVA_CHECK_ARG(ldseq >= (int64_t)n * ldrow && ldseq % 8 == 0,
                    "fork_extend_rope_append: sequence stride %lld (needs >= n * row stride and a multiple of 8)", (long long)ldseq);
    HALVA_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)cos | (uintptr_t)sin | (uintptr_t)kown | (uintptr_t)vown) % 16 == 0,
                    "fork_extend_rope_append: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(fork_extend_rope_append_kernel, dim3(n, M), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldrow / 8, ldseq / 8,
                       (const u32x4*)cos, (const u32x4*)sin, max_pos, prefix_lens, prefix_of, (u32x4*)kown, (u32x4*)vown, own_lens, n_new, n, P, H,
                       Lown);
    HALVA_CHECK_LAUNCH("fork_extend_rope_append");
    return HALVA_OK;
}

extern "C" int halva_fork_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens,
                                      const int32_t* n_new, void* out, int64_t ld_out_row, int64_t ld_out_seq, int M, int n, int P, int H, int D,
                                      int Lpre, int Lown, float scale, void* stream) {
    HALVA_CHECK_ARG(q && pk && pv && prefix_lens && prefix_of && kown && vown && own_lens && n_new && out, "fork_extend_attn: null pointer");
    HALVA_CHECK_ARG(D == kExtD, "fork_extend_attn: head_dim=%d (only 128)", D);
    HALVA_CHECK_ARG(M > 0 && n > 0 && P > 0 && H > 0 && Lpre > 0 && Lown > 0 && H <= 65535 && M <= 65535,
                    "fork_extend_attn: bad M=%d / n=%d / P=%d / H=%d / Lpre=%d / Lown=%d", M, n, P, H, Lpre, Lown);
    HALVA_CHECK_ARG(ldrow >= (int64_t)H * D && ldrow % 8 == 0, "fork_extend_attn: q row stride %lld (needs >= H*D and a multiple of 8)",
                    (long long)ldrow);
    HALVA_CHECK_ARG(ldseq >= (int64_t)n * ldrow && ldseq % 8 == 0,
                    "fork_extend_attn: q sequence stride %lld (needs >= n * row stride and a multiple of 8)", (long long)ldseq);
    HALVA_CHECK_ARG(ld_out_row >= (int64_t)H * D && ld_out_row % 8 == 0, "fork_extend_attn: out row stride %lld (needs >= H*D and a multiple of 8)",
                    (long long)ld_out_row);
    HALVA_CHECK_ARG(ld_out_seq >= (int64_t)n * ld_out_row && ld_out_seq % 8 == 0,
                    "fork_extend_attn: out sequence stride %lld (needs >= n * row stride and a multiple of 8)", (long long)ld_out_seq);
    HALVA_CHECK_ARG(((uintptr_t)q | (uintptr_t)pk | (uintptr_t)pv | (uintptr_t)kown | (uintptr_t)vown | (uintptr_t)out) % 16 == 0,
                    "fork_extend_attn: q / cache / out pointers must be 16-byte aligned");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    hipLaunchKernelGGL(fork_extend_attn_kernel, dim3((n + kExtBM - 1) / kExtBM, H, M), dim3(64 * kExtWaves), 0, (hipStream_t)stream,
                       (const bf16_t*)q, ldrow, ldseq, (const bf16_t*)pk, (const bf16_t*)pv, prefix_lens, prefix_of, (const bf16_t*)kown,
                       (const bf16_t*)vown, own_lens, n_new, (bf16_t*)out, ld_out_row, ld_out_seq, n, P, H, Lpre, Lown, scale * kLog2e);
    HALVA_CHECK_LAUNCH("fork_extend_attn");
    return HALVA_OK;
}

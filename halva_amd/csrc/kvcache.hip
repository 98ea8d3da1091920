// The KV-cache kernels of generation (halva_amd/decode.py: KVCache, ForkCache, BeamCache) on gfx950, written once over a CacheView
// (cache_view.h: the layout).  A plain cache is the fork without a prefix, a beam cache the fork whose own pass reads through a table; the
// entry points differ only in the view they build.
//
// Step (one new row per cache row; HBM-bound, no MFMA):
//   rope_append_kernel<true>    rope_append.h's routine at position prefix + lens[m], own slot lens[m]; the workgroup advances lens[m].
//   split-KV attention          one query row per (row, head) in chunks of KC keys (256; 64 / 128 through the measurement entry).  A partial
//                               pass writes a record (m, l, o[128]) per chunk to the fp32 workspace, a combine pass merges a row's records:
//                                 prefix_partial_kernel   only with a prefix: a chunk of prefix row p loaded ONCE per workgroup and served to
//                                                         up to 16 members of that row - record c of each member;
//                                 own_partial_kernel      a chunk of the row's own keys, chunked from own key 0 - record npre_cap + c;
//                                 combine_kernel          the ceil(prefix / KC) prefix records, then the ceil(lens[m] / KC) own ones.
//                               Workspace: [rows, H, nrec, 128] o, then [rows, H, nrec, 2] (m, l), nrec = ceil(Lpre / KC) + ceil(L / KC) with
//                               Lpre = 0 for a plain cache.  Both partial passes run decode_partial.h's one routine on the VALU (DESIGN.md
//                               section 11 for why not MFMA); a row's records and their order are fixed by (prefix length, lens[m]) alone:
//                               its bits do not depend on the number of rows, on the other rows, or on its place in a block of 16.
// Rows (up to n new rows per cache row - sessions, chunked prefill, questions about one image), three launches, so that no workgroup reads
// a lens value written by its own launch:
//   rope_append_kernel<false>   row i < n_new[m] at position prefix + lens[m] + i, own slot lens[m] + i; lens is only read.
//   rows_attn_kernel            causal attention of the new rows on MFMA (extend_attn.h's body; with a prefix its 64-key tiles come first).
//   extend_advance_kernel       lens[m] += n_new[m].
#include "cache_view.h"
#include "decode_partial.h"      // kDecD / kDecChunks / kDecWaves, DecChunkRegs, decode_chunk_partial: one chunk's partial
#include "rope_append.h"
#include <climits>
#include <cmath>
#include <initializer_list>

namespace {

#include "sdpa_common.h"      // tile_off / mfma32 / frag_rows / frag_cols / Stage / store_rows_T, mask_half / half_max / xhalf_*: the attention kernels' tile pieces
#include "extend_attn.h"      // kExt*, ext_rows, ext_tile, extend_attn_body: the rows attention's kernel body

static_assert(kDecChunks == kRopeChunks && kExtD == kDecD, "one head_dim");
constexpr int kDecodeKC = 256;       // keys per split-KV chunk (tools/bench_decode.py: 4.85 TB/s at 256, 4.73 at 128, 4.54 at 64)
constexpr int kPrefixBlock = 16;     // members served from one load of a prefix chunk

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------------------------------------------
// RoPE + append.  STEP: one workgroup per cache row m - every thread reads lens[m] before the barrier, thread 0 advances it after, so no
// other reader of this launch sees the new value.  Otherwise one workgroup per (row i, cache row m) and lens is only read
// (extend_advance_kernel moves it).  rope_append_row takes one index for the cos / sin row and the cache slot; the tables are handed
// over shifted by the prefix length, so that own slot t reads the row of position prefix + t.  A full cache is left untouched, a position
// at or beyond max_pos and a prefix_of[m] that names no prefix row are refused: nothing is written out of bounds.
// ---------------------------------------------------------------------------------------------------
template <bool STEP>
__global__ __launch_bounds__(256) void rope_append_kernel(u32x4* __restrict__ qkv, int64_t ldrow_chunks, int64_t ldseq_chunks,
                                                          const u32x4* __restrict__ cosb, const u32x4* __restrict__ sinb, int max_pos, CacheView cv,
                                                          const int32_t* __restrict__ n_new, int n) {
    const int i = STEP ? 0 : blockIdx.x, m = STEP ? blockIdx.x : blockIdx.y;
    int p;
    const int plen = cv.prefix_len(m, p);
    const int past = cv.lens[m];
    const int t = past + i;
    bool ok = p >= 0 && plen >= 0 && past >= 0 && t < cv.L && (int64_t)plen + t < max_pos;
    if (!STEP) ok = ok && i < min(n_new[m], n);
    if (ok) {
        const int64_t shift = (int64_t)plen * (kRopeChunks / 2);
        rope_append_row(qkv + (int64_t)m * ldseq_chunks + (int64_t)i * ldrow_chunks, cosb + shift, sinb + shift, cv.k, cv.v, m, t, cv.H, cv.L);
    }
    if (STEP) {
        __syncthreads();
        if (threadIdx.x == 0 && ok) cv.lens[m] = t + 1;
    }
}

__global__ void extend_advance_kernel(int32_t* __restrict__ lens, const int32_t* __restrict__ n_new, int B, int Lcap) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) lens[b] = min(max(lens[b], 0) + max(n_new[b], 0), Lcap);
}

// ---------------------------------------------------------------------------------------------------
// Prefix pass.  Grid (chunk c, head h, member m0); the workgroup works only when m0 opens a block of 16 among the members of its prefix
// row p (they are contiguous: the row's first member is found by bisection of prefix_of), and then serves members m0 .. m0 + cnt - 1 from
// one load of keys [c KC, (c + 1) KC) ∩ [0, prefix length) of row p.  Every other workgroup leaves at once.  Record c of member m.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prefix_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, CacheView cv, int nrec, float qscale,
                                                             float* __restrict__ ws_o, float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, m0 = blockIdx.z;
    int p;
    const int plen = cv.prefix_len(m0, p);
    if (p < 0) return;                             // (every exit is uniform over the workgroup: no barrier is skipped by part of it)
    const int k0 = c * kDecodeKC;
    if (k0 >= plen) return;
    int lo = 0, hi = m0;                           // first member of row p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cv.prefix_of[mid] < p) lo = mid + 1; else hi = mid;
    }
    if ((m0 - lo) % kPrefixBlock != 0) return;
    int cnt = 1;
    while (cnt < kPrefixBlock && m0 + cnt < cv.rows && cv.prefix_of[m0 + cnt] == p) ++cnt;
    const int sub = threadIdx.x & 15;
    const int64_t ph = ((int64_t)p * cv.H + h) * cv.Lpre * kDecChunks + sub;
    DecChunkRegs<kDecodeKC> ch;
    ch.load(cv.pk + ph, cv.pv + ph, k0, plen);
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
        const int64_t m = m0 + j;
        // keep the chunk packed (128 VGPRs) across members: left alone, the compiler unpacks it to fp32 once in front of the loop, which
        // takes every register of the wave (256 VGPRs + AGPRs, one wave per SIMD) to save two VALU operations per element
#pragma unroll
        for (int i = 0; i < DecChunkRegs<kDecodeKC>::NI; ++i) asm volatile("" : "+v"(ch.kr[i]), "+v"(ch.vr[i]));
        const u32x4 q8 = q[m * ldq_chunks + h * kDecChunks + sub];
        decode_chunk_partial<kDecodeKC>(q8, ch, k0, plen, qscale, ws_o, ws_ml, (m * cv.H + h) * nrec + c);
        __syncthreads();                           // the routine's LDS is free again
    }
}

// ---------------------------------------------------------------------------------------------------
// Own pass.  Workgroup (chunk c, head h, row m) covers own keys [c KC, (c + 1) KC) ∩ [0, lens[m]); 4 waves of KC / 4 keys each, straight
// to VGPRs (decode_partial.h).  VIA_TABLE (beam search): key t is fetched from own slot (anc[m][t], h, t) - the ancestry table says whose
// slot holds row t of m's history; no K / V row is ever copied when a beam continues another beam, and no slot (m', t) with
// m' != anc[m][t] is read on behalf of m.  Record npre_cap + c of row m.
// ---------------------------------------------------------------------------------------------------
template <int KC, bool VIA_TABLE>
__global__ __launch_bounds__(256) void own_partial_kernel(const u32x4* __restrict__ q, int64_t ldq_chunks, CacheView cv, int npre_cap, int nrec,
                                                          float qscale, float* __restrict__ ws_o, float* __restrict__ ws_ml) {
    const int c = blockIdx.x, h = blockIdx.y, m = blockIdx.z;
    const int len = clampi(cv.lens[m], 0, cv.L);
    const int k0 = c * KC;
    if (k0 >= len) return;                         // (uniform over the workgroup: no barrier is skipped by part of it)
    const int sub = threadIdx.x & 15;
    const int64_t mh = (int64_t)m * cv.H + h;
    const u32x4 q8 = q[(int64_t)m * ldq_chunks + h * kDecChunks + sub];
    DecChunkRegs<KC> ch;
    if constexpr (VIA_TABLE)
        ch.load_via(cv.k + sub, cv.v + sub, cv.anc + (int64_t)m * cv.L, h, cv.H, cv.L, cv.rows, k0, len);
    else
        ch.load(cv.k + mh * cv.L * kDecChunks + sub, cv.v + mh * cv.L * kDecChunks + sub, k0, len);
    decode_chunk_partial<KC>(q8, ch, k0, len, qscale, ws_o, ws_ml, mh * nrec + npre_cap + c);
}

// Combine: one workgroup of 128 threads per (head, row) merges the row's prefix records and then its own records, in that order, in the
// log2 domain.  A row without a key gives 0.  PREFIX = false is the plain cache's instantiation: no prefix record exists, and the loops
// are those over the own records alone (measured: with the prefix range left to run time, the plain attention at 64-key chunks - 32
// records a row - came out 1 - 2 % above the spread of the kernel it replaces, profiles/r15_one_cache_kernel_set.md).
template <int KC, bool PREFIX>
__global__ __launch_bounds__(128) void combine_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml, CacheView cv, int npre_cap,
                                                      int nrec, bf16_t* __restrict__ out, int64_t ld_out) {
    const int h = blockIdx.x, m = blockIdx.y, d = threadIdx.x;
    int p;
    const int plen = PREFIX ? max(cv.prefix_len(m, p), 0) : 0;
    const int olen = clampi(cv.lens[m], 0, cv.L);
    const int npre = (plen + KC - 1) / KC, n = npre + (olen + KC - 1) / KC;
    const int64_t slot0 = ((int64_t)m * cv.H + h) * nrec;
    const int gap = PREFIX ? npre_cap - npre : 0;      // the own records sit behind room for npre_cap prefix records
    auto rec = [&](int c) { return slot0 + c + (c < npre ? 0 : gap); };
    float M = -INFINITY;
    for (int c = 0; c < n; ++c) M = fmaxf(M, ws_ml[rec(c) * 2]);
    float acc = 0.f, L = 0.f;
    for (int c = 0; c < n; ++c) {
        const int64_t s = rec(c);
        const float f = exp2f(ws_ml[s * 2] - M);
        acc = fmaf(f, ws_o[s * kDecD + d], acc);
        L = fmaf(f, ws_ml[s * 2 + 1], L);
    }
    out[(int64_t)m * ld_out + h * kDecD + d] = f32_to_bf16(n > 0 ? acc / L : 0.f);
}

// ---------------------------------------------------------------------------------------------------
// Attention of the new rows: workgroup (row block qb, head h, cache row m) runs extend_attn.h's body, with its prefix phase when the view
// has a prefix.
// ---------------------------------------------------------------------------------------------------
template <bool PREFIX>
__global__ __launch_bounds__(64 * kExtWaves, 2) void rows_attn_kernel(const bf16_t* __restrict__ q, int64_t ldrow, int64_t ldseq, CacheView cv,
                                                                   const int32_t* __restrict__ n_new, bf16_t* __restrict__ out,
                                                                   int64_t ld_out_row, int64_t ld_out_seq, int n, float sc) {
    const int qb = blockIdx.x, hd = blockIdx.y, m = blockIdx.z;
    int p;
    const int plen = max(cv.prefix_len(m, p), 0);
    const int past = cv.lens[m];
    if (p < 0 || past < 0) return;
    const int nn = ext_rows(past, n_new[m], n, cv.L);
    const int64_t ph = ((int64_t)p * cv.H + hd) * cv.Lpre * kExtD, mh = ((int64_t)m * cv.H + hd) * cv.L * kExtD;
    const bf16_t* pk = (const bf16_t*)cv.pk;
    const bf16_t* pv = (const bf16_t*)cv.pv;
    extend_attn_body<PREFIX>(q + (int64_t)m * ldseq, ldrow, PREFIX ? pk + ph : nullptr, PREFIX ? pv + ph : nullptr, plen,
                             (const bf16_t*)cv.k + mh, (const bf16_t*)cv.v + mh, past, nn, out + (int64_t)m * ld_out_seq, ld_out_row, qb, hd, sc);
}

// ===================================================================================================
// Host side: one view builder, each check once, one launcher per operation.  `name` is the entry's, for its messages; `fork` says that
// the entry takes a prefix (its pointers and sizes are then required, not optional).
// ===================================================================================================
CacheView view(const void* k, const void* v, const int32_t* lens, int rows, int H, int L, const int32_t* prefix_lens = nullptr,
               const int32_t* prefix_of = nullptr, int P = 0, const void* pk = nullptr, const void* pv = nullptr, int Lpre = 0,
               const int32_t* anc = nullptr) {
    return CacheView{(u32x4*)k, (u32x4*)v, (int32_t*)lens, rows, H, L, (const u32x4*)pk, (const u32x4*)pv, prefix_lens, prefix_of, P, Lpre, anc};
}

bool all_set(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (!p) return false;
    return true;
}
bool aligned16(std::initializer_list<const void*> ptrs) {      // (a null pointer is aligned: optional ones pass)
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= (uintptr_t)p;
    return bits % 16 == 0;
}

#define HALVA_TRY(call)         \
    do {                        \
        const int rc_ = (call); \
        if (rc_) return rc_;    \
    } while (0)

// The cache of an entry: pointers, head_dim, sizes, alignment.  attn: the entry reads the prefix rows (pk, pv, Lpre) and puts H in the
// grid; max_rows: 65535 where the rows go to grid.y / grid.z.
int check_cache(const char* name, const CacheView& cv, int D, bool fork, bool attn, int max_rows) {
    HALVA_CHECK_ARG(all_set({cv.k, cv.v, cv.lens}) && (!fork || all_set({cv.prefix_lens, cv.prefix_of})) && (!fork || !attn || all_set({cv.pk, cv.pv})),
                    "%s: null pointer", name);
    HALVA_CHECK_ARG(D == kDecD, "%s: head_dim=%d (only 128)", name, D);
    const bool sizes = cv.rows > 0 && cv.rows <= max_rows && cv.H > 0 && (!attn || cv.H <= 65535) && cv.L > 0 &&
                       (!fork || (cv.P > 0 && (!attn || cv.Lpre > 0)));
    if (fork)
        HALVA_CHECK_ARG(sizes, "%s: bad M=%d / P=%d / H=%d / Lpre=%d / Lown=%d", name, cv.rows, cv.P, cv.H, cv.Lpre, cv.L);
    else
        HALVA_CHECK_ARG(sizes, "%s: bad B=%d / H=%d / Lcap=%d", name, cv.rows, cv.H, cv.L);
    HALVA_CHECK_ARG(aligned16({cv.k, cv.v, cv.pk, cv.pv}), "%s: cache pointers must be 16-byte aligned", name);
    return HALVA_OK;
}

// Rows of `width` elements moved 16 bytes at a time: row i of cache row m at base[m * ldseq + i * ldrow] (a step entry has n = 1 and
// ldseq = ldrow).  what: "", "q " or "out ".
int check_rows(const char* name, const char* what, int64_t ldrow, int64_t ldseq, int n, int64_t width) {
    HALVA_CHECK_ARG(ldrow >= width && ldrow % 8 == 0, "%s: %srow stride %lld (needs >= %lld and a multiple of 8)", name, what, (long long)ldrow,
                    (long long)width);
    HALVA_CHECK_ARG(ldseq >= (int64_t)n * ldrow && ldseq % 8 == 0, "%s: %ssequence stride %lld (needs >= n * row stride and a multiple of 8)", name,
                    what, (long long)ldseq);
    return HALVA_OK;
}

int64_t step_ws_bytes(int rows, int H, int Lpre, int L, int kc) {      // Lpre = 0: no prefix records
    if (rows <= 0 || H <= 0 || Lpre < 0 || L <= 0) return 0;
    const int64_t nrec = (int64_t)(Lpre + kc - 1) / kc + (L + kc - 1) / kc;
    return (int64_t)rows * H * nrec * (kDecD + 2) * (int64_t)sizeof(float);
}

// step = true: qkv [rows] rows, n = 1, n_new unused; otherwise qkv [rows, n] rows
int rope_append(const char* name, bool fork, bool step, void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos,
                const CacheView& cv, const int32_t* n_new, int n, int D, void* stream) {
    HALVA_CHECK_ARG(all_set({qkv, cos, sin}) && (step || n_new), "%s: null pointer", name);
    HALVA_TRY(check_cache(name, cv, D, fork, false, step ? INT_MAX : 65535));
    HALVA_CHECK_ARG(n > 0 && max_pos > 0, "%s: bad n=%d / max_pos=%d", name, n, max_pos);
    HALVA_TRY(check_rows(name, "", ldrow, ldseq, n, 3LL * cv.H * D));
    HALVA_CHECK_ARG(aligned16({qkv, cos, sin}), "%s: pointers must be 16-byte aligned", name);
    if (step)
        hipLaunchKernelGGL(rope_append_kernel<true>, dim3(cv.rows), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldrow / 8, ldseq / 8,
                           (const u32x4*)cos, (const u32x4*)sin, max_pos, cv, n_new, n);
    else
        hipLaunchKernelGGL(rope_append_kernel<false>, dim3(n, cv.rows), dim3(256), 0, (hipStream_t)stream, (u32x4*)qkv, ldrow / 8, ldseq / 8,
                           (const u32x4*)cos, (const u32x4*)sin, max_pos, cv, n_new, n);
    HALVA_CHECK_LAUNCH(name);
    return HALVA_OK;
}

// the prefix pass (only with a prefix), the own pass, the combine
template <int KC, bool VIA_TABLE, bool PREFIX>
void launch_step_attn(const void* q, int64_t ldq, const CacheView& cv, void* out, int64_t ld_out, float* ws, float scale, hipStream_t stream) {
    const int npre_cap = PREFIX ? (cv.Lpre + KC - 1) / KC : 0, nown_cap = (cv.L + KC - 1) / KC, nrec = npre_cap + nown_cap;
    float* ws_o = ws;
    float* ws_ml = ws + (int64_t)cv.rows * cv.H * nrec * kDecD;
    const float qscale = scale * 1.4426950408889634f;
    if (PREFIX)
        hipLaunchKernelGGL(prefix_partial_kernel, dim3(npre_cap, cv.H, cv.rows), dim3(64 * kDecWaves), 0, stream, (const u32x4*)q, ldq / 8, cv, nrec,
                           qscale, ws_o, ws_ml);
    hipLaunchKernelGGL((own_partial_kernel<KC, VIA_TABLE>), dim3(nown_cap, cv.H, cv.rows), dim3(64 * kDecWaves), 0, stream, (const u32x4*)q, ldq / 8,
                       cv, npre_cap, nrec, qscale, ws_o, ws_ml);
    hipLaunchKernelGGL((combine_kernel<KC, PREFIX>), dim3(cv.H, cv.rows), dim3(kDecD), 0, stream, (const float*)ws_o, (const float*)ws_ml, cv, npre_cap, nrec,
                       (bf16_t*)out, ld_out);
}

// kc: kDecodeKC, or the measurement entry's chunk (a plain cache only: the prefix pass is written for kDecodeKC)
int step_attn(const char* name, bool fork, const void* q, int64_t ldq, const CacheView& cv, void* out, int64_t ld_out, void* ws, int64_t ws_bytes,
              int D, float scale, int kc, void* stream) {
    HALVA_CHECK_ARG(all_set({q, out, ws}), "%s: null pointer", name);
    HALVA_TRY(check_cache(name, cv, D, fork, true, 65535));
    HALVA_CHECK_ARG((kc == 64 || kc == 128 || kc == 256) && (!fork || kc == kDecodeKC), "%s: chunk of %d keys (64, 128 or 256)", name, kc);
    HALVA_TRY(check_rows(name, "q ", ldq, ldq, 1, (int64_t)cv.H * D));
    HALVA_CHECK_ARG(ld_out >= (int64_t)cv.H * D, "%s: out row stride %lld < H*D", name, (long long)ld_out);
    HALVA_CHECK_ARG(aligned16({q, ws}), "%s: q / workspace pointers must be 16-byte aligned", name);
    const int64_t need = step_ws_bytes(cv.rows, cv.H, cv.Lpre, cv.L, kc);
    HALVA_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (halva_%sdecode_attn_ws_bytes)", name, (long long)ws_bytes,
                    (long long)need, fork ? "fork_" : "");
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    const hipStream_t st = (hipStream_t)stream;
    switch (kc) {
        case 64: launch_step_attn<64, false, false>(q, ldq, cv, out, ld_out, (float*)ws, scale, st); break;
        case 128: launch_step_attn<128, false, false>(q, ldq, cv, out, ld_out, (float*)ws, scale, st); break;
        default:
            if (!fork)
                launch_step_attn<256, false, false>(q, ldq, cv, out, ld_out, (float*)ws, scale, st);
            else if (cv.anc)
                launch_step_attn<256, true, true>(q, ldq, cv, out, ld_out, (float*)ws, scale, st);
            else
                launch_step_attn<256, false, true>(q, ldq, cv, out, ld_out, (float*)ws, scale, st);
    }
    HALVA_CHECK_LAUNCH(name);
    return HALVA_OK;
}

int rows_attn(const char* name, bool fork, const void* q, int64_t ldrow, int64_t ldseq, const CacheView& cv, const int32_t* n_new, void* out,
              int64_t ld_out_row, int64_t ld_out_seq, const void* ws, int64_t ws_bytes, int n, int D, float scale, void* stream) {
    HALVA_CHECK_ARG(all_set({q, n_new, out}), "%s: null pointer", name);
    HALVA_TRY(check_cache(name, cv, D, fork, true, 65535));
    HALVA_CHECK_ARG(n > 0, "%s: bad n=%d", name, n);
    HALVA_TRY(check_rows(name, "q ", ldrow, ldseq, n, (int64_t)cv.H * D));
    HALVA_TRY(check_rows(name, "out ", ld_out_row, ld_out_seq, n, (int64_t)cv.H * D));
    HALVA_CHECK_ARG(aligned16({q, out, ws}), "%s: q / out / workspace pointers must be 16-byte aligned", name);
    const int64_t need = halva_extend_attn_ws_bytes(cv.rows, n, cv.H, cv.L);
    HALVA_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (halva_extend_attn_ws_bytes)", name, (long long)ws_bytes,
                    (long long)need);
    if (scale <= 0.f) scale = 1.0f / sqrtf((float)D);
    const dim3 grid((n + kExtBM - 1) / kExtBM, cv.H, cv.rows);
    if (fork)
        hipLaunchKernelGGL(rows_attn_kernel<true>, grid, dim3(64 * kExtWaves), 0, (hipStream_t)stream, (const bf16_t*)q, ldrow, ldseq, cv, n_new,
                           (bf16_t*)out, ld_out_row, ld_out_seq, n, scale * kLog2e);
    else
        hipLaunchKernelGGL(rows_attn_kernel<false>, grid, dim3(64 * kExtWaves), 0, (hipStream_t)stream, (const bf16_t*)q, ldrow, ldseq, cv, n_new,
                           (bf16_t*)out, ld_out_row, ld_out_seq, n, scale * kLog2e);
    HALVA_CHECK_LAUNCH(name);
    return HALVA_OK;
}

}  // namespace

// ---- plain cache
extern "C" int halva_decode_attn_kc(void) { return kDecodeKC; }

extern "C" int64_t halva_decode_attn_ws_bytes(int B, int H, int Lcap) { return step_ws_bytes(B, H, 0, Lcap, kDecodeKC); }

extern "C" int64_t halva_extend_attn_ws_bytes(int B, int n, int H, int Lcap) {
    (void)B, (void)n, (void)H, (void)Lcap;
    return 0;      // one workgroup owns a row from its first key to its last: no partials
}

extern "C" int halva_decode_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, void* kcache, void* vcache,
                                        int32_t* lens, int B, int H, int D, int Lcap, void* stream) {
    return rope_append("decode_rope_append", false, true, qkv, ldqkv, ldqkv, cos, sin, max_pos, view(kcache, vcache, lens, B, H, Lcap), nullptr, 1,
                       D, stream);
}

extern "C" int halva_decode_attn(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out,
                                 int64_t ld_out, void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, void* stream) {
    return step_attn("decode_attn", false, q, ldq, view(kcache, vcache, lens, B, H, Lcap), out, ld_out, ws, ws_bytes, D, scale, kDecodeKC, stream);
}

extern "C" int halva_decode_attn_chunked(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out,
                                         int64_t ld_out, void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, int kc,
                                         void* stream) {
    return step_attn("decode_attn", false, q, ldq, view(kcache, vcache, lens, B, H, Lcap), out, ld_out, ws, ws_bytes, D, scale, kc, stream);
}

extern "C" int halva_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos, void* kcache,
                                        void* vcache, const int32_t* lens, const int32_t* n_new, int B, int n, int H, int D, int Lcap,
                                        void* stream) {
    return rope_append("extend_rope_append", false, false, qkv, ldrow, ldseq, cos, sin, max_pos, view(kcache, vcache, lens, B, H, Lcap), n_new, n, D,
                       stream);
}

extern "C" int halva_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* kcache, const void* vcache, const int32_t* lens,
                                 const int32_t* n_new, void* out, int64_t ld_out_row, int64_t ld_out_seq, void* ws, int64_t ws_bytes, int B, int n,
                                 int H, int D, int Lcap, float scale, void* stream) {
    return rows_attn("extend_attn", false, q, ldrow, ldseq, view(kcache, vcache, lens, B, H, Lcap), n_new, out, ld_out_row, ld_out_seq, ws, ws_bytes,
                     n, D, scale, stream);
}

extern "C" int halva_extend_advance(int32_t* lens, const int32_t* n_new, int B, int Lcap, void* stream) {
    HALVA_CHECK_ARG(lens && n_new, "extend_advance: null pointer");
    HALVA_CHECK_ARG(B > 0 && Lcap > 0, "extend_advance: bad B=%d / Lcap=%d", B, Lcap);
    hipLaunchKernelGGL(extend_advance_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lens, n_new, B, Lcap);
    HALVA_CHECK_LAUNCH("extend_advance");
    return HALVA_OK;
}

// ---- forks and beams
extern "C" int64_t halva_fork_decode_attn_ws_bytes(int M, int H, int Lpre, int Lown) {
    return Lpre > 0 ? step_ws_bytes(M, H, Lpre, Lown, kDecodeKC) : 0;
}

extern "C" int halva_fork_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, void* kown, void* vown, int32_t* own_lens, int M, int P, int H, int D, int Lown,
                                      void* stream) {
    return rope_append("fork_rope_append", true, true, qkv, ldqkv, ldqkv, cos, sin, max_pos, view(kown, vown, own_lens, M, H, Lown, prefix_lens, prefix_of, P),
                       nullptr, 1, D, stream);
}

extern "C" int halva_fork_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens, void* out,
                                      int64_t ld_out, void* ws, int64_t ws_bytes, int M, int P, int H, int D, int Lpre, int Lown, float scale,
                                      void* stream) {
    return step_attn("fork_decode_attn", true, q, ldq, view(kown, vown, own_lens, M, H, Lown, prefix_lens, prefix_of, P, pk, pv, Lpre), out, ld_out, ws,
                     ws_bytes, D, scale, kDecodeKC, stream);
}

extern "C" int halva_beam_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens, const int32_t* anc,
                                      void* out, int64_t ld_out, void* ws, int64_t ws_bytes, int M, int P, int H, int D, int Lpre, int Lown,
                                      float scale, void* stream) {
    HALVA_CHECK_ARG(anc, "beam_decode_attn: null pointer");
    HALVA_CHECK_ARG((uintptr_t)anc % 4 == 0, "beam_decode_attn: the ancestry table must be 4-byte aligned");
    return step_attn("beam_decode_attn", true, q, ldq, view(kown, vown, own_lens, M, H, Lown, prefix_lens, prefix_of, P, pk, pv, Lpre, anc), out, ld_out,
                     ws, ws_bytes, D, scale, kDecodeKC, stream);
}

extern "C" int halva_fork_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos,
                                             const int32_t* prefix_lens, const int32_t* prefix_of, void* kown, void* vown,
                                             const int32_t* own_lens, const int32_t* n_new, int M, int n, int P, int H, int D, int Lown,
                                             void* stream) {
    return rope_append("fork_extend_rope_append", true, false, qkv, ldrow, ldseq, cos, sin, max_pos,
                       view(kown, vown, own_lens, M, H, Lown, prefix_lens, prefix_of, P), n_new, n, D, stream);
}

extern "C" int halva_fork_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* pk, const void* pv, const int32_t* prefix_lens,
                                      const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens,
                                      const int32_t* n_new, void* out, int64_t ld_out_row, int64_t ld_out_seq, int M, int n, int P, int H, int D,
                                      int Lpre, int Lown, float scale, void* stream) {
    return rows_attn("fork_extend_attn", true, q, ldrow, ldseq, view(kown, vown, own_lens, M, H, Lown, prefix_lens, prefix_of, P, pk, pv, Lpre), n_new,
                     out, ld_out_row, ld_out_seq, nullptr, 0, n, D, scale, stream);
}

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

constexpr int kExtD = 128;                // head_dim of the decoder
static_assert(kExtD == 8 * kRopeChunks, "rope_append_row serves this head_dim");
constexpr int kExtBM = 128;               // query rows per workgroup: 4 waves x 32
constexpr int kExtBN = 64;                // keys per LDS tile
constexpr int kExtWaves = kExtBM / 32;
constexpr int kExtTileBytes = kExtBN * kExtD * 2;

// how many of the n rows of sequence b are new: n_new[b] cut to [0, n] and to the free slots of the cache
__device__ __forceinline__ int ext_rows(int past, int nn, int n, int Lcap) { return max(min(min(nn, n), Lcap - past), 0); }

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
// Attention of the new rows.  Workgroup (row block qb, head h, sequence b): 4 waves x 32 query rows i = 128 qb + 32 w + (lane & 31) against
// the keys [0, past + min(n_new, 128 (qb + 1))) in 64-key tiles, K and V double-buffered in LDS (tile_off layout, register staged: the
// loads of tile t + 1 are issued before the MFMAs of tile t and written to LDS behind them; one barrier per tile).  Per tile and wave:
// S^T = K Q^T (two 32x32 accumulators, 8 MFMAs each), per-row maximum, P = exp2(S sc - m_ref) rounded to bf16, O^T += V^T P^T (16 MFMAs, V
// read transposed with ds_read_b64_tr_b16).  A lane owns ONE query row (its other half sits 32 lanes away), so the softmax state is per lane.
//
// The exponent reference m_ref of a row moves only when the row's own tile maximum exceeds it by more than 2^64 (the first tile, which
// holds key 0, always does): the decision, the sums and their order depend on (past, i) and the row's own scores alone - never on the
// other rows of the wave, on B or on another sequence's n_new.  Key rows outside [0, past + n_new) are replaced by the nearest valid row
// when the tile is staged (Stage::load_clamped) and masked to -inf; key past + j is visible to row i iff j <= i.
// ---------------------------------------------------------------------------------------------------
// P = exp2(S sc - m) of one 32-key half: the bf16 B-operand fragments of the two 16-key slices, and the fp32 sum of the unrounded P.
// Not sdpa_fwd.h's half_exp: scalar multiply and subtract, one running sum - the order tests/extend_ref_util.py models.
__device__ __forceinline__ float ext_half_exp(const f32x16& st, float sc, float m, s16x8& p_lo, s16x8& p_hi) {
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
        const float e0 = __builtin_amdgcn_exp2f(st[r] * sc - m), e1 = __builtin_amdgcn_exp2f(st[r + 1] * sc - m);
        sum += e0 + e1;
        const unsigned w = pack_bf16x2(e0, e1);
        if (r < 8) {
            p_lo[r] = (short)(w & 0xffffu);
            p_lo[r + 1] = (short)(w >> 16);
        } else {
            p_hi[r - 8] = (short)(w & 0xffffu);
            p_hi[r - 7] = (short)(w >> 16);
        }
    }
    return sum;
}
template <bool MASK>
__device__ __forceinline__ void ext_tile(const char* kt, const char* vt, const s16x8 (&qf)[kExtD / 16], f32x16 (&oacc)[kExtD / 32], float& m_ref,
                                         float& l_run, float sc, int kv0, int len, int qpos, int lane) {
    constexpr int KS = kExtD / 16, DT = kExtD / 32;
    const int h = lane >> 5;
    f32x16 s0, s1;
#pragma unroll
    for (int r = 0; r < 16; ++r) s0[r] = 0.f, s1[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s0 = mfma32(frag_rows<kExtD>(kt, 0, ks, lane), qf[ks], s0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s1 = mfma32(frag_rows<kExtD>(kt, 32, ks, lane), qf[ks], s1);
    mask_half<MASK, true>(s0, kv0, h, len, qpos);
    mask_half<MASK, true>(s1, kv0 + 32, h, len, qpos);
    const float tmax = xhalf_max(fmaxf(half_max(s0), half_max(s1))) * sc;      // (sc > 0; -inf when the row sees no key of the tile)
    const bool move = tmax > m_ref + kRescaleAt;      // per row; the first tile (m_ref = -inf, key 0 visible) always moves
    if (__any(move)) {
        const float m_next = move ? tmax : m_ref;
        const float alpha = move ? __builtin_amdgcn_exp2f(m_ref - m_next) : 1.f;      // exp2(-inf) = 0 on the first tile, where O = l = 0
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        m_ref = m_next;
    }
    s16x8 p0a, p0b, p1a, p1b;
    const float sum0 = ext_half_exp(s0, sc, m_ref, p0a, p0b);
    const float sum1 = ext_half_exp(s1, sc, m_ref, p1a, p1b);
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) {
        const int ks = i / DT, dt = i % DT;
        oacc[dt] = mfma32(frag_cols<kExtD, false>(vt, 16 * ks, 32 * dt, lane), ks ? p0b : p0a, oacc[dt]);
    }
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) {
        const int ks = i / DT, dt = i % DT;
        oacc[dt] = mfma32(frag_cols<kExtD, false>(vt, 32 + 16 * ks, 32 * dt, lane), ks ? p1b : p1a, oacc[dt]);
    }
    l_run += sum0 + sum1;
}

__global__ __launch_bounds__(64 * kExtWaves, 2) void extend_attn_kernel(const bf16_t* __restrict__ q, int64_t ldrow, int64_t ldseq,
                                                                     const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                                                                     const int32_t* __restrict__ lens, const int32_t* __restrict__ n_new,
                                                                     bf16_t* __restrict__ out, int64_t ld_out_row, int64_t ld_out_seq, int n, int H,
                                                                     int Lcap, float sc) {
    constexpr int KS = kExtD / 16, DT = kExtD / 32, NT = 64 * kExtWaves;
    __shared__ __attribute__((aligned(16))) char smem[4 * kExtTileBytes];
    char* k_lds = smem;                           // [2][64][128]
    char* v_lds = smem + 2 * kExtTileBytes;       // [2][64][128]
    const int qb = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int past = lens[b];
    if (past < 0) return;
    const int nn = ext_rows(past, n_new[b], n, Lcap);
    const int i0 = qb * kExtBM;
    if (i0 >= nn) return;                         // (uniform over the workgroup: no barrier is skipped by part of it)
    const int len = past + nn;                    // 1 <= len <= Lcap
    const int kv_end = min(len, past + i0 + kExtBM);
    const int ntiles = (kv_end + kExtBN - 1) / kExtBN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int i = i0 + 32 * wave + (lane & 31);
    const bool valid = i < nn;
    const int qpos = past + i;
    const bool wave_live = i0 + 32 * wave < nn;   // wave-uniform
    const int wq_min = past + i0 + 32 * wave, wq_max = wq_min + 31;

    s16x8 qf[KS];
    const bf16_t* qrow = q + (int64_t)b * ldseq + (int64_t)i * ldrow + hd * kExtD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        qf[ks] = valid ? *reinterpret_cast<const s16x8*>(qrow + 16 * ks + 8 * h) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};

    const bf16_t* kp = kc + ((int64_t)b * H + hd) * Lcap * kExtD;
    const bf16_t* vp = vc + ((int64_t)b * H + hd) * Lcap * kExtD;
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m_ref = -INFINITY, l_run = 0.f;

    Stage<kExtD, kExtBN, NT> kst, vst;
    kst.load_clamped(kp, kExtD, 0, 0, len);
    vst.load_clamped(vp, kExtD, 0, 0, len);
    kst.store(k_lds);
    vst.store(v_lds);
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < ntiles; ++it) {
        const int kv0 = it * kExtBN;
        const int slot = it & 1;
        const char* kt = k_lds + slot * kExtTileBytes;
        const char* vt = v_lds + slot * kExtTileBytes;
        if (it + 1 < ntiles) {
            kst.load_clamped(kp, kExtD, 0, kv0 + kExtBN, len);
            vst.load_clamped(vp, kExtD, 0, kv0 + kExtBN, len);
        }
        if (wave_live && kv0 <= wq_max) {         // wave-uniform
            if (kv0 + kExtBN > len || kv0 + kExtBN - 1 > wq_min)
                ext_tile<true>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, len, qpos, lane);
            else
                ext_tile<false>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, len, qpos, lane);
        }
        if (it + 1 < ntiles) {
            kst.store(k_lds + (slot ^ 1) * kExtTileBytes);
            vst.store(v_lds + (slot ^ 1) * kExtTileBytes);
        }
        __syncthreads();
    }
    if (!wave_live) return;
    const float l_tot = xhalf_sum(l_run);
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    bf16_t* orow = out + (int64_t)b * ld_out_seq + (int64_t)i * ld_out_row + hd * kExtD;
    store_rows_T<kExtD>(orow, oacc, inv, valid, lane);
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

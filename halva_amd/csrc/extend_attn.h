// Causal attention of a block of new rows over a kept KV cache on MFMA - the kernel body behind rows_attn_kernel (kvcache.hip; for a
// fork, the same walk with the 64-key tiles of a shared prefix row in front).  Included inside the
// translation unit's anonymous namespace, behind sdpa_common.h.
#pragma once

constexpr int kExtD = 128;                // head_dim of the decoder
constexpr int kExtBM = 128;               // query rows per workgroup: 4 waves x 32
constexpr int kExtBN = 64;                // keys per LDS tile
constexpr int kExtWaves = kExtBM / 32;
constexpr int kExtTileBytes = kExtBN * kExtD * 2;

// how many of the n rows of sequence b are new: n_new[b] cut to [0, n] and to the free slots of the cache
__device__ __forceinline__ int ext_rows(int past, int nn, int n, int Lcap) { return max(min(min(nn, n), Lcap - past), 0); }

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

// PREFIX = false: the keys are the own cache's [0, past + n_new).  PREFIX = true: the tiles of the prefix row pk / pv [plen, 128] come
// first - every key of them visible to every row, the last one masked at plen - and the own tiles follow exactly as without a prefix
// (tile boundaries count from own key 0).  The exponent reference starts at the first tile walked, which holds a key 0 either way.  There is
// one tile loop; without a prefix the prefix pieces fold away at compile time.
template <bool PREFIX>
__device__ __forceinline__ void extend_attn_body(const bf16_t* __restrict__ qseq, int64_t ldrow, const bf16_t* __restrict__ pk,
                                                 const bf16_t* __restrict__ pv, int plen, const bf16_t* __restrict__ kp,
                                                 const bf16_t* __restrict__ vp, int past, int nn, bf16_t* __restrict__ oseq, int64_t ld_out_row,
                                                 int qb, int hd, float sc) {
    constexpr int KS = kExtD / 16, DT = kExtD / 32, NT = 64 * kExtWaves;
    __shared__ __attribute__((aligned(16))) char smem[4 * kExtTileBytes];
    char* k_lds = smem;                           // [2][64][128]
    char* v_lds = smem + 2 * kExtTileBytes;       // [2][64][128]
    const int i0 = qb * kExtBM;
    if (i0 >= nn) return;                         // (uniform over the workgroup: no barrier is skipped by part of it)
    const int len = past + nn;                    // 1 <= len <= Lcap
    const int kv_end = min(len, past + i0 + kExtBM);
    const int npre = PREFIX ? (plen + kExtBN - 1) / kExtBN : 0;
    const int ntiles = npre + (kv_end + kExtBN - 1) / kExtBN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int i = i0 + 32 * wave + (lane & 31);
    const bool valid = i < nn;
    const int qpos = past + i;
    const bool wave_live = i0 + 32 * wave < nn;   // wave-uniform
    const int wq_min = past + i0 + 32 * wave, wq_max = wq_min + 31;

    s16x8 qf[KS];
    const bf16_t* qrow = qseq + (int64_t)i * ldrow + hd * kExtD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
        qf[ks] = valid ? *reinterpret_cast<const s16x8*>(qrow + 16 * ks + 8 * h) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};

    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m_ref = -INFINITY, l_run = 0.f;

    Stage<kExtD, kExtBN, NT> kst, vst;
    auto fetch = [&](int it) {                    // tile `it` of the walk into the staging registers
        const bool pre = PREFIX && it < npre;     // workgroup-uniform
        const int kv0 = (pre ? it : it - npre) * kExtBN, lim = pre ? plen : len;
        kst.load_clamped(pre ? pk : kp, kExtD, 0, kv0, lim);
        vst.load_clamped(pre ? pv : vp, kExtD, 0, kv0, lim);
    };
    fetch(0);
    kst.store(k_lds);
    vst.store(v_lds);
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < ntiles; ++it) {
        const int slot = it & 1;
        const char* kt = k_lds + slot * kExtTileBytes;
        const char* vt = v_lds + slot * kExtTileBytes;
        if (it + 1 < ntiles) fetch(it + 1);
        // inside the prefix every key below plen is visible to every row (no causal cut: qp beyond any key); behind it, the own walk
        const bool pre = PREFIX && it < npre;
        const int kv0 = (pre ? it : it - npre) * kExtBN, lim = pre ? plen : len, qp = pre ? 0x7fffffff : qpos;
        const bool live = wave_live && (pre || kv0 <= wq_max);                                     // wave-uniform
        const bool masked = kv0 + kExtBN > lim || (!pre && kv0 + kExtBN - 1 > wq_min);
        if (live) {
            if (masked)
                ext_tile<true>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, lim, qp, lane);
            else
                ext_tile<false>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, lim, qp, lane);
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
    store_rows_T<kExtD>(oseq + (int64_t)i * ld_out_row + hd * kExtD, oacc, inv, valid, lane);
}

// A fragment of the sdpa.hip translation unit, not compiled alone: included there inside its anonymous namespace, behind common.h and
// the sdpa_*.h listed before it.  Holds sdpa_fwd_kernel, the two-waves-per-SIMD forward.
// ===================================================================================================
// forward
// ===================================================================================================
// 8 waves x 32 query rows (two waves per SIMD), 64-key K/V tiles double-buffered in LDS, register staged (the loads of
// tile t+1 are issued before the MFMAs of tile t and written to LDS after them; one barrier per tile).
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The tile body is two straight-line blocks in which the wave's own vector work rides in the shadow of its own MFMAs
// (the interleave is written out in the source and pinned with scheduling fences):
//   A:  S0 = K[0:32] Q^T ; S1 = K[32:64] Q^T  ||  max(S0), P0 = exp2(S0*sc - m_ref), sum      then max(S1)
//   B:  O^T += V^T[:, 0:32] P0^T              ||  P1 = exp2(S1*sc - m_ref), sum ;  O^T += V^T[:, 32:64] P1^T
// The exponent reference m_ref is only moved when a row's maximum exceeds it by more than 2^kRescaleAt (the first tile
// always does): that rare path sits between A and B, rescales O / l and recomputes P0 from the untouched S0; O is not
// multiplied every tile.  Cross-half reductions use v_permlane32_swap (no LDS round trip), the exp2 argument / row sums use
// packed fp32 ops, full tiles are fetched by pointer bumps (no per-tile 64-bit address arithmetic).
// Variants built and measured on MI355X at S=8,T=2048,H=32 (numbers and PMC breakdown in DESIGN.md), none faster: 4 waves x
// 64 rows at one wave per SIMD; a ping-pong of GEMM-only / softmax-only phases between the two waves of a SIMD (two barriers
// per tile; the later-dispatched wave of each SIMD is starved whatever s_setprio says); the same with the two blocks in
// rotated order and one barrier; 4-wave workgroups at two per CU.
// ---------------------------------------------------------------------------------------------------
// One 2-element slice of P = exp2(S * sc - m): elements r, r+1 of the accumulator -> bf16 pair in the B-operand fragment
__device__ __forceinline__ void exp_pair(const f32x16& st, int r, f32x2 sc2, f32x2 ms2, f32x2& ps, s16x8& p_lo, s16x8& p_hi) {
    f32x2 x = {st[r], st[r + 1]};
    x = x * sc2 + ms2;
    const f32x2 e = {__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
    ps = ps + e;
    const unsigned w = pack_bf16x2(e[0], e[1]);
    if (r < 8) {
        p_lo[r] = (short)(w & 0xffffu);
        p_lo[r + 1] = (short)(w >> 16);
    } else {
        p_hi[r - 8] = (short)(w & 0xffffu);
        p_hi[r - 7] = (short)(w >> 16);
    }
}
__device__ __forceinline__ float half_exp(const f32x16& st, float sc, float m_sub, s16x8& p_lo, s16x8& p_hi) {
    const f32x2 sc2 = {sc, sc}, ms2 = {-m_sub, -m_sub};
    f32x2 ps = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; r += 2) exp_pair(st, r, sc2, ms2, ps, p_lo, p_hi);
    return ps[0] + ps[1];
}

// scheduling fence that only LDS reads and scalar ops may cross: pins the MFMA / VALU interleave written in the source
#define FENCE() __builtin_amdgcn_sched_barrier(0x100 | 0x004)

#ifdef HALVA_STAMP
#define STAMP_ARGS , unsigned long long (&stamp_acc)[6], unsigned long long& stamp_prev
#define STAMP_PASS , stamp_acc, stamp_prev
#else
#define STAMP_ARGS
#define STAMP_PASS
#endif
// The scale stays in fp32 and is applied after the product (a multiply-add in front of every exponential), as flash-attn does.  Folding it
// and -m_ref into the MFMA chain (Q * scale * log2 e rounded to bf16 once per row block, the chains started from -m_ref) measured -1.8 % and
// was rejected for its numerics: 2.1e-2 against the 1e-2 bound of test_sdpa_exponent_reference_moves_when_later_keys_dominate
// ("Retired kernel variants").
template <int D, bool CAUSAL, bool MASK, bool SLOW_TR>
__device__ __forceinline__ void fwd_tile(const char* kt, const char* vt, const s16x8 (&qf)[D / 16], f32x16 (&oacc)[D / 32],
                                          float& m_ref, float& l_run, float sc, int kv0, int len, int ql, int lane STAMP_ARGS) {
    constexpr int KS = D / 16, DT = D / 32;
    static_assert(KS == 8 || KS == 4, "head_dim 128 or 64");
    constexpr int PPS = 8 / KS;            // exp pairs handled per S1 MFMA (1 for D=128, 2 for D=64)
    const int h = lane >> 5;
    f32x16 s0, s1;
    s16x8 p0a, p0b, p1a, p1b;
    const f32x2 sc2 = {sc, sc};
    // ---------------- block A: S0 bare, then S1 with softmax(S0) in its shadow ----------------
#pragma unroll
    for (int r = 0; r < 16; ++r) s0[r] = 0.f, s1[r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) s0 = mfma32(frag_rows<D>(kt, 0, ks, lane), qf[ks], s0);
    mask_half<MASK, CAUSAL>(s0, kv0, h, len, ql);
    STAMP(1);
    const float msub_a = (m_ref == -INFINITY) ? 0.f : m_ref;
    const f32x2 ms2a = {-msub_a, -msub_a};
    f32x2 ps0 = {0.f, 0.f};
    float mx0a = -INFINITY, mx0b = -INFINITY;
    FENCE();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        s1 = mfma32(frag_rows<D>(kt, 32, ks, lane), qf[ks], s1);
        FENCE();
#pragma unroll
        for (int q = 0; q < PPS; ++q) {
            const int r = 2 * (ks * PPS + q);
            exp_pair(s0, r, sc2, ms2a, ps0, p0a, p0b);
            if (q & 1 || PPS == 1 ? (ks & 1) : false) mx0b = fmaxf(fmaxf(mx0b, s0[r]), s0[r + 1]);
            else mx0a = fmaxf(fmaxf(mx0a, s0[r]), s0[r + 1]);
        }
        FENCE();
    }
    mask_half<MASK, CAUSAL>(s1, kv0 + 32, h, len, ql);
    // P0 and its row sums are dead on the rare path below (which recomputes them), so LLVM sinks the whole exponential block out of
    // the S1 chain into the common successor - behind the chain, where no MFMA covers it.  Pin the values where they are produced.
    asm volatile("" : "+v"(p0a), "+v"(p0b), "+v"(ps0));
    float sum0 = ps0[0] + ps0[1];
    const float tmax = xhalf_max(fmaxf(fmaxf(mx0a, mx0b), half_max(s1))) * sc;
    STAMP(2);
    // ---------------- rare: move the exponent reference ----------------
    if (__any(tmax > m_ref + kRescaleAt)) {
        const float m_next = fmaxf(m_ref, tmax);
        const float alpha = (m_next == -INFINITY) ? 1.f : __builtin_amdgcn_exp2f(m_ref - m_next);
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        m_ref = m_next;
        sum0 = half_exp(s0, sc, (m_ref == -INFINITY) ? 0.f : m_ref, p0a, p0b);
    }
    STAMP(3);
    // ---------------- block B: PV(P0) with softmax(S1) in its shadow, then PV(P1) bare ----------------
    const float msub_b = (m_ref == -INFINITY) ? 0.f : m_ref;
    const f32x2 ms2b = {-msub_b, -msub_b};
    f32x2 ps1 = {0.f, 0.f};
    FENCE();
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) {
        const int ks = i / DT, dt = i % DT;
        oacc[dt] = mfma32(frag_cols<D, SLOW_TR>(vt, 16 * ks, 32 * dt, lane), ks ? p0b : p0a, oacc[dt]);
        FENCE();
#pragma unroll
        for (int q = 0; q < 8 / (2 * DT); ++q) {
            exp_pair(s1, 2 * (i * (8 / (2 * DT)) + q), sc2, ms2b, ps1, p1a, p1b);
        }
        FENCE();
    }
#pragma unroll
    for (int i = 0; i < 2 * DT; ++i) {
        const int ks = i / DT, dt = i % DT;
        oacc[dt] = mfma32(frag_cols<D, SLOW_TR>(vt, 32 + 16 * ks, 32 * dt, lane), ks ? p1b : p1a, oacc[dt]);
    }
    l_run += sum0 + ps1[0] + ps1[1];
    STAMP(4);
}

// Geometry of one 256-row block of one (sequence, head) for this lane / wave.
struct FwdGeom {
    int g0, gq, ql, ntiles, skip_lo, skip_hi, wq_min, wq_max;
    bool q_in_T, q_valid;
    __device__ __forceinline__ int first_tile() const { return skip_lo > 0 ? 0 : skip_hi; }      // == ntiles when the block has no tile
};
template <bool CAUSAL>
__device__ __forceinline__ FwdGeom fwd_geom(const SdpaParams& p, int qb, int start, int len, const Branch& br, int wave, int lane) {
    constexpr int BN = 64, BM = 256;
    FwdGeom g;
    g.g0 = qb * BM;
    g.gq = g.g0 + 32 * wave + (lane & 31);
    g.ql = g.gq - start;
    g.q_in_T = g.gq < p.T;
    g.q_valid = g.q_in_T && g.ql >= 0 && g.ql < len;
    int kv_end = len;
    if (CAUSAL) kv_end = min(len, g.g0 + BM - start);
    g.ntiles = kv_end > 0 ? (kv_end + BN - 1) / BN : 0;
    g.wq_min = g.g0 + 32 * wave - start;
    g.wq_max = g.wq_min + 31;
    // A row block wholly in branch B does not even stage the key tiles that lie wholly inside [a, b): the tile range is walked
    // in (up to) two segments [0, skip_lo) and [skip_hi, ntiles), each a plain double-buffered loop (one barrier per tile).
    g.skip_lo = g.skip_hi = g.ntiles;
    if (g.g0 - start >= br.b) {
        g.skip_lo = min(g.ntiles, (br.a + BN - 1) / BN);
        g.skip_hi = max(g.skip_lo, min(g.ntiles, br.b / BN));
    }
    return g;
}

// One row block.  `qf` (the Q fragments) belongs to the caller so that a block can fetch its SUCCESSOR's operands: when the tile loop
// of a block has passed its last barrier the LDS ring is free and the Q registers are dead, so the next block's Q rows and first K/V
// tile are requested THEN - in front of this block's store tail - instead of in the next block's prologue (measured per block,
// s_memtime: 7 000-8 800 cycles from the Q request to the first tile in LDS, 3 000-4 700 for the store tail, against ~4 300 per tile).
//   qb_next    : the block this workgroup runs next (-1: none)          prefetched : this block's operands were requested by its predecessor
//   first_in_wg: nothing of this workgroup has touched the LDS ring yet
template <int D, bool CAUSAL, bool SLOW_TR>
__device__ __forceinline__ void sdpa_fwd_block(const SdpaParams& p, char* smem, int s, int hd, int qb, int qb_next, bool prefetched,
                                               bool first_in_wg, s16x8 (&qf)[D / 16], int start, int len, const Branch br) {
    constexpr int NW = 8, BN = 64, KS = D / 16, DT = D / 32, NT = 64 * NW;
    constexpr int TILE_BYTES = BN * D * 2;
    char* k_lds = smem;                    // [2][BN][D]
    char* v_lds = smem + 2 * TILE_BYTES;   // [2][BN][D]

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int64_t seq_row0 = (int64_t)s * p.T;
    const FwdGeom g = fwd_geom<CAUSAL>(p, qb, start, len, br, wave, lane);
    const int gq = g.gq, ql = g.ql, ntiles = g.ntiles, skip_lo = g.skip_lo, skip_hi = g.skip_hi, wq_min = g.wq_min, wq_max = g.wq_max;
    const bool q_in_T = g.q_in_T, q_valid = g.q_valid;

    const bf16_t* kp = p.k + hd * D;
    const bf16_t* vp = p.v + hd * D;
    bf16_t* orow = p.o + (seq_row0 + gq) * p.ld_o + hd * D;
    // K/V tiles arrive by LDS-DMA (no staging registers, no ds_write pass); the slow-transpose debug build keeps register staging
    constexpr bool DMA = !SLOW_TR;
    const int wave_u = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // used for the DMA addresses only
    const int64_t krow0 = seq_row0 + start;
    auto request_q = [&](const FwdGeom& gg) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (gg.q_valid)
                qf[ks] = *reinterpret_cast<const s16x8*>(p.q + hd * D + (seq_row0 + gg.gq) * p.ld_qkv + 16 * ks + 8 * h);
            else
                qf[ks] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    auto request_first_tile = [&](const FwdGeom& gg) {      // DMA builds only; the caller vouches that nobody reads slot 0 any more
        const int t = gg.first_tile();
        if (t < gg.ntiles) {
            stage_tile_dma<D, NW>(k_lds, kp, p.ld_qkv, krow0, t * BN, len, wave_u, lane);
            stage_tile_dma<D, NW>(v_lds, vp, p.ld_qkv, krow0, t * BN, len, wave_u, lane);
        }
    };
    auto prefetch_next = [&]() {
        if (DMA && qb_next >= 0) {
            const FwdGeom gn = fwd_geom<CAUSAL>(p, qb_next, start, len, br, wave, lane);
            request_q(gn);
            request_first_tile(gn);
        }
    };
    const bool pre = DMA && prefetched;

    if (ntiles == 0) {
        if (q_in_T) {
            store_rows_zero<D>(orow, lane);
            if (h == 0 && p.lse) p.lse[((int64_t)s * p.H + hd) * p.T + gq] = 0.f;
        }
        if (!pre && !first_in_wg) __syncthreads();      // (a predecessor's readers; a prefetching predecessor has passed its last barrier)
        prefetch_next();
        return;
    }
    if (!pre) request_q(g);

    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
    float m_ref = -INFINITY, l_run = 0.f;
    const float sc = p.scale * kLog2e;
    const bool wave_in_b = wq_min >= br.b;             // wave-uniform (br.b is a multiple of 64, strips are 32 rows)
    Stage<D, BN, NT> kst, vst;
    TileDma<D, NW> kdma, vdma;
#ifdef HALVA_STAMP
    unsigned long long stamp_acc[6] = {0, 0, 0, 0, 0, 0}, stamp_prev, blk_t[4];
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
    blk_t[0] = stamp_prev;      // (Q requested, scalars known)
    blk_t[1] = 0;
#endif
    bool first_seg = true;
#pragma unroll 1
    for (int seg = 0; seg < 2; ++seg) {
        const int t0 = seg ? skip_hi : 0, t1 = seg ? ntiles : skip_lo;
        if (t0 >= t1) continue;
        const bool staged = pre && first_seg;      // tile t0 was requested by the previous block
        if (!staged && !(first_in_wg && first_seg)) __syncthreads();      // earlier readers of the LDS slots (previous segment / row block) are done
        if (DMA) {
            if (!staged) {
                stage_tile_dma<D, NW>(k_lds, kp, p.ld_qkv, krow0, t0 * BN, len, wave_u, lane);
                stage_tile_dma<D, NW>(v_lds, vp, p.ld_qkv, krow0, t0 * BN, len, wave_u, lane);
            }
            kdma.init(kp, p.ld_qkv, krow0, (t0 + 1) * BN, wave_u, lane);
            vdma.init(vp, p.ld_qkv, krow0, (t0 + 1) * BN, wave_u, lane);
            stage_tile_dma_wait();
        } else {
            kst.load_clamped(kp, p.ld_qkv, krow0, t0 * BN, len);
            vst.load_clamped(vp, p.ld_qkv, krow0, t0 * BN, len);
            kst.store(k_lds);
            vst.store(v_lds);
        }
        first_seg = false;
        __syncthreads();
#ifdef HALVA_STAMP
        if (blk_t[1] == 0) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[1])::"memory");      // first tile in LDS
#endif
#pragma unroll 1
        for (int it = t0; it < t1; ++it) {
            const int kv0 = it * BN;
            const int slot = (it - t0) & 1;
            const char* kt = k_lds + slot * TILE_BYTES;
            const char* vt = v_lds + slot * TILE_BYTES;
            if (it + 1 < t1) {
                if (!DMA) {
                    kst.load_clamped(kp, p.ld_qkv, krow0, kv0 + BN, len);
                    vst.load_clamped(vp, p.ld_qkv, krow0, kv0 + BN, len);
                } else if (kv0 + 2 * BN <= len) {
                    kdma.issue_and_advance(k_lds + (slot ^ 1) * TILE_BYTES, p.ld_qkv, wave_u);
                    vdma.issue_and_advance(v_lds + (slot ^ 1) * TILE_BYTES, p.ld_qkv, wave_u);
                } else {      // the sequence's last, partial tile
                    stage_tile_dma<D, NW>(k_lds + (slot ^ 1) * TILE_BYTES, kp, p.ld_qkv, krow0, kv0 + BN, len, wave_u, lane);
                    stage_tile_dma<D, NW>(v_lds + (slot ^ 1) * TILE_BYTES, vp, p.ld_qkv, krow0, kv0 + BN, len, wave_u, lane);
                }
            }
            STAMP(0);
            const bool hidden = wave_in_b && kv0 >= br.a && kv0 < br.b;                       // tile wholly inside [a, b)
            const int len_t = (wave_in_b && kv0 < br.a && kv0 + BN > br.a) ? br.a : len;       // tile cut at a
            if ((!CAUSAL || kv0 <= wq_max) && !hidden) {
                if ((kv0 + BN > len_t) || (CAUSAL && kv0 + BN - 1 > wq_min))      // wave-uniform: boundary tiles only
                    fwd_tile<D, CAUSAL, true, SLOW_TR>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, len_t, ql, lane STAMP_PASS);
                else
                    fwd_tile<D, CAUSAL, false, SLOW_TR>(kt, vt, qf, oacc, m_ref, l_run, sc, kv0, len_t, ql, lane STAMP_PASS);
            }
            if (DMA) {
                stage_tile_dma_wait();
            } else if (it + 1 < t1) {
                kst.store(k_lds + (slot ^ 1) * TILE_BYTES);
                vst.store(v_lds + (slot ^ 1) * TILE_BYTES);
            }
            __syncthreads();
            STAMP(5);
        }
    }
#ifdef HALVA_STAMP
    if (p.dbg && lane == 0 && s == 0 && hd == 0 && qb == p.nblk - 1) {
        for (int i = 0; i < 6; ++i) p.dbg[wave * 8 + i] = stamp_acc[i];
        p.dbg[wave * 8 + 6] = ntiles;
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[2])::"memory");      // tile loop done
#endif
    // every wave has passed the last tile's barrier: the ring is free and Q is dead - fetch the next block's operands in front of the stores
    prefetch_next();
    const float l_tot = xhalf_sum(l_run);
    const float inv = (q_valid && l_tot > 0.f) ? 1.f / l_tot : 0.f;
    if (q_in_T) {
        store_rows_T<D>(orow, oacc, inv, true, lane);
        if (h == 0 && p.lse) p.lse[((int64_t)s * p.H + hd) * p.T + gq] = q_valid ? (m_ref + log2f(l_tot)) * kLn2 : 0.f;
    }
#ifdef HALVA_STAMP
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[3])::"memory");      // rows stored
    if (p.dbg && lane == 0 && s == 0 && hd == 0)
        for (int i = 0; i < 4; ++i) p.dbg[2048 + (qb * 8 + wave) * 4 + i] = blk_t[i];
#endif
}

// Under the causal mask row block b needs (b+1) units of work; one workgroup takes blocks b and nblk-1-b so every
// workgroup does the same (nblk+1) units and the grid has no heavy tail.
template <int D, bool CAUSAL, bool SLOW_TR>
__global__ __launch_bounds__(512) void sdpa_fwd_kernel(const SdpaParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int s, hd, b;
    map_block(blockIdx.x, CAUSAL ? (p.nblk + 1) / 2 : p.nblk, p.H, p.npairs, false, s, hd, b);
    // the sequence's geometry is read once per workgroup
    const int start = p.seq_start ? p.seq_start[s] : 0;
    const int len = p.seq_len ? p.seq_len[s] : p.T;
    const Branch br = load_branch(p, s);
    s16x8 qf[D / 16];
    WG_CLOCK_BEGIN();
    if (CAUSAL) {
        int first, second;
        paired_blocks(p.nblk, start, br, b, first, second);
        if (second == first) second = -1;
        if (p.repair) {
            // sdpa_fwd3 fixes a row block's exponent reference on the row's first visible keys and repeats the block a bounded number of times when
            // later keys outgrow it (gen_fwd3_loop.py: MAX_REDO); a FINITE row whose maximum lies further out than that leaves it with l = inf, i.e.
            // lse = inf and NaN for output.  This kernel tracks a running maximum and has no such bound (as flash-attn): launched behind every
            // sdpa_fwd3 launch, a workgroup looks at the lse of its two blocks' valid rows and recomputes a block only if one of them is not finite
            // (NaN / inf inputs are recomputed to the same NaN / inf).  Ordinary activations: 2 x 256 loads and an exit.
            bool did = false;
            for (int k = 0; k < 2; ++k) {
                const int qb = k ? second : first;
                if (qb < 0) continue;
                const int gq = qb * 256 + (threadIdx.x & 255), ql = gq - start;
                const bool bad = threadIdx.x < 256 && gq < p.T && ql >= 0 && ql < len && !__builtin_isfinite(p.lse[((int64_t)s * p.H + hd) * p.T + gq]);
                if (!__syncthreads_or(bad)) continue;
                sdpa_fwd_block<D, CAUSAL, SLOW_TR>(p, smem, s, hd, qb, -1, false, !did, qf, start, len, br);
                did = true;
            }
            return;
        }
        sdpa_fwd_block<D, CAUSAL, SLOW_TR>(p, smem, s, hd, first, second, false, true, qf, start, len, br);
        if (second >= 0) sdpa_fwd_block<D, CAUSAL, SLOW_TR>(p, smem, s, hd, second, -1, true, false, qf, start, len, br);
    } else {
        sdpa_fwd_block<D, CAUSAL, SLOW_TR>(p, smem, s, hd, b, -1, false, true, qf, start, len, br);
    }
    WG_CLOCK_END(p.dbg, 0);
}

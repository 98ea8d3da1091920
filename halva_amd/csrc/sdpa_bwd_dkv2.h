// A fragment of the sdpa.hip translation unit, not compiled alone: included there inside its anonymous namespace, behind common.h and
// the sdpa_*.h listed before it.  Holds sdpa_bwd_dkv2_kernel, the two-role dK / dV.
// ===================================================================================================
// backward, part 2: dK, dV, two-role form.  A workgroup owns 128 keys and streams 64-row tiles of Q and dO (one dual-use LDS image
// each) from the diagonal to the end of the sequence.  Keeping K, V, dK and dV of a 32-key strip in one wave needs 362 registers,
// i.e. one wave per SIMD; that form (round 1) was replaced by the split below and is gone.

// The two waves of a SIMD split that state: wave w (0..3, "V side") owns K fragments and dV of key strip w, wave w+4
// ("K side") owns V fragments and dK of the SAME strip, so both fit the 256-register budget of two waves per SIMD and one's
// MFMAs run beside the other's vector work.  Per 32-row sub-tile:
//   V side:  S = Q K^T  ->  P = exp2(S*sc - lse) (masks applied here)  ->  P to LDS (bf16, accumulator layout)  ->  dV^T += dO^T P
//   K side:  dP = dO V^T  ->  P from LDS  ->  dZ = P o (dP - delta)  ->  dK^T += Q^T dZ
// With a dS workspace (SdpaParams::ds_ws) the K side also stores dZ = dS - which it holds as packed bf16 anyway, as the B operand of
// dK^T += Q^T dZ - for the dQ kernel that follows (sdpa_bwd_dq2): four 1-KiB stores per step and wave, each lane's 16 bytes next to its
// neighbour's.  dS is then formed ONCE in the whole backward (5 matrix products per (query, key) tile pair instead of 7).
// The K side runs one staged step behind the V side, so the workgroup barrier of the step (needed for the Q/dO ring anyway) is the
// only synchronisation; the Q/dO ring has 3 slots (steps t-1, t and the one being fetched), P has 2 (by step parity).
// ---------------------------------------------------------------------------------------------------
// Geometry of one 128-key block for this lane (key = lane % 32 of strip `strip`).
struct DkvGeom {
    int gk, kl, kblk_min, q_begin, q_stop, ntiles;
    bool k_in_T, k_valid;
};
template <bool CAUSAL>
__device__ __forceinline__ DkvGeom dkv_geom(const SdpaParams& p, int kb, int strip, int start, int len, const Branch& br, int lane) {
    constexpr int BQ = 64;
    DkvGeom g;
    g.gk = kb * 128 + 32 * strip + (lane & 31);
    g.kl = g.gk - start;
    g.k_in_T = g.gk < p.T;
    g.k_valid = g.k_in_T && g.kl >= 0 && g.kl < len;
    g.kblk_min = kb * 128 - start;
    g.q_begin = 0;
    if (CAUSAL) g.q_begin = max(0, g.kblk_min) / BQ * BQ;
    const bool block_has_keys = (g.kblk_min < len) && (g.kblk_min + 128 > 0);
    g.q_stop = (g.kblk_min >= br.a && g.kblk_min + 127 < br.b) ? min(len, br.b) : len;
    g.ntiles = (block_has_keys && g.q_stop > g.q_begin) ? (g.q_stop - g.q_begin + BQ - 1) / BQ : 0;
    return g;
}

// `sf` (the stationary K or V fragments) and `st` (the row statistics in flight) belong to the caller so that a key block can fetch its
// SUCCESSOR's operands: once the step loop has passed its last barrier the Q/dO ring is free and the stationary registers are dead, so
// the next block's K/V rows, first Q/dO tile and first statistics are requested then - in front of this block's store tail - instead
// of in the next block's prologue (measured per block, s_memtime: 10 000-12 000 cycles from entry to the first step, of which three
// memory round trips one behind the other; a step is ~3 850).
//   kb_next: the key block this workgroup runs next (-1: none)      prefetched: this block's operands were requested by its predecessor
// A row constant as the initial accumulator (cdna_hip_programming.md, attention backward), on the K side: the
// dP = dO V^T chain starts from -delta (exact: the same fp32 additions in another order), so dZ = P * dP' needs no subtraction - 32
// vector instructions fewer per K-side wave and step, and the 32 registers that held delta during the vector work are free after each
// chain's first MFMA.  The V side's analogue (S chain from -lse, K pre-multiplied by scale * log2 e so that P = exp2(S')) is NOT
// taken: it needs a second bf16 rounding of an operand, which moves P by up to ~1 % (the forward tried it: see fwd_tile).
template <int D, bool CAUSAL, bool SLOW_TR, int ROLE>
__device__ __forceinline__ void sdpa_bwd_dkv2_block(const SdpaParams& p, char* smem, int s, int hd, int kb, int kb_next, bool prefetched,
                                                    int strip, int start, int len, const Branch br, s16x8 (&sf)[D / 16], float (&st)[2]) {
    constexpr int BQ = 64, SUB = 2, KS = D / 16, DT = D / 32;
    constexpr int TILE_BYTES = BQ * D * 2;
    char* q_lds = smem;                                    // [3][BQ][D]
    char* do_lds = smem + 3 * TILE_BYTES;                  // [3][BQ][D]
    float* lse_lds = reinterpret_cast<float*>(smem + 6 * TILE_BYTES);   // [3][BQ]
    float* dlt_lds = lse_lds + 3 * BQ;                                  // [3][BQ]
    char* p_lds = reinterpret_cast<char*>(dlt_lds + 3 * BQ);            // [2 parity][4 strips][SUB][64 lanes][2][16 B]

    const int lane = threadIdx.x & 63, h = lane >> 5;
#ifdef HALVA_STAMP
    unsigned long long blk_t[8];
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[0])::"memory");
    blk_t[5] = blk_t[6] = blk_t[7] = blk_t[0];
#endif
    const int64_t seq_row0 = (int64_t)s * p.T;
    const DkvGeom g = dkv_geom<CAUSAL>(p, kb, strip, start, len, br, lane);
    const int gk = g.gk, kl = g.kl, kblk_min = g.kblk_min, q_begin = g.q_begin, ntiles = g.ntiles;
    const bool k_in_T = g.k_in_T, k_valid = g.k_valid;
    bf16_t* outrow = (ROLE ? p.dk : p.dv) + (seq_row0 + gk) * p.ld_qkv + hd * D;
    const bool key_hidden = kl >= br.a && kl < br.b;

    const bf16_t* qp = p.q + hd * D;
    const bf16_t* dop = p.d_o + hd * D;
    const int64_t qrow0 = seq_row0 + start;
    const float* lse_g = p.lse + ((int64_t)s * p.H + hd) * p.T + start;
    const float* dlt_g = p.delta + ((int64_t)s * p.H + hd) * p.T + start;
    float& st_lse = st[0];
    float& st_dlt = st[1];
    // the row statistics of a tile are fetched by ONE wave that requests no tiles (K side, strip 0): on a tile-requesting wave the wait
    // for these two loads in the prologue also waited for the stationary operand and held back the first tile request - a second
    // memory round trip in front of the loop
    const bool stats_wave = ROLE == 1 && strip == 0;
    auto load_stats = [&](int q0) {
        if (stats_wave) {
            const int ql = min(q0 + lane, len - 1);
            st_lse = lse_g[ql];
            st_dlt = dlt_g[ql];
        }
    };
    auto store_stats = [&](int buf) {
        if (stats_wave) {
            lse_lds[buf * BQ + lane] = st_lse * kLog2e;
            dlt_lds[buf * BQ + lane] = -st_dlt;      // stored NEGATED: the values are the initial accumulator of the K side's dP chain (see below)
        }
    };
    // The four V-side waves fetch the tiles: they finish a step's arithmetic ahead of their K-side partners (measured against
    // all eight waves taking a share: -0.5 %).
    constexpr int NDMA = 4;
    constexpr bool dma_wave = ROLE == 0;
    const int dma_id = strip;
    // this wave's stationary operand: K fragments (V side) or V fragments (K side)
    auto request_stationary = [&](const DkvGeom& gg) {
        const bf16_t* stat = (ROLE ? p.v : p.k) + (seq_row0 + gg.gk) * p.ld_qkv + hd * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            sf[ks] = gg.k_valid ? *reinterpret_cast<const s16x8*>(stat + 16 * ks + 8 * h) : s16x8{0, 0, 0, 0, 0, 0, 0, 0};
    };
    auto request_first_tile = [&](const DkvGeom& gg) {      // the caller vouches that nobody reads ring slot 0 any more
        if (dma_wave && gg.ntiles > 0) {
            stage_tile_dma<D, NDMA>(q_lds, qp, p.ld_qkv, qrow0, gg.q_begin, len, dma_id, lane);
            stage_tile_dma<D, NDMA>(do_lds, dop, p.ld_do, qrow0, gg.q_begin, len, dma_id, lane);
        }
    };
    auto prefetch_next = [&]() {
        if (kb_next >= 0) {
            const DkvGeom gn = dkv_geom<CAUSAL>(p, kb_next, strip, start, len, br, lane);
            if (gn.ntiles > 0) {
                request_stationary(gn);
                load_stats(gn.q_begin);
            }
            request_first_tile(gn);
        }
    };

    if (ntiles == 0) {
        if (k_in_T) store_rows_zero<D>(outrow, lane);
        prefetch_next();      // (no step loop ran here, and a predecessor - if any - has passed its last barrier: the rings are free)
        return;
    }
    if (!prefetched) {
        request_stationary(g);
        load_stats(q_begin);
    }
#ifdef HALVA_STAMP
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[5])::"memory");      // scalars known, stationary loads issued
#endif
    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
    const float sc = p.scale * kLog2e;
    const int wk_min = kblk_min + 32 * strip;
    const bool wave_has_pad_keys = __any(!k_valid);

    if (!prefetched) request_first_tile(g);      // (not prefetched = first block of the workgroup: nobody is reading the rings)
    TileDma<D, NDMA> qdma, dodma;
    if (dma_wave) {
        qdma.init(qp, p.ld_qkv, qrow0, q_begin + BQ, dma_id, lane);      // stand on tile 1
        dodma.init(dop, p.ld_do, qrow0, q_begin + BQ, dma_id, lane);
    }
#ifdef HALVA_STAMP
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[7])::"memory");      // first tile requested
#endif
    store_stats(0);
    stage_tile_dma_wait();
    __syncthreads();

#ifdef HALVA_STAMP
    unsigned long long stamp_acc[6] = {0, 0, 0, 0, 0, 0}, stamp_prev;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
#endif
#ifdef HALVA_STAMP
    blk_t[4] = stamp_prev;            // loop start
#endif
    int slot = ROLE ? 2 : 0;          // ring slot of step t - ROLE (the K side's first pass, t = 0, is idle)
    int slot_next = 1;                // ring slot the fetch of step t + 1 goes to
#pragma unroll 1
    for (int t = 0; t <= ntiles; ++t) {
        STAMP(5);
        if (t + 1 < ntiles) {
            const int qn = q_begin + (t + 1) * BQ;
            load_stats(qn);
            // The V side requests the whole tile: its waves finish a step's arithmetic some 500 cycles before the K side's, and a request
            // costs its wave about 100 cycles wherever it is placed (tried: between the MFMAs of the first block - no cheaper).
            if (dma_wave) {
                if (qn + BQ <= len) {
                    qdma.issue_and_advance(q_lds + slot_next * TILE_BYTES, p.ld_qkv, dma_id);
                    dodma.issue_and_advance(do_lds + slot_next * TILE_BYTES, p.ld_do, dma_id);
                } else {      // the sequence's last, partial tile
                    stage_tile_dma<D, NDMA>(q_lds + slot_next * TILE_BYTES, qp, p.ld_qkv, qrow0, qn, len, dma_id, lane);
                    stage_tile_dma<D, NDMA>(do_lds + slot_next * TILE_BYTES, dop, p.ld_do, qrow0, qn, len, dma_id, lane);
                }
            }
        }
        STAMP(0);
        const int tt = t - ROLE;                           // the step this wave works on
        if (tt >= 0 && tt < ntiles) {
            const int qt0 = q_begin + tt * BQ;
            const char* qt = q_lds + slot * TILE_BYTES;
            const char* dot = do_lds + slot * TILE_BYTES;
            const float* lse_t = lse_lds + slot * BQ;
            const float* dlt_t = dlt_lds + slot * BQ;
            char* pt = p_lds + (((tt & 1) * 4 + strip) * SUB) * 2048 + lane * 32;
            const char* rows_tile = ROLE ? dot : qt;       // S = Q K^T  |  dP = dO V^T
            const char* cols_tile = ROLE ? qt : dot;       // dV^T += dO^T P  |  dK^T += Q^T dZ
            const bool q_in_b = qt0 >= br.b;               // br.b and qt0 are multiples of 64: uniform over the step
            const bool hidden = q_in_b && wk_min >= br.a && wk_min + 31 < br.b;
            // this (key block, query step, strip)'s 4 KiB of the dS workspace
            char* ds_step = (ROLE && p.ds_ws) ? p.ds_ws + ((((int64_t)s * p.H + hd) * p.ds_nkb + kb) * p.ds_nt + qt0 / BQ) * 16384 + strip * 4096
                                              : nullptr;
            // Both sub-tiles are always computed; a step that is not whole and unmasked (sequence tail, causal diagonal, pad keys, the
            // rows of branch B meeting keys of branch A) turns the affected scores into -inf on the V side, which makes P - and with
            // it dZ on the K side - exactly zero there.  A strip entirely hidden from this step's rows skips the step.
            const bool interior = (qt0 + BQ <= len) && (!CAUSAL || qt0 >= wk_min + 31) && !wave_has_pad_keys &&
                                  !(q_in_b && wk_min < br.b && wk_min + 31 >= br.a);      // wave-uniform
            if (!hidden) {
                // Every LDS read is placed by hand one block ahead of its use and nothing may cross a slot boundary: left to itself the
                // scheduler hoists all reads to the top of the step and the register allocator spills.
#define SLOT() __builtin_amdgcn_sched_barrier(0)
                constexpr bool CINIT = ROLE == 1;         // K side: the dP chain starts from -delta
                constexpr int PPS = 8 / KS, PPD = 8 / (2 * DT), NS = KS;      // NS slots per block (KS == 2 * DT)
                static_assert(KS == 2 * DT, "slot count");
                const float* stat_t = ROLE ? dlt_t : lse_t;
                auto pair = [&](const f32x16& x, int r, const f32x4& st, unsigned pw) -> unsigned {
                    const float t0 = st[r & 3], t1 = st[(r & 3) + 1];
                    (void)t0, (void)t1;
                    if (ROLE == 0)
                        return pack_bf16x2(__builtin_amdgcn_exp2f(__builtin_fmaf(x[r], sc, -t0)), __builtin_amdgcn_exp2f(__builtin_fmaf(x[r + 1], sc, -t1)));
                    return pack_bf16x2(bf16_lo(pw) * x[r], bf16_hi(pw) * x[r + 1]);      // K side: x = dP - delta already
                };
                auto mask_scores = [&](f32x16& x, int q0) {
                    const bool lane_off = !k_valid || (q_in_b && key_hidden);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ql = q0 + acc_row(r, h);
                        if (ql >= len || (CAUSAL && kl > ql) || lane_off) x[r] = -INFINITY;      // -> P = 0
                    }
                };
                auto col_frag = [&](int sub, int i) { return frag_cols<D, SLOW_TR>(cols_tile, 32 * sub + 16 * (i / DT), 32 * (i % DT), lane); };
                s16x8 fa[NS], fb[NS], fc[NS], fd[NS];
                f32x4 st0[4], st1[4];
                u32x4 p0[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}}, p1[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
                u32x4 w0[2], w1[2];
                f32x16 x0, x1;
                if (CINIT) {
                // ---- block 1: sub-tile 0's statistics ARE the first chain's initial accumulator (register r <-> query acc_row(r, h)): read
                //      them with the first row fragments; sub-tile 1's are fetched during the chain
#pragma unroll
                for (int j = 0; j < 4; ++j) st0[j] = *reinterpret_cast<const f32x4*>(stat_t + 8 * j + 4 * h);
#pragma unroll
                for (int ks = 0; ks < NS; ++ks) fa[ks] = frag_rows<D>(rows_tile, 0, ks, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) x0[r] = st0[r >> 2][r & 3];
                SLOT();
#pragma unroll
                for (int ks = 0; ks < NS; ++ks) {
                    x0 = mfma32(fa[ks], sf[ks], x0);
                    fb[ks] = frag_rows<D>(rows_tile, 32, ks, lane);
                    if (ks % (NS / 4) == 0) st1[ks / (NS / 4)] = *reinterpret_cast<const f32x4*>(stat_t + 32 + 8 * (ks / (NS / 4)) + 4 * h);
                    if (ROLE && ks == NS - 2) p0[0] = *reinterpret_cast<const u32x4*>(pt);
                    if (ROLE && ks == NS - 1) p0[1] = *reinterpret_cast<const u32x4*>(pt + 16);
                    SLOT();
                }
                } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) x0[r] = 0.f, x1[r] = 0.f;
                // ---- block 1: first product of sub-tile 0; fetch the second sub-tile's row fragments and sub-tile 0's statistics
#pragma unroll
                for (int ks = 0; ks < NS; ++ks) fa[ks] = frag_rows<D>(rows_tile, 0, ks, lane);
                SLOT();
#pragma unroll
                for (int ks = 0; ks < NS; ++ks) {
                    x0 = mfma32(fa[ks], sf[ks], x0);
                    fb[ks] = frag_rows<D>(rows_tile, 32, ks, lane);
                    if (ks % (NS / 4) == 0) st0[ks / (NS / 4)] = *reinterpret_cast<const f32x4*>(stat_t + 8 * (ks / (NS / 4)) + 4 * h);
                    if (ROLE && ks == NS - 2) p0[0] = *reinterpret_cast<const u32x4*>(pt);
                    if (ROLE && ks == NS - 1) p0[1] = *reinterpret_cast<const u32x4*>(pt + 16);
                    SLOT();
                }
                }
                if (ROLE == 0 && !interior) mask_scores(x0, qt0);
                STAMP(1);
                SLOT();
                // ---- block 2: first product of sub-tile 1 || vector work of sub-tile 0; fetch sub-tile 0's column fragments
                if (CINIT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) x1[r] = st1[r >> 2][r & 3];
                }
#pragma unroll
                for (int ks = 0; ks < NS; ++ks) {
                    x1 = mfma32(fb[ks], sf[ks], x1);
                    fc[ks] = col_frag(0, ks);
#pragma unroll
                    for (int q = 0; q < PPS; ++q) {
                        const int i = ks * PPS + q;      // pair i: accumulator registers 2i, 2i+1
                        w0[i >> 2][i & 3] = pair(x0, 2 * i, st0[i >> 1], p0[i >> 2][i & 3]);
                    }
                    if (!CINIT && ks % (NS / 4) == NS / 4 - 1) st1[ks / (NS / 4)] = *reinterpret_cast<const f32x4*>(stat_t + 32 + 8 * (ks / (NS / 4)) + 4 * h);
                    if (ROLE && ks == NS / 2 - 1) p1[0] = *reinterpret_cast<const u32x4*>(pt + 2048);
                    if (ROLE && ks == NS - 1) p1[1] = *reinterpret_cast<const u32x4*>(pt + 2048 + 16);
                    SLOT();
                }
                if (!ROLE) {
                    *reinterpret_cast<u32x4*>(pt) = w0[0];
                    *reinterpret_cast<u32x4*>(pt + 16) = w0[1];
                    if (!interior) mask_scores(x1, qt0 + 32);
                } else if (ds_step) {      // nontemporal: written once, read once by another kernel - keep Q / dO / K / V in L2
                    __builtin_nontemporal_store(w0[0], reinterpret_cast<u32x4*>(ds_step + lane * 16));
                    __builtin_nontemporal_store(w0[1], reinterpret_cast<u32x4*>(ds_step + 1024 + lane * 16));
                }
                STAMP(2);
                SLOT();
                // ---- block 3: second product of sub-tile 0 || vector work of sub-tile 1; fetch sub-tile 1's column fragments
#pragma unroll
                for (int i = 0; i < NS; ++i) {
                    acc[i % DT] = mfma32(fc[i], __builtin_bit_cast(s16x8, w0[i / DT]), acc[i % DT]);
                    fd[i] = col_frag(1, i);
#pragma unroll
                    for (int q = 0; q < PPD; ++q) {
                        const int j = i * PPD + q;
                        w1[j >> 2][j & 3] = pair(x1, 2 * j, st1[j >> 1], p1[j >> 2][j & 3]);
                    }
                    SLOT();
                }
                if (!ROLE) {
                    *reinterpret_cast<u32x4*>(pt + 2048) = w1[0];
                    *reinterpret_cast<u32x4*>(pt + 2048 + 16) = w1[1];
                } else if (ds_step) {
                    __builtin_nontemporal_store(w1[0], reinterpret_cast<u32x4*>(ds_step + 2048 + lane * 16));
                    __builtin_nontemporal_store(w1[1], reinterpret_cast<u32x4*>(ds_step + 3072 + lane * 16));
                }
                // ---- block 4: second product of sub-tile 1
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i % DT] = mfma32(fd[i], __builtin_bit_cast(s16x8, w1[i / DT]), acc[i % DT]);
#undef SLOT
            }
        }
#ifdef HALVA_STAMP
        asm volatile("" : "+v"(acc[0][15]), "+v"(acc[DT - 1][15]));
#endif
        STAMP(3);
        if (t + 1 < ntiles) store_stats(slot_next);
        if (dma_wave) stage_tile_dma_wait();      // (the K side has only its dS stores in flight: nothing of this step waits for them)
        STAMP(4);
        slot = (slot == 2) ? 0 : slot + 1;
        slot_next = (slot_next == 2) ? 0 : slot_next + 1;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // not __syncthreads(): its fence would drain the dS stores
    }
#ifdef HALVA_STAMP
    if (p.dbg && lane == 0 && kb == 0 && s == 0 && hd < 4) {
        const int wave = strip + 4 * ROLE;
        for (int i = 0; i < 6; ++i) p.dbg[(hd * 8 + wave) * 8 + i] = stamp_acc[i];
        p.dbg[(hd * 8 + wave) * 8 + 6] = ntiles;
    }
    blk_t[1] = stamp_prev;      // (the loop's last stamp)
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[2])::"memory");
#endif
    // every wave has passed the last step's barrier: the rings are free and the stationary fragments dead
    prefetch_next();
    if (k_in_T) store_rows_T<D>(outrow, acc, k_valid ? (ROLE ? p.scale : 1.f) : 0.f, true, lane);
#ifdef HALVA_STAMP
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(blk_t[3])::"memory");
    if (p.dbg && lane == 0 && s == 0 && hd == 0) {      // whole-block anatomy: [entry, loop end, before the stores, after the stores]
        const int wave = strip + 4 * ROLE;
        for (int i = 0; i < 8; ++i) p.dbg[1024 + (kb * 8 + wave) * 8 + i] = blk_t[i];
    }
#endif
}

template <int D, bool CAUSAL, bool SLOW_TR, int ROLE>
__device__ __forceinline__ void sdpa_bwd_dkv2_role(const SdpaParams& p, char* smem, int strip) {
    int s, hd, b;
    map_block(blockIdx.x, CAUSAL ? (p.nblk + 1) / 2 : p.nblk, p.H, p.npairs, false, s, hd, b);
    // the sequence's geometry is read ONCE per workgroup (both key blocks belong to the same sequence): in a block's prologue these
    // scalar loads are a memory round trip of their own in front of everything else
    const int start = p.seq_start ? p.seq_start[s] : 0;
    const int len = p.seq_len ? p.seq_len[s] : p.T;
    const Branch br = load_branch(p, s);
    s16x8 sf[D / 16];
    float st[2] = {0.f, 0.f};
    // under the causal mask key block b is visited by (nblk - b) query blocks: pair b with nblk-1-b
    const int second = (CAUSAL && b != p.nblk - 1 - b) ? p.nblk - 1 - b : -1;
    sdpa_bwd_dkv2_block<D, CAUSAL, SLOW_TR, ROLE>(p, smem, s, hd, b, second, false, strip, start, len, br, sf, st);
    if (second >= 0) sdpa_bwd_dkv2_block<D, CAUSAL, SLOW_TR, ROLE>(p, smem, s, hd, second, -1, true, strip, start, len, br, sf, st);
}

template <int D, bool CAUSAL, bool SLOW_TR>
__global__ __launch_bounds__(512) void sdpa_bwd_dkv2_kernel(const SdpaParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the role is a per-wave constant: branch on it once, on the scalar unit, so that each side gets its own register allocation
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    WG_CLOCK_BEGIN();
    if (wave < 4) sdpa_bwd_dkv2_role<D, CAUSAL, SLOW_TR, 0>(p, smem, wave);
    else sdpa_bwd_dkv2_role<D, CAUSAL, SLOW_TR, 1>(p, smem, wave - 4);      // (raising these waves' s_setprio changes nothing)
    WG_CLOCK_END(p.dbg, 1);
}

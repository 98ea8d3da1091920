// A fragment of the sdpa.hip translation unit, not compiled alone: included there inside its anonymous namespace, behind common.h and
// the sdpa_*.h listed before it.  Holds sdpa_bwd_dq_kernel, the 3-product dQ.
// ===================================================================================================
// backward, part 1: dQ  (same skeleton as the forward), and delta[s, h, t] = sum_d dO * O for both backward kernels
// ===================================================================================================
template <int D, bool CAUSAL, bool SLOW_TR, int NW>
__device__ __forceinline__ void sdpa_bwd_dq_block(const SdpaParams& p, char* smem, int s, int hd, int qb) {
    constexpr int BN = 64, KS = D / 16, DT = D / 32, BM = 32 * NW, NT = 64 * NW;
    constexpr int TILE_BYTES = BN * D * 2;
    char* k_lds = smem;
    char* v_lds = smem + 2 * TILE_BYTES;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
    const int start = p.seq_start ? p.seq_start[s] : 0;
    const int len = p.seq_len ? p.seq_len[s] : p.T;
    const int g0 = qb * BM;
    const int64_t seq_row0 = (int64_t)s * p.T;
    const int gq = g0 + 32 * wave + (lane & 31);
    const int ql = gq - start;
    const bool q_in_T = gq < p.T;
    const bool q_valid = q_in_T && ql >= 0 && ql < len;

    int kv_end = len;
    if (CAUSAL) kv_end = min(len, g0 + BM - start);
    const int ntiles = kv_end > 0 ? (kv_end + BN - 1) / BN : 0;

    const bf16_t* qp = p.q + hd * D;
    const bf16_t* kp = p.k + hd * D;
    const bf16_t* vp = p.v + hd * D;
    bf16_t* dqrow = p.dq + (seq_row0 + gq) * p.ld_qkv + hd * D;
    if (ntiles == 0) {
        if (q_in_T) store_rows_zero<D>(dqrow, lane);
        return;
    }

    s16x8 qf[KS], dof[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (q_valid) {
            qf[ks] = *reinterpret_cast<const s16x8*>(qp + (seq_row0 + gq) * p.ld_qkv + 16 * ks + 8 * h);
            dof[ks] = *reinterpret_cast<const s16x8*>(p.d_o + (seq_row0 + gq) * p.ld_do + hd * D + 16 * ks + 8 * h);
        } else {
            qf[ks] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
            dof[ks] = s16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    const int64_t stat = ((int64_t)s * p.H + hd) * p.T + gq;
    const float lse2 = q_valid ? p.lse[stat] * kLog2e : INFINITY;      // padded query rows: P = exp2(-inf) = 0
    // delta = rowsum(O o dO): this lane holds half of its row of dO already; the other half sits on lane ^ 32.  Written out for the
    // dK/dV kernel, which runs after this one (this used to be a launch of its own: 52 us of the backward's 1.2 ms).
    float dsum = 0.f;
    if (q_valid) {
        const bf16_t* orow = p.o_in + (seq_row0 + gq) * p.ld_o + hd * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4 ov = *reinterpret_cast<const u32x4*>(orow + 16 * ks + 8 * h);
            const u32x4 dv = __builtin_bit_cast(u32x4, dof[ks]);
#pragma unroll
            for (int i = 0; i < 4; ++i) dsum += bf16_lo(ov[i]) * bf16_lo(dv[i]) + bf16_hi(ov[i]) * bf16_hi(dv[i]);
        }
    }
    const float dlt = xhalf_sum(dsum);
    if (q_valid && h == 0) p.delta[stat] = dlt;
    const float sc = p.scale * kLog2e;

    f32x16 dqacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dqacc[dt][r] = 0.f;

    const int wq_min = g0 + 32 * wave - start, wq_max = wq_min + 31;
    const Branch br = load_branch(p, s);
    const bool wave_in_b = wq_min >= br.b;             // wave-uniform (br.b is a multiple of 64, strips are 32 rows)
    // K/V tiles arrive by LDS-DMA (no staging registers, no ds_write pass); the slow-transpose debug build keeps register staging
    constexpr bool DMA = !SLOW_TR && NW == 8;
    Stage<D, BN, NT> kst, vst;
    TileDma<D, NW> kdma, vdma;
    const int64_t krow0 = seq_row0 + start;
    // key-tile range in (up to) two segments around the tiles a branch-B row block never needs (see the forward)
    int skip_lo = ntiles, skip_hi = ntiles;
    if (g0 - start >= br.b) {
        skip_lo = min(ntiles, (br.a + BN - 1) / BN);
        skip_hi = max(skip_lo, min(ntiles, br.b / BN));
    }
#pragma unroll 1
    for (int seg = 0; seg < 2; ++seg) {
        const int t0 = seg ? skip_hi : 0, t1 = seg ? ntiles : skip_lo;
        if (t0 >= t1) continue;
        __syncthreads();      // earlier readers of the LDS slots (previous segment / previous row block) are done
        if (DMA) {
            stage_tile_dma<D, NW>(k_lds, kp, p.ld_qkv, krow0, t0 * BN, len, wave, lane);
            stage_tile_dma<D, NW>(v_lds, vp, p.ld_qkv, krow0, t0 * BN, len, wave, lane);
            kdma.init(kp, p.ld_qkv, krow0, (t0 + 1) * BN, wave, lane);
            vdma.init(vp, p.ld_qkv, krow0, (t0 + 1) * BN, wave, lane);
            stage_tile_dma_wait();
        } else {
            kst.load_clamped(kp, p.ld_qkv, krow0, t0 * BN, len);
            vst.load_clamped(vp, p.ld_qkv, krow0, t0 * BN, len);
            kst.store(k_lds);
            vst.store(v_lds);
        }
        __syncthreads();
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
                kdma.issue_and_advance(k_lds + (slot ^ 1) * TILE_BYTES, p.ld_qkv, wave);
                vdma.issue_and_advance(v_lds + (slot ^ 1) * TILE_BYTES, p.ld_qkv, wave);
            } else {      // the sequence's last, partial tile
                stage_tile_dma<D, NW>(k_lds + (slot ^ 1) * TILE_BYTES, kp, p.ld_qkv, krow0, kv0 + BN, len, wave, lane);
                stage_tile_dma<D, NW>(v_lds + (slot ^ 1) * TILE_BYTES, vp, p.ld_qkv, krow0, kv0 + BN, len, wave, lane);
            }
        }
        const bool hidden = wave_in_b && kv0 >= br.a && kv0 < br.b;                       // tile wholly inside [a, b)
        const int len_t = (wave_in_b && kv0 < br.a && kv0 + BN > br.a) ? br.a : len;       // tile cut at a
        const bool active = (!CAUSAL || kv0 <= wq_max) && !hidden;
        if (active) {
            f32x16 st[2], dp[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    st[t][r] = 0.f;
                    dp[t][r] = 0.f;
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    st[t] = mfma32(frag_rows<D>(kt, 32 * t, ks, lane), qf[ks], st[t]);
                    dp[t] = mfma32(frag_rows<D>(vt, 32 * t, ks, lane), dof[ks], dp[t]);
                }
            }
            if ((kv0 + BN > len_t) || (CAUSAL && kv0 + BN - 1 > wq_min)) {      // wave-uniform: boundary tiles only
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kl = kv0 + 32 * t + acc_row(r, h);
                        if (kl >= len_t || (CAUSAL && kl > ql)) st[t][r] = -INFINITY;      // -> P = 0
                    }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(st[t][r], sc, -lse2));
                    st[t][r] = pr * (dp[t][r] - dlt);   // dZ^T
                }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const s16x8 zb = acc_to_frag(st[ks >> 1], ks & 1);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
                    dqacc[dt] = mfma32(frag_cols<D, SLOW_TR>(kt, 16 * ks, 32 * dt, lane), zb, dqacc[dt]);
            }
        }
        if (DMA) {
            stage_tile_dma_wait();
        } else if (it + 1 < t1) {
            kst.store(k_lds + (slot ^ 1) * TILE_BYTES);
            vst.store(v_lds + (slot ^ 1) * TILE_BYTES);
        }
        __syncthreads();
        }
    }
    if (q_in_T) store_rows_T<D>(dqrow, dqacc, q_valid ? p.scale : 0.f, true, lane);
}

template <int D, bool CAUSAL, bool SLOW_TR, int NW>
__global__ __launch_bounds__(64 * NW, (NW == 4 ? 2 : 1)) void sdpa_bwd_dq_kernel(const SdpaParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int s, hd, b;
    if (CAUSAL) {
        map_block(blockIdx.x, (p.nblk + 1) / 2, p.H, p.npairs, false, s, hd, b);
        sdpa_bwd_dq_block<D, CAUSAL, SLOW_TR, NW>(p, smem, s, hd, p.nblk - 1 - b);
        if (b != p.nblk - 1 - b) sdpa_bwd_dq_block<D, CAUSAL, SLOW_TR, NW>(p, smem, s, hd, b);
    } else {
        map_block(blockIdx.x, p.nblk, p.H, p.npairs, false, s, hd, b);
        sdpa_bwd_dq_block<D, CAUSAL, SLOW_TR, NW>(p, smem, s, hd, b);
    }
}

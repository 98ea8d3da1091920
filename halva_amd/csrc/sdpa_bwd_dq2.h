// A fragment of the sdpa.hip translation unit, not compiled alone: included there inside its anonymous namespace, behind common.h and
// the sdpa_*.h listed before it.  Holds sdpa_bwd_delta_kernel and sdpa_bwd_dq2_kernel, the first and the last pass of the backward with a dS workspace.
// ===================================================================================================
// backward with a dS workspace: delta / zero-fill pass, then dK/dV (+ dS store), then dQ = dS K
// ===================================================================================================
// delta[s, h, t] = sum_d dO o O for every valid query row (both later kernels read it), and zeros into dq of the PADDED rows (the dQ
// kernel below walks a sequence in its own coordinates and only writes its valid rows).  One wave per (row, 4 heads); HBM-bound.
// for_dkv3: also what sdpa_bwd_dkv3 needs before it starts - its work-queue counters zeroed and (round 6) its item records (sdpa_dkv3_items.h).
template <int D>
__global__ __launch_bounds__(256) void sdpa_bwd_delta_kernel(const SdpaParams p, int S, int for_dkv3) {
    constexpr int HPW = 512 / D;                       // heads per wave pass: 64 lanes x 8 elements
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (for_dkv3 && blockIdx.x == 0 && threadIdx.x < 8) p.sched[32 * threadIdx.x] = 0;
    if (for_dkv3) {      // one thread per record (8 192 - 13 824 of them at the step's shapes: the first few dozen workgroups)
        const int total = p.npairs * p.nblk;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= total; i += (int64_t)gridDim.x * 256)
            dkv3_build_record<true>(p, (int)i, total, p.items + i * DKV3_REC_DWORDS);
    }
    if (row >= (int64_t)S * p.T) return;
    const int s = (int)(row / p.T), t = (int)(row % p.T);
    const int start = p.seq_start ? p.seq_start[s] : 0;
    const int len = p.seq_len ? p.seq_len[s] : p.T;
    const bool valid = t >= start && t < start + len;
    const int sub = lane / (D / 8), e = (lane % (D / 8)) * 8;      // head within the pass, first element
    for (int h0 = 0; h0 < p.H; h0 += HPW) {
        const int hd = h0 + sub;
        if (hd >= p.H) continue;
        if (!valid) {
            *reinterpret_cast<u32x4*>(p.dq + row * p.ld_qkv + hd * D + e) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
        // (out is read here for the last time; dO once more, tile by tile, by the dK/dV kernel - from HBM either way: 0.27 - 0.45 GB per tensor)
        const u32x4 ov = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.o_in + row * p.ld_o + hd * D + e));
        const u32x4 dv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.d_o + row * p.ld_do + hd * D + e));
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += bf16_lo(ov[i]) * bf16_lo(dv[i]) + bf16_hi(ov[i]) * bf16_hi(dv[i]);
#pragma unroll
        for (int o = D / 16; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane % (D / 8) == 0) {
            const int64_t at = ((int64_t)s * p.H + hd) * p.T + t;
            if (for_dkv3) {      // sdpa_bwd_dkv3 starts its dP chain from -delta and fetches both statistics of a 64-row step with ONE request (sdpa_dkv3.h)
                const int loc = t - start;
                float* rec = p.lse2 + (((int64_t)s * p.H + hd) * p.stat_nt + (loc >> 6)) * 128;
                rec[loc & 63] = p.lse[at] * kLog2e;
                rec[64 + (loc & 63)] = -acc;
                if (loc == len - 1)      // the rest of the sequence's last record: zeros (a padded query row then yields P = 1, dS = 0 - finite)
                    for (int j = (loc & 63) + 1; j < 64; ++j) rec[j] = 0.f, rec[64 + j] = 0.f;
            } else {
                p.delta[at] = acc;
            }
        }
    }
}

// dQ = scale * dS K with dS read back from the workspace the dK/dV kernel filled.  A workgroup takes 256 query rows of one (sequence,
// head) in SEQUENCE coordinates (row 0 = seq_start: the grid of query steps the producer used), a wave 32 of them = one 32-row half of
// a producer step; per 64-key tile (GLOBAL key coordinates = the producer's 128-key blocks) a wave multiplies
//     dQ^T[128 x 32] += K^T[128 x 64] dS^T[64 x 32]          (16 MFMAs: A = K^T by transposed reads of the shared K tile,
//                                                             B = dS^T by transposed reads of the wave's own 4 KiB of dS)
// The producer's layout is, per (key block, step, 32-key strip, 32-row half, register half j): 64 lanes x 16 bytes, lane (key n, h')
// holding the query rows 16 j + 8 g + 4 h' + (0..3), g = 0, 1: the 8-byte unit (one key, four consecutive queries) is exactly what
// ds_read_b64_tr_b16 gathers from, so the image is copied to LDS byte for byte (LDS-DMA) and transposed by the read.
// HBM-bound: 2 bytes per (query, key) pair, the same pairs the producer wrote.
__device__ __forceinline__ int ds_piece_off(int key, int qgroup) {      // byte offset of (key 0..31, queries 4 G .. 4 G + 3) in a strip's 2 KiB
    return 1024 * (qgroup >> 2) + 16 * (key + 32 * (qgroup & 1)) + 8 * ((qgroup >> 1) & 1);
}
// The LDS copy (round 4): the same image with its 1-KiB pieces 1152 bytes apart (strips 2304, ring slots 4608).  One transposed read has, in
// each half of the wave, its lanes on byte pairs that differ in G >> 2 (the piece) and G & 1 (512 bytes apart inside the piece) only: 1 KiB and
// 512 bytes are multiples of the 256-byte bank row - the same banks FOUR times (SQ_LDS_BANK_CONFLICT = 37 % of this kernel's LDS cycles,
// profiles/r04_sdpa_all_pmc.json).  The 128 bytes of padding move the odd pieces half a bank row: two-way.  Measured and NOT kept: the last
// factor of two by an XOR of the chunk position, applied by the LDS-DMA lanes (lane l fetches chunk l ^ swizzle; LDS-DMA writes lane l to
// byte 16 l) - zero conflicts, but the requests no longer ask for their 1 KiB in lane order and the kernel, which is HBM-bound, ran 1.6 % SLOWER
// (950-959 -> 971-973 us at the step's shapes, same box).
constexpr int DS_LDS_PIECE = 1024 + 128, DS_LDS_STRIP = 2 * DS_LDS_PIECE, DS_LDS_SLOT = 2 * DS_LDS_STRIP;
__device__ __forceinline__ int ds_lds_off(int key, int qgroup) {      // (inside a strip)
    return DS_LDS_PIECE * (qgroup >> 2) + 16 * (key + 32 * (qgroup & 1)) + 8 * ((qgroup >> 1) & 1);
}
template <int D, bool SLOW_TR, bool FAST>
__device__ __forceinline__ void sdpa_bwd_dq2_block(const SdpaParams& p, char* smem, int s, int hd, int qb, int wave, int lane) {
    constexpr int NW = 8, BN = 64, DT = D / 32, BM = 32 * NW, RING = 3;
    constexpr int TILE_BYTES = BN * D * 2;
    char* k_lds = smem;                                            // [RING][BN][D]
    char* ds_lds = smem + RING * TILE_BYTES + wave * (RING * DS_LDS_SLOT);  // per wave: [RING][2 strips][2 pieces of 1 KiB + 128 B]
    const int h = lane >> 5;
    const int start = p.seq_start ? p.seq_start[s] : 0;
    const int len = p.seq_len ? p.seq_len[s] : p.T;
    const int64_t seq_row0 = (int64_t)s * p.T;
    const int lq0 = qb * BM;                             // first local row of the block
    if (lq0 >= len) return;                              // workgroup-uniform
    const int wr0 = lq0 + 32 * wave;                     // this wave's first local row
    const int lq = wr0 + (lane & 31);
    const bool q_valid = lq < len;
    const bool wave_live = wr0 < len;
    const Branch br = load_branch(p, s);
    const bool wave_in_b = wr0 >= br.b;
    // global key tiles that hold a key some row of the block may see: local key index kv0g - start <= last row of the block
    const int first_tile = max(0, start) / BN;
    const int last_key_local = min(len, lq0 + BM) - 1;                 // causal: keys <= row
    const int ntile_end = (start + last_key_local) / BN + 1;           // exclusive, global tile index
    f32x16 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
    const bf16_t* kp = p.k + hd * D;
    const int64_t krow0 = seq_row0 + start;
    const int step = wr0 / 64, sub = (wr0 / 32) & 1;
    const char* ds_pair = p.ds_ws + ((int64_t)s * p.H + hd) * p.ds_nkb * p.ds_nt * 16384;
    const unsigned ds_dst = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ds_lds;
    // a tile is skipped by this wave when none of its rows sees any of its keys (tiles are walked upwards: once skipped, always skipped);
    // a 32-key strip when the branch mask hides it wholly (the producer then wrote nothing for it: its bytes are fetched but not used)
    auto tile_live = [&](int kt) { return wave_live && (kt * BN - start) <= wr0 + 31; };
    auto strip_hidden = [&](int kt, int si) {
        const int k0 = kt * BN + 32 * si - start;
        return wave_in_b && k0 >= br.a && k0 + 31 < br.b;
    };
    // requests of one tile by this wave: its 2 chunks of the shared K tile, and - while the tile is live for it - its own 4 KiB of dS
    auto stage = [&](int kt, int slot) {
        stage_tile_dma<D, NW>(k_lds + slot * TILE_BYTES, kp, p.ld_qkv, krow0, kt * BN - start, len, wave, lane);
        if (tile_live(kt)) {
            const char* src = ds_pair + ((int64_t)(kt >> 1) * p.ds_nt + step) * 16384 + 2 * (kt & 1) * 4096 + sub * 2048;
#pragma unroll
            for (int c = 0; c < 4; ++c) {                 // strip c >> 1, register half c & 1
                const unsigned dst = ds_dst + slot * DS_LDS_SLOT + (c >> 1) * DS_LDS_STRIP + (c & 1) * DS_LDS_PIECE;
                const unsigned voff = lane * 16;
                const char* rows = src + (c >> 1) * 4096 + (c & 1) * 1024;
                unsigned keep;
                // nt: these bytes are read once, by this CU only - they must not evict the K tiles the XCD's workgroups share in L2
                asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3 nt\n\ts_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(voff), "s"(dst), "s"(rows) : "memory");
            }
        }
    };
    // per-lane byte offsets of the transposed reads of dS^T (see frag_cols for the lane roles): key 8 jj + 4 hb + q4, query group 4 (g & 1) + pp
    const int g = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pp = i16 & 3, hb = g >> 1;
    const int ds_rd0 = ds_lds_off(4 * hb + q4, 4 * (g & 1) + pp);           // jj = 0; jj = 1 adds 8 keys = 128 bytes
    // frag_cols' addresses in the K tile, as two per-lane bases (jj = 0, 1: rows 8 jj + 4 hb + q4 of a 16-key group) + 4096 ks + 512 dt (tile_off)
    const unsigned k_u32 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)k_lds;
    unsigned klane[2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj)
        klane[jj] = 2048 * jj + 64 * (4 * hb + q4) + 16 * ((2 * (g & 1) + (pp >> 1)) ^ ((2 * jj + hb) & 3)) + 8 * (pp & 1);
    // A row block wholly in branch B never needs the key tiles that lie wholly inside [a, b) (the producer wrote no dS for them either):
    // the walk jumps from tile skip_lo - 1 to tile skip_hi, as the forward's does.  In the bench's packed rows [668 | 1380 | 1380] that
    // is 21 of the 33..54 tiles of each of the six B blocks - 30 % of this kernel's tile steps, each a 16-KiB K tile and up to 32 KiB
    // of dS fetched for nothing.  (Branch points come with start == 0: halva_amd/splice.py packs right-padded rows only.)
    int skip_lo = ntile_end, skip_hi = ntile_end;
    if (start == 0 && lq0 >= br.b) {
        skip_lo = min(ntile_end, max(first_tile, (br.a + BN - 1) / BN));
        skip_hi = max(skip_lo, min(ntile_end, br.b / BN));
    }
    const int n_lo = skip_lo - first_tile, n_walk = n_lo + (ntile_end - skip_hi);
    auto tile_at = [&](int i) { return i < n_lo ? first_tile + i : skip_hi + (i - n_lo); };
    // TWO tiles in flight (HBM-bound kernel: the queue must not run dry while a tile is multiplied): ring of three slots, counted waits
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // the previous row block's readers are done
    if (n_walk > 0) stage(tile_at(0), 0);
    if (n_walk > 1) stage(tile_at(1), 1);
#pragma unroll 1
    for (int i = 0; i < n_walk; ++i) {
        const int kt = tile_at(i);
        const int slot = i % RING;
        // tile i has landed: everything but the requests of tile i + 1 (2 pieces, 6 while that tile is live for this wave)
        if (i + 1 < n_walk) {
            if (tile_live(tile_at(i + 1))) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // ... for every wave; and tile i - 1 has been read by all
        if (i + 2 < n_walk) stage(tile_at(i + 2), (slot + 2) % RING);         // into the slot of tile i - 1
        if (tile_live(kt)) {
            const char* ktile = k_lds + slot * TILE_BYTES;
            const char* dst_t = ds_lds + slot * DS_LDS_SLOT;
            if (FAST && !SLOW_TR) {
                // All 40 operand reads of the tile from three per-lane bases + immediates, asked for ahead of the 16 products (the same products in the
                // same order as the general path below: identical sums).  Compiled from the loop below, every product waited for operand reads issued just
                // in front of it (s_waitcnt lgkmcnt(0) x 16 per tile) and each read cost two vector instructions of address arithmetic: without any dS
                // traffic at all the kernel still took 0.82 of its time (experiments/ds_residency: dq2 anatomy by removal, profiles/r05_dq2_anatomy.log).
                const unsigned a0 = k_u32 + slot * TILE_BYTES + klane[0], a1 = k_u32 + slot * TILE_BYTES + klane[1];
                const unsigned da = ds_dst + slot * DS_LDS_SLOT + ds_rd0;
                auto rd = [](unsigned addr) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)addr); };
                s16x4 zt[4][2], kt4[4][DT][2];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    zt[ks][0] = rd(da + (ks >> 1) * DS_LDS_STRIP + 256 * (ks & 1));
                    zt[ks][1] = rd(da + (ks >> 1) * DS_LDS_STRIP + 256 * (ks & 1) + 128);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        kt4[ks][dt][0] = rd(a0 + 4096 * ks + 512 * dt);
                        kt4[ks][dt][1] = rd(a1 + 4096 * ks + 512 * dt);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    s16x8 zb;
#pragma unroll
                    for (int j = 0; j < 4; ++j) zb[j] = zt[ks][0][j], zb[4 + j] = zt[ks][1][j];
                    // a strip the branch mask hides wholly was never written by the producer: its bytes are whatever the workspace held - zeros instead
                    // (the general path skips its products; adding exact zeros leaves the sums as they are).  ONE path for every tile: with a second one
                    // the accumulators changed registers between the two (32 moves per tile).
                    // Branch-free (an AND with a scalar mask): the tile stays one basic block and the order asked for below holds.
                    {
                        u32x4 w = __builtin_bit_cast(u32x4, zb);
                        const unsigned keep = strip_hidden(kt, ks >> 1) ? 0u : 0xffffffffu;
                        w[0] &= keep, w[1] &= keep, w[2] &= keep, w[3] &= keep;
                        zb = __builtin_bit_cast(s16x8, w);
                    }
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        s16x8 ka;
#pragma unroll
                        for (int j = 0; j < 4; ++j) ka[j] = kt4[ks][dt][0][j], ka[4 + j] = kt4[ks][dt][1][j];
                        acc[dt] = mfma32(ka, zb, acc[dt]);
                    }
                }
                // the order asked of the scheduler: ten reads (the first product's operands and the next one's), then a product per two reads
                __builtin_amdgcn_sched_group_barrier(0x100, 14, 0);
#pragma unroll
                for (int i = 0; i < 13; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            } else
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {               // 16 keys each: strip ks >> 1, half ks & 1
                if (strip_hidden(kt, ks >> 1)) continue;
                s16x8 zb;
                if (SLOW_TR) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int key = 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3), qq = lane & 31;
                        zb[j] = *reinterpret_cast<const short*>(dst_t + (ks >> 1) * DS_LDS_STRIP + ds_lds_off(key, qq >> 2) + (qq & 3) * 2);
                    }
                } else {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const char* a = dst_t + (ks >> 1) * DS_LDS_STRIP + ds_rd0 + 16 * (16 * (ks & 1) + 8 * jj);
                        const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)a);
                        zb[4 * jj + 0] = t[0];
                        zb[4 * jj + 1] = t[1];
                        zb[4 * jj + 2] = t[2];
                        zb[4 * jj + 3] = t[3];
                    }
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma32(frag_cols<D, SLOW_TR>(ktile, 16 * ks, 32 * dt, lane), zb, acc[dt]);
            }
        }
    }
    bf16_t* dq_row = p.dq + (seq_row0 + start + lq) * p.ld_qkv + hd * D;
    if constexpr (D == 128) {
        if (p.rope_cos) {      // (workgroup-uniform) positions: halva_rope_qk's convention; the wave's 32 rows sit at consecutive positions
            if (wave_live) {   // (wave-uniform)
                char* scratch = ds_lds;      // the wave's own dS ring: its last tile has been read (the loop's MFMAs consumed it), nobody else touches it
                rope_rows_to_lds(scratch, p.rope_cos, p.rope_sin, rope_position(start + wr0, br), p.rope_max_pos, lane);
                store_rows_T_rope<D>(dq_row, acc, p.scale, q_valid, lane, scratch);
            }
            return;
        }
    }
    if (q_valid) store_rows_T<D>(dq_row, acc, p.scale, true, lane);
}

template <int D, bool SLOW_TR, bool FAST = true>      // (FAST = false: every tile through the general per-strip loop - HALVA_DQ2_FAST_TILE=0, the bitwise twin of the fast tile)
__global__ __launch_bounds__(512) void sdpa_bwd_dq2_kernel(const SdpaParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int s, hd, b;
    map_block(blockIdx.x, (p.nblk + 1) / 2, p.H, p.npairs, false, s, hd, b);
    int heavy, light;      // (the same pairing as the forward: the blocks' work is the same count of key tiles)
    paired_blocks(p.nblk, p.seq_start ? p.seq_start[s] : 0, load_branch(p, s), b, heavy, light);
    const int npass = (heavy != light) ? 2 : 1;
    WG_CLOCK_BEGIN();
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) sdpa_bwd_dq2_block<D, SLOW_TR, FAST>(p, smem, s, hd, pass ? light : heavy, wave, lane);
    WG_CLOCK_END(p.dbg, 2);
}

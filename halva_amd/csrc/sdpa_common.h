// A fragment of the sdpa.hip translation unit, not compiled alone: included there inside its anonymous namespace, behind common.h and
// the sdpa_*.h listed before it.  Holds what the attention kernels share (vector types, STAMP, SdpaParams, Branch, tiles and their LDS-DMA, the softmax tile pieces, store epilogues, block maps).
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

#ifdef HALVA_STAMP
#define STAMP(i)                                                                                   \
    do {                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        unsigned long long t_;                                                                     \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");              \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        stamp_acc[i] += t_ - stamp_prev;                                                           \
        stamp_prev = t_;                                                                           \
    } while (0)
unsigned long long* g_dbg = nullptr;
extern "C" unsigned long long* halva_dbg_buffer() {
    if (!g_dbg) {
        (void)hipMalloc(&g_dbg, 8192 * 8);
        (void)hipMemset(g_dbg, 0, 8192 * 8);
    }
    return g_dbg;
}
// whole-workgroup clock stamp: cycles (s_memtime) and 100 MHz ticks (s_memrealtime) of every 8th workgroup -> in-kernel clock of THIS kernel
// (MI355X_MICROARCH.md, DVFS give-back item 6); slot k of the debug buffer's upper half: {cycles, ticks, start tick, block}
#ifndef HALVA_STAMP_STRIDE
#define HALVA_STAMP_STRIDE 8      // 8: the first 120 workgroups of XCD 0;  17: every XCD and every round of a 2048-workgroup launch
#endif
#define WG_CLOCK_BEGIN() const unsigned long long wgc0_ = __builtin_amdgcn_s_memtime(), wgr0_ = __builtin_amdgcn_s_memrealtime()
#define WG_CLOCK_END(dbg, region)                                                                                     \
    do {                                                                                                              \
        if ((dbg) && threadIdx.x == 0 && blockIdx.x % HALVA_STAMP_STRIDE == 0 && blockIdx.x / HALVA_STAMP_STRIDE < 120) { \
            unsigned long long* o_ = (dbg) + 4096 + (region)*480 + (blockIdx.x / HALVA_STAMP_STRIDE) * 4;             \
            o_[0] = __builtin_amdgcn_s_memtime() - wgc0_;                                                             \
            o_[1] = __builtin_amdgcn_s_memrealtime() - wgr0_;                                                         \
            o_[2] = wgr0_;                                                                                            \
            o_[3] = blockIdx.x;                                                                                       \
        }                                                                                                             \
    } while (0)
#else
#define STAMP(i)
#define WG_CLOCK_BEGIN()
#define WG_CLOCK_END(dbg, region)
#endif

struct SdpaParams {
    const bf16_t* q;      // [S, T, ...] row stride ld_qkv, head offset hd * D
    const bf16_t* k;
    const bf16_t* v;
    bf16_t* o;            // fwd: out; bwd: unused
    const bf16_t* o_in;   // bwd: forward output
    const bf16_t* d_o;    // bwd: grad of out, row stride ld_o
    bf16_t* dq;           // bwd outputs, row stride ld_qkv (packed like q/k/v)
    bf16_t* dk;
    bf16_t* dv;
    float* lse;           // [S, H, T]
    float* delta;         // [S, H, T]
    float* lse2;          // sdpa_bwd_dkv3's row statistics, written by the delta pass (tail of the dS workspace; nullptr without one): per (sequence,
                          // head) stat_nt records of 512 bytes, one per 64-row step in SEQUENCE coordinates: [lse * log2(e) x 64][-delta x 64]
    int stat_nt;          // records per (sequence, head) = ceil(T / 64)
    int sched_order;      // order of the items inside a queue (sdpa_dkv3.h)
    int* sched;           // sdpa_bwd_dkv3's eight work-queue counters, 128 B apart (behind lse2 in the workspace), zeroed by the delta pass
    int* items;           // sdpa_bwd_dkv3's item records, 64 dwords each in queue order + one all-zero record (behind the counters), written by the delta pass
    const int32_t* seq_start;
    const int32_t* seq_len;
    const int32_t* br_a;  // optional per-sequence branch points (local indices; br_b a multiple of 64), include/halva_hip.h:
    const int32_t* br_b;  // rows [br_b, len) do not attend to rows [br_a, br_b)
    int64_t ld_qkv;       // elements between consecutive tokens in q/k/v
    int64_t ld_o;         // elements between consecutive tokens in out
    int64_t ld_do;        // elements between consecutive tokens in dout
    int T, H;
    int nblk, npairs;     // row blocks per (sequence, head) pair; number of pairs (S * H)
    unsigned long long* dbg;   // diagnostic builds only
    char* ds_ws;          // backward: dS = P o (dP - delta) as bf16 in the dK/dV kernel's register layout (see ds_chunk), or nullptr
    int ds_nkb, ds_nt;    // key blocks of 128 / query steps of 64 per (sequence, head) in ds_ws
    float scale;          // softmax scale
    // backward, optional: the inverse RoPE of dq / dk applied in the store epilogues of sdpa_bwd_dq2 / sdpa_bwd_dkv3 (halva_sdpa_branch_bwd_rope);
    // a row's position follows from its index and the branch points (rope_position below)
    const bf16_t* rope_cos;      // [max_pos, D / 2] bf16 tables of halva_rope_qk, or nullptr = dq / dk leave un-rotated
    const bf16_t* rope_sin;
    int rope_max_pos;            // rows of the tables
    int repair;           // sdpa_fwd_kernel behind sdpa_fwd3: redo only the row blocks that hold a valid row with a non-finite lse (choose_fwd)
};

// Two responses sharing one prefix are packed as [prefix | A | pad | B] in one sequence: B (rows >= b, b a multiple of 64 so
// that no 32-row strip and no 64-key tile straddles it) must not see [a, b) = A and the padding.  For a strip of B rows a
// key tile is therefore either untouched, wholly hidden (dropped), or cut at `a` - which is the ordinary "sequence ends at a"
// mask.  Without branch points a = b = INT_MAX and nothing changes.
struct Branch {
    int a, b;
};
__device__ __forceinline__ Branch load_branch(const SdpaParams& p, int s) {
    Branch br;
    br.a = p.br_a ? p.br_a[s] : 0x7fffffff;
    br.b = p.br_b ? p.br_b[s] : 0x7fffffff;
    return br;
}

// RoPE position of row t (index inside its T rows) of a sequence: its index - and for a branch-packed row [prefix | A | pad | B] the rows of B
// continue from the prefix (include/halva_hip.h, halva_sdpa_branch_fwd: "RoPE positions of branch B restart at br_a"; halva_amd/splice.py:pack_pairs)
__device__ __forceinline__ int rope_position(int t, const Branch& br) { return t >= br.b ? br.a + (t - br.b) : t; }

// Byte offset of 16-byte chunk `ch` of row `row` in a [rows][D] bf16 LDS tile.  The tile is cut into 8-row x 32-column
// subtiles of 512 B; inside a subtile the four chunks of a row are XOR-ed with (row >> 2) & 3.  Conflict-free for the
// ds_read_b128 row reads of an MFMA A/B operand and for ds_read_b64_tr_b16 transposed reads alike, and - unlike a
// whole-row XOR - every fragment address is one of TWO per-lane bases plus an immediate (ch >> 2 and row >> 3 only add
// multiples of 512 B), which keeps ~40 VGPRs of address arithmetic out of the main loops.
template <int D>
__device__ __forceinline__ int tile_off(int row, int ch) {
    constexpr int SUBROW = (D / 32) * 512;   // bytes of one 8-row band
    return SUBROW * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

__device__ __forceinline__ f32x16 mfma32(const s16x8& a, const s16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// A/B fragment of a row-major tile: lane (r = lane & 31, h = lane >> 5) gets row (row0 + r), elements 16*ks + 8*h .. +7
template <int D>
__device__ __forceinline__ s16x8 frag_rows(const char* tile, int row0, int ks, int lane) {
    const int r = row0 + (lane & 31);
    return *reinterpret_cast<const s16x8*>(tile + tile_off<D>(r, 2 * ks + (lane >> 5)));
}

// Transposed fragment for a product that sums over the tile's ROW index with an accumulator tile as the other
// operand.  Lane (c = lane & 31, h = lane >> 5) gets column (col0 + c) of rows
//   row0 + 8*jj + 4*h + e,  jj = 0,1, e = 0..3   (element j = 4*jj + e)
// which is exactly the row order of registers 8*s'..8*s'+7 of a 32x32 accumulator (row0 = 16*s' + tile base).
template <int D, bool SLOW>
__device__ __forceinline__ s16x8 frag_cols(const char* tile, int row0, int col0, int lane) {
    s16x8 out;
    if (SLOW) {
        const int c = col0 + (lane & 31), h = lane >> 5;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = row0 + 8 * (j >> 2) + 4 * h + (j & 3);
            out[j] = *reinterpret_cast<const short*>(tile + tile_off<D>(r, c >> 3) + (c & 7) * 2);
        }
    } else {
        // ds_read_b64_tr_b16: per 16-lane group a 4-row x 16-column block; lane 4q+p supplies the address of
        // row q, columns 4p..4p+3 and receives column (lane & 15), rows 0..3.
        const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3, h = g >> 1;
        const int c = col0 + 16 * (g & 1) + 4 * pp;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int r = row0 + 8 * jj + 4 * h + q;
            const int off = tile_off<D>(r, c >> 3) + (c & 7) * 2;
            const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(tile + off));
            out[4 * jj + 0] = t[0];
            out[4 * jj + 1] = t[1];
            out[4 * jj + 2] = t[2];
            out[4 * jj + 3] = t[3];
        }
    }
    return out;
}

// registers 8*s..8*s+7 of a 32x32 f32 accumulator -> bf16 fragment usable as the B (or A) operand
__device__ __forceinline__ s16x8 acc_to_frag(const f32x16& x, int s) {
    s16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (short)f32_to_bf16(x[8 * s + j]);
    return out;
}

// row index (0..31) inside a 32x32 accumulator tile of register `reg` on a lane of half h
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---------------------------------------------------------------------------------------------------
// softmax pieces of a [32 keys x 32 queries] score accumulator (the query on the lane, its other 16 keys on the lane 32 away)
// ---------------------------------------------------------------------------------------------------
// a row's exponent reference moves only when its maximum exceeds it by more than this (log2 units: P stays below 2^64, far inside fp32 /
// bf16 range)
constexpr float kRescaleAt = 64.f;

__device__ __forceinline__ float xhalf_max(float v) {   // max with the lane 32 away (v_permlane32_swap: no LDS round trip)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// keys at or beyond len, and under CAUSAL keys behind the lane's query ql, to -inf
template <bool MASK, bool CAUSAL>
__device__ __forceinline__ void mask_half(f32x16& st, int kbase, int h, int len, int ql) {
    if (!MASK) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int kl = kbase + acc_row(r, h);
        if (kl >= len || (CAUSAL && kl > ql)) st[r] = -INFINITY;
    }
}
__device__ __forceinline__ float half_max(const f32x16& st) {
    float a = fmaxf(st[0], st[1]), b = fmaxf(st[2], st[3]);
#pragma unroll
    for (int r = 4; r < 16; r += 4) {
        a = fmaxf(fmaxf(a, st[r]), st[r + 1]);
        b = fmaxf(fmaxf(b, st[r + 2]), st[r + 3]);
    }
    return fmaxf(a, b);
}

// ---------------------------------------------------------------------------------------------------
// cooperative tile staging: ROWS x D bf16, 256 threads, register staged
// ---------------------------------------------------------------------------------------------------
template <int D, int ROWS, int NT = 256>
struct Stage {
    static constexpr int NCH = D / 8;
    static constexpr int PER_THREAD = ROWS * NCH / NT;
    static_assert(ROWS * NCH % NT == 0, "tile must split evenly over the workgroup");
    u32x4 r[PER_THREAD];

    // rows outside [0, limit) read the nearest valid row (finite data; callers mask those rows): branch-free
    __device__ __forceinline__ void load_clamped(const bf16_t* base, int64_t ld, int64_t grow_local0, int local0, int limit) {
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const int cid = threadIdx.x + NT * i;
            const int row = cid / NCH, ch = cid % NCH;
            const int loc = min(max(local0 + row, 0), limit - 1);
            r[i] = *reinterpret_cast<const u32x4*>(base + (grow_local0 + loc) * ld + ch * 8);
        }
    }
    __device__ __forceinline__ void store(char* tile) const {
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const int cid = threadIdx.x + NT * i;
            const int row = cid / NCH, ch = cid % NCH;
            *reinterpret_cast<u32x4*>(tile + tile_off<D>(row, ch)) = r[i];
        }
    }
};

// Fill one [64][D] tile image (the tile_off layout) straight from global memory, no register staging: each
// global_load_lds_dwordx4 writes 1 KiB of LDS at (wave-uniform base + 16 * lane), so lane l of chunk c fetches the 16 bytes
// whose tile_off is 1024 c + 16 l - the swizzle is applied to the SOURCE address.  Rows outside [0, limit) read the nearest
// valid row, as Stage::load_clamped.  NW waves share the tile's chunks.
template <int D, int NW, int ROWS = 64>      // ROWS = 128: two consecutive 64-row images
__device__ __forceinline__ void stage_tile_dma(char* tile, const bf16_t* base, int64_t ld, int64_t grow_local0, int local0, int limit,
                                               int wave, int lane) {
    constexpr int CHUNKS = ROWS * D * 2 / 1024, SUBROW = (D / 32) * 512;
    static_assert(CHUNKS % NW == 0, "chunks must split evenly over the waves");
#pragma unroll
    for (int i = 0; i < CHUNKS / NW; ++i) {
        const int c = wave + NW * i;
        const int o = 1024 * c + 16 * lane;
        const int band = o / SUBROW, rem = o % SUBROW;
        const int row = 8 * band + ((rem % 512) >> 6);
        const int ch = 4 * (rem / 512) + (((rem >> 4) & 3) ^ ((row >> 2) & 3));
        const int loc = min(max(local0 + row, 0), limit - 1);
        const bf16_t* src = base + (grow_local0 + loc) * ld + ch * 8;
        // written as asm: the builtin makes hipcc drain vmcnt(0) before the next ds_read_b64_tr_b16, i.e. in the middle of the step
        const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(tile + 1024 * c);
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    }
}
// The same fill for a run of whole tiles 64 rows apart, with next to no per-lane state: a wave's chunks c = wave + NW i hold the same
// (row, chunk) pattern shifted by a whole number of rows, so ONE 32-bit lane offset serves all of them and the rest of the address -
// tile origin + that row shift - is scalar (the saddr form of the instruction).  No 64-bit vector arithmetic in the loop.
template <int D, int NW, int ROWS = 64>
struct TileDma {
    static constexpr int CHUNKS = ROWS * D * 2 / 1024, SUBROW = (D / 32) * 512, PER_WAVE = CHUNKS / NW;
    static_assert((1024 * NW) % SUBROW == 0, "chunks of one wave must differ by whole 8-row bands");
    static constexpr int ROWS_PER_I = 8 * (1024 * NW / SUBROW);
    unsigned voff;          // byte offset of this lane's 16 bytes of chunk `wave` from the tile's first row
    const char* origin;     // the next tile's first row (wave-uniform)
    __device__ __forceinline__ void init(const bf16_t* base, int64_t ld, int64_t grow_local0, int local0, int wave, int lane) {
        const int o = 1024 * wave + 16 * lane;
        const int band = o / SUBROW, rem = o % SUBROW;
        const int row = 8 * band + ((rem % 512) >> 6);
        const int ch = 4 * (rem / 512) + (((rem >> 4) & 3) ^ ((row >> 2) & 3));
        voff = (unsigned)((row * ld + ch * 8) * 2);
        origin = reinterpret_cast<const char*>(base + (grow_local0 + local0) * ld);
    }
    // fetch the tile at `origin` (all ROWS rows must exist), then move one tile down
    __device__ __forceinline__ void issue_and_advance(char* tile, int64_t ld, int wave) {
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            const unsigned dst = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(tile + 1024 * (wave + NW * i));
            const char* rows = origin + (int64_t)i * ROWS_PER_I * ld * 2;
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(voff), "s"(dst), "s"(rows) : "memory");
        }
        origin += ROWS * ld * 2;
    }
};
// the loads above are invisible to the compiler's counters: wait for them by hand before the barrier that publishes the tile
// (s_waitcnt vmcnt(0) as the builtin, not asm: the compiler then also knows that nothing of its own is pending afterwards)
__device__ __forceinline__ void stage_tile_dma_wait() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// Write a [D x 32] transposed accumulator (lane = row of the output, registers = columns d) as bf16 rows.  A lane holds the columns
// 32*dt + 8*g + 4*h + (0..3) of its row (h = lane / 32: the two lanes of a row sit 32 apart), i.e. 8-byte pieces: 16 stores per lane,
// and the store tail of a row block is bound by the NUMBER of store instructions (measured: ~5 600 cycles for a V-side wave of the
// dK/dV kernel, ~10 000 for the K-side wave that finishes last).  v_permlane32_swap trades the pieces of two neighbouring groups
// between the two lanes of a row, after which each holds 16 contiguous bytes: 8 stores per lane, same bytes, same addresses.
// the o / dq / dk / dv rows leave through this with plain stores: nontemporal ones measured sdpa_bwd_dq2 +4 %, sdpa_bwd_dkv3 +0.5 %,
// sdpa_fwd3 +0.6 % at the step's shapes (alternating runs, rocprofv3; DESIGN.md, "Retired kernel variants")
// one [32 x 32] tile of a transposed accumulator (columns 32 dt .. 32 dt + 31 of the lanes' rows): two 16-byte stores per lane
__device__ __forceinline__ void store_tile_T(bf16_t* row_ptr_dt, const f32x16& t, float mul, int h) {
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
        unsigned w[2][2];      // [group 2gp, 2gp+1][word]
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int g = 2 * gp + k;
            w[k][0] = pack_bf16x2(t[4 * g + 0] * mul, t[4 * g + 1] * mul);
            w[k][1] = pack_bf16x2(t[4 * g + 2] * mul, t[4 * g + 3] * mul);
        }
        // upper lanes' group-2gp words <-> lower lanes' group-(2gp+1) words
        const auto x = __builtin_amdgcn_permlane32_swap(w[0][0], w[1][0], false, false);
        const auto y = __builtin_amdgcn_permlane32_swap(w[0][1], w[1][1], false, false);
        *reinterpret_cast<u32x4*>(row_ptr_dt + 16 * gp + 8 * h) = u32x4{x[0], y[0], x[1], y[1]};
    }
}
template <int D>
__device__ __forceinline__ void store_rows_T(bf16_t* row_ptr, const f32x16 (&acc)[D / 32], float mul, bool valid, int lane) {
    if (!valid) return;      // (both lanes of a row take the same side: the swap below never pairs an active lane with an inactive one)
    const int h = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) store_tile_T(row_ptr + 32 * dt, acc[dt], mul, h);
}
// The same rows with the INVERSE RoPE applied on the way out (halva_sdpa_branch_bwd_rope): what halva_rope_qk(inverse = 1) would do to the
// stored row in a launch of its own - the row is rounded to bf16 first, rotated in fp32 with the bf16 table entries of its position, rounded
// again (rope_pair, common.h: the same expression as rope_qk_kernel).  Elements d and d + 64 of a row sit in the same lane, same register
// index, accumulator tiles dt and dt + 2.  cr / sr: this lane's row of the cos / sin tables ([D / 2] bf16).
// The table rows of a wave's 32 consecutive positions (pos0 .. pos0 + 31: a 32-row group never straddles a branch point) = 4 KiB of cos + 4 KiB of sin,
// CONTIGUOUS in the tables: fetched with four coalesced 16-byte loads per lane and table and handed to the lanes through `scratch` (9 KiB of LDS that
// only this wave touches, rows 144 bytes apart).  The first version let every lane gather its own row - 16 loads of 8 bytes per lane, 32 different
// 128-byte lines per instruction: +28 .. +40 us per sdpa_bwd_dq2 launch (profiles/r05_rope_cost.log).
constexpr int ROPE_LDS_ROW = 144, ROPE_LDS_BYTES = 2 * 32 * ROPE_LDS_ROW;
__device__ __forceinline__ void rope_rows_to_lds(char* scratch, const bf16_t* cos, const bf16_t* sin, int pos0, int max_pos, int lane) {
    typedef __attribute__((address_space(3))) char lchar;
    u32x4 c[4], sn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * i + (lane >> 3), ch = lane & 7;
        const int64_t at = (int64_t)min(pos0 + row, max_pos - 1) * 64 + ch * 8;
        c[i] = *reinterpret_cast<const u32x4*>(cos + at);
        sn[i] = *reinterpret_cast<const u32x4*>(sin + at);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 8 * i + (lane >> 3), ch = lane & 7;
        *reinterpret_cast<__attribute__((address_space(3))) u32x4*>((lchar*)(scratch + row * ROPE_LDS_ROW + ch * 16)) = c[i];
        *reinterpret_cast<__attribute__((address_space(3))) u32x4*>((lchar*)(scratch + 32 * ROPE_LDS_ROW + row * ROPE_LDS_ROW + ch * 16)) = sn[i];
    }
}
// The same rows with the INVERSE RoPE applied on the way out (halva_sdpa_branch_bwd_rope): what halva_rope_qk(inverse = 1) would do to the
// stored row in a launch of its own - the row is rounded to bf16 first, rotated in fp32 with the bf16 table entries of its position, rounded
// again (rope_pair, common.h: the same expression as rope_qk_kernel).  Elements d and d + 64 of a row sit in the same lane, same register
// index, accumulator tiles dt and dt + 2.  scratch: rope_rows_to_lds' block of this wave (row lane & 31 = this lane's row).
template <int D>
__device__ __forceinline__ void store_rows_T_rope(bf16_t* row_ptr, const f32x16 (&acc)[D / 32], float mul, bool valid, int lane, const char* scratch) {
    static_assert(D == 128, "the rotating store is the head_dim-128 instantiation");
    typedef __attribute__((address_space(3))) const char lchar;
    const int h = lane >> 5;
    lchar* cr = (lchar*)(scratch + (lane & 31) * ROPE_LDS_ROW + 8 * h);
    lchar* sr = cr + 32 * ROPE_LDS_ROW;
#pragma unroll
    for (int dtl = 0; dtl < 2; ++dtl) {
        f32x16 lo, hi;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const u32x2 cw = *reinterpret_cast<__attribute__((address_space(3))) const u32x2*>(cr + 64 * dtl + 16 * g);
            const u32x2 sw = *reinterpret_cast<__attribute__((address_space(3))) const u32x2*>(sr + 64 * dtl + 16 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c = (j & 1) ? bf16_hi(cw[j >> 1]) : bf16_lo(cw[j >> 1]);
                const float sn = (j & 1) ? bf16_hi(sw[j >> 1]) : bf16_lo(sw[j >> 1]);
                float y1, y2;
                rope_pair(bf16_round(acc[dtl][4 * g + j] * mul), bf16_round(acc[dtl + 2][4 * g + j] * mul), c, sn * -1.f, y1, y2);
                lo[4 * g + j] = y1, hi[4 * g + j] = y2;
            }
        }
        if (valid) {      // (both lanes of a row take the same side: the swap in store_tile_T never pairs an active lane with an inactive one)
            store_tile_T(row_ptr + 32 * dtl, lo, 1.f, h);
            store_tile_T(row_ptr + 32 * (dtl + 2), hi, 1.f, h);
        }
    }
}
template <int D>
__device__ __forceinline__ void store_rows_zero(bf16_t* row_ptr, int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<u32x2*>(row_ptr + 32 * dt + 8 * g + 4 * h) = u32x2{0u, 0u};
}

// Workgroup -> (sequence, head, row block).  1-D grid; workgroups are dealt round-robin over the 8 XCDs, so the blocks
// L, L+8, L+16, ... share an L2: give those the row blocks of ONE (sequence, head) pair, whose K/V (or Q/dO) tiles they all
// stream, heaviest (latest) block first under the causal mask.  Placement only changes speed, never results.
__device__ __forceinline__ void map_block(int L, int nblk, int H, int npairs, bool heavy_first, int& s, int& hd, int& blk) {
    int pair, o;
    if ((npairs & 7) == 0) {
        const int slot = L >> 3;
        pair = (slot / nblk) * 8 + (L & 7);
        o = slot % nblk;
    } else {
        pair = L / nblk;
        o = L % nblk;
    }
    blk = heavy_first ? nblk - 1 - o : o;
    hd = pair % H;
    s = pair / H;
}

// Which two 256-row blocks of a (sequence, head) pair a workgroup takes under the causal mask.  Plain causal: block b needs b + 1 units of
// key tiles, so b goes with nblk-1-b and every workgroup does nblk + 1 units.  A packed sequence [prefix | A | pad | B] breaks that: the blocks
// wholly inside B (first row >= br.b) do not visit the tiles inside [br.a, br.b), so their work is (b + 1) - hid with hid = (br.b - br.a) / 256 units -
// for the bench's row [668 | 1380 | 1380] the old pairing gave six workgroups of 37-39 units and one of 60 per pair, and the launch waited for
// the sixties.  Here the blocks are RANKED by that work (two increasing runs merged in closed form) and pair k takes the k-th heaviest and the
// k-th lightest (44 units at most in the example).  Without a branch the ranks are the block numbers: the old pairing.
__host__ __device__ __forceinline__ int block_rank(int qb, int n1, int n2, int hid) {      // n1 blocks below br.b, n2 inside B
    if (qb < n1) return qb + min(max(qb - n1 + hid, 0), n2);
    const int j = qb - n1;
    return j + min(max(n1 + j - hid + 1, 0), n1);
}
__host__ __device__ __forceinline__ void paired_blocks(int nblk, int start, const Branch& br, int k, int& heavy, int& light) {
    int n1 = nblk, hid = 0;
    if (br.b != 0x7fffffff && br.b > br.a) {
        n1 = (br.b + start + 255) / 256;      // first block whose first row is >= br.b (local rows: row - start)
        n1 = n1 < nblk ? n1 : nblk;
        hid = (br.b - br.a + 128) / 256;
    }
    const int n2 = nblk - n1, want_h = nblk - 1 - k, want_l = k;
    heavy = nblk - 1 - k, light = k;
    if (n2 == 0 || hid == 0) return;
    for (int qb = 0; qb < nblk; ++qb) {
        const int r = block_rank(qb, n1, n2, hid);
        if (r == want_h) heavy = qb;
        if (r == want_l) light = qb;
    }
}

// The LoRA weight gradients of gemm.hip (included there after gemm_tile.h, inside its anonymous namespace; not compiled alone): the tile body, the
// two table kernels (tiles, reduction), the four-stage A/B wrapper, the slab planner, and the one host path every call takes (wgrad_run).
// Round 4: the TN form for the LoRA weight gradients (halva_wgrad_accumulate: C[M, N] f32 += A^T B over `rows`, A [rows, M] and B [rows, N] column
// windows of row-major activations, M and N multiples of 128) with the operand tiles brought in by LDS-DMA instead of through registers:
//   * a k-tile = 64 rows of 128 columns (256 bytes each) per operand = sixteen 1-KiB pieces of four rows; wave w requests pieces w, w + 4, w + 8,
//     w + 12 of both operands with `buffer_load_dwordx4 ... offen lds` through a bounds-checked descriptor over the k-slab (a row past the slab
//     arrives as ZEROS: no tail case; experiments/fwd3/oob_probe.hip) - no staging registers, no ds_write (8 x 13 cycles per thread and tile before);
//   * the LDS image keeps the XOR swizzle of Operand<true> (its ds_read_b64_tr_b16 fragments are conflict-free on it): LDS-DMA writes lane l
//     to byte 16 l of the piece, so the swizzle is applied to WHICH chunk of its row a lane fetches - constant per wave (piece & 3 == wave);
//   * two stages (64 KiB: two workgroups per CU): iteration t waits for its own requests of tile t, barrier (tile t complete for everyone; everyone
//     has finished tile t - 1), requests tile t + 1 into the other stage, multiplies tile t.
// Same arithmetic and summation order inside a slab as gemm_kernel<true, true>: bitwise the same partials.
// KT = 64: two stages, one tile in flight per workgroup while it multiplies.  KT = 32: FOUR stages of half the height - tile t + 3 is requested
// when tile t has landed, so three tiles (48 KiB per workgroup) stay in flight all the time, at twice the barriers (HALVA_WGRAD_KT=32).
// (the body of one workgroup = one [128 x 128] tile of one k-slab: bx / by / bz = the tile's column, row and slab - blockIdx of the single-problem launch,
// decoded from a linear index by the batched one)
template <int KT, int NT_MODE>      // NT_MODE bit 0: A streamed nontemporally, bit 1: B (see `request`)
__device__ __forceinline__ void wgrad_dma_body(const GemmParams& p, int bx, int by, int bz, char* smem) {
    constexpr int TILE = 128 * KT * 2, NST = 128 / KT, PPW = KT / 16;      // bytes of an operand tile; stages; 1-KiB pieces per wave and operand
    char* a_lds = smem;                 // [NST][TILE]
    char* b_lds = smem + NST * TILE;    // [NST][TILE]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = by * 128, n0 = bx * 128;
    const int64_t kb = (int64_t)bz * p.ksplit;
    const int K = (int)min((int64_t)p.ksplit, p.K - kb);
    const int nk = (K + KT - 1) / KT;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // descriptors over the slab's rows of this tile's 128 columns: base, stride 0, bytes up to the end of the last row's 128 columns, raw dwords
    auto desc = [&](const bf16_t* base, int64_t ld) {
        const uint64_t a = (uint64_t)(size_t)base;
        u32x4 d;
        d[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
        d[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
        d[2] = __builtin_amdgcn_readfirstlane((unsigned)(((int64_t)(K - 1) * ld + 128) * 2));
        d[3] = 0x00020000u;
        return d;
    };
    const u32x4 da = desc(p.A + kb * p.lda + m0, p.lda), db = desc(p.B + kb * p.ldb + n0, p.ldb);
    // lane (row l >> 4 of the piece, position l & 15) fetches chunk (position ^ swizzle(row)) of its row: off128's image
    const int prow = lane >> 4, chunk = (lane & 15) ^ ((prow << 2) | wave);
    const unsigned voa = (unsigned)(prow * p.lda * 2 + chunk * 16), vob = (unsigned)(prow * p.ldb * 2 + chunk * 16);
    const unsigned lds_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)a_lds, lds_b = (unsigned)(size_t)(__attribute__((address_space(3))) char*)b_lds;
    auto request = [&](int it, int stage) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int piece = wave + 4 * i;
            const unsigned sa = (unsigned)(((int64_t)it * KT + 4 * piece) * p.lda * 2), sb = (unsigned)(((int64_t)it * KT + 4 * piece) * p.ldb * 2);
            const unsigned dst_a = lds_a + stage * TILE + piece * 1024, dst_b = lds_b + stage * TILE + piece * 1024;
            // An operand whose 128-column slab is read by ONE workgroup of the grid (the wide side of a LoRA factor's gradient: gridDim.x == 1 for A,
            // gridDim.y == 1 for B: NT_MODE, chosen by the launcher) is streamed nontemporally - read once, it would only push the other operand's slab, which every workgroup of the
            // row / column re-reads, out of the L2 (round 5: the row kernels gained 6-16 % from the same policy, experiments/rowops_stream).
            unsigned keep;
#define WGRAD_REQ(NTA, NTB)                                                                                                                  \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %7 offen" NTA " lds\n\t"                  \
                 "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %4, %8 offen" NTB " lds\n\ts_mov_b32 m0, %0"                      \
                 : "=&s"(keep) : "v"(voa), "v"(vob), "s"(da), "s"(db), "s"(dst_a), "s"(dst_b), "s"(sa), "s"(sb) : "memory")
            if constexpr (NT_MODE == 0) WGRAD_REQ("", "");
            else if constexpr (NT_MODE == 1) WGRAD_REQ(" nt", "");
            else if constexpr (NT_MODE == 2) WGRAD_REQ("", " nt");
            else WGRAD_REQ(" nt", " nt");
#undef WGRAD_REQ
        }
    };
    // NST - 1 tiles ahead (every wave issues 2 PPW requests per tile, whether the tile exists or not: rows past the slab bring zeros and the
    // counted wait stays the same to the end)
#pragma unroll
    for (int t = 0; t < NST - 1; ++t) request(t, t);
#pragma unroll 1
    for (int it = 0; it < nk; ++it) {
        // tile `it` is complete for every wave (the NST - 2 younger tiles may stay in flight); every wave is through with tile it - 1
        if (NST == 2) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");      // (NST = 4: 2 tiles x 4 requests)
        request(it + NST - 1, (it + NST - 1) % NST);
        const char* at = a_lds + (it % NST) * TILE;
        const char* bt = b_lds + (it % NST) * TILE;
#pragma unroll
        for (int ks = 0; ks < KT / 16; ++ks) {
            s16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = Operand<true>::frag(at, 64 * wm + 32 * i, ks, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = Operand<true>::frag(bt, 64 * wn + 32 * j, ks, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i]),
                                                                       __builtin_bit_cast(bf16x8, bf[j]), acc[i][j], 0, 0, 0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the requests past the slab's end)
    float* cz = (float*)p.C + (int64_t)bz * p.M * p.ldc;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 64 * wn + 32 * j + (lane & 31);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + 64 * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                cz[(int64_t)m * p.ldc + n] = acc[i][j][r];
            }
    }
}
template <int KT, int NT_MODE>      // (only the four-stage A/B form, <32, 0>, is launched by itself: KT = 64 goes through the table kernel below)
__global__ __launch_bounds__(256, 2) void wgrad_dma_kernel(const GemmParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    wgrad_dma_body<KT, NT_MODE>(p, blockIdx.x, blockIdx.y, blockIdx.z, smem);
}

// Round 6: the weight gradients of ONE LoRA group - its A factor and its one to three B factors, two to four products that
// become available together in the group's backward (halva_amd/llama.py:_LoraGroupLinear) - as ONE launch of the tile kernel and ONE of the reduction
// instead of two launches per factor (1 408 -> 512 per bench step): every workgroup finds its problem from a prefix table in the kernel arguments and
// runs the body on it.  Every product's k-slabs are planned by itself (wgrad_slabs over the whole workspace), so the partials, their order and the
// results are BITWISE the same whether products share a call or not (tests/test_gemm_elementwise_gpu.py).  What it saves is kernel boundaries
// (each one drains and refills the chip), not work.
constexpr int WGRAD_BATCH_MAX = 4;
struct WgradBatch {
    GemmParams p[WGRAD_BATCH_MAX];      // p[q].C: the partials of problem q in the workspace
    float* C[WGRAD_BATCH_MAX];
    float alpha[WGRAD_BATCH_MAX];
    int64_t mn[WGRAD_BATCH_MAX];
    int splits[WGRAD_BATCH_MAX], nt_mode[WGRAD_BATCH_MAX], gx[WGRAD_BATCH_MAX], gy[WGRAD_BATCH_MAX];
    int first_block[WGRAD_BATCH_MAX + 1];       // prefix sums of gx * gy * splits
    int first_rblock[WGRAD_BATCH_MAX + 1];      // prefix sums of the reduction's blocks (1 024 elements each)
    int n;
};
__global__ __launch_bounds__(256, 2) void wgrad_dma_batch_kernel(const WgradBatch b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int q = 0;
    while (q + 1 < b.n && (int)blockIdx.x >= b.first_block[q + 1]) ++q;      // (uniform: scalar loads from the kernel arguments)
    const int i = (int)blockIdx.x - b.first_block[q], gx = b.gx[q], gy = b.gy[q];
    const int bx = i % gx, by = (i / gx) % gy, bz = i / (gx * gy);
    const GemmParams& p = b.p[q];
    switch (b.nt_mode[q]) {
    case 0: wgrad_dma_body<64, 0>(p, bx, by, bz, smem); break;
    case 1: wgrad_dma_body<64, 1>(p, bx, by, bz, smem); break;
    case 2: wgrad_dma_body<64, 2>(p, bx, by, bz, smem); break;
    default: wgrad_dma_body<64, 3>(p, bx, by, bz, smem); break;
    }
}

// C[i] += alpha * sum_z ws[z][i]  (fixed order: the split-k weight gradients stay bitwise reproducible)
__global__ __launch_bounds__(256) void splitk_reduce_batch_kernel(const WgradBatch b) {
    int q = 0;
    while (q + 1 < b.n && (int)blockIdx.x >= b.first_rblock[q + 1]) ++q;
    const int64_t i = ((int64_t)((int)blockIdx.x - b.first_rblock[q]) * 256 + threadIdx.x) * 4, mn = b.mn[q];
    if (i >= mn) return;
    const float* ws = (const float*)b.p[q].C;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < b.splits[q]; ++z) s += *reinterpret_cast<const f32x4*>(ws + z * mn + i);
    f32x4* c = reinterpret_cast<f32x4*>(b.C[q] + i);
    *c = *c + s * b.alpha[q];
}

// the k-slabs of one weight-gradient product: as many as keep the whole grid resident at once (2 workgroups per CU x 256 CUs): a second, partial
// round of workgroups costs more than the extra parallelism brings (measured at 256..1536 workgroups, tools/bench_wgrad.py)
static void wgrad_slabs(int M, int N, int64_t rows, int64_t ws_floats, int& splits, int& ksplit) {
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    const int64_t mn = (int64_t)M * N;
    splits = (int)max((int64_t)1, min((int64_t)min(64, 512 / tiles), ws_floats / mn));
    ksplit = (int)(((rows + splits - 1) / splits + 63) / 64 * 64);
    splits = (int)((rows + ksplit - 1) / ksplit);
}
static bool wgrad_dma_ok(int M, int N, int64_t lda, int64_t ldb, int ksplit) {      // HALVA_WGRAD_DMA=0: the register-staged gemm_kernel<true, true> of rounds 2-3 (also what odd shapes take)
    const char* e_dma = getenv("HALVA_WGRAD_DMA");
    const int64_t slab_bytes = (int64_t)ksplit * (lda > ldb ? lda : ldb) * 2;
    return !(e_dma && e_dma[0] == '0') && M % 128 == 0 && N % 128 == 0 && slab_bytes < (1ll << 31);
}

// Host side: every call of the two C entry points is validated, planned and launched here.
int wgrad_check_item(int q, const halva_wgrad_item& it, int64_t ws_floats) {
    HALVA_CHECK_ARG(it.A && it.B && it.C, "wgrad_accumulate: item %d: null pointer", q);
    HALVA_CHECK_ARG(it.M > 0 && it.N > 0 && it.rows > 0 && it.rows < (1ll << 31), "wgrad_accumulate: item %d: bad sizes %d %d %lld", q, it.M, it.N,
                    (long long)it.rows);
    HALVA_CHECK_ARG(it.M % 8 == 0 && it.N % 8 == 0 && it.lda % 8 == 0 && it.ldb % 8 == 0 && it.lda >= it.M && it.ldb >= it.N,
                    "wgrad_accumulate: item %d: M, N, lda, ldb must be multiples of 8 and the strides cover the columns", q);
    HALVA_CHECK_ARG((((uintptr_t)it.A | (uintptr_t)it.B | (uintptr_t)it.C) & 15) == 0, "wgrad_accumulate: item %d: 16-byte aligned pointers", q);
    HALVA_CHECK_ARG(ws_floats >= (int64_t)it.M * it.N, "wgrad_accumulate: item %d: workspace of %lld floats, need at least M * N = %lld", q,
                    (long long)ws_floats, (long long)it.M * it.N);
    return HALVA_OK;
}

// appends one product, with its partials at `part`, to a table (gx, gy, nt_mode and first_block are read by the LDS-DMA table kernel only)
void wgrad_append(WgradBatch& b, const halva_wgrad_item& it, float* part, int splits, int ksplit) {
    const int q = b.n++;
    GemmParams& p = b.p[q];
    p.A = (const bf16_t*)it.A, p.B = (const bf16_t*)it.B, p.C = part;
    p.lda = it.lda, p.ldb = it.ldb, p.ldc = it.N, p.M = it.M, p.N = it.N, p.K = (int)it.rows, p.out_f32 = 1, p.ksplit = ksplit;
    b.C[q] = it.C, b.alpha[q] = it.alpha, b.mn[q] = (int64_t)it.M * it.N, b.splits[q] = splits, b.gx[q] = (it.N + 127) / 128, b.gy[q] = (it.M + 127) / 128;
    b.nt_mode[q] = (b.gx[q] == 1 ? 1 : 0) | (b.gy[q] == 1 ? 2 : 0);
    b.first_block[q + 1] = b.first_block[q] + b.gx[q] * b.gy[q] * splits;
    b.first_rblock[q + 1] = b.first_rblock[q] + (int)((b.mn[q] / 4 + 255) / 256);
}

constexpr size_t WGRAD_LDS = 4 * 128 * 64 * 2;      // all stages of both operands, KT = 64 and KT = 32 alike
template <typename Kern, typename Arg>
int wgrad_launch_dma(Kern kern, dim3 grid, const Arg& arg, hipStream_t st) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WGRAD_LDS);
    hipLaunchKernelGGL(kern, grid, dim3(256), WGRAD_LDS, st, arg);
    HALVA_CHECK_LAUNCH("wgrad_dma");
    return HALVA_OK;
}
int wgrad_launch_table(const WgradBatch& b, hipStream_t st) { return wgrad_launch_dma(wgrad_dma_batch_kernel, dim3((unsigned)b.first_block[b.n]), b, st); }

// 1. every item is checked before anything is launched: a call that fails has touched no C.
// 2. every item gets the k-slabs it would get alone (wgrad_slabs over the WHOLE workspace: the bits do not depend on what shares the call) and its
//    tile kernel; the items are cut greedily, in order, into chunks of at most WGRAD_BATCH_MAX whose partials fit the workspace side by side (an
//    item alone always fits: wgrad_slabs plans no more slabs than the workspace holds).
// 3. per chunk: ONE launch of the table kernel when every item takes the LDS-DMA kernel with KT = 64 (the training step's launch), else one tile
//    kernel per item into its region of the workspace; then ONE launch of the reduction over the chunk's table.
int wgrad_run(int n, const halva_wgrad_item* items, float* ws, int64_t ws_floats, hipStream_t st) {
    HALVA_CHECK_ARG(n > 0 && items && ws, "wgrad_accumulate: no items / null pointer");
    HALVA_CHECK_ARG(((uintptr_t)ws & 15) == 0, "wgrad_accumulate: 16-byte aligned workspace");
    int rc;
    for (int q = 0; q < n; ++q)
        if ((rc = wgrad_check_item(q, items[q], ws_floats)) != HALVA_OK) return rc;
    const char* e_kt = getenv("HALVA_WGRAD_KT");
    const bool kt32 = e_kt && atoi(e_kt) == 32;
    enum Tile { DMA64, DMA32, STAGED };      // STAGED: the register-staged gemm_kernel<true, true>
    for (int q0 = 0; q0 < n;) {
        WgradBatch b{};
        Tile tile[WGRAD_BATCH_MAX];
        bool all_dma64 = true;
        int64_t ws_at = 0;
        while (b.n < WGRAD_BATCH_MAX && q0 + b.n < n) {
            const halva_wgrad_item& it = items[q0 + b.n];
            int splits, ksplit;
            wgrad_slabs(it.M, it.N, it.rows, ws_floats, splits, ksplit);
            const int64_t part = (int64_t)splits * it.M * it.N;
            if (b.n > 0 && ws_at + part > ws_floats) break;
            tile[b.n] = !wgrad_dma_ok(it.M, it.N, it.lda, it.ldb, ksplit) ? STAGED : kt32 ? DMA32 : DMA64;
            all_dma64 = all_dma64 && tile[b.n] == DMA64;
            wgrad_append(b, it, ws + ws_at, splits, ksplit);
            ws_at += (part + 3) / 4 * 4;
        }
        if (all_dma64) {
            if ((rc = wgrad_launch_table(b, st)) != HALVA_OK) return rc;
        } else {
            for (int q = 0; q < b.n; ++q) {
                if (tile[q] == DMA64) {
                    WgradBatch one{};
                    wgrad_append(one, items[q0 + q], (float*)b.p[q].C, b.splits[q], b.p[q].ksplit);
                    rc = wgrad_launch_table(one, st);
                } else {
                    const GemmParams& p = b.p[q];
                    rc = tile[q] == DMA32 ? wgrad_launch_dma(wgrad_dma_kernel<32, 0>, dim3(p.N / 128, p.M / 128, b.splits[q]), p, st) : launch_gemm<true, true>(p, st);
                }
                if (rc != HALVA_OK) return rc;
            }
        }
        hipLaunchKernelGGL(splitk_reduce_batch_kernel, dim3((unsigned)b.first_rblock[b.n]), dim3(256), 0, st, b);
        HALVA_CHECK_LAUNCH("splitk_reduce_batch");
        q0 += b.n;
    }
    return HALVA_OK;
}

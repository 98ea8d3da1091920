// The dense bf16 products outside the library GEMMs, on v_mfma_f32_32x32x16_bf16, and the small passes that go with them.  This file is their one
// translation unit: the two tile-kernel families live in the headers included below (inside one anonymous namespace; neither is compiled alone),
// the C ABI - argument checks and launches - and the small kernels follow here.
//   gemm_tile.h   halva_gemm_bf16: C[M,N] = epi( opA(A) @ opB(B)^T + bias ), NN / NT / TN - the mm_projector MLP (fwd: bias + GELU epilogue; bwd) and
//                 the patch-embeds of CLIP / SigLIP (im2col + GEMM)
//   wgrad.h       halva_wgrad_accumulate(_batch): the LoRA weight gradients C[M,N] f32 += alpha A^T B over all token rows, one planned launch path
//   here          im2col, gelu_bwd, colsum, halva_lora_merge (the load-time W += scale B A), halva_transpose_bf16
#include "common.h"
#include <cstdlib>

namespace {

#include "gemm_tile.h"
#include "wgrad.h"

// images [n, 3, hw, hw] bf16 -> col [n * (hw/p)^2, Kp] bf16, k = (c, ky, kx), zero padded to Kp
__global__ __launch_bounds__(256) void im2col_kernel(const bf16_t* __restrict__ img, bf16_t* __restrict__ col, int n, int hw,
                                                     int p, int Kp, int64_t total) {
    const int np1 = hw / p, K = 3 * p * p;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int k = (int)(i % Kp);
        const int64_t row = i / Kp;
        bf16_t v = 0;
        if (k < K) {
            const int px = (int)(row % np1), py = (int)((row / np1) % np1);
            const int64_t b = row / ((int64_t)np1 * np1);
            const int c = k / (p * p), ky = (k / p) % p, kx = k % p;
            v = img[((b * 3 + c) * hw + (py * p + ky)) * hw + px * p + kx];
        }
        col[i] = v;
    }
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ hpre,
                                                       bf16_t* __restrict__ dh, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const float x = bf16_to_f32(hpre[i]);
        const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
        const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
        dh[i] = f32_to_bf16(bf16_to_f32(dy[i]) * (cdf + x * pdf));
    }
}

// out[n] += sum_m x[m][n]; grid (ceil(N/256), splits); each block sums a slab of rows, one atomic per column
__global__ __launch_bounds__(256) void colsum_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, int64_t M, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int64_t per = (M + gridDim.y - 1) / gridDim.y;
    const int64_t lo = blockIdx.y * per, hi = lo + per < M ? lo + per : M;
    float s = 0.f;
    for (int64_t m = lo; m < hi; ++m) s += bf16_to_f32(x[m * N + n]);
    atomicAdd(out + n, s);
}

// ---------------------------------------------------------------------------------------------------
// halva_lora_merge: w[n, k] <- bf16( w[n, k] + scale * sum_j B[n, j] A[j, k] ) in place on a strided window of a fused weight - a load-time
// pass whose whole cost is reading and writing w once, so: no LDS, no pipeline, one plain tile per wave.
// Workgroup = 4 waves over a [32 n x 256 k] tile, wave w the 64 columns from 64 w on, as two 32x32x16 MFMA tiles.  The MFMA's row index is the
// k of w and its column index the n, with rows PERMUTED so that the 16 accumulator registers of a lane are 16 CONSECUTIVE k of one weight row:
// MFMA row i = 8 q + 4 h + e (q = i >> 3, h = (i >> 2) & 1, e = i & 3) stands for column 16 h + 4 q + e of the tile, so lane (n = lane & 31,
// h = lane >> 5) holds columns 16 h + (4 q + e) = 16 h + reg in acc[reg]: two 16-byte loads and two 16-byte stores of w per lane and tile.
// The A fragment (LoRA A^T: k on the row, j contracted) is gathered element by element from [r, K] (one j per load; A is at most r x K, L2-resident),
// the B fragment is one 16-byte load of B[n, 8 h' ..] where the factor's rows allow it.  j runs in steps of 16 in ascending order, zero-filled past r:
// one fixed summation order, no split, no atomics - the same bits on every run.
struct MergeParams {
    bf16_t* w;
    const bf16_t* B;
    const bf16_t* A;
    int64_t ldw, ldb, lda;
    int N, K, r;
    float scale;
    int w_vec, b_vec;      // 16-byte accesses allowed on w / B (base pointer and row stride aligned)
};

__device__ __forceinline__ bf16_t merge_one(bf16_t w, float acc, float scale) {
    const float u = scale * acc;
    return u == 0.f ? w : f32_to_bf16(bf16_to_f32(w) + u);      // (a zero update keeps the weight's own bits, -0 and NaN payloads included)
}

__global__ __launch_bounds__(256) void lora_merge_kernel(const MergeParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int n = blockIdx.y * 32 + c;
    const int kw = blockIdx.x * 256 + wave * 64;      // this wave's first column
    if (kw >= p.K) return;
    const bool n_ok = n < p.N;
    // the column of w that MFMA row (lane & 31) of tile t stands for: kw + 32 t + krow
    const int krow = 16 * ((c >> 2) & 1) + 4 * (c >> 3) + (c & 3);
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    const bf16_t* brow = p.B + (int64_t)n * p.ldb;
    for (int j0 = 0; j0 < p.r; j0 += 16) {
        const int jl = j0 + 8 * h;      // this lane's 8 values of j
        s16x8 bfrag = {0, 0, 0, 0, 0, 0, 0, 0};
        if (n_ok) {
            if (p.b_vec && jl + 8 <= p.r) {
                bfrag = *reinterpret_cast<const s16x8*>(brow + jl);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (jl + e < p.r) bfrag[e] = (short)brow[jl + e];
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = kw + 32 * t + krow;
            s16x8 afrag = {0, 0, 0, 0, 0, 0, 0, 0};
            if (k < p.K) {
                const bf16_t* acol = p.A + (int64_t)jl * p.lda + k;
                if (jl + 8 <= p.r) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) afrag[e] = (short)acol[(int64_t)e * p.lda];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (jl + e < p.r) afrag[e] = (short)acol[(int64_t)e * p.lda];
                }
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, afrag), __builtin_bit_cast(bf16x8, bfrag), acc[t], 0, 0, 0);
        }
    }
    if (!n_ok) return;
    bf16_t* wrow = p.w + (int64_t)n * p.ldw;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k0 = kw + 32 * t + 16 * h;      // acc[t][i] <-> column k0 + i
        if (k0 >= p.K) continue;
        if (p.w_vec && k0 + 16 <= p.K) {
            u32x4* wp = reinterpret_cast<u32x4*>(wrow + k0);
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                u32x4 x = wp[v];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const unsigned lo = merge_one((bf16_t)(x[d] & 0xffffu), acc[t][8 * v + 2 * d], p.scale);
                    const unsigned hi = merge_one((bf16_t)(x[d] >> 16), acc[t][8 * v + 2 * d + 1], p.scale);
                    x[d] = lo | (hi << 16);
                }
                wp[v] = x;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (k0 + i < p.K) wrow[k0 + i] = merge_one(wrow[k0 + i], acc[t][i], p.scale);
        }
    }
}

}  // namespace

extern "C" int halva_gemm_bf16(const void* A, const void* B, const void* bias, void* C, void* pre_act, int M, int N, int K,
                               int trans_a, int trans_b, int epilogue, halva_dtype out_dtype, int accumulate, void* stream) {
    HALVA_CHECK_ARG(A && B && C, "gemm_bf16: null pointer");
    HALVA_CHECK_ARG(M > 0 && N > 0 && K > 0, "gemm_bf16: bad sizes %d %d %d", M, N, K);
    HALVA_CHECK_ARG(epilogue == 0 || epilogue == 1, "gemm_bf16: unknown epilogue %d", epilogue);
    // 16-byte row chunks: the contiguous dimension of every operand must be a multiple of 8 elements
    HALVA_CHECK_ARG((trans_a ? M : K) % 8 == 0, "gemm_bf16: contiguous dim of A must be a multiple of 8");
    HALVA_CHECK_ARG((trans_b ? N : K) % 8 == 0, "gemm_bf16: contiguous dim of B must be a multiple of 8");
    HALVA_CHECK_ARG(!(trans_a && !trans_b), "gemm_bf16: (trans_a, !trans_b) is not used on this path");
    GemmParams p{};
    p.A = (const bf16_t*)A;
    p.B = (const bf16_t*)B;
    p.bias = (const bf16_t*)bias;
    p.C = C;
    p.pre = pre_act;
    p.lda = trans_a ? M : K;
    p.ldb = trans_b ? N : K;
    p.ldc = N;
    p.M = M;
    p.N = N;
    p.K = K;
    p.epilogue = epilogue;
    p.out_f32 = out_dtype == HALVA_F32;
    p.accumulate = accumulate;
    if (!trans_a && !trans_b) return launch_gemm<false, false>(p, (hipStream_t)stream);
    if (!trans_a && trans_b) return launch_gemm<false, true>(p, (hipStream_t)stream);
    return launch_gemm<true, true>(p, (hipStream_t)stream);
}

extern "C" int halva_wgrad_accumulate_batch(int n, const halva_wgrad_item* items, float* ws, int64_t ws_floats, void* stream) {
    return wgrad_run(n, items, ws, ws_floats, (hipStream_t)stream);
}

extern "C" int halva_wgrad_accumulate(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int M, int N, int64_t rows,
                                      float alpha, float* ws, int64_t ws_floats, void* stream) {
    halva_wgrad_item it{};
    it.A = A, it.lda = lda, it.B = B, it.ldb = ldb, it.C = C, it.M = M, it.N = N, it.rows = rows, it.alpha = alpha;
    return halva_wgrad_accumulate_batch(1, &it, ws, ws_floats, stream);
}

extern "C" int halva_vit_patch_embed(const void* images, const void* weight_kp, const void* bias, void* col_ws, void* out, int n,
                                     int hw, int p, int d, int Kp, void* stream) {
    HALVA_CHECK_ARG(images && weight_kp && col_ws && out, "vit_patch_embed: null pointer");
    HALVA_CHECK_ARG(n > 0 && p > 0 && hw >= p, "vit_patch_embed: bad image/patch size");
    HALVA_CHECK_ARG(Kp % 8 == 0 && Kp >= 3 * p * p, "vit_patch_embed: Kp=%d must be a multiple of 8 and >= 3*p*p", Kp);
    const int np = (hw / p) * (hw / p);   // 'valid' convolution: a trailing partial patch is dropped (384 = 27*14 + 6)
    const int64_t total = (int64_t)n * np * Kp;
    int64_t grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(im2col_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)images,
                       (bf16_t*)col_ws, n, hw, p, Kp, total);
    HALVA_CHECK_LAUNCH("im2col");
    return halva_gemm_bf16(col_ws, weight_kp, bias, out, nullptr, n * np, d, Kp, 0, 0, 0, HALVA_BF16, 0, stream);
}

extern "C" int halva_clip_patch_embed(const void* images, const void* weight_kp, void* col_ws, void* out, int n, int hw, int p,
                                      int d, int Kp, void* stream) {
    HALVA_CHECK_ARG(p > 0 && hw % p == 0, "clip_patch_embed: bad image/patch size");
    return halva_vit_patch_embed(images, weight_kp, nullptr, col_ws, out, n, hw, p, d, Kp, stream);
}

extern "C" int halva_gelu_bwd(const void* dy, const void* h, void* dh, int64_t M, int N, void* stream) {
    HALVA_CHECK_ARG(dy && h && dh, "gelu_bwd: null pointer");
    const int64_t total = M * N;
    if (total <= 0) return HALVA_OK;
    int64_t grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy,
                       (const bf16_t*)h, (bf16_t*)dh, total);
    HALVA_CHECK_LAUNCH("gelu_bwd");
    return HALVA_OK;
}

// dst[c][r] = src[r][c] for a [rows x cols] bf16 matrix with row strides ld_src / ld_dst (elements): 64 x 64 tiles through LDS (33-word rows:
// the transposed reads of a wave fall on different banks), 16-byte global loads and stores on both sides.
__global__ __launch_bounds__(256) void transpose_bf16_kernel(const bf16_t* __restrict__ src, int64_t ld_src, bf16_t* __restrict__ dst, int64_t ld_dst,
                                                             int rows, int cols) {
    __shared__ unsigned tile[64][33];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64, v = threadIdx.x & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (threadIdx.x >> 3) + 32 * i, gr = r0 + r, gc = c0 + 8 * v;
        u32x4 x = {0u, 0u, 0u, 0u};
        if (gr < rows && gc < cols) x = *reinterpret_cast<const u32x4*>(src + (int64_t)gr * ld_src + gc);
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[r][4 * v + j] = x[j];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = (threadIdx.x >> 3) + 32 * i, gc = c0 + c, gr = r0 + 8 * v;
        if (gc < cols && gr < rows) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned a = tile[8 * v + 2 * j][c >> 1], b = tile[8 * v + 2 * j + 1][c >> 1];
                o[j] = (c & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
            }
            *reinterpret_cast<u32x4*>(dst + (int64_t)gc * ld_dst + gr) = o;
        }
    }
}

extern "C" int halva_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols, void* stream) {
    HALVA_CHECK_ARG(src && dst, "transpose_bf16: null pointer");
    HALVA_CHECK_ARG(rows >= 0 && cols >= 0 && rows % 8 == 0 && cols % 8 == 0 && ld_src % 8 == 0 && ld_dst % 8 == 0 && ld_src >= cols && ld_dst >= rows,
                    "transpose_bf16: rows, cols and both row strides must be multiples of 8 (16-byte accesses); got %d x %d, strides %lld / %lld", rows,
                    cols, (long long)ld_src, (long long)ld_dst);
    HALVA_CHECK_ARG(((size_t)src | (size_t)dst) % 16 == 0, "transpose_bf16: 16-byte aligned pointers");
    if (rows == 0 || cols == 0) return HALVA_OK;
    hipLaunchKernelGGL(transpose_bf16_kernel, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, ld_src,
                       (bf16_t*)dst, ld_dst, rows, cols);
    HALVA_CHECK_LAUNCH("transpose_bf16");
    return HALVA_OK;
}

extern "C" int halva_lora_merge(void* w, int64_t ldw, const void* B, int64_t ldb, const void* A, int64_t lda, int N, int K, int r, float scale,
                                void* stream) {
    HALVA_CHECK_ARG(w && B && A, "lora_merge: null pointer");
    HALVA_CHECK_ARG(N > 0 && K > 0, "lora_merge: bad sizes N=%d K=%d", N, K);
    HALVA_CHECK_ARG(r >= 1, "lora_merge: rank r=%d must be at least 1", r);
    HALVA_CHECK_ARG(ldw >= K && lda >= K && ldb >= r, "lora_merge: row strides ldw=%lld lda=%lld ldb=%lld must cover K=%d, K and r=%d columns",
                    (long long)ldw, (long long)lda, (long long)ldb, K, r);
    MergeParams p{};
    p.w = (bf16_t*)w;
    p.B = (const bf16_t*)B;
    p.A = (const bf16_t*)A;
    p.ldw = ldw, p.ldb = ldb, p.lda = lda;
    p.N = N, p.K = K, p.r = r;
    p.scale = scale;
    p.w_vec = ((uintptr_t)w % 16 == 0) && ldw % 8 == 0;
    p.b_vec = ((uintptr_t)B % 16 == 0) && ldb % 8 == 0;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((K + 255) / 256, (N + 31) / 32), dim3(256), 0, (hipStream_t)stream, p);
    HALVA_CHECK_LAUNCH("lora_merge");
    return HALVA_OK;
}

extern "C" int halva_colsum(const void* x, float* out, int64_t M, int N, void* stream) {
    HALVA_CHECK_ARG(x && out, "colsum: null pointer");
    if (M <= 0 || N <= 0) return HALVA_OK;
    int splits = (int)((M + 127) / 128);
    if (splits > 64) splits = 64;
    hipLaunchKernelGGL(colsum_kernel, dim3((N + 255) / 256, splits), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, out, M,
                       N);
    HALVA_CHECK_LAUNCH("colsum");
    return HALVA_OK;
}

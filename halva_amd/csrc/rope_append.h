// RoPE + KV-cache append of ONE qkv row - the one routine behind rope_append_kernel (kvcache.hip: the step's row of sequence b at
// position lens[b], or row i of a block of rows at position lens[b] + i; behind a prefix, the tables come shifted by its length).
#pragma once
#include "common.h"

constexpr int kRopeChunks = 128 / 8;      // 16-byte pieces per head row (head_dim 128)

// row = [3, H, 128] of sequence b; the whole workgroup calls this with the same arguments.  q is rotated in place (rope_qk_kernel's
// arithmetic), the rotated k and the plain v go to slot p of the [B, H, Lcap, 128] caches.  The caller has checked 0 <= p < Lcap and
// p < rows of the cos / sin tables.
__device__ __forceinline__ void rope_append_row(u32x4* __restrict__ row, const u32x4* __restrict__ cosb, const u32x4* __restrict__ sinb,
                                                u32x4* __restrict__ kc, u32x4* __restrict__ vc, int b, int p, int H, int Lcap) {
    constexpr int CH = kRopeChunks / 2;          // 16-byte pieces per half head row
    for (int t = threadIdx.x; t < 2 * H * CH; t += blockDim.x) {
        const int c = t % CH;
        const int h = (t / CH) % H;
        const int part = t / (CH * H);          // 0 = q, 1 = k
        const int64_t base = (int64_t)(part * H + h) * kRopeChunks + c;
        float x1[8], x2[8], cs[8], sn[8], y1[8], y2[8];
        unpack8(row[base], x1);
        unpack8(row[base + CH], x2);
        unpack8(cosb[(int64_t)p * CH + c], cs);
        unpack8(sinb[(int64_t)p * CH + c], sn);
#pragma unroll
        for (int j = 0; j < 8; ++j) rope_pair(x1[j], x2[j], cs[j], sn[j], y1[j], y2[j]);
        if (part == 0) {
            row[base] = pack8(y1);
            row[base + CH] = pack8(y2);
        } else {
            u32x4* dst = kc + (((int64_t)b * H + h) * Lcap + p) * kRopeChunks + c;
            dst[0] = pack8(y1);
            dst[CH] = pack8(y2);
        }
    }
    for (int t = threadIdx.x; t < H * kRopeChunks; t += blockDim.x) {
        const int h = t / kRopeChunks, c = t % kRopeChunks;
        vc[(((int64_t)b * H + h) * Lcap + p) * kRopeChunks + c] = row[(int64_t)(2 * H + h) * kRopeChunks + c];
    }
}

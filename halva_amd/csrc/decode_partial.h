// The split-KV partial of ONE query row over ONE chunk of KC keys - the one routine behind the two partial passes of kvcache.hip
// (own_partial_kernel: a chunk of a row's own keys; prefix_partial_kernel: a chunk of a shared prefix row, held in registers once and
// served to every member of the workgroup's block).  The per-key arithmetic, the order of every sum and the
// record (m, l, o[128]) are therefore the same wherever a chunk is reduced.
#pragma once
#include "common.h"
#include <cmath>

constexpr int kDecD = 128;          // head_dim of the LLaVA-1.5 decoder
constexpr int kDecChunks = kDecD / 8;      // 16-byte pieces per head row
constexpr int kDecWaves = 4;        // waves per split-KV workgroup

// A workgroup's share of a chunk: 4 waves of KC / 4 keys each; a wave takes 4 keys per step, 16 lanes per key row (one 16-byte piece of K
// and V per lane, straight to VGPRs - all of the wave's K and V loads are issued before the first dot).
template <int KC>
struct DecChunkRegs {
    static constexpr int NI = KC / (4 * kDecWaves);       // steps of 4 keys per wave
    u32x4 kr[NI], vr[NI];

    // kb / vb: the (sequence, head) row of the cache + this lane's piece; keys [k0, k0 + KC) ∩ [0, len); slots at or beyond len are never read
    __device__ __forceinline__ void load(const u32x4* __restrict__ kb, const u32x4* __restrict__ vb, int k0, int len) {
        const int kw0 = first_key(k0);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = kw0 + 4 * i;
            kr[i] = key < len ? kb[(int64_t)key * kDecChunks] : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = kw0 + 4 * i;
            vr[i] = key < len ? vb[(int64_t)key * kDecChunks] : u32x4{0, 0, 0, 0};
        }
    }
    // As load(), with key t of the (member, head) row fetched from the slot of ANOTHER member: anc_row[t] names the member whose own slot t
    // holds the row (beam search's ancestry table, kvcache.hip:own_partial_kernel<256, true>).  kbase / vbase: the [M, H, Lown, 128] caches + this
    // lane's piece.  The 16 lanes of a key row read the same word of anc_row; the lane's NI words are loaded first, then all K, then all V.
    // The member index is clamped into [0, M): whatever the table holds, no address leaves the allocation.
    __device__ __forceinline__ void load_via(const u32x4* __restrict__ kbase, const u32x4* __restrict__ vbase, const int32_t* __restrict__ anc_row,
                                             int h, int H, int Lown, int M, int k0, int len) {
        const int kw0 = first_key(k0);
        int src[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = kw0 + 4 * i;
            src[i] = key < len ? min(max(anc_row[key], 0), M - 1) : 0;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = kw0 + 4 * i;
            kr[i] = key < len ? kbase[(((int64_t)src[i] * H + h) * Lown + key) * kDecChunks] : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int key = kw0 + 4 * i;
            vr[i] = key < len ? vbase[(((int64_t)src[i] * H + h) * Lown + key) * kDecChunks] : u32x4{0, 0, 0, 0};
        }
    }
    static __device__ __forceinline__ int first_key(int k0) {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        return k0 + w * (KC / kDecWaves) + (lane >> 4);
    }
};

// q8: this lane's 16-byte piece of the query row (piece lane & 15).  Scores in fp32 in the log2 domain (q pre-scaled by qscale =
// log2(e) / sqrt(D)).  The 4 waves combine in LDS in a fixed order; the chunk's (m, l, o[128]) go to record `slot` of the fp32 workspace.
// The whole workgroup calls this (it holds a barrier) with k0 < len; a caller that calls it again puts a barrier in between.
template <int KC>
__device__ __forceinline__ void decode_chunk_partial(u32x4 q8, const DecChunkRegs<KC>& ch, int k0, int len, float qscale, float* __restrict__ ws_o,
                                                     float* __restrict__ ws_ml, int64_t slot) {
    constexpr int NI = DecChunkRegs<KC>::NI;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sub = lane & 15;
    const int kw0 = DecChunkRegs<KC>::first_key(k0);
    float qf[8];
    unpack8(q8, qf);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] *= qscale;
    float s[NI];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        float f[8];
        unpack8(ch.kr[i], f);
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(qf[j], f[j], d);
        d += __shfl_xor(d, 8, 64);
        d += __shfl_xor(d, 4, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 1, 64);
        s[i] = (kw0 + 4 * i < len) ? d : -INFINITY;
        m = fmaxf(m, s[i]);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m != -INFINITY) {                          // (a wave whose keys all lie beyond len contributes nothing)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float p = exp2f(s[i] - m);
            float f[8];
            unpack8(ch.vr[i], f);
            l += p;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = fmaf(p, f[j], o[j]);
        }
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        o[j] += __shfl_xor(o[j], 16, 64);
        o[j] += __shfl_xor(o[j], 32, 64);
    }
    __shared__ float s_o[kDecWaves][kDecD];
    __shared__ float s_ml[kDecWaves][2];
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) s_o[w][sub * 8 + j] = o[j];
    }
    if (lane == 0) {
        s_ml[w][0] = m;
        s_ml[w][1] = l;
    }
    __syncthreads();
    if (threadIdx.x < kDecD) {
        const int d = threadIdx.x;
        float M = s_ml[0][0];                      // finite: key k0 < len belongs to wave 0
#pragma unroll
        for (int ww = 1; ww < kDecWaves; ++ww) M = fmaxf(M, s_ml[ww][0]);
        float acc = 0.f, L = 0.f;
#pragma unroll
        for (int ww = 0; ww < kDecWaves; ++ww) {
            const float f = s_ml[ww][0] == -INFINITY ? 0.f : exp2f(s_ml[ww][0] - M);
            acc = fmaf(f, s_o[ww][d], acc);
            L = fmaf(f, s_ml[ww][1], L);
        }
        ws_o[slot * kDecD + d] = acc;
        if (d == 0) {
            ws_ml[slot * 2] = M;
            ws_ml[slot * 2 + 1] = L;
        }
    }
}

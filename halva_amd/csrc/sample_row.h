// The row machinery of the token selects (sample.hip, contrast.hip) on gfx950: one workgroup of 1024 lanes holds a row of up to 32768 fp32
// values in registers (32 per lane) and picks one column under temperature / top-k / top-p.
//
// No sort.  Both cuts are thresholds on the order-preserving uint32 image of the scaled value, found by bisection: top-k is the smallest
// key t with #{key > t} < k (counts: wave ballots, then 16 wave counts summed in wave order), top-p the smallest key t with
// sum_{key > t} e < top_p * Z1 (sums: each lane's 32 values in index order, the wave's butterfly, the 16 waves in wave order).  Both
// predicates are monotone in t also in fp32 (a rounded sum of non-negative terms in a fixed order never falls when a term is added), so
// the kept set is always {x >= thr}, ties included.  Nothing depends on B, on the row's position or on its address: the element ->
// (lane, slot) map is by column index alone, every reduction has one order, there are no float atomics.
#pragma once
#include "common.h"
#include <cmath>

namespace {

constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpGroups = 8;                                   // 16-byte groups per lane
constexpr int kSmpSpan = kSmpThreads * 4;                       // columns one group index covers
constexpr int kSmpMaxV = kSmpSpan * kSmpGroups;                 // 32768
constexpr unsigned kSmpKeyMinFinite = 0x00800000u;              // key(-inf) + 1: the smallest key of a value above -inf

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // rows with an odd stride start on any 4-byte address

// larger float <-> larger key (no NaN reaches this; -0 was made +0)
__device__ __forceinline__ unsigned smp_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Workgroup reductions over 16 waves.  `red` is [2][16] words used alternately (`par` flips per call, uniformly), so one barrier per
// reduction is enough: a wave can only reach its next write of the same half after every wave has passed the barrier in between.
__device__ __forceinline__ float smp_sum(float v, unsigned (*red)[kSmpWaves], int& par) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = __float_as_uint(v);
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kSmpWaves; ++i) t += __uint_as_float(red[par][i]);
    par ^= 1;
    return t;
}
enum { SMP_ADD, SMP_MIN, SMP_MAX, SMP_OR };
template <int OP>
__device__ __forceinline__ unsigned smp_comb(unsigned a, unsigned b) {
    return OP == SMP_ADD ? a + b : OP == SMP_MIN ? min(a, b) : OP == SMP_MAX ? max(a, b) : (a | b);
}
// v: already uniform over the wave (SMP_ADD: the wave's count), or per lane for MIN / MAX / OR (reduced over the wave here)
template <int OP>
__device__ __forceinline__ unsigned smp_red_u(unsigned v, unsigned (*red)[kSmpWaves], int& par) {
    if (OP != SMP_ADD) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = smp_comb<OP>(v, (unsigned)__shfl_xor((int)v, o, 64));
    }
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = red[par][0];
#pragma unroll
    for (int i = 1; i < kSmpWaves; ++i) t = smp_comb<OP>(t, red[par][i]);
    par ^= 1;
    return t;
}

struct SmpShared {
    unsigned red[2][kSmpWaves];
    float s_wave[kSmpGroups][kSmpWaves];
    float s_total;
};

// One group of 4 columns of a row: columns at or beyond V stand as `fill` (never loaded).
__device__ __forceinline__ void smp_load4(const float* __restrict__ row, int i0, int V, float fill, float (&v)[4]) {
    v[0] = v[1] = v[2] = v[3] = fill;
    if (i0 + 3 < V) {
        const f32x4_a4 q = *(const f32x4_a4*)(row + i0);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (i0 + c < V) v[c] = row[i0 + c];
    }
}

// A column's value -> the scaled value the select runs on, with the lane's running flag and maximum.
__device__ __forceinline__ float smp_scale(float v, float temperature, unsigned& bad, float& m) {
    float x = v / temperature;
    if (x == 0.f) x = 0.f;                                      // -0 -> +0: equal values, equal keys
    bad |= (x != x || x == INFINITY) ? 1u : 0u;                 // NaN, or +inf (softmax would be NaN)
    m = fmaxf(m, x);
    return x;
}

// The select of row b from its scaled values in registers.  Column of slot j = 4 g + c of this lane: g * 4096 + 4 * tid + c (ascending
// column order = g, then wave, then lane, then c); e[j] = smp_scale() of the column, -inf at or beyond V; bad, m: the lane's flag and
// maximum from those calls (bad may also carry what else the caller saw that makes the row unservable).  Every lane of the workgroup
// calls this; it ends with token, thr and kept written and returns (uniformly) whether the row was served: false = the -1 rule applied.
__device__ __forceinline__ bool smp_select_row(float (&e)[4 * kSmpGroups], unsigned bad, float m, const float* __restrict__ u, int V,
                                               int top_k, float top_p, int64_t* __restrict__ token, float* __restrict__ thr_out,
                                               int32_t* __restrict__ kept_out, SmpShared& sh, int& par) {
    unsigned (*red)[kSmpWaves] = sh.red;
    float (*s_wave)[kSmpWaves] = sh.s_wave;
    float& s_total = sh.s_total;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned key[4 * kSmpGroups];
    bad = smp_red_u<SMP_OR>(bad, red, par);
    const unsigned kmax = smp_red_u<SMP_MAX>(bad ? 0u : smp_key(m), red, par);
    if (bad || kmax < kSmpKeyMinFinite) {                       // (uniform) a NaN / +inf in the row, or nothing above -inf
        if (tid == 0) {
            token[b] = -1;
            if (thr_out) thr_out[b] = __uint_as_float(0x7fc00000u);
            if (kept_out) kept_out[b] = 0;
        }
        return false;
    }
    m = smp_unkey(kmax);
#pragma unroll
    for (int j = 0; j < 4 * kSmpGroups; ++j) {
        key[j] = smp_key(e[j]);
        e[j] = expf(e[j] - m);                                  // exp(-inf) = 0
    }

    // ---- top-k: t1 = the smallest key t in [key_min_finite, kmax] with #{key > t} < top_k; K1 = {key >= t1}
    unsigned t1 = kSmpKeyMinFinite;
    if (top_k > 0 && top_k < V) {
        unsigned lo = kSmpKeyMinFinite, hi = kmax;
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            unsigned cnt = 0;
#pragma unroll
            for (int j = 0; j < 4 * kSmpGroups; ++j) cnt += (unsigned)__popcll(__ballot(key[j] > mid));
            cnt = smp_red_u<SMP_ADD>(cnt, red, par);
            if (cnt < (unsigned)top_k) hi = mid; else lo = mid + 1;
        }
        t1 = lo;
    }

    // ---- top-p over K1: t2 = the smallest key t in [t1, kmax] with sum_{K1, key > t} e < top_p * Z1; K2 = {key >= t2}
    unsigned t2 = t1;
    if (top_p < 1.f) {
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < 4 * kSmpGroups; ++j) {
            e[j] = key[j] >= t1 ? e[j] : 0.f;
            z += e[j];
        }
        const float target = top_p * smp_sum(z, red, par);
        unsigned lo = t1, hi = kmax;
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4 * kSmpGroups; ++j) s += key[j] > mid ? e[j] : 0.f;
            s = smp_sum(s, red, par);
            if (s < target) hi = mid; else lo = mid + 1;
        }
        t2 = lo;
    }

    // ---- the kept set: its size, its smallest member (thr), its last column
    unsigned cnt = 0, kmin = 0xffffffffu, in_mask = 0;          // in_mask: bit j = slot j is kept (its e may have underflowed to 0)
    int last = -1;
#pragma unroll
    for (int j = 0; j < 4 * kSmpGroups; ++j) {
        const bool in = key[j] >= t2;
        cnt += (unsigned)__popcll(__ballot(in));
        e[j] = in ? e[j] : 0.f;
        if (in) {
            in_mask |= 1u << j;
            kmin = min(kmin, key[j]);
            last = (j >> 2) * kSmpSpan + 4 * tid + (j & 3);      // (slots ascend in column)
        }
    }
    cnt = smp_red_u<SMP_ADD>(cnt, red, par);
    kmin = smp_red_u<SMP_MIN>(kmin, red, par);
    last = (int)smp_red_u<SMP_MAX>((unsigned)(last + 1), red, par) - 1;
    if (tid == 0) {                                              // (written here, not beside the token: nothing of them stays live)
        if (thr_out) thr_out[b] = smp_unkey(kmin);
        if (kept_out) kept_out[b] = (int32_t)cnt;
    }

    // ---- the draw: cumulative kept mass in ascending column order; token = the first kept column whose inclusive sum exceeds u * total
    float incl[kSmpGroups];                                      // inclusive scan over the wave's lanes of each group's 4-column sums
#pragma unroll
    for (int g = 0; g < kSmpGroups; ++g) {
        float s = ((e[4 * g] + e[4 * g + 1]) + e[4 * g + 2]) + e[4 * g + 3];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(s, o, 64);
            if (lane >= o) s += t;
        }
        incl[g] = s;
        if (lane == 63) s_wave[g][w] = s;
    }
    __syncthreads();
    if (w == 0) {                                                // the 128 wave sums, in ascending column order -> their exclusive prefix (the
        float* flat = &s_wave[0][0];                             // mass before that wave's first column of group g), and the kept mass
        const float v0 = flat[2 * lane], v1 = flat[2 * lane + 1];
        float s = v0 + v1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(s, o, 64);
            if (lane >= o) s += t;
        }
        const float below = __shfl_up(s, 1, 64);
        const float ex = lane == 0 ? 0.f : below;
        flat[2 * lane] = ex;
        flat[2 * lane + 1] = ex + v0;
        if (lane == 63) s_total = s;
    }
    __syncthreads();
    const float target = u[b] * s_total;
    unsigned pick = 0x7fffffffu;
#pragma unroll
    for (int g = kSmpGroups - 1; g >= 0; --g) {                  // highest column first, so the smallest qualifying column is what stays
        const float below = __shfl_up(incl[g], 1, 64);          // the exclusive scan value, bit for bit what the lane below holds
        float cum[4];
        float run = s_wave[g][w] + (lane == 0 ? 0.f : below);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            run += e[4 * g + k];
            cum[k] = run;
        }
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (((in_mask >> (4 * g + k)) & 1u) && cum[k] > target) pick = (unsigned)(g * kSmpSpan + 4 * tid + k);
    }
    pick = smp_red_u<SMP_MIN>(pick, red, par);
    if (tid == 0) {
        token[b] = pick == 0x7fffffffu ? (int64_t)last : (int64_t)pick;      // rounding left no column above u * total: the last kept one
    }
    return true;
}

}  // namespace

// Beam search's candidate selection (halva_amd/decode.py:beam_search) on gfx950: for each prompt, the C best of its K beams' K * V
// continuations by  beam_scores[k] + log_softmax(logits[k])[i],  descending, ties by the lower flat index k * V + i.  Two launches, no sort.
//
// Row pass - one workgroup of 1024 lanes per beam, the row read from HBM once and held in registers (32 values per lane), as sample.hip:
//   lse = max + log(sum exp(x - max)), the sum in ONE order set by V alone (a lane's 32 values by index, the wave butterfly, the 16 waves in
//   order); score_i = beam_score + (x_i - lse) in fp32.  The row's own C-th largest score is found by count-bisection over the
//   order-preserving uint32 image of the score (smallest t with #{key > t} < C); ties at the cut go by lowest column (a second bisection, over
//   the column index).  The row's min(C, V) survivors go to the workspace, in no particular order.
// Group pass - one workgroup per prompt ranks the K * C survivors by counting those that beat each one under the total order (score
//   descending, flat index ascending) and writes ranks below C.  The order is total, so the arbitrary workspace order never shows.
// A row with a NaN or +inf logit, with nothing above -inf, or with a beam score that is not finite flags its prompt: every cand_token of that
// prompt is -1, other prompts are unaffected.  Nothing depends on B, on the prompt's position or on the row stride; no float atomics.
#include "common.h"
#include <cmath>

namespace {

constexpr int kBsThreads = 1024;
constexpr int kBsWaves = kBsThreads / 64;
constexpr int kBsGroups = 8;                                    // 16-byte groups per lane
constexpr int kBsSpan = kBsThreads * 4;                         // columns one group index covers
constexpr int kBsMaxV = kBsSpan * kBsGroups;                    // 32768
constexpr int kBsMaxK = 16, kBsMaxC = 64;
constexpr unsigned kBsKeyNegInf = 0x007fffffu;                  // key(-inf); slots at or beyond V carry key 0, below every real column

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));      // rows with an odd stride start on any 4-byte address

__device__ __forceinline__ unsigned bs_key(float f) {           // larger float <-> larger key (no NaN reaches this; -0 was made +0)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bs_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Workgroup reductions over 16 waves; `red` is [2][16] words used alternately, so one barrier per reduction is enough (sample.hip).
__device__ __forceinline__ float bs_sum(float v, unsigned (*red)[kBsWaves], int& par) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = __float_as_uint(v);
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < kBsWaves; ++i) t += __uint_as_float(red[par][i]);
    par ^= 1;
    return t;
}
enum { BS_ADD, BS_MAX, BS_OR };
template <int OP>
__device__ __forceinline__ unsigned bs_comb(unsigned a, unsigned b) { return OP == BS_ADD ? a + b : OP == BS_MAX ? max(a, b) : (a | b); }
// v: already uniform over the wave (BS_ADD: the wave's count), or per lane for MAX / OR (reduced over the wave here)
template <int OP>
__device__ __forceinline__ unsigned bs_red_u(unsigned v, unsigned (*red)[kBsWaves], int& par) {
    if (OP != BS_ADD) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = bs_comb<OP>(v, (unsigned)__shfl_xor((int)v, o, 64));
    }
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = red[par][0];
#pragma unroll
    for (int i = 1; i < kBsWaves; ++i) t = bs_comb<OP>(t, red[par][i]);
    par ^= 1;
    return t;
}

// Column of slot j = 4 g + c of this lane: g * 4096 + 4 * tid + c.  Survivors of row r: ws_score / ws_token [r * C, r * C + C), unused
// places with token -1; ws_flag[r] = 1 when the row cannot be served.
__global__ __launch_bounds__(kBsThreads) void beam_select_row_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ beam_scores,
                                                                     int V, int C, float* __restrict__ ws_score, int32_t* __restrict__ ws_token,
                                                                     int32_t* __restrict__ ws_flag) {
    __shared__ unsigned red[2][kBsWaves];
    __shared__ float s_score[kBsMaxC];
    __shared__ int s_token[kBsMaxC];
    __shared__ int s_fill;
    int par = 0;
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (int64_t)r * ld;
    const float bscore = beam_scores[r];
    float e[4 * kBsGroups];
    unsigned key[4 * kBsGroups];

    // ---- the one read of the row; columns at or beyond V stand as -inf (never loaded)
    float m = -INFINITY;
    unsigned bad = (bscore - bscore == 0.f) ? 0u : 1u;         // a beam score that is NaN or infinite
#pragma unroll
    for (int g = 0; g < kBsGroups; ++g) {
        const int i0 = g * kBsSpan + 4 * tid;
        float v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (i0 + 3 < V) {
            const f32x4_a4 q = *(const f32x4_a4*)(row + i0);
            v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i0 + c < V) v[c] = row[i0 + c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float x = v[c];
            bad |= (x != x || x == INFINITY) ? 1u : 0u;
            m = fmaxf(m, x);
            e[4 * g + c] = x;
        }
    }
    if (tid == 0) s_fill = 0;
    if (tid < kBsMaxC) {
        s_score[tid] = -INFINITY;
        s_token[tid] = -1;
    }
    bad = bs_red_u<BS_OR>(bad, red, par);
    const unsigned kmaxx = bs_red_u<BS_MAX>(bad ? 0u : bs_key(m == 0.f ? 0.f : m), red, par);
    if (bad || kmaxx <= kBsKeyNegInf) {                         // (uniform)
        if (tid == 0) ws_flag[r] = 1;
        return;
    }
    m = bs_unkey(kmaxx);

    // ---- lse, then every column's score and its key
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < 4 * kBsGroups; ++j) z += expf(e[j] - m);      // exp(-inf) = 0
    z = bs_sum(z, red, par);
    const float lse = m + logf(z);
    unsigned kmax = 0;
#pragma unroll
    for (int j = 0; j < 4 * kBsGroups; ++j) {
        float s = bscore + (e[j] - lse);
        if (s == 0.f) s = 0.f;                                  // -0 -> +0: equal values, equal keys
        e[j] = s;
        const int col = (j >> 2) * kBsSpan + 4 * tid + (j & 3);
        key[j] = col < V ? bs_key(s) : 0u;
        kmax = max(kmax, key[j]);
    }
    kmax = bs_red_u<BS_MAX>(kmax, red, par);

    // ---- the cut: t = the smallest key in [key(-inf), kmax] with #{key > t} < C; every key > t survives, and of those equal to t the
    // first C - #{key > t} in column order: columns below cb
    unsigned lo = kBsKeyNegInf, hi = kmax;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        unsigned cnt = 0;
#pragma unroll
        for (int j = 0; j < 4 * kBsGroups; ++j) cnt += (unsigned)__popcll(__ballot(key[j] > mid));
        cnt = bs_red_u<BS_ADD>(cnt, red, par);
        if (cnt < (unsigned)C) hi = mid; else lo = mid + 1;
    }
    const unsigned t = lo;
    unsigned above = 0, at = 0;
#pragma unroll
    for (int j = 0; j < 4 * kBsGroups; ++j) {
        above += (unsigned)__popcll(__ballot(key[j] > t));
        at += (unsigned)__popcll(__ballot(key[j] == t));
    }
    above = bs_red_u<BS_ADD>(above, red, par);
    at = bs_red_u<BS_ADD>(at, red, par);
    int cb = V;
    if (above + at > (unsigned)C) {                             // (uniform) smallest cb with #{key == t, column < cb} >= C - above
        const unsigned need = (unsigned)C - above;
        int clo = 1, chi = V;
        while (clo < chi) {
            const int mid = clo + (chi - clo) / 2;
            unsigned cnt = 0;
#pragma unroll
            for (int j = 0; j < 4 * kBsGroups; ++j) {
                const int col = (j >> 2) * kBsSpan + 4 * tid + (j & 3);
                cnt += (unsigned)__popcll(__ballot(key[j] == t && col < mid));
            }
            cnt = bs_red_u<BS_ADD>(cnt, red, par);
            if (cnt >= need) chi = mid; else clo = mid + 1;
        }
        cb = clo;
    }

    // ---- the survivors (at most C of them) into LDS places handed out by an integer counter, then out
#pragma unroll
    for (int j = 0; j < 4 * kBsGroups; ++j) {
        const int col = (j >> 2) * kBsSpan + 4 * tid + (j & 3);
        if (key[j] > t || (key[j] == t && col < cb)) {
            const int at_ = atomicAdd(&s_fill, 1);
            if (at_ < C) {
                s_score[at_] = e[j];
                s_token[at_] = col;
            }
        }
    }
    __syncthreads();
    if (tid < C) {
        ws_score[(int64_t)r * C + tid] = s_score[tid];
        ws_token[(int64_t)r * C + tid] = s_token[tid];
    }
    if (tid == 0) ws_flag[r] = 0;
}

__global__ __launch_bounds__(kBsThreads) void beam_select_group_kernel(const float* __restrict__ ws_score, const int32_t* __restrict__ ws_token,
                                                                       const int32_t* __restrict__ ws_flag, int K, int C, int V,
                                                                       float* __restrict__ cand_score, int32_t* __restrict__ cand_token,
                                                                       int32_t* __restrict__ cand_beam) {
    __shared__ float s_score[kBsMaxK * kBsMaxC];
    __shared__ int s_flat[kBsMaxK * kBsMaxC];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = K * C;
    int flagged = 0;
    for (int k = 0; k < K; ++k) flagged |= ws_flag[(int64_t)b * K + k];
    if (flagged) {                                              // (uniform)
        if (tid < C) {
            cand_score[(int64_t)b * C + tid] = __uint_as_float(0x7fc00000u);
            cand_token[(int64_t)b * C + tid] = -1;
            cand_beam[(int64_t)b * C + tid] = -1;
        }
        return;
    }
    float mine = 0.f;
    int flat = -1;
    if (tid < n) {
        const int tok = ws_token[(int64_t)b * n + tid];
        mine = ws_score[(int64_t)b * n + tid];
        flat = tok < 0 ? -1 : (tid / C) * V + tok;
        s_score[tid] = mine;
        s_flat[tid] = flat;
    }
    __syncthreads();
    if (flat < 0) return;
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float sj = s_score[j];
        const int fj = s_flat[j];
        rank += (fj >= 0 && (sj > mine || (sj == mine && fj < flat))) ? 1 : 0;
    }
    if (rank < C) {
        cand_score[(int64_t)b * C + rank] = mine;
        cand_token[(int64_t)b * C + rank] = flat % V;
        cand_beam[(int64_t)b * C + rank] = flat / V;
    }
}

int64_t beam_ws_bytes(int M, int C) {
    if (M <= 0 || C <= 0 || C > kBsMaxC) return 0;
    return (int64_t)M * C * 8 + (int64_t)M * 4;
}

}  // namespace

extern "C" int halva_beam_select_max_vocab(void) { return kBsMaxV; }
extern "C" int halva_beam_select_max_beams(void) { return kBsMaxK; }
extern "C" int halva_beam_select_max_candidates(void) { return kBsMaxC; }
extern "C" int64_t halva_beam_select_ws_bytes(int M, int C) { return beam_ws_bytes(M, C); }

extern "C" int halva_beam_select(const float* logits, int64_t ld, const float* beam_scores, float* cand_score, int32_t* cand_token,
                                 int32_t* cand_beam, void* ws, int64_t ws_bytes, int B, int K, int C, int V, void* stream) {
    HALVA_CHECK_ARG(logits && beam_scores && cand_score && cand_token && cand_beam && ws, "beam_select: null pointer");
    HALVA_CHECK_ARG(B >= 1 && B <= 65535 && V >= 1, "beam_select: bad B=%d / V=%d", B, V);
    HALVA_CHECK_ARG(V <= kBsMaxV, "beam_select: V=%d exceeds the %d columns a workgroup holds (halva_beam_select_max_vocab)", V, kBsMaxV);
    HALVA_CHECK_ARG(K >= 1 && K <= kBsMaxK, "beam_select: K=%d beams (needs 1 .. %d)", K, kBsMaxK);
    HALVA_CHECK_ARG(C >= K && C <= kBsMaxC && (int64_t)C <= (int64_t)K * V, "beam_select: C=%d candidates (needs K=%d <= C <= min(%d, K*V))", C, K,
                    kBsMaxC);
    HALVA_CHECK_ARG(ld >= V, "beam_select: row stride %lld < V=%d", (long long)ld, V);
    HALVA_CHECK_ARG(((uintptr_t)logits | (uintptr_t)beam_scores | (uintptr_t)cand_score | (uintptr_t)cand_token | (uintptr_t)cand_beam |
                     (uintptr_t)ws) % 4 == 0, "beam_select: pointers must be 4-byte aligned");
    const int M = B * K;
    const int64_t need = beam_ws_bytes(M, C);
    HALVA_CHECK_ARG(ws_bytes >= need, "beam_select: workspace of %lld bytes, %lld needed (halva_beam_select_ws_bytes)", (long long)ws_bytes,
                    (long long)need);
    float* ws_score = (float*)ws;
    int32_t* ws_token = (int32_t*)(ws_score + (int64_t)M * C);
    int32_t* ws_flag = ws_token + (int64_t)M * C;
    hipLaunchKernelGGL(beam_select_row_kernel, dim3(M), dim3(kBsThreads), 0, (hipStream_t)stream, logits, ld, beam_scores, V, C, ws_score, ws_token,
                       ws_flag);
    hipLaunchKernelGGL(beam_select_group_kernel, dim3(B), dim3(kBsThreads), 0, (hipStream_t)stream, (const float*)ws_score,
                       (const int32_t*)ws_token, (const int32_t*)ws_flag, K, C, V, cand_score, cand_token, cand_beam);
    HALVA_CHECK_LAUNCH("beam_select");
    return HALVA_OK;
}

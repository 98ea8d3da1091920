// Beam search's ancestry table (halva_amd/decode.py:BeamCache) on gfx950.  The members of a beam cache are B prompts x K beams, and a beam
// that continues another beam's history moves no K / V row: anc int32 [M, Lown] names, per member and own row, the member whose slot holds
// it.  The attention reads through the table (kvcache.hip: own_partial_kernel<256, true>); halva_beam_advance, here, derives the next
// step's table from this step's parents.  The cache kernels themselves are kvcache.hip's.
#include "common.h"

namespace {

// The ancestry table of the next step from this step's parents, one workgroup per member: with t = own_lens[m] (before this step's
// append), dst[m][j] = src[parent[m]][j] for j < t and dst[m][t] = m, the slot halva_fork_rope_append is about to write.  dst[m][j] for
// j > t is not written; a parent outside [0, M) or t outside [0, Lown) leaves row m untouched.
__global__ __launch_bounds__(256) void beam_advance_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                           const int32_t* __restrict__ parent, const int32_t* __restrict__ own_lens, int M, int Lown) {
    const int m = blockIdx.x;
    const int p = parent[m], t = own_lens[m];
    if (p < 0 || p >= M || t < 0 || t >= Lown) return;
    const int32_t* s = src + (int64_t)p * Lown;
    int32_t* d = dst + (int64_t)m * Lown;
    for (int j = threadIdx.x; j < t; j += blockDim.x) d[j] = s[j];
    if (threadIdx.x == 0) d[t] = m;
}

}  // namespace

extern "C" int halva_beam_advance(const int32_t* anc_src, int32_t* anc_dst, const int32_t* parent, const int32_t* own_lens, int M, int Lown,
                                  void* stream) {
    HALVA_CHECK_ARG(anc_src && anc_dst && parent && own_lens, "beam_advance: null pointer");
    HALVA_CHECK_ARG(M > 0 && Lown > 0 && M <= 65535, "beam_advance: bad M=%d / Lown=%d", M, Lown);
    HALVA_CHECK_ARG(((uintptr_t)anc_src | (uintptr_t)anc_dst | (uintptr_t)parent | (uintptr_t)own_lens) % 4 == 0,
                    "beam_advance: pointers must be 4-byte aligned");
    const int64_t bytes = (int64_t)M * Lown * (int64_t)sizeof(int32_t);
    const intptr_t gap = (intptr_t)((uintptr_t)anc_dst - (uintptr_t)anc_src);
    HALVA_CHECK_ARG(gap >= bytes || gap <= -bytes, "beam_advance: source and destination tables overlap (they are the two halves of one pair)");
    hipLaunchKernelGGL(beam_advance_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, anc_src, anc_dst, parent, own_lens, M, Lown);
    HALVA_CHECK_LAUNCH("beam_advance");
    return HALVA_OK;
}

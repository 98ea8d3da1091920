// Fused self-attention for gfx950 (CDNA4): forward and backward kernels on v_mfma_f32_32x32x16_bf16.
//
// Replaces flash_attn_varlen_qkvpacked_func + unpad_input/pad_input of the reference
// (llava/train/llama_flash_attn_monkey_patch.py:71-91) for Llama (causal, head_dim 128) and HF CLIPAttention's
// softmax(QK^T)V for the frozen vision tower (non-causal, head_dim 64, forward only).
//
// This file is the one translation unit of the attention: the kernels live in the headers included below (in this order, inside one
// anonymous namespace; none is compiled alone), the host side - what runs for a call, the launches, the C ABI - follows them here.
//
// The kernels, (*) = what the training step runs by default:
//   sdpa_fwd3 (*)              sdpa_fwd3.h       the causal head_dim-128 forward: one wave per SIMD, the tile loop in generated asm, persistent workgroups
//                                                of 256 query rows with 129 KiB of LDS (four K / V tile slots).  Selected by choose_fwd.
//   sdpa_fwd3_twin             sdpa_fwd3_twin.h  HALVA_FWD3_ASM=0: sdpa_fwd3 in plain HIP, its bit reference; one workgroup per row block
//   sdpa_fwd_kernel (*: tower) sdpa_fwd.h        two waves per SIMD: head_dim 64, the non-causal vision tower, HALVA_SDPA_FWD3=0, HALVA_SDPA_SLOW_TR=1;
//                                                and once more behind sdpa_fwd3 as its repair pass (HALVA_FWD3_REPAIR=1)
//   sdpa_bwd_delta_kernel (*)  sdpa_bwd_dq2.h    backward with a dS workspace (head_dim 128), pass 1: delta, zeros into the padded dq rows, and
//                                                sdpa_bwd_dkv3's work-queue counters and item records (sdpa_dkv3_items.h)
//   sdpa_bwd_dkv3 (*)          sdpa_dkv3.h       pass 2: dK / dV and the dS store; one wave per SIMD, every step in generated asm (HALVA_DKV3_ASM=0: in
//                                                plain HIP), persistent workgroups of 128 keys with 130 KiB of LDS.  Selected by choose_bwd.
//   sdpa_bwd_dkv2_kernel       sdpa_bwd_dkv2.h   the two-role dK / dV: pass 2 under HALVA_SDPA_DKV3=0 / HALVA_SDPA_SLOW_TR=1; head_dim 64, calls without a workspace
//   sdpa_bwd_dq2_kernel (*)    sdpa_bwd_dq2.h    pass 3: dQ = dS K (HALVA_DQ2_FAST_TILE=0: every tile through the general per-strip loop)
//   sdpa_bwd_dq_kernel         sdpa_bwd_dq.h     the 3-product dQ (forms delta itself): head_dim 64 and calls without a workspace, in front of sdpa_bwd_dkv2
// sdpa_common.h holds what they share: SdpaParams, the branch mask, LDS tiles (one XOR swizzle, conflict-free for ds_read_b128 row reads
// and transposed reads) and their LDS-DMA, the softmax pieces of a score tile (mask_half, half_max, xhalf_max / xhalf_sum, kRescaleAt: also
// what the rows attention of kvcache.hip uses), the store epilogues (with the inverse RoPE), the block maps.
// No atomics on results: dQ has its own kernels, so results are bitwise reproducible.
// Each kernel is compiled ONE way: the only -D switches are HALVA_STAMP / HALVA_STAMP_STRIDE (the in-kernel clock); the variants that were
// measured and retired are described in DESIGN.md 5.3.
#include "common.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <type_traits>

namespace {
#include "sdpa_common.h"
#include "sdpa_fwd.h"
#include "sdpa_bwd_dq.h"
#include "sdpa_bwd_dkv2.h"
#include "sdpa_dkv3_items.h"
#include "sdpa_bwd_dq2.h"

#include "sdpa_dkv3.h"
#include "sdpa_fwd3.h"
#include "sdpa_fwd3_twin.h"

// ======== host side: switches -> choose_fwd / choose_bwd (what runs) -> launch_fwd / launch_bwd (run it) -> the C ABI ========
// Every environment switch of the attention: A/B and debugging switches, filled once per C-ABI call and never cached across calls (a test
// flips them inside one process; plain environment reads, no allocation).  A switch that another one makes meaningless is not read, so it
// keeps its default here: HALVA_SDPA_SLOW_TR=1 selects the legacy kernels outright, a kernel that is switched off has no variants.
constexpr int kOrderUnset = INT_MIN;      // SdpaSwitches::dkv3_order without HALVA_DKV3_ORDER
constexpr int kPerCu = -1;               // launch(): a grid capped at one workgroup per CU
struct SdpaSwitches {
    bool slow_tr = false;        // HALVA_SDPA_SLOW_TR=1 (tests): scalar transposed reads instead of ds_read_b64_tr_b16 (legacy kernels and sdpa_bwd_dq2)
    bool fwd3 = false;           // HALVA_SDPA_FWD3=0: the two-waves-per-SIMD forward of rounds 1-3 instead of sdpa_fwd3
    bool fwd3_asm = true;        // HALVA_FWD3_ASM=0: the plain-HIP twin of the generated block (sdpa_fwd3_twin.h; one workgroup per row block)
    int fwd3_grid = 0;           // HALVA_FWD3_GRID (diagnostic): workgroups of the persistent launch (0 = one per virtual block: no pipelining across items)
    bool fwd3_repair = false;    // HALVA_FWD3_REPAIR=1: the repair pass behind sdpa_fwd3 (choose_fwd)
    bool dkv3 = false;           // HALVA_SDPA_DKV3=0: the two-role dK/dV kernel of rounds 1-2 instead of sdpa_bwd_dkv3
    bool dkv3_asm = true;        // HALVA_DKV3_ASM=0: sdpa_bwd_dkv3 with every step in plain HIP (the generated loop off)
    int dkv3_order = kOrderUnset;      // HALVA_DKV3_ORDER: order of the items inside a work queue (sdpa_dkv3.h)
    bool rope_fused_bwd = false; // HALVA_ROPE_FUSED_BWD=0: dq / dk leave the backward un-rotated, the rotation follows as its own launch
    bool dq2_fast_tile = true;   // HALVA_DQ2_FAST_TILE=0: every tile of sdpa_bwd_dq2 through the general per-strip path
};
// fwd3_call: a causal head_dim-128 forward; ds_call: a head_dim-128 backward with a workspace - the calls the respective switches can bear on
SdpaSwitches read_switches(bool fwd3_call, bool ds_call) {
    const auto starts = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
    const auto on = [&](const char* name) { return !starts(name, '0'); };      // the default-on switches: anything but a leading 0
    SdpaSwitches sw;
    sw.slow_tr = starts("HALVA_SDPA_SLOW_TR", '1');
    if (sw.slow_tr) return sw;
    if (fwd3_call && (sw.fwd3 = on("HALVA_SDPA_FWD3"))) {
        if (const char* e = getenv("HALVA_FWD3_GRID")) sw.fwd3_grid = atoi(e) > 0 ? atoi(e) : (1 << 30);
        sw.fwd3_asm = on("HALVA_FWD3_ASM");
        sw.fwd3_repair = starts("HALVA_FWD3_REPAIR", '1');
    }
    if (ds_call) {
        if ((sw.dkv3 = on("HALVA_SDPA_DKV3"))) {
            if (const char* e = getenv("HALVA_DKV3_ORDER")) sw.dkv3_order = atoi(e);
            if ((sw.dkv3_asm = on("HALVA_DKV3_ASM"))) sw.rope_fused_bwd = on("HALVA_ROPE_FUSED_BWD");
        }
        sw.dq2_fast_tile = on("HALVA_DQ2_FAST_TILE");
    }
    return sw;
}

enum class FwdKernel { fwd3, fwd3_twin, fwd_legacy };
struct FwdPlan {
    FwdKernel kernel;
    bool slow_tr;           // (fwd_legacy only)
    bool repair_pass;       // sdpa_fwd_kernel once more behind sdpa_fwd3, over the row blocks it gave up on (p.repair)
    int grid_cap;           // (fwd3 only) workgroups of the persistent launch: kPerCu unless HALVA_FWD3_GRID overrides it
};
template <int D, bool CAUSAL>
FwdPlan choose_fwd(int T, int64_t ld_qkv, const SdpaSwitches& sw) {
    // sdpa_fwd3: one wave per SIMD, the tile loop in generated asm (sdpa_fwd3.h).  (Its tile counts travel as 16-bit fields, a sequence's
    // K / V rows are addressed through one 32-bit buffer descriptor.)
    const bool fwd3 = D == 128 && CAUSAL && !sw.slow_tr && T < (1 << 21) && (int64_t)T * ld_qkv * 2 < (1ll << 31) && sw.fwd3;
    if (!fwd3) return {FwdKernel::fwd_legacy, sw.slow_tr, false, 0};
    // HALVA_FWD3_REPAIR=1: the unbounded-range repair pass over the row blocks sdpa_fwd3 gave up on (sdpa_fwd_kernel, p.repair).  Off by
    // default: measured 32 us per launch (fwd_in_step 0.777 -> 0.809 ms, profiles/r05_ab_rope_repair.log) against rows that would need scores
    // 5 300 nats above their first keys (sdpa_fwd3.h); such rows come back as NaN, not as wrong numbers.
    return {sw.fwd3_asm ? FwdKernel::fwd3 : FwdKernel::fwd3_twin, false, sw.fwd3_repair, sw.fwd3_grid ? sw.fwd3_grid : kPerCu};
}

enum class DkvKernel { dkv3_asm, dkv3_hip, dkv2 };
enum class DqKernel { dq2_fast, dq2_general, dq };
struct BwdPlan {
    bool ds_path;           // dS formed once: delta (+ zero-fill of padded dq rows) -> dK/dV (+ dS store) -> dQ = dS K;  false: 3-product dQ -> dK/dV
    DkvKernel dkv;
    DqKernel dq;
    bool slow_tr;           // (dkv2, dq, dq2_fast)
    bool rope_fused;        // the store epilogues rotate dq / dk; false: they leave un-rotated (halva_sdpa_branch_bwd_rope follows up)
    int sched_order;        // sdpa_bwd_dkv3 only
};
template <int D, bool CAUSAL>
BwdPlan choose_bwd(int S, int T, int H, int64_t ld_qkv, int64_t ld_do, bool have_ws, bool have_lse2, bool have_rope, const SdpaSwitches& sw) {
    BwdPlan plan{false, DkvKernel::dkv2, DqKernel::dq, sw.slow_tr, false, 0};
    if (!(have_ws && D == 128)) return plan;      // head_dim 64, calls without a workspace: the 3-product dQ and the two-role dK/dV, no rotation
    plan.ds_path = true;
    const int64_t rows = (int64_t)S * T;
    // (sdpa_bwd_dkv3's step counts travel as 16-bit fields, its scheduler divides in fp32, and a sequence's Q / dO rows are addressed through
    // 32-bit buffer descriptors - q_rec / do_rec / *_soff in sdpa_dkv3.h are (rows * ld * 2) as unsigned: the same bound as choose_fwd's)
    const bool dkv3 = !sw.slow_tr && have_lse2 && rows >= 16 && T < (1 << 22) && (int64_t)S * H * ((T + 127) / 128) < (1 << 23) &&
                      (int64_t)T * std::max(ld_qkv, ld_do) * 2 < (1ll << 31) && sw.dkv3;
    if (dkv3) {
        static_assert(CAUSAL || D != 128, "sdpa_bwd_dkv3's item records are written for the causal backward (dkv3_build_record<true>)");
        plan.dkv = sw.dkv3_asm ? DkvKernel::dkv3_asm : DkvKernel::dkv3_hip;
        plan.sched_order = sw.dkv3_order != kOrderUnset ? sw.dkv3_order : (CAUSAL ? 2 : 0);
    }
    // the inverse RoPE of dq / dk rides in the store epilogues of sdpa_bwd_dq2 and of sdpa_bwd_dkv3's generated build; any other kernel
    // combination leaves them un-rotated
    plan.rope_fused = have_rope && plan.dkv == DkvKernel::dkv3_asm && sw.rope_fused_bwd;
    plan.dq = sw.slow_tr || sw.dq2_fast_tile ? DqKernel::dq2_fast : DqKernel::dq2_general;      // (the SLOW_TR build has the fast tile only)
    return plan;
}

// One launch.  Two things are remembered per (kernel, device) in atomics - Kern is a template VALUE, so each kernel has its own tables:
// the dynamic-LDS limit, an attribute that is set once and again only to grow (two host threads racing here both set the same value -
// harmless; a process that drives several devices sets it on each; a device index outside the table sets it on every launch), and the CU
// count for the persistent kernels (cap = kPerCu: one workgroup per CU - it takes the CU's whole register file and most of its LDS - fewer
// when there is less to do).  cap > 0: at most that many workgroups; 0: one per block.
template <auto Kern, typename... Args>
int launch(const char* name, int64_t blocks, int cap, int threads, size_t lds, hipStream_t st, const Args&... args) {
    constexpr int kMaxDev = 64;
    static std::atomic<size_t> lds_set[kMaxDev];
    static std::atomic<int> n_cu[kMaxDev];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int slot = (dev >= 0 && dev < kMaxDev) ? dev : -1;
    if (lds > (slot < 0 ? 0 : lds_set[slot].load(std::memory_order_acquire))) {
        const hipError_t ea = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) {
            halva_set_error("%s: hipFuncSetAttribute(%zu B of LDS) failed: %s", name, lds, hipGetErrorString(ea));
            return HALVA_ERR_LAUNCH;
        }
        if (slot >= 0) {
            size_t cur = lds_set[slot].load(std::memory_order_relaxed);
            while (cur < lds && !lds_set[slot].compare_exchange_weak(cur, lds, std::memory_order_release)) {}
        }
    }
    if (cap == kPerCu) {
        cap = slot >= 0 ? n_cu[slot].load(std::memory_order_acquire) : 0;
        if (cap == 0) {
            if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cap <= 0) cap = 256;
            if (slot >= 0) n_cu[slot].store(cap, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(Kern, dim3((unsigned)(cap > 0 ? std::min<int64_t>(blocks, cap) : blocks)), dim3(threads), lds, st, args...);
    HALVA_CHECK_LAUNCH(name);
    return HALVA_OK;
}
// a run-time flag as a template argument: f(std::true_type{}) or f(std::false_type{})
template <typename F>
int with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
// p cut into blocks of `rows` rows, and the workgroups that makes: the causal legacy kernels and sdpa_fwd3 take a heavy and a light block each
SdpaParams in_blocks(SdpaParams p, int rows, int S) { return p.nblk = (p.T + rows - 1) / rows, p.npairs = S * p.H, p; }
int64_t n_wg(const SdpaParams& p, bool paired) { return (int64_t)(paired ? (p.nblk + 1) / 2 : p.nblk) * p.npairs; }

template <int D, bool CAUSAL>
int launch_fwd(SdpaParams p, int S, hipStream_t st, const FwdPlan& plan) {
    p = in_blocks(p, 256, S);
    const auto legacy = [&](const char* name) {
        return with_flag(plan.slow_tr, [&](auto slow) {
            return launch<sdpa_fwd_kernel<D, CAUSAL, decltype(slow)::value>>(name, n_wg(p, CAUSAL), 0, 512, 4 * 64 * D * 2, st, p);
        });
    };
    const int rc = plan.kernel == FwdKernel::fwd3      ? launch<sdpa_fwd3_kernel<true>>("sdpa_fwd3", n_wg(p, true), plan.grid_cap, 256, FWD3_LDS, st, p)
                   : plan.kernel == FwdKernel::fwd3_twin ? launch<sdpa_fwd3_twin_kernel<true>>("sdpa_fwd3_twin", n_wg(p, false), 0, 256, 0, st, p)
                                                         : legacy("sdpa_fwd");
    if (rc != HALVA_OK || !plan.repair_pass) return rc;
    p.repair = 1;
    return legacy("sdpa_fwd (repair)");
}

template <int D, bool CAUSAL>
int launch_bwd(SdpaParams p, int S, hipStream_t st, const BwdPlan& plan) {
    if (!plan.rope_fused) p.rope_cos = p.rope_sin = nullptr;
    p.sched_order = plan.sched_order;
    p = in_blocks(p, 128, S);      // (in front of the delta pass: it writes sdpa_bwd_dkv3's item records from nblk / npairs / sched_order)
    const SdpaParams p256 = in_blocks(p, 256, S);
    const auto dkv2 = [&] {
        return with_flag(plan.slow_tr, [&](auto slow) {
            return launch<sdpa_bwd_dkv2_kernel<D, CAUSAL, decltype(slow)::value>>("sdpa_bwd_dkv2", n_wg(p, CAUSAL), 0, 512,
                                                                                 6 * 64 * D * 2 + 6 * 64 * sizeof(float) + 2 * 4 * 2 * 2048, st, p);
        });
    };
    int rc;
    if (!plan.ds_path) {
        rc = with_flag(plan.slow_tr, [&](auto slow) {
            return launch<sdpa_bwd_dq_kernel<D, CAUSAL, decltype(slow)::value, 8>>("sdpa_bwd_dq", n_wg(p256, CAUSAL), 0, 512, 4 * 64 * D * 2, st, p256);
        });
        return rc != HALVA_OK ? rc : dkv2();
    }
    // (a failed delta launch would leave stale delta / unzeroed padded dq rows for the two kernels behind it)
    rc = launch<sdpa_bwd_delta_kernel<D>>("sdpa_bwd_delta", ((int64_t)S * p.T + 3) / 4, 0, 256, 0, st, p, S, plan.dkv != DkvKernel::dkv2 ? 1 : 0);
    if (rc != HALVA_OK) return rc;
    rc = plan.dkv == DkvKernel::dkv2 ? dkv2() : with_flag(plan.dkv == DkvKernel::dkv3_asm, [&](auto use_asm) {
        return launch<sdpa_bwd_dkv3_kernel<128, CAUSAL, decltype(use_asm)::value>>("sdpa_bwd_dkv3", n_wg(p, false), kPerCu, 256, DKV3_LDS, st, p);
    });
    if (rc != HALVA_OK) return rc;
    const size_t lds_dq2 = 3 * 64 * D * 2 + 8 * 3 * DS_LDS_SLOT;
    if (plan.dq == DqKernel::dq2_general)
        return launch<sdpa_bwd_dq2_kernel<D, false, false>>("sdpa_bwd_dq2 (general tile)", n_wg(p256, true), 0, 512, lds_dq2, st, p256);
    return with_flag(plan.slow_tr, [&](auto slow) {
        return launch<sdpa_bwd_dq2_kernel<D, decltype(slow)::value>>("sdpa_bwd_dq2", n_wg(p256, true), 0, 512, lds_dq2, st, p256);
    });
}

// what the entry points share: q / k / v carved from the packed qkv rows, the sizes, the softmax scale (<= 0: 1 / sqrt(head_dim))
SdpaParams base_params(const void* qkv, int T, int H, int D, float scale) {
    SdpaParams p{};
    p.q = (const bf16_t*)qkv;
    p.k = p.q + (int64_t)H * D;
    p.v = p.q + 2 * (int64_t)H * D;
    p.ld_qkv = 3 * (int64_t)H * D;
    p.T = T, p.H = H;
    p.scale = scale > 0.f ? scale : 1.f / sqrtf((float)D);
#ifdef HALVA_STAMP
    p.dbg = halva_dbg_buffer();
#endif
    return p;
}
template <bool CAUSAL>
int run_fwd(const SdpaParams& p, int S, int D, hipStream_t st) {
    const SdpaSwitches sw = read_switches(D == 128 && CAUSAL, false);
    return D == 128 ? launch_fwd<128, CAUSAL>(p, S, st, choose_fwd<128, CAUSAL>(p.T, p.ld_qkv, sw))
                    : launch_fwd<64, CAUSAL>(p, S, st, choose_fwd<64, CAUSAL>(p.T, p.ld_qkv, sw));
}

// The backward workspace: dS, then [S, H, T] f32 lse * log2(e) for sdpa_bwd_dkv3 (+ one padding row), then its work-queue counters, then
// its item records
int64_t lse2_region_bytes(int S, int T, int H) { return (((int64_t)S * H * ((T + 63) / 64) * 512 + 256) + 127) / 128 * 128; }
int64_t ds_region_bytes(int S, int T, int H) { return (int64_t)S * H * ((T + 127) / 128) * ((T + 63) / 64) * 16384; }
int64_t items_region_bytes(int S, int T, int H) { return ((int64_t)S * H * ((T + 127) / 128) + 1) * 256; }      // sdpa_dkv3_items.h: one record per item + the empty one
struct BwdWorkspace { int64_t ds_bytes, lse2_off, sched_off, items_off, total; };
BwdWorkspace bwd_workspace(int S, int T, int H) {
    const int64_t ds = ds_region_bytes(S, T, H), sched = ds + lse2_region_bytes(S, T, H), items = sched + 1024;
    return {ds, ds, sched, items, items + items_region_bytes(S, T, H)};
}

}  // namespace

extern "C" int halva_sdpa_block_pairs(int nblk, int start, int br_a, int br_b, int32_t* out) {
    HALVA_CHECK_ARG(nblk > 0 && out, "sdpa_block_pairs: bad arguments");
    const Branch br{br_a, br_b};
    for (int k = 0; k < (nblk + 1) / 2; ++k) {
        int heavy, light;
        paired_blocks(nblk, start, br, k, heavy, light);
        out[2 * k] = heavy, out[2 * k + 1] = light;
    }
    return HALVA_OK;
}

extern "C" int halva_sdpa_causal_fwd(const void* qkv, void* out, float* lse, const int32_t* seq_start, const int32_t* seq_len,
                                     int S, int T, int H, int D, float scale, void* stream) {
    return halva_sdpa_causal_fwd_ld(qkv, out, (int64_t)H * D, lse, seq_start, seq_len, S, T, H, D, scale, stream);
}

extern "C" int halva_sdpa_causal_fwd_ld(const void* qkv, void* out, int64_t ld_out, float* lse, const int32_t* seq_start,
                                        const int32_t* seq_len, int S, int T, int H, int D, float scale, void* stream) {
    return halva_sdpa_branch_fwd(qkv, out, ld_out, lse, seq_start, seq_len, nullptr, nullptr, S, T, H, D, scale, stream);
}

extern "C" int halva_sdpa_branch_fwd(const void* qkv, void* out, int64_t ld_out, float* lse, const int32_t* seq_start,
                                     const int32_t* seq_len, const int32_t* br_a, const int32_t* br_b, int S, int T, int H, int D,
                                     float scale, void* stream) {
    HALVA_CHECK_ARG((br_a == nullptr) == (br_b == nullptr), "sdpa_branch_fwd: br_a and br_b go together");
    HALVA_CHECK_ARG(qkv && out && lse, "sdpa_causal_fwd: null pointer");
    HALVA_CHECK_ARG(ld_out >= (int64_t)H * D && ld_out % 8 == 0, "sdpa_causal_fwd: bad output row stride %lld", (long long)ld_out);
    HALVA_CHECK_ARG(D == 128 || D == 64, "sdpa_causal_fwd: head_dim %d not supported (64 or 128)", D);
    HALVA_CHECK_ARG(S > 0 && T > 0 && H > 0, "sdpa_causal_fwd: bad sizes");
    SdpaParams p = base_params(qkv, T, H, D, scale);
    p.o = (bf16_t*)out;
    p.lse = lse;
    p.seq_start = seq_start, p.seq_len = seq_len;
    p.br_a = br_a, p.br_b = br_b;
    p.ld_o = ld_out;
    return run_fwd<true>(p, S, D, (hipStream_t)stream);
}

extern "C" int halva_sdpa_causal_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                                     float* delta_ws, float* dq_ws, const int32_t* seq_start, const int32_t* seq_len, int S,
                                     int T, int H, int D, float scale, void* stream) {
    return halva_sdpa_causal_bwd_ld(qkv, out, (int64_t)H * D, dout, (int64_t)H * D, lse, dqkv, delta_ws, dq_ws, seq_start, seq_len,
                                    S, T, H, D, scale, stream);
}

extern "C" int halva_sdpa_causal_bwd_ld(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                                        const float* lse, void* dqkv, float* delta_ws, float* dq_ws, const int32_t* seq_start,
                                        const int32_t* seq_len, int S, int T, int H, int D, float scale, void* stream) {
    (void)dq_ws;      // reserved for an atomics-based dQ variant; the shipped dQ kernels need no scratch
    return halva_sdpa_branch_bwd(qkv, out, ld_out, dout, ld_dout, lse, dqkv, delta_ws, seq_start, seq_len, nullptr, nullptr, S, T, H, D,
                                 scale, stream);
}

extern "C" int64_t halva_sdpa_bwd_ws_bytes(int S, int T, int H, int D) {
    return D == 128 ? bwd_workspace(S, T, H).total : 0;      // the dS path is the head_dim-128 instantiation; others use the 3-product dQ kernel
}

extern "C" int halva_sdpa_branch_bwd(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                                     const float* lse, void* dqkv, float* delta_ws, const int32_t* seq_start, const int32_t* seq_len,
                                     const int32_t* br_a, const int32_t* br_b, int S, int T, int H, int D, float scale, void* stream) {
    return halva_sdpa_branch_bwd_ws(qkv, out, ld_out, dout, ld_dout, lse, dqkv, delta_ws, nullptr, 0, seq_start, seq_len, br_a, br_b, S, T, H, D,
                                    scale, stream);
}

extern "C" int halva_sdpa_branch_bwd_ws(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                                        const float* lse, void* dqkv, float* delta_ws, void* ds_ws, int64_t ds_ws_bytes,
                                        const int32_t* seq_start, const int32_t* seq_len, const int32_t* br_a, const int32_t* br_b, int S,
                                        int T, int H, int D, float scale, void* stream) {
    return halva_sdpa_branch_bwd_rope(qkv, out, ld_out, dout, ld_dout, lse, dqkv, delta_ws, ds_ws, ds_ws_bytes, seq_start, seq_len, br_a, br_b,
                                      nullptr, nullptr, 0, S, T, H, D, scale, stream);
}

extern "C" int halva_sdpa_branch_bwd_rope(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                                          const float* lse, void* dqkv, float* delta_ws, void* ds_ws, int64_t ds_ws_bytes,
                                          const int32_t* seq_start, const int32_t* seq_len, const int32_t* br_a, const int32_t* br_b,
                                          const void* rope_cos, const void* rope_sin, int max_pos, int S, int T, int H, int D, float scale,
                                          void* stream) {
    HALVA_CHECK_ARG((rope_cos == nullptr) == (rope_sin == nullptr), "sdpa_branch_bwd_rope: cos and sin go together");
    HALVA_CHECK_ARG(rope_cos == nullptr || T <= max_pos, "sdpa_branch_bwd_rope: T=%d exceeds the cos/sin table (%d rows)", T, max_pos);
    HALVA_CHECK_ARG(ds_ws == nullptr || ds_ws_bytes >= halva_sdpa_bwd_ws_bytes(S, T, H, D),
                    "sdpa_branch_bwd_ws: workspace of %lld bytes, %lld needed", (long long)ds_ws_bytes,
                    (long long)halva_sdpa_bwd_ws_bytes(S, T, H, D));
    HALVA_CHECK_ARG((br_a == nullptr) == (br_b == nullptr), "sdpa_branch_bwd: br_a and br_b go together");
    HALVA_CHECK_ARG(ld_out >= (int64_t)H * D && ld_out % 8 == 0 && ld_dout >= (int64_t)H * D && ld_dout % 8 == 0,
                    "sdpa_causal_bwd: bad row strides %lld / %lld", (long long)ld_out, (long long)ld_dout);
    HALVA_CHECK_ARG(qkv && out && dout && lse && dqkv && delta_ws, "sdpa_causal_bwd: null pointer");
    HALVA_CHECK_ARG(D == 128 || D == 64, "sdpa_causal_bwd: head_dim %d not supported (64 or 128)", D);
    HALVA_CHECK_ARG(S > 0 && T > 0 && H > 0, "sdpa_causal_bwd: bad sizes");
    SdpaParams p = base_params(qkv, T, H, D, scale);
    p.o_in = (const bf16_t*)out;
    p.d_o = (const bf16_t*)dout;
    p.dq = (bf16_t*)dqkv;
    p.dk = p.dq + (int64_t)H * D;
    p.dv = p.dq + 2 * (int64_t)H * D;
    p.lse = const_cast<float*>(lse);
    p.delta = delta_ws;
    p.seq_start = seq_start, p.seq_len = seq_len;
    p.br_a = br_a, p.br_b = br_b;
    p.ld_o = ld_out, p.ld_do = ld_dout;
    if (D == 128 && ds_ws != nullptr) {
        const BwdWorkspace w = bwd_workspace(S, T, H);
        p.ds_ws = (char*)ds_ws;
        p.lse2 = reinterpret_cast<float*>(p.ds_ws + w.lse2_off);
        p.sched = reinterpret_cast<int*>(p.ds_ws + w.sched_off);
        p.items = reinterpret_cast<int*>(p.ds_ws + w.items_off);
    }
    p.ds_nkb = (T + 127) / 128, p.ds_nt = p.stat_nt = (T + 63) / 64;
    p.rope_cos = (const bf16_t*)rope_cos, p.rope_sin = (const bf16_t*)rope_sin, p.rope_max_pos = max_pos;
    const SdpaSwitches sw = read_switches(false, p.ds_ws != nullptr);
    const auto run = [&](auto d) {
        constexpr int HD = decltype(d)::value;
        const BwdPlan plan = choose_bwd<HD, true>(S, T, H, p.ld_qkv, p.ld_do, p.ds_ws != nullptr, p.lse2 != nullptr, rope_cos != nullptr, sw);
        const int rc = launch_bwd<HD, true>(p, S, (hipStream_t)stream, plan);
        if (rc != HALVA_OK || rope_cos == nullptr || plan.rope_fused) return rc;
        // a kernel combination without the rotating epilogues (head_dim 64, no dS workspace, the debugging builds): the rotation as its own launch
        return halva_rope_qk_branch(dqkv, rope_cos, rope_sin, br_a, br_b, (int64_t)S * T, T, H, D, max_pos, 1, stream);
    };
    return D == 128 ? run(std::integral_constant<int, 128>{}) : run(std::integral_constant<int, 64>{});
}

extern "C" int halva_sdpa_full_fwd(const void* qkv, void* out, int N, int S, int H, int D, float scale, void* stream) {
    HALVA_CHECK_ARG(qkv && out, "sdpa_full_fwd: null pointer");
    HALVA_CHECK_ARG(D == 128 || D == 64, "sdpa_full_fwd: head_dim %d not supported (64 or 128)", D);
    HALVA_CHECK_ARG(N > 0 && S > 0 && H > 0, "sdpa_full_fwd: bad sizes");
    SdpaParams p = base_params(qkv, S, H, D, scale);
    p.o = (bf16_t*)out;
    p.ld_o = (int64_t)H * D;
    return run_fwd<false>(p, N, D, (hipStream_t)stream);
}

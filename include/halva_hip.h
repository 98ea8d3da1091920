/* libhalva_hip.so - C ABI of the hand-written gfx950 (MI355X / CDNA4) kernels behind the HALVA DPA step.
 *
 * The reference (pritamqu/HALVA) is pure Python and owns no FFI; its only optimisation seam is the
 * attention monkey-patch (reference llava/train/llama_flash_attn_monkey_patch.py:16-115).  This header is
 * therefore the drop-in boundary defined by this build: each entry point names the reference call it
 * replaces (file:line, relative to the reference tree).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C: raw device pointers + explicit sizes; no torch types.  The caller owns every buffer; no entry
 *     point allocates, frees or synchronises.  All work is enqueued on `stream` (a hipStream_t, NULL = default).
 *   - return value: 0 on success, a negative HALVA_ERR_* otherwise; halva_last_error() gives the text
 *     (thread-local).  Entry points are re-entrant and hold no mutable global state.
 *   - dtype arguments use halva_dtype.  "rows" are tokens (S*T); matrices are row-major.
 *   - sequences are described by seq_start[S], seq_len[S] (int32): the valid tokens of sequence s are
 *     [seq_start[s], seq_start[s]+seq_len[s]) on its T-long padded row (right padding: start 0).
 */
#ifndef HALVA_HIP_H
#define HALVA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALVA_ABI_VERSION 1

typedef enum { HALVA_BF16 = 0, HALVA_F32 = 1 } halva_dtype;

#define HALVA_OK 0
#define HALVA_ERR_INVALID_ARG (-1)
#define HALVA_ERR_LAUNCH (-2)
#define HALVA_ERR_UNSUPPORTED (-3)

int halva_abi_version(void);
const char* halva_last_error(void);

/* ---- Llama RMSNorm.  replaces LlamaRMSNorm.forward (llava/model/language_model/modelling_llama.py:65-70)
 * y = bf16(w * x_f32 * rsqrt(mean(x_f32^2) + eps)) - the module's fp32 value, rounded once (its intermediate cast to the input
 * dtype is a no-op on the fp32 CPU path that parity is defined against); rstd[rows] (f32) is saved for the backward.
 * With HALVA_RMSNORM_MODULE_ROUNDING=1 in the environment (read once per process) the forward instead rounds x * rstd to bf16 before
 * the multiplication with w - bit for bit what the module computes on a bf16 device - for comparisons with the reference's GPU numerics.
 * bwd gives dx only (norm weights are frozen on the LoRA DPA path; llava/train/train_halva.py:1085-1101). */
int halva_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int d, float eps, void* stream);
int halva_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, int64_t rows, int d,
                      void* stream);
/* same with an explicit row stride (elements) for y / dy: lets the normalised rows land directly in the left columns of the
 * [rows, d + G*r] LoRA operand buffer of the next projection (no concat copy). */
int halva_rmsnorm_fwd_ld(const void* x, const void* w, void* y, int64_t ldy, float* rstd, int64_t rows, int d, float eps,
                         void* stream);
int halva_rmsnorm_bwd_ld(const void* dy, int64_t lddy, const void* x, const void* w, const float* rstd, void* dx, int64_t rows,
                         int d, void* stream);
/* the forward of the decoder layer's residual fork: as halva_rmsnorm_fwd_ld, and the row is also written to x_copy [rows, d]
 * (may be NULL) - the buffer the residual connection then accumulates the block's output onto IN PLACE
 * (`hidden_states = residual + ...`, modelling_llama.py:395-417, as a beta = 1 GEMM).  Saves the pass that would otherwise copy the
 * residual into the GEMM's output buffer (hipMemcpy D2D of [rows, d] per residual add: 0.8 % of the 7B step). */
int halva_rmsnorm_fwd_fork_ld(const void* x, const void* w, void* y, int64_t ldy, float* rstd, void* x_copy, int64_t rows, int d,
                              float eps, void* stream);
/* the decoder layer's residual fork in one pass: dx = rmsnorm_bwd(dy) + dres, where dres [rows, d] is the gradient that reaches
 * the same hidden state through the residual connection (modelling_llama.py:395-417: `hidden_states = residual + ...`).  Saves
 * the separate read-read-write pass of autograd's accumulation.  dres == NULL: plain halva_rmsnorm_bwd_ld.  dx may alias dres. */
int halva_rmsnorm_bwd_res_ld(const void* dy, int64_t lddy, const void* x, const void* w, const float* rstd, const void* dres,
                             void* dx, int64_t rows, int d, void* stream);

/* ---- RoPE, in place on the q and k thirds of a packed qkv buffer [rows, 3, H, D] (bf16).
 * replaces apply_rotary_pos_emb (modelling_llama.py:154-169) as called from
 * llava/train/llama_flash_attn_monkey_patch.py:51-55.  cos/sin: [max_pos, D/2] bf16 (the table halves are equal,
 * modelling_llama.py:98-100).  pos: int32 [rows] or NULL for pos = row % T.  inverse != 0 applies the transpose
 * rotation (the backward). */
int halva_rope_qk(void* qkv, const void* cos, const void* sin, const int32_t* pos, int64_t rows, int T, int H, int D,
                  int max_pos, int inverse, void* stream);
/* The same with the positions of branch-packed rows [prefix | A | pad | B] implied by the branch points instead of a table: row t of sequence s
 * (rows = S * T) sits at position t, and at br_a[s] + (t - br_b[s]) once t >= br_b[s] (branch B continues from the prefix: what
 * halva_amd/splice.py:pack_pairs writes into `pos` for every row that carries a token).  br_a / br_b: int32 [S] or both NULL (= pos NULL above). */
int halva_rope_qk_branch(void* qkv, const void* cos, const void* sin, const int32_t* br_a, const int32_t* br_b, int64_t rows, int T, int H,
                         int D, int max_pos, int inverse, void* stream);

/* ---- CLIP's activation.  replaces `input * torch.sigmoid(1.702 * input)` (transformers QuickGELUActivation, reached through
 * llava/model/multimodal_encoder/clip_encoder.py:46 -> CLIPMLP) of the frozen tower: one pass instead of three element-wise kernels, with the
 * same three bf16 roundings.  n elements (multiple of 8), out may be x. */
int halva_quick_gelu(const void* x, void* out, int64_t n, void* stream);

/* ---- SwiGLU.  replaces act_fn(gate_proj(x)) * up_proj(x) (modelling_llama.py:197).  gu = [rows, 2F] (gate | up). */
int halva_swiglu_fwd(const void* gu, void* out, int64_t rows, int F, void* stream);
int halva_swiglu_bwd(const void* dout, const void* gu, void* dgu, int64_t rows, int F, void* stream);
int halva_swiglu_fwd_ld(const void* gu, void* out, int64_t ldo, int64_t rows, int F, void* stream);
int halva_swiglu_bwd_ld(const void* dout, int64_t lddo, const void* gu, void* dgu, int64_t rows, int F, void* stream);

/* ---- causal self-attention on right/left padded rows, bf16, head_dim 128 (Llama) - THE headline kernel.
 * replaces flash_attn_varlen_qkvpacked_func(qkv, cu_q_lens, max_s, 0.0, softmax_scale=None, causal=True)
 * together with unpad_input / pad_input (llava/train/llama_flash_attn_monkey_patch.py:71-91).
 * qkv: [S, T, 3, H, D] packed (RoPE already applied); out: [S, T, H, D]; lse: [S, H, T] f32 (natural log).
 * Padded query rows get zeros (pad_input semantics).  scale = 1/sqrt(D) when <= 0.
 * bwd: dqkv [S, T, 3, H, D] bf16 is fully written (zeros on padded rows); delta_ws: [S, H, T] f32 scratch owned by the
 * caller (written by the dQ launch, read by the dK/dV launch).  dq_ws is IGNORED (may be NULL): the argument survives from an
 * atomics-based dQ design that was never shipped; dQ has its own kernel and needs no scratch. */
int halva_sdpa_causal_fwd(const void* qkv, void* out, float* lse, const int32_t* seq_start, const int32_t* seq_len,
                          int S, int T, int H, int D, float scale, void* stream);
int halva_sdpa_causal_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                          float* delta_ws, float* dq_ws, const int32_t* seq_start, const int32_t* seq_len, int S, int T,
                          int H, int D, float scale, void* stream);
/* same with explicit row strides (elements) of out / dout */
int halva_sdpa_causal_fwd_ld(const void* qkv, void* out, int64_t ld_out, float* lse, const int32_t* seq_start,
                             const int32_t* seq_len, int S, int T, int H, int D, float scale, void* stream);
int halva_sdpa_causal_bwd_ld(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                             const float* lse, void* dqkv, float* delta_ws, float* dq_ws, const int32_t* seq_start,
                             const int32_t* seq_len, int S, int T, int H, int D, float scale, void* stream);

/* Branched causal attention: one packed sequence [prefix | A | pad | B] per row; rows >= br_b[s] (branch B) do not attend to
 * rows [br_a[s], br_b[s]) (branch A and the padding); everything else is causal.  Lets the correct and the hallucinated
 * response of a pair share ONE forward/backward over their common prefix (image + prompt + identical start of the response) -
 * the reference runs the prefix twice, once per row of the concatenated batch (llava/train/halva_trainer.py:434-470).
 * br_a / br_b: int32 [S] row indices, or both NULL = plain causal (the entries above).  Contract: br_b[s] is a multiple of 64
 * (no 32-row strip / 64-key tile straddles it; rows in [br_a + len(A), br_b) are padding whose output is unspecified) and
 * seq_start[s] == 0 for a branched sequence; br_a[s] = br_b[s] >= seq_len[s] marks a sequence without a branch.  RoPE
 * positions of branch B restart at br_a (halva_rope_qk's `pos` argument). */
int halva_sdpa_branch_fwd(const void* qkv, void* out, int64_t ld_out, float* lse, const int32_t* seq_start, const int32_t* seq_len,
                          const int32_t* br_a, const int32_t* br_b, int S, int T, int H, int D, float scale, void* stream);
int halva_sdpa_branch_bwd(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout, const float* lse,
                          void* dqkv, float* delta_ws, const int32_t* seq_start, const int32_t* seq_len, const int32_t* br_a,
                          const int32_t* br_b, int S, int T, int H, int D, float scale, void* stream);
/* The same backward with a caller-owned workspace for dS = P o (dP - delta) (bf16, halva_sdpa_bwd_ws_bytes(S, T, H, D) bytes; 0 for
 * head dims the workspace path does not serve).  With it the backward forms dS once - three launches: delta (+ zeros into dq of padded
 * rows), dK/dV (which stores dS in its register layout), dQ = scale * dS K (which reads it back, HBM-bound) - five matrix products per
 * (query, key) tile pair instead of the seven of the split backward above (S and dP are otherwise formed in both kernels).  Same
 * results to bf16 rounding of dS (which the split backward applies as well before its dQ/dK products); bitwise reproducible.
 * ds_ws == NULL: identical to halva_sdpa_branch_bwd.  The workspace holds no state between calls.
 * Behind the dS region the workspace also carries the row statistics of the dK/dV kernel of this path (sdpa_bwd_dkv3, one wave per SIMD, its
 * steps in generated inline-asm blocks - halva_amd/csrc/sdpa_dkv3.h), written by the delta pass: per (sequence, head) ceil(T / 64) records
 * of 512 bytes, one per 64-row step in sequence coordinates, [lse * log2(e) x 64][-delta x 64] f32 (round 4; round 3 kept two [S, H, T]
 * arrays and wrote -delta to delta_ws, which this path now leaves untouched) - one LDS-DMA request per step fetches both, the dP chain
 * starts from -delta; and 1 KiB of work-queue counters (zeroed by the delta pass of each call): that kernel runs as one persistent workgroup per
 * CU drawing (sequence, head, key block) items from a queue per XCD.  The workspace still holds no state between calls, but one workspace
 * serves ONE call at a time.  HALVA_SDPA_DKV3=0 selects the two-role kernel of rounds 1-2 instead (same results up to bf16 rounding of P
 * before dZ). */
int64_t halva_sdpa_bwd_ws_bytes(int S, int T, int H, int D);
int halva_sdpa_branch_bwd_ws(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout, const float* lse,
                             void* dqkv, float* delta_ws, void* ds_ws, int64_t ds_ws_bytes, const int32_t* seq_start,
                             const int32_t* seq_len, const int32_t* br_a, const int32_t* br_b, int S, int T, int H, int D, float scale,
                             void* stream);
/* The same backward with the INVERSE RoPE of dq and dk applied on the way out: autograd of apply_rotary_pos_emb on the query / key gradients
 * (reference llava/model/language_model/modelling_llama.py:154-169 differentiated; llava/train/llama_flash_attn_monkey_patch.py:58-66 applies the
 * rotation in front of the attention) = halva_sdpa_branch_bwd_ws followed by halva_rope_qk_branch(dqkv, cos, sin, br_a, br_b, ..., inverse = 1),
 * with the same roundings (row rounded to bf16, rotated in fp32 with the bf16 table entries, rounded again) - but inside the store epilogues of
 * the dQ and dK/dV kernels where that kernel combination runs (head_dim 128 with the workspace: sdpa_bwd_dq2 + sdpa_bwd_dkv3), saving one launch
 * and a read-modify-write pass over dq and dk per call; any other combination ends with the rotation as its own launch.  Positions: row t of a
 * sequence sits at position t; rows of branch B (t >= br_b) at br_a + (t - br_b) - what halva_amd/splice.py:pack_pairs feeds the forward's
 * halva_rope_qk.  rope_cos / rope_sin: the [max_pos, D / 2] bf16 tables of halva_rope_qk; both NULL = halva_sdpa_branch_bwd_ws.
 * HALVA_ROPE_FUSED_BWD=0 (A/B switch): always the separate launch. */
int halva_sdpa_branch_bwd_rope(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout, const float* lse,
                               void* dqkv, float* delta_ws, void* ds_ws, int64_t ds_ws_bytes, const int32_t* seq_start,
                               const int32_t* seq_len, const int32_t* br_a, const int32_t* br_b, const void* rope_cos, const void* rope_sin,
                               int max_pos, int S, int T, int H, int D, float scale, void* stream);
/* ---- non-causal self-attention, bf16, head_dim 64, forward only (the CLIP tower runs under no_grad:
 * llava/model/multimodal_encoder/clip_encoder.py:37-49; replaces HF CLIPAttention's softmax(QK^T*scale)V).
 * qkv: [N, S, 3, H, D] packed; out [N, S, H, D]. */
int halva_sdpa_full_fwd(const void* qkv, void* out, int N, int S, int H, int D, float scale, void* stream);

/* ---- bf16 GEMM on MFMA with fused epilogue: C[M,N] = epi(A[M,K] @ B[N,K]^T + bias[N]).
 * replaces the mm_projector Linear/GELU/Linear (llava/model/multimodal_projector/builder.py:39-46) and,
 * with im2col addressing, CLIP's patch-embed Conv2d(3, d, k=14, s=14, bias=False) reached through
 * clip_encoder.py:46.  epilogue: 0 none, 1 GELU(erf).  trans_a / trans_b select the backward forms
 * (A given as [K,M] / B given as [K,N]).  bias may be NULL.  pre_act (optional) receives A B^T + bias before the
 * epilogue (needed by the GELU backward); accumulate != 0 adds into C (gradient accumulation, f32 or bf16). */
int halva_gemm_bf16(const void* A, const void* B, const void* bias, void* C, void* pre_act, int M, int N, int K,
                    int trans_a, int trans_b, int epilogue, halva_dtype out_dtype, int accumulate, void* stream);

/* ---- LoRA weight gradients: C[M, N] (f32) += alpha * A^T B with A [rows, M] and B [rows, N] bf16 column windows of wider row-major
 * buffers (row strides lda / ldb), i.e. what peft's lora_A / lora_B receive from autograd on the DPA path
 * (llava/train/train_halva.py:1085-1101 makes them the only trainable decoder tensors): dB_g = scale * dy_g^T (x A_g^T),
 * dA = (scale * dy B)^T x.  One side of the product is 128..384 wide, the contraction runs over all token rows, so the library
 * GEMM has 32-86 tiles for 256 CUs; here the rows are split into k-slabs (partials in ws, summed in a fixed order - no atomics).
 * ws: scratch of ws_floats >= M * N floats; the number of slabs is what fits, up to one resident
 * round of workgroups (512).  This is halva_wgrad_accumulate_batch with one item. */
int halva_wgrad_accumulate(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int M, int N, int64_t rows, float alpha,
                           float* ws, int64_t ws_floats, void* stream);
/* The same for the two to four products of ONE LoRA group at once (its A factor and its B factors: they become available together in the group's
 * backward - halva_amd/llama.py:_LoraGroupLinear, i.e. peft's LoRA linear backward as used by llava/train/train_halva.py:1085-1101): one launch of
 * the tile kernel and one of the reduction instead of two per product.  Results are BITWISE those of halva_wgrad_accumulate called once per item
 * with the same workspace (same k-slabs, same summation order).  The items are cut in order into chunks of at most 4 whose partials fit the
 * workspace side by side; a chunk whose every item takes the LDS-DMA tile kernel (M and N multiples of 128) is one tile launch, any other chunk one
 * tile launch per item; every chunk ends with one launch of the reduction.  ALL items are validated before anything is launched: an invalid item
 * returns HALVA_ERR_INVALID_ARG with its index in the message and no C of any item has been touched.  items: HOST array of n descriptors. */
typedef struct halva_wgrad_item {
    const void* A;      /* [rows, M] bf16 window, row stride lda */
    int64_t lda;
    const void* B;      /* [rows, N] bf16 window, row stride ldb */
    int64_t ldb;
    float* C;           /* [M, N] f32, += alpha * A^T B */
    int32_t M, N;
    int64_t rows;
    float alpha;
    int32_t reserved;
} halva_wgrad_item;
int halva_wgrad_accumulate_batch(int n, const halva_wgrad_item* items, float* ws, int64_t ws_floats, void* stream);
/* images [n, 3, hw, hw] bf16; weight_kp [d, Kp] bf16 = the conv weight flattened to [d, 3*p*p] and zero padded to
 * Kp (multiple of 8); col_ws: caller scratch [n * (hw/p)^2, Kp] bf16 -> out [n, (hw/p)^2, d] bf16 */
int halva_clip_patch_embed(const void* images, const void* weight_kp, void* col_ws, void* out, int n, int hw, int p, int d,
                           int Kp, void* stream);
/* Same with a bias and a 'valid' grid of floor(hw/p)^2 patches: SigLIP's Conv2d(3, d, k=14, s=14, padding="valid") of
 * the VILA path (vila/model/multimodal_encoder/siglip/modeling_siglip.py SiglipVisionEmbeddings, reached through
 * vila/model/multimodal_encoder/vision_encoder.py:136-140).  bias [d] bf16 or NULL. */
int halva_vit_patch_embed(const void* images, const void* weight_kp, const void* bias, void* col_ws, void* out, int n, int hw,
                          int p, int d, int Kp, void* stream);
/* dh[M,N] = dy[M,N] * gelu'(h[M,N]) (h = pre-activation), and column sums for the bias grads. */
int halva_gelu_bwd(const void* dy, const void* h, void* dh, int64_t M, int N, void* stream);
int halva_colsum(const void* x, float* out, int64_t M, int N, void* stream);
/* dst[c][r] = src[r][c], bf16, [rows x cols] with row strides ld_src / ld_dst in elements (rows, cols, strides multiples of 8; 16-byte
 * aligned pointers).  Serves the once-per-optimizer-step refresh of the transposed, LoRA-merged weight copy the decoder's dgrad GEMMs read
 * (halva_amd/llama.py:LoraGroup.refresh_tail; the reference has no counterpart - peft keeps W, A, B apart and autograd forms dx from each):
 * `torch.addmm(W.t(), ...)` spent 0.45 ms per group copying the strided W^T with the framework's element-wise copy kernel. */
int halva_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols, void* stream);
/* Merge one LoRA target into its base weight, in place (peft's merge_and_unload, which the reference's loaders call before evaluation:
 * llava/model/builder.py:70-71, vila/model/builder_halva.py:137-138):
 *   w[n, k] <- bf16_rne( float(w[n, k]) + scale * sum_{j < r} float(B[n, j]) * float(A[j, k]) ),   n < N, k < K
 * w [N, K] is a window of a wider row-major bf16 buffer (row stride ldw >= K elements: rows [off, off + n) and columns [0, in) of a fused
 * weight); B [N, r] and A [r, K] bf16 with row strides ldb, lda.  fp32 accumulation on the MFMA in ascending j (one fixed order: no split
 * over j, no atomics - the same bits on every run, whatever GEMM tables the framework uses), one rounding, every element of w read and
 * written once; nothing outside the window is read or written.  Any N, K, r >= 1; 16-byte accesses where pointer and stride allow. */
int halva_lora_merge(void* w, int64_t ldw, const void* B, int64_t ldb, const void* A, int64_t lda, int N, int K, int r, float scale,
                     void* stream);

/* ---- vision-side row kernels (VILA path).
 * LayerNorm over rows of [rows, d] bf16 (d % 8 == 0, d <= 8192): the nn.LayerNorm of mlp_downsample
 * (vila/model/multimodal_projector/base_projector.py:78) and of the CLIP / SigLIP encoder blocks.
 * stats (optional) receives (mean, rstd) per row as f32 [rows, 2] for the parameter gradients:
 * dw[j] += sum_r dy[r,j] * xhat[r,j], db[j] += sum_r dy[r,j] (f32 accumulators; the input carries no gradient
 * because the vision tower is frozen, src_vila/halva_vila_13b.sh:44).
 * downsample2x2: DownSampleBlock.flat_square (base_projector.py:33-54): x [n, g*g, c] -> out [n, G*G, 4c], G = ceil(g/2),
 * odd grids zero padded, token order and channel order exactly as the reference's view/permute chain. */
int halva_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* stats, int64_t rows, int d, float eps,
                        void* stream);
int halva_layernorm_bwd_params(const void* dy, const void* x, const float* stats, float* dw, float* db, int64_t rows, int d,
                               void* stream);
int halva_downsample2x2(const void* x, void* out, int n, int g, int c, void* stream);

/* ---- image preprocessing on the GPU.  replaces, for a batch of DECODED uint8 RGB images, the per-sample
 * expand2square + processor.preprocess of HallDataset.__getitem__ (llava/train/train_halva.py:735-751: PIL paste on a
 * mean-coloured square, CLIPImageProcessor resize(shortest_edge, BICUBIC) / center_crop / rescale / normalize) and the
 * VILA twin's `image.resize((S, S))` + SiglipImageProcessor (vila/mm_utils.py:150-193).  Pillow's 8-bit resample arithmetic
 * is reproduced exactly (uint8 results bit-exact; the float output is a per-channel 256-entry table built by the host from
 * rescale_factor / mean / std, so it is bit-exact too).  One descriptor per image; coefficient / bounds tables are the
 * host's precompute_coeffs (22-bit fixed point), shared between images of equal geometry.
 * tmp: uint8 scratch for the horizontal pass, out: [n_images, 3, crop_h, crop_w] bf16 or f32. */
typedef struct {
    int64_t src_off;              /* byte offset of the [src_h, src_w, 3] image in src_pack */
    int64_t tmp_off;              /* byte offset of the [tmp_rows, out_w, 3] horizontal-pass result in tmp */
    int32_t src_h, src_w;
    int32_t pad_x, pad_y;         /* position of the image on the (virtual) expand2square canvas */
    int32_t bg[3];                /* canvas fill colour */
    int32_t out_h, out_w;         /* size after the resize, before the crop */
    int32_t row0, tmp_rows;       /* canvas rows [row0, row0 + tmp_rows) feed the vertical pass */
    int32_t kh_off, ksize_h, bh_off;
    int32_t kv_off, ksize_v, bv_off;   /* vertical bounds are relative to row0 */
    int32_t crop_y, crop_x;
    int32_t need_h, need_v;
} HalvaImageDesc;
int halva_image_preprocess(const void* src_pack, const HalvaImageDesc* descs, const int32_t* coef, const int32_t* bounds,
                           const float* lut, void* tmp, void* out, int n_images, int max_tmp_pixels, int crop_h, int crop_w,
                           halva_dtype out_dtype, void* stream);

/* ---- splice gather.  replaces the per-sample python loop of prepare_inputs_labels_for_multimodal[_signed]
 * (llava/model/llava_arch.py:285-374): out[r] = embed[src[r]] if src[r] >= 0, feats[-src[r]-2] if src[r] <= -2,
 * zeros if src[r] == -1 (padding).  src is the host-computed index plan, rows = S*T. */
int halva_splice_rows(const void* embed, const void* feats, const int32_t* src, void* out, int64_t rows, int d,
                      void* stream);

/* ---- token log-prob.  replaces logits.log_softmax(-1) + gather (llava/train/halva_trainer.py:406-407).
 * logits [R, V] (row stride ld elements), target int32 [R] (already shifted; IGNORE_INDEX mapped to 0 by the
 * caller exactly as halva_trainer.py:406).  logp[R], lse[R] f32.
 * bwd: dlogits[r, v] = g[r] * (1[v == target[r]] - exp(logits[r,v] - lse[r])); may alias logits. */
int halva_token_logp_fwd(const void* logits, halva_dtype dt, int64_t ld, const int32_t* target, float* logp, float* lse,
                         int64_t R, int V, void* stream);
int halva_token_logp_bwd(const void* logits, halva_dtype dt, int64_t ld, const int32_t* target, const float* lse,
                         const float* g, void* dlogits, int64_t R, int V, void* stream);

/* ---- KL(ref || policy) per row.  replaces the softmax/log/product/mask/sum chain (halva_trainer.py:583-588).
 * kl[r] = w[r] * sum_v p_ref (log p_ref - log p_pol), computed with log-softmax algebra (identical where the
 * reference's softmax().log() is finite).  If dpol != NULL it also receives d kl[r] / d pol_logits[r, :]
 * = w[r] * (p_pol - p_ref) * gscale (may alias pol). */
int halva_kl_rows(const void* pol, const void* ref, halva_dtype dt, int64_t ld, const float* w, float* kl, void* dpol,
                  float gscale, int64_t R, int V, void* stream);

/* ---- phrase accumulation.  replaces accumulate_logps (halva_trainer.py:411-419) incl. the loss-mask multiply
 * (:556-557): acc[b, p] = sum_t logp[b,t] * (labels[b,t] != -100) * (signs[b,t] == slot_ids[p]).
 * slot_ids: sorted unique non-zero sign ids of the WHOLE half batch (host computed).  bwd scatters dacc back. */
int halva_phrase_sum_fwd(const float* logp, const int64_t* labels, const int64_t* signs, const int64_t* slot_ids, int P,
                         float* acc, int B, int T1, void* stream);
int halva_phrase_sum_bwd(const float* dacc, const int64_t* labels, const int64_t* signs, const int64_t* slot_ids, int P,
                         float* dlogp, int B, int T1, void* stream);

/* ---- KV-cached decoding (greedy generation, halva_amd/decode.py).  Cache per layer: kcache, vcache bf16 [B, H, Lcap, D] with D = 128,
 * lens int32 [B] on the device (the filled slots of row b are [0, lens[b]); no host-side length reaches a launch).
 *
 * RoPE + append of the new token.  replaces the decode branch of LlamaAttention.forward: apply_rotary_pos_emb at position
 * `attention_mask.sum(1) - 1` (llava/model/llava_arch.py:90-98) and `torch.cat([past_key_value[0], key_states], dim=2)` /
 * the value concat (llava/model/language_model/modelling_llama.py:295-305).  qkv: [B, 3, H, D] rows with stride ldqkv elements (the fused
 * q|k|v projection).  With p = lens[b]: q of row b rotated in place at position p (halva_rope_qk's arithmetic), the rotated k and the plain
 * v written to slot p of the cache, then lens[b] = p + 1.  cos / sin: [max_pos, D/2] bf16 (kernels.rope_tables).  A row with
 * p >= min(Lcap, max_pos) is left untouched (the caller sizes the cache; nothing is written out of bounds). */
int halva_decode_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, void* kcache, void* vcache,
                             int32_t* lens, int B, int H, int D, int Lcap, void* stream);
/* Single-query attention over the cache.  replaces the decode-time attention of LlamaAttention.forward (modelling_llama.py:307-340:
 * q_len = 1, softmax(q K^T / sqrt(D)) V over the cached keys).  q: row b, head h at q[b * ldq + h * D] (the rotated q third of the qkv rows);
 * out: bf16 row b at out[b * ld_out] (the o projection's operand buffer).  fp32 scores, online softmax.  Split KV: one workgroup per
 * (chunk of KC keys, head, row) writes a partial (m, l, o[D]) in fp32 to `ws`; a second launch combines the ceil(lens[b] / KC) partials of
 * (b, h) in chunk order.  KC (halva_decode_attn_kc) does not depend on B: row b's output is bitwise the same in any batch.  Slots at or
 * beyond lens[b] and unused workspace are never read.  scale = 1/sqrt(D) when <= 0.  ws_bytes >= halva_decode_attn_ws_bytes(B, H, Lcap). */
int halva_decode_attn(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out, int64_t ld_out,
                      void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, void* stream);
/* Keys per split-KV chunk of halva_decode_attn (the compile-time constant 256) and its workspace size in bytes (0 for bad sizes). */
int halva_decode_attn_kc(void);
int64_t halva_decode_attn_ws_bytes(int B, int H, int Lcap);
/* Measurement aid (tools/bench_decode.py; no reference counterpart): halva_decode_attn with an explicit chunk of kc = 64, 128 or 256
 * keys - how the constant above was chosen.  Workspace: B * H * ceil(Lcap / kc) * (D + 2) floats. */
int halva_decode_attn_chunked(const void* q, int64_t ldq, const void* kcache, const void* vcache, const int32_t* lens, void* out,
                              int64_t ld_out, void* ws, int64_t ws_bytes, int B, int H, int D, int Lcap, float scale, int kc, void* stream);

/* ---- Extending a kept cache by up to n rows per sequence (halva_amd/decode.py:extend - sessions, chunked prefill, block teacher forcing).
 * stands in for the reference's multi-turn use of HF's cache: a forward with past_key_values and q_len = n (modelling_llama.py:295-340, the
 * cache concat and the [q_len, past + q_len] causal mask).  Same cache layout, D = 128; lens int32 [B] (past[b] = lens[b]) and n_new int32 [B]
 * (0 <= n_new[b] <= n) live on the device, no launch takes a host-side length.  Three launches in this order; the first two only read lens,
 * so no workgroup reads a lens value written by its own launch.
 *
 * RoPE + append.  qkv: bf16 [B, n, 3, H, D], row i of sequence b at qkv[b * ldseq + i * ldrow].  For i < n_new[b], p = lens[b] + i: q and k of
 * the row rotated with row p of cos / sin (halva_decode_rope_append's arithmetic by construction: both kernels call one routine), q in place, the rotated k and the plain v written
 * to slot p.  Rows i >= n_new[b] are neither read nor written; a row with p >= min(Lcap, max_pos) is skipped (the caller refuses such calls;
 * nothing is written out of bounds).  One workgroup per (row, sequence). */
int halva_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos, void* kcache, void* vcache,
                             const int32_t* lens, const int32_t* n_new, int B, int n, int H, int D, int Lcap, void* stream);
/* Attention of the new rows, after the append and before the advance:
 *   out[b, i, h, :] = softmax(scale q[b, i, h] . K[b, h, 0 .. past[b] + i]) V[b, h, 0 .. past[b] + i]      for i < n_new[b]
 * (key past + j is visible to row i iff j <= i); other out rows are untouched.  q: row at q[b * ldseq + i * ldrow + h * D] (the rotated q third of
 * the qkv rows), out: bf16 row at out[b * ld_out_seq + i * ld_out_row + h * D].  One workgroup of 4 waves per (128 query rows, head, sequence)
 * walks the keys from 0 in 64-key LDS tiles: Q K^T and P V on v_mfma_f32_32x32x16_bf16 (V read transposed by ds_read_b64_tr_b16), fp32 online
 * softmax in the log2 domain whose exponent reference starts at the first tile (it always holds key 0: finite for any real logits) and moves
 * per row.  One reduction order fixed by (past[b], i) alone, no float atomics: row (b, i) is bitwise the same at any B and any n_new of the
 * other sequences.  Slots at or beyond past[b] + n_new[b] and q rows at or beyond n_new[b] are never read.  scale = 1/sqrt(D) when <= 0.
 * ws_bytes >= halva_extend_attn_ws_bytes(B, n, H, Lcap), which is 0 (no partials; ws may be NULL). */
int halva_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* kcache, const void* vcache, const int32_t* lens,
                      const int32_t* n_new, void* out, int64_t ld_out_row, int64_t ld_out_seq, void* ws, int64_t ws_bytes, int B, int n, int H,
                      int D, int Lcap, float scale, void* stream);
int64_t halva_extend_attn_ws_bytes(int B, int n, int H, int Lcap);
/* lens[b] = min(lens[b] + n_new[b], Lcap): a launch of its own behind the attention. */
int halva_extend_advance(int32_t* lens, const int32_t* n_new, int B, int Lcap, void* stream);

/* ---- Forks of a kept cache (halva_amd/decode.py:ForkCache - n continuations over one shared prompt, many questions about one image; no
 * reference counterpart: HF repeats the prompt's cache per returned sequence).  M members read P prefix rows of a parent cache
 * pk, pv bf16 [Bp, H, Lpre, D] in place and own kown, vown bf16 [M, H, Lown, D], D = 128.  prefix_of int32 [M]: the parent row of each member,
 * non-decreasing (members of one row are contiguous), values in [0, P); prefix_lens int32 [P]: the rows of each prefix, recorded at fork
 * time; own_lens int32 [M].  All of them live on the device.  Own row t of member m sits at position prefix_lens[prefix_of[m]] + t.  Parent
 * slots at or beyond prefix_lens[p] and own slots at or beyond own_lens[m] are never read; nothing is copied from the parent.
 *
 * RoPE + append of one new row per member: halva_decode_rope_append (the same routine) with the row rotated at position
 * prefix_lens[prefix_of[m]] + own_lens[m] and written to own slot own_lens[m]; own_lens[m] += 1.  A full own cache, or a position at or
 * beyond max_pos, leaves member m untouched. */
int halva_fork_rope_append(void* qkv, int64_t ldqkv, const void* cos, const void* sin, int max_pos, const int32_t* prefix_lens,
                           const int32_t* prefix_of, void* kown, void* vown, int32_t* own_lens, int M, int P, int H, int D, int Lown,
                           void* stream);
/* Single-query attention of member m over parent keys [0, prefix_lens[p]) of row p = prefix_of[m] followed by its own keys
 * [0, own_lens[m]).  Split-KV with 256-key chunks: a prefix pass (one workgroup per chunk, head, prefix row and block of up to 16 members
 * loads the chunk's K and V once and serves every member of the block from it), an own pass (halva_decode_attn's partial pass over the own
 * rows, chunked from own key 0) and a combine pass over ceil(prefix_lens / 256) + ceil(own_lens / 256) partials in that order.  No float
 * atomics; one reduction order fixed by (prefix_lens[p], own_lens[m]) alone: member m's bits do not depend on M, on the other members, on
 * its place in a block or on other prefix rows.  own_lens[m] = 0 is attention over the prefix alone.  Unused workspace is never read.
 * scale = 1/sqrt(D) when <= 0.  ws_bytes >= halva_fork_decode_attn_ws_bytes(M, H, Lpre, Lown) (0 for bad sizes). */
int halva_fork_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens, const int32_t* prefix_of,
                           const void* kown, const void* vown, const int32_t* own_lens, void* out, int64_t ld_out, void* ws, int64_t ws_bytes,
                           int M, int P, int H, int D, int Lpre, int Lown, float scale, void* stream);
int64_t halva_fork_decode_attn_ws_bytes(int M, int H, int Lpre, int Lown);
/* Up to n rows per member: halva_extend_rope_append and halva_extend_attn with the prefix in front.  Row i < n_new[m] goes to own slot
 * own_lens[m] + i at position prefix_lens[p] + own_lens[m] + i; the attention walks the 64-key tiles of the prefix row first (all visible,
 * the last one masked at prefix_lens[p]; the exponent reference starts there) and then the own tiles exactly as halva_extend_attn does with
 * past = own_lens[m] - one kernel body, one tile loop.  Row (m, i)'s bits do not depend on the other members or their n_new.  The prefix
 * read is not shared between members here.  halva_extend_advance(own_lens, n_new, M, Lown) follows. */
int halva_fork_extend_rope_append(void* qkv, int64_t ldrow, int64_t ldseq, const void* cos, const void* sin, int max_pos,
                                  const int32_t* prefix_lens, const int32_t* prefix_of, void* kown, void* vown, const int32_t* own_lens,
                                  const int32_t* n_new, int M, int n, int P, int H, int D, int Lown, void* stream);
int halva_fork_extend_attn(const void* q, int64_t ldrow, int64_t ldseq, const void* pk, const void* pv, const int32_t* prefix_lens,
                           const int32_t* prefix_of, const void* kown, const void* vown, const int32_t* own_lens, const int32_t* n_new, void* out,
                           int64_t ld_out_row, int64_t ld_out_seq, int M, int n, int P, int H, int D, int Lpre, int Lown, float scale, void* stream);

/* ---- Beam search over a forked cache (halva_amd/decode.py:BeamCache, beam_search).  HF re-gathers every layer's cache by the chosen beams
 * after every step (`reorder_cache`: an index_select over all K / V rows); here the M = B * K members of a fork (prefix_of[m] = m / K) write
 * own slot (m, t) once and never move it, and an ancestry table anc int32 [M, Lown] says, for member m and own row t < own_lens[m], whose own
 * slot t holds row t of m's history.
 *
 * halva_beam_decode_attn: halva_fork_decode_attn with key t of member m's own pass fetched from slot (anc[m][t], h, t).  The prefix pass, the
 * combine pass, the workspace and every reduction order are halva_fork_decode_attn's: with anc[m][t] = m the two give the same bits, and with
 * any table the bits of the fork attention on own caches materialised by that gather.  A table entry outside [0, M) is clamped into it (never
 * an address outside the caches).  Own slots at or beyond own_lens[m], and slots (m', t) with m' != anc[m][t], are never read for member m. */
int halva_beam_decode_attn(const void* q, int64_t ldq, const void* pk, const void* pv, const int32_t* prefix_lens, const int32_t* prefix_of,
                           const void* kown, const void* vown, const int32_t* own_lens, const int32_t* anc, void* out, int64_t ld_out,
                           void* ws, int64_t ws_bytes, int M, int P, int H, int D, int Lpre, int Lown, float scale, void* stream);
/* The next step's table from this step's parents: with t = own_lens[m] (one layer's lengths, BEFORE this step's append),
 * anc_dst[m][j] = anc_src[parent[m]][j] for j < t and anc_dst[m][t] = m - the slot halva_fork_rope_append is about to write.  anc_dst[m][j]
 * for j > t is not written.  A parent outside [0, M), or t outside [0, Lown), leaves row m of anc_dst untouched.  The two tables must not
 * overlap (anc_dst == anc_src included): HALVA_ERR_INVALID_ARG. */
int halva_beam_advance(const int32_t* anc_src, int32_t* anc_dst, const int32_t* parent, const int32_t* own_lens, int M, int Lown, void* stream);
/* Candidate selection, one prompt = K consecutive rows: logits fp32 [B * K, V] with row stride ld >= V, beam_scores fp32 [B * K] ->
 * cand_score fp32, cand_token int32, cand_beam int32, each [B, C]: the C best of the prompt's K * V values
 *     beam_scores[k] + (x_i - lse_k),   lse_k = max + log(sum exp(x - max))  of row k in fp32,
 * descending, ties by the lower flat index k * V + i; cand_beam is k (within the prompt), cand_token is i.  What HF's beam search computes as
 * log_softmax + running score, reshape to [B, K * V], topk(C) - without materialising [B, K * V] and without a sort: a row pass (one
 * 1024-lane workgroup per row holds it in registers, finds the row's own C-th largest score by count-bisection and compacts its <= C
 * survivors) and a group pass that ranks the K * C survivors by counting.  Every sum runs in one order fixed by V alone, no float atomics: a
 * prompt's outputs are bitwise the same for any B, at any position and row stride.  If a row holds a NaN or +inf, or nothing above -inf, or
 * its beam score is not finite, every cand_token of that prompt is -1 (cand_beam -1, cand_score NaN); other prompts are unaffected.
 * Limits: V <= halva_beam_select_max_vocab() (32768), K <= halva_beam_select_max_beams() (16), K <= C <= min(64, K * V)
 * (halva_beam_select_max_candidates()); anything else is HALVA_ERR_INVALID_ARG.  ws_bytes >= halva_beam_select_ws_bytes(B * K, C). */
int halva_beam_select(const float* logits, int64_t ld, const float* beam_scores, float* cand_score, int32_t* cand_token, int32_t* cand_beam,
                      void* ws, int64_t ws_bytes, int B, int K, int C, int V, void* stream);
int halva_beam_select_max_vocab(void);
int halva_beam_select_max_beams(void);
int halva_beam_select_max_candidates(void);
int64_t halva_beam_select_ws_bytes(int M, int C);

/* ---- Sampling (generate with do_sample=True, halva_amd/decode.py:sample).  replaces what HF's generate runs per step behind the reference's
 * `model.generate(..., do_sample=True, temperature=args.temperature, top_p=args.top_p, ...)` (eval_hall/model_chair_loader.py:124-130):
 * TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1) -> softmax -> torch.multinomial, i.e. about ten
 * launches and a [B, V] sort, as ONE launch without a sort (one workgroup per row, the row read once and held in registers).
 *   logits fp32 [B, V], row stride ld >= V elements (columns [V, ld) are never read); u fp32 [B] on the device, each in [0, 1) - the
 *   caller's random numbers, the kernel holds no generator; temperature > 0; top_k >= 0 (0 = off); 0 < top_p <= 1.
 * With x_i = l_i / temperature:  K1 = { i : x_i > -inf and #{ j : x_j > x_i } < top_k }  (top_k = 0 or >= V: every x_i > -inf);
 * p = softmax of x over K1;  K2 = { i in K1 : sum_{j in K1, x_j > x_i} p_j < top_p }  (top_p = 1: K1).  K2 is never empty and always
 * { i : x_i >= thr }: ties at either cut are all kept, as in HF.  With q = p renormalised over K2, token[b] = the first column k of K2, in
 * ascending column order, with sum_{i in K2, i <= k} q_i > u[b]; the last column of K2 when rounding leaves none.
 * token int64 [B]; thr fp32 [B] (the threshold on x) and kept int32 [B] (|K2|) are diagnostics, NULL allowed.  A row that holds a NaN or
 * +inf, or nothing above -inf, gets token -1, kept 0, thr NaN; other rows are unaffected.  Every sum runs in one fixed order that depends on
 * V alone and there are no float atomics: row b's outputs are bitwise the same in any batch and at any row position.
 * V <= halva_sample_max_vocab() (32768, what the registers of one 1024-lane workgroup hold); larger V is HALVA_ERR_INVALID_ARG. */
int halva_sample_top_k_top_p(const float* logits, int64_t ld, const float* u, int64_t* token, float* thr, int32_t* kept, int B, int V,
                             float temperature, int top_k, float top_p, void* stream);
int halva_sample_max_vocab(void);

/* ---- Contrastive decoding (generate with images_cd= / negative_input_ids= / guidance_scale=, halva_amd/decode.py:contrast).  One launch for
 * the per-step token rule of visual contrastive decoding (Leng et al., "Mitigating Object Hallucinations in Large Vision-Language Models
 * through Visual Contrastive Decoding", CVPR 2024, eqs. 3 and 4: logits of the prompt as given against logits of the prompt with a degraded
 * image, under an adaptive plausibility constraint) and of classifier-free guidance as HF's generate runs it
 * (transformers/generation/logits_process.py:UnbatchedClassifierFreeGuidanceLogitsProcessor, guidance_scale = 1 + alpha, beta = 0), followed
 * by the warpers and the draw of halva_sample_top_k_top_p.
 *   logits, logits_cd fp32 [B, V] with row strides ld, ld_cd >= V elements (columns [V, ld) are never read); u as in
 *   halva_sample_top_k_top_p; alpha >= 0, finite; log_beta = log(beta) <= 0, -inf for beta = 0; temperature, top_k, top_p as there.
 * Per row, in fp32, each operation rounded once and none fused (float32 arithmetic on the host gives the same bits):
 *   m = max_i l_i;  cut = m + log_beta;  x_i = -inf where l_i < cut, else (1 + alpha) * l_i - alpha * lcd_i as product, product, difference,
 *   1 + alpha being formed once on the host as a float.
 * From x on the rule is halva_sample_top_k_top_p's with x in place of the logits: / temperature, K1, K2, ties kept at both cuts, the draw,
 * the same fixed reduction orders.  top_k = 1, top_p = 1, temperature = 1, u = 0 is greedy contrast: the lowest index among the maxima of x.
 * The raw-logit rule (VCD) and the log-softmax rule (HF: g * (s - s_u) + s_u) differ by a constant per row, hence in nothing that is
 * returned but thr, which is on this x.
 * A masked column's lcd does not matter: it is masked before x is formed, so a NaN or an inf there changes nothing.
 * token int64 [B]; thr fp32 [B] (the threshold on x / temperature), kept int32 [B] (|K2|) and plausible int32 [B] (#{ i : l_i >= cut }) are
 * diagnostics, NULL allowed.  token -1, kept 0, thr NaN for a row where l holds a NaN or +inf or nothing above -inf (plausible 0; lcd is not
 * read), where lcd holds a NaN or +inf in a column that is not masked, or where x holds a NaN or +inf (-inf - -inf; lcd = -inf with
 * alpha > 0); other rows are unaffected.  No float atomics; row b's outputs are bitwise the same in any batch, at any row position and with
 * any strides.  Each row is read from HBM once.  V <= halva_sample_max_vocab(); anything else is HALVA_ERR_INVALID_ARG. */
int halva_contrast_select(const float* logits, int64_t ld, const float* logits_cd, int64_t ld_cd, const float* u, int64_t* token, float* thr,
                          int32_t* kept, int32_t* plausible, int B, int V, float alpha, float log_beta, float temperature, int top_k,
                          float top_p, void* stream);

/* ---- hardware-layout probes used by the GPU tests (MFMA fragment maps, ds_read_b64_tr_b16). */
int halva_probe_layouts(int32_t* out, int n, void* stream);
/* ---- measurement aid (bench.py's clock trace; no reference counterpart): `blocks` one-wave workgroups each spin for `spin_ticks` ticks of
 * the constant 100 MHz counter and report out[4 b + {0,1,2,3}] = {shader cycles elapsed (s_memtime), 100 MHz ticks elapsed (s_memrealtime),
 * start tick, XCC id}: shader MHz = 100 * out[4b] / out[4b+1], the clock the chip holds while the step's kernels run beside the probe. */
int halva_clock_probe(uint64_t* out, int blocks, int spin_ticks, void* stream);
/* Host-side mirror (same inline function the kernels call) of how the forward and the dQ kernel pair the 256-row blocks of a sequence under
 * the causal mask: out[2k], out[2k+1] = the heavier and the lighter block of workgroup k, k < (nblk + 1) / 2 (equal for the middle block of
 * an odd count).  br_a / br_b as in halva_sdpa_branch_fwd (0x7fffffff for both: plain causal, i.e. nblk-1-k with k).  No GPU work: for
 * tests of the index arithmetic. */
int halva_sdpa_block_pairs(int nblk, int start, int br_a, int br_b, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* HALVA_HIP_H */

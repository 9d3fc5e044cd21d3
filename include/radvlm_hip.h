/* radvlm_hip.h -- C ABI of libradvlm_hip.so: the MI355X (gfx950) kernels of the LLaVA training hot path.
 *
 * Drop-in boundary: the reference (rfahrn/RadVLM) has no C/FFI surface of its own -- its
 * hot path bottoms out in torch/HF Python calls.  Each entry point below therefore names the reference call site
 * (file:line under /root/reference/finetuning/llava, or HF: = transformers as pinned by the reference) whose
 * arithmetic it replaces.  Conventions for every function:
 *   - plain device pointers + sizes, no torch types; bf16 = raw uint16 storage; strides (ld*) in ELEMENTS;
 *   - asynchronous on `stream` (a hipStream_t), no allocation, no host sync;
 *   - no state that depends on a call's arguments.  What the library does keep, per process (one process drives one GPU): the
 *     GEMM launch configuration (CU budget, rv_gemm_set_cu_budget; tile-selection hook, rv_gemm_select_kernel) and "dynamic LDS
 *     size attribute already set" flags per kernel instantiation.  Results never depend on it, only the launch shape does;
 *   - `zeros16` is any 16-byte-aligned device buffer of >= 16 zero bytes (source for out-of-range tile chunks);
 *   - returns 0 (RV_OK) or a negative error code (RV_ERR_*), which the Python binding raises as an exception.
 */
#ifndef RADVLM_HIP_H
#define RADVLM_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RV_ACT_NONE 0
#define RV_ACT_QUICK_GELU 1 /* x*sigmoid(1.702x): HF:activations.py QuickGELUActivation (CLIP MLP) */
#define RV_ACT_GELU 2       /* erf GELU: torch.nn.GELU in multimodal_projector/builder.py:44 */
#define RV_ACT_GELU_TANH 3  /* gelu_pytorch_tanh: SigLipMLP, multimodal_encoder/siglip_encoder.py:83,:243-256 */

/* Library version / build arch string ("gfx950"). */
const char* rv_version(void);

/* ---- GEMM -------------------------------------------------------------------------------------------------
 * C[M,N] = act(A[M,K] * B[N,K]^T + bias[N]) + residual[M,N]          (bf16 in, fp32 accumulate)
 * = torch.nn.functional.linear at: modeling_llama.py:332-338,377 (q/k/v/o), :226 (gate/up/down), :1323 (lm_head);
 *   HF:models/clip/modeling_clip.py:298-350 (CLIP q/k/v/out/fc1/fc2), :209 (patch conv as GEMM over im2col rows);
 *   multimodal_projector/builder.py:41-48.  Backward (dgrad / wgrad) goes through rv_gemm_bf16 below, which reads its operands
 *   contraction-major in place (no transposed copies).
 * K % 8 == 0, lda % 8 == 0, ldb % 8 == 0.  out_f32: C is fp32 (else bf16).  residual may alias C (accumulate).
 */
int rv_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias,
                    const void* residual, int64_t ldr, int M, int N, int K, int act, int out_f32, int res_f32,
                    const void* zeros16, void* stream);
/* General form: op(A)[M,K] * op(B)[N,K]^T with either operand stored contraction-major instead:
 *   trans_a != 0: A is stored [K, M] (row stride lda);  trans_b != 0: B is stored [K, N] (row stride ldb).
 * Lets the autograd GEMMs read their operands in place (hardware-transposed LDS reads, ds_read_b64_tr_b16):
 *   dgrad dX[M,Kin] = dY[M,Nout] * W[Nout,Kin]        -> trans_b (W is [contraction, Kin]);
 *   wgrad dW[Nout,Kin] = dY[M,Nout]^T * X[M,Kin]      -> trans_a and trans_b (both are [contraction=tokens, features]).
 * Feature dimensions of transposed operands must be multiples of 8.  C = act(alpha * op(A) op(B)^T + bias) + residual;
 * alpha carries the LoRA scaling lora_alpha / r (peft LoraLayer, train/train.py:1515-1532). */
int rv_gemm_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias,
                 const void* residual, int64_t ldr, int M, int N, int K, int trans_a, int trans_b, float alpha, int act,
                 int out_f32, int res_f32, const void* zeros16, void* stream);
/* Extended form:  C = act(alpha * (op(A) op(B)^T + op(A2) op(B2)^T) + bias) + residual.
 *  - (A2, B2, K2): optional second operand pair sharing the transposition flags -- the fused LoRA GEMM
 *    y = [x | t] [W | B]^T (forward) and dx = [dy | dt] [W ; A] (dgrad) of peft's LoraLayer (train/train.py:1515-1532)
 *    in one launch, without a second pass over y.  NULL / 0 disables it.
 *  - workspace (optional fp32 scratch): lets outputs with few tiles and a long contraction (LoRA dA/dB) run split-K over
 *    the idle CUs; partial sums are combined by a deterministic reduce kernel (no atomics). */
int rv_gemm_bf16_ex(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias,
                    const void* residual, int64_t ldr, int M, int N, int K, int trans_a, int trans_b, float alpha, int act,
                    int out_f32, int res_f32, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, int K2,
                    void* workspace, int64_t workspace_bytes, const void* zeros16, void* stream);
/* ---- GEMMs with a fused elementwise epilogue (HBM passes removed from the decoder layer) ----------------------------------
 * Each runs on the 256x256-tile kernel when the output is large enough for it and otherwise performs the unfused sequence itself
 * (GEMM, then the elementwise kernel) -- bit-identical results either way: the fused epilogues round where the unfused path stored.
 *
 * rv_gemm_rope_bf16: C[M,N] = A[M,K] B[N,K]^T + bias, then rotary embedding on the first rope_heads heads of hd columns each
 *   (q heads followed by k heads of the fused q|k|v projection; the v columns pass through):
 *   LlamaAttention q_proj/k_proj/v_proj + apply_rotary_pos_emb, modeling_llama.py:332-338 and :167-198 (Qwen2: with q/k/v bias).
 *   cos_sin: fp32 [positions, hd/2, 2] (LlamaRotaryEmbedding.forward :123-139, rounded through bf16 by the caller);
 *   position of token row m: positions[m], or m % S when positions is NULL (training: position_ids = arange(S), llava_arch.py:534-545).
 *   The B rows of a tile are staged in an order that puts the rotation partners (e, e + hd/2) into one lane.  hd 64 or 128 fused. */
int rv_gemm_rope_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, const void* bias, int M, int N, int K,
                      const float* cos_sin, const int32_t* positions, int S, int rope_heads, int hd, void* workspace,
                      int64_t workspace_bytes, const void* zeros16, void* stream);
/* rv_gemm_swiglu_fwd_bf16: LlamaMLP's gate/up projections and activation in one launch (modeling_llama.py:226):
 *   GU[M, 2F] = A[M,K] [Wgate; Wup][2F,K]^T (kept for backward), ACT[M,F] = silu(GU[:, :F]) * GU[:, F:].  Wgu = the stacked [2F, K]
 *   weight (gate rows then up rows); a tile holds gate and up of the same 128 features, so the product is lane-local. */
int rv_gemm_swiglu_fwd_bf16(const void* A, int64_t lda, const void* Wgu, int64_t ldb, void* GU, int64_t ldgu, void* ACT, int64_t ldact,
                            int M, int F, int K, void* workspace, int64_t workspace_bytes, const void* zeros16, void* stream);
/* rv_gemm_swiglu_bwd_bf16: backward of the same through down_proj's input gradient: dGU[M, 2F] = swiglu'(GU) * (dY[M,K] Wd[K,F])
 *   with Wd = down_proj.weight stored [K = hidden, F] (read contraction-major, in place); d(act) never reaches memory.
 *   dact_scratch [M, F] is only used by the unfused fallback (may be NULL when the fused form is certain to run). */
int rv_gemm_swiglu_bwd_bf16(const void* dY, int64_t ldy, const void* Wd, int64_t ldw, const void* GU, int64_t ldgu, void* dGU, int64_t lddgu,
                            void* dact_scratch, int64_t ld_dact, int M, int F, int K, void* workspace, int64_t workspace_bytes,
                            const void* zeros16, void* stream);
/* Launch-shape selection, process-wide.  Measurement hooks (A/B tools and tests only): 0 = automatic tile selection (default),
 * 1 = 128x128 tile kernel, 2 = 256x256 tile kernel, 20 / 21 = tail split off / on, 30 / 31 = buffer-addressed staging off / on.
 * 40 / 41 = persistent tile-walking blocks off / on (default on): the engine turns them OFF for world size > 1, where RCCL kernels
 * share the CUs -- a persistent block that cannot start delays its whole share of the tiles.  Results never depend on any of it. */
int rv_gemm_select_kernel(int which);
/* Compute units the GEMM plans its tile rounds for (whole rounds of one 256x256 tile per CU, the K-split of a half-empty last
 * round, split-K of small outputs).  total_cus <= 0: the current device's multiProcessorCount (256 on MI355X); reserved_cus:
 * units left to concurrently running work -- the bucketed RCCL all-reduce that overlaps backward in data-parallel runs
 * (what DDP's NCCL kernels take on the reference's GPUs).  Default without a call: all units, or
 * RV_GEMM_RESERVED_CUS from the environment.  Returns the resulting budget (>= 8) or a negative error code.  Process-wide.
 * An explicit total (total_cus > 0) needs no device; without a budget and without a device every GEMM entry point (and rv_gemm_plan)
 * returns RV_ERR_LAUNCH. */
int rv_gemm_set_cu_budget(int total_cus, int reserved_cus);
/* The launch shape a GEMM call takes for these sizes, layouts and workspace under the current rv_gemm_set_cu_budget /
 * rv_gemm_select_kernel configuration; launches nothing and needs no device once a budget is set (the planner every entry point itself
 * calls: plain integer arithmetic, radvlm_amd/csrc/gemm_plan.h).  K2 = 0: no second operand pair; workspace_bytes = 0: no workspace.
 * kind: 0 = rv_gemm_bf16_ex; 1 = rv_gemm_dropout_add_bf16 with p > 0; 2 = a fused-epilogue entry point (rv_gemm_rope_bf16,
 * rv_gemm_swiglu_fwd_bf16 with N = 2F, rv_gemm_swiglu_bwd_bf16 with trans_b = 1; trans_a = 0, no second pair, no workspace), for which
 * kernel 1 means that the entry point runs its unfused sequence.
 * out[6] = { kernel (1 = 128x128 tiles, 2 = 256x256 tiles), MODE (0 whole tiles, 1 second pair, 2 split-K, 3 tail split), K-slices,
 * n_full (MODE 3: tiles computed whole), blocks of the GEMM kernel, buffer-addressed staging (0 / 1) }.  A launch is persistent when it has
 * fewer blocks than tiles (MODE 0 / 1) or than n_full + (tiles - n_full) * K-slices (MODE 3).  Tests use it to prove which form they ran. */
int rv_gemm_plan(int M, int N, int K, int trans_a, int trans_b, int64_t lda, int64_t ldb, int K2, int64_t lda2, int64_t ldb2,
                 int64_t workspace_bytes, int kind, int32_t* out);

/* Batched strided transpose of bf16 matrices: out[bz][c][r] = in[bz][r][c], r < R, c < C; columns r in [R, R_pad)
 * of every output row are written as zero.  bz = b0 * nb1 + b1; offsets in elements.
 * Used for the [b,h,hd,S_pad] head-transposed attention operands (perm32 = 1: within every aligned group of 32
 * output columns, column 8g + 4h + j holds input row 16h + 4g + j -- the order in which an MFMA accumulator tile
 * presents the sequence axis as the next MFMA's contraction index, so each lane's 8 operands are one 16-byte read;
 * requires R_pad % 64 == 0). */
int rv_transpose_bf16(const void* in, int64_t in_ld, int64_t in_bs0, int64_t in_bs1, void* out, int64_t out_ld,
                      int64_t out_bs0, int64_t out_bs1, int R, int C, int R_pad, int nb0, int nb1, int perm32,
                      void* stream);

/* ---- normalisation ------------------------------------------------------------------------------------------
 * LlamaRMSNorm.forward (modeling_llama.py:82-87): y = w * bf16(x * rsqrt(mean(x^2) + eps)), fp32 internal.
 * rstd (fp32 [rows], optional) is saved for backward. */
int rv_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int rows, int d, float eps, void* stream);
/* dx = rstd * (w*dy - xhat * mean(w*dy*xhat)); dw_partial[blk, d] (fp32, nblk rows) holds per-block sums of dy*xhat
 * (finish with rv_colsum_f32).  If dx_add != 0, dx += (residual-stream gradient accumulation). */
int rv_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, int dx_add,
                   float* dw_partial, int nblk, int rows, int d, void* stream);
/* torch.nn.LayerNorm as used by CLIP (HF:modeling_clip.py:362-384, pre_layrnorm :744).  stats (optional, fp32
 * [rows,2] = mean, rstd) is saved for backward.  Backward: dx (+)= ..., partial[blk] = [sum dy*xhat (d) | sum dy (d)]
 * (fp32 [nblk, 2d]; finish both halves with rv_colsum_f32) -- used when the vision tower is tunable
 * (mm_tunable_parts contains mm_vision_tower, train/train.py:1658-1661). */
int rv_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* stats, int rows, int d, float eps,
                     void* stream);
int rv_layernorm_bwd(const void* dy, const void* x, const void* w, const float* stats, void* dx, int dx_add,
                     float* partial, int nblk, int rows, int d, void* stream);
/* CLIP MLP activation x*sigmoid(1.702x) (HF:activations.py QuickGELUActivation) and its derivative. */
int rv_quick_gelu_fwd(const void* x, void* y, int64_t n, void* stream);
int rv_quick_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);

/* SigLIP MLP activation 0.5x(1+tanh(sqrt(2/pi)(x+0.044715x^3))) (siglip_encoder.py:83 hidden_act) and its derivative. */
int rv_gelu_tanh_fwd(const void* x, void* y, int64_t n, void* stream);
int rv_gelu_tanh_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);

/* out[c] (+)= sum_r in[r, c]  (fp32 partial rows -> bf16 vector). */
int rv_colsum_f32(const float* in, int rows, int cols, void* out_bf16, int accumulate, void* stream);
/* partial[blk, c] = sum over the block's rows of x[r, c]  (bf16 [rows, cols] with stride ld -> fp32 [nblk, cols]);
 * bias gradients of nn.Linear. */
int rv_colsum_partial_bf16(const void* x, int64_t ld, int rows, int cols, float* partial, int nblk, void* stream);

/* ---- rotary embedding ------------------------------------------------------------------------------------------
 * apply_rotary_pos_emb (modeling_llama.py:167-198), half-split convention, in place on `nsec` consecutive
 * [heads*hd] sections of each token row (q and k of a fused qkv row).  cos_sin: fp32 [S, hd/2, 2];
 * position = row % S (position_ids = arange(S) for every sample, llava_arch.py:534-545).  dir = +1 fwd, -1 bwd. */
int rv_rope_inplace(void* x, int64_t ld, const float* cos_sin, int rows, int S, int heads, int hd, int nsec, int dir,
                    void* stream);

/* ---- attention ----------------------------------------------------------------------------------------------------
 * softmax_fp32(scale * Q K^T + causal + key-padding) V: modeling_llama.py:349-368 + :1191-1225,
 * llama_flash_attn_monkey_patch.py:51-69; non-causal for HF:modeling_clip.py:259-277.
 * q/k/out: token-major [(b*S+s)*ld + h*hd + e]; vT: [b,h,hd,S_pad] (zero padded); lse: fp32 [b,h,S_pad];
 * lens (optional int32 [B]): valid keys per sample (right padding).  hd in {64,128}; S_pad % 64 == 0.
 * Precondition (all attention entry points): 1 <= lens[b] <= S -- it is not checked; a sample without a valid key has no softmax.
 * Rows at or beyond lens[b] (padded layout): the forward still writes out and lse for every row below S -- such a row attends the
 * keys below lens[b] (and, causal, not after itself); the values are finite, and they are no contract.  The backward expects dout = 0
 * in those rows and then writes dq, dk and dv of those rows as exact zeros.  It never lets lse / delta of a row at or beyond lens[b]
 * (or the sample's length in a packed batch), or of [S, S_pad), reach a gradient: those entries may hold anything, NaN included.
 * Nothing is written at or beyond row S of a sample's lse / delta, and nothing outside the [rows, H*hd] extent of out / dq / dk / dv. */
int rv_attn_fwd(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* vT, void* out, int64_t ld_o,
                float* lse, const int32_t* lens, int B, int H, int S, int S_pad, int hd, int causal, float scale,
                const void* zeros16, void* stream);
/* Backward of the above: dQ (query-block pass, which also produces delta = rowsum(dO*O)), then dK/dV (key-block pass).
 * qT/kT/doT are [b,h,hd,S_pad] transposed copies of q, k, dout (rv_transpose_bf16). */
int rv_attn_bwd(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o,
                int64_t ld_o, const void* dout, int64_t ld_do, const void* qT, const void* kT, const void* doT,
                const float* lse, float* delta, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk, void* dv,
                int64_t ld_dv, const int32_t* lens, int B, int H, int S, int S_pad, int hd, int causal, float scale,
                const void* zeros16, void* stream);

/* Grouped-query form (Qwen2: language_model/llava_qwen.py:46-58 -> HF Qwen2Attention with num_key_value_heads < heads;
 * repeat_kv modeling_llama.py:201-210): k / v / kT / vT / dk / dv hold H_kv heads, query head h uses key/value head
 * h / (H / H_kv); the dK/dV pass sums the group's query heads in registers (no expanded copies).  H % H_kv == 0.
 * Packed (variable-length) batches -- SURVEY 8f.2, no padding rows: cu_rows (int32 [B+1], device; may be NULL) gives the
 * first token row of every sample in q/k/v/out/dq/dk/dv (total_rows = cu_rows[B], host copy); S is then the LONGEST sample (grid extent, S_pad >= S), `lens` is
 * ignored, and the [b,h,hd,S_pad] transposed operands and lse/delta stay per-sample padded (rv_transpose_bf16_varlen).
 * Optional `workspace` (>= 2*B*S*H*hd*2 bytes, 16-byte aligned; may be NULL): when the dK/dV grid (key blocks x H_kv x B)
 * is too small to balance a long causal sequence over the chip, the pass runs one block per QUERY head into the
 * workspace and a deterministic group sum folds the partials. */
int rv_attn_fwd_gqa(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* vT, void* out, int64_t ld_o,
                    float* lse, const int32_t* lens, const int32_t* cu_rows, int B, int H, int H_kv, int S, int S_pad, int hd,
                    int causal, float scale, const void* zeros16, void* stream);
/* Forward for head_dim 128 on the operands as they lie in memory: v is the token-major [(b*S+s), H_kv*hd] view like k (no V^T copy).
 * Every tile is staged once into an LDS image that serves row reads (contraction over head_dim) and hardware-transposed column
 * reads (contraction over the tile's keys, ds_read_b64_tr_b16).  Same semantics, masks and packed-batch conventions as
 * rv_attn_fwd_gqa. */
int rv_attn_fwd_nat(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, void* out, int64_t ld_o,
                    float* lse, const int32_t* lens, const int32_t* cu_rows, int B, int H, int H_kv, int S, int S_pad, int hd, int causal,
                    float scale, const void* zeros16, void* stream);
/* 1 when rv_attn_fwd_nat runs a causal [B, H, S] batch as query-block pairs on the current device, 0 for single query blocks (test hook). */
int rv_attn_fwd_nat_pairs(int B, int H, int S, int causal);
int rv_attn_bwd_gqa(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o,
                    int64_t ld_o, const void* dout, int64_t ld_do, const void* qT, const void* kT, const void* doT,
                    const float* lse, float* delta, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk, void* dv,
                    int64_t ld_dv, const int32_t* lens, const int32_t* cu_rows, int total_rows, int B, int H, int H_kv, int S,
                    int S_pad, int hd, int causal, float scale, void* workspace, int64_t workspace_bytes, const void* zeros16,
                    void* stream);
/* The same with the adjoint of the rotary embedding folded into the dQ / dK epilogues (the backward of apply_rotary_pos_emb,
 * modeling_llama.py:167-198, on q and k that are stored rotated): dq and dk come out as gradients of the UN-rotated projections,
 * no separate pass over d(q|k|v).  rope_cos_sin: fp32 [positions, hd/2, 2] (NULL = plain rv_attn_bwd_gqa); position of a token row =
 * rope_positions[row] (required for packed batches) or its index inside the sample.
 * ld_dq, ld_dk, ld_dv: multiples of 4 elements.  With grouped-query heads and a workspace the per-query-head dK/dV launch shape (partials
 * summed by a second kernel that stores 16-byte vectors) is only taken when ld_dk and ld_dv are multiples of 8 and dk, dv are 16-byte
 * aligned; otherwise the register-accumulating shape runs, whose results differ from it only in bf16 rounding points.  The same rule
 * holds for rv_attn_bwd_nat. */
int rv_attn_bwd_gqa_rope(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o,
                         int64_t ld_o, const void* dout, int64_t ld_do, const void* qT, const void* kT, const void* doT,
                         const float* lse, float* delta, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk, void* dv,
                         int64_t ld_dv, const int32_t* lens, const int32_t* cu_rows, int total_rows, int B, int H, int H_kv, int S,
                         int S_pad, int hd, int causal, float scale, void* workspace, int64_t workspace_bytes,
                         const float* rope_cos_sin, const int32_t* rope_positions, const void* zeros16, void* stream);

/* Backward for head_dim 128 on the operands as they lie in memory (no q^T / k^T / dO^T copies: every staged tile serves row reads and
 * hardware-transposed column reads, see rv_attn_fwd_nat), with the optional rotary-embedding adjoint of rv_attn_bwd_gqa_rope.
 * delta [B,H,S_pad] fp32 is scratch written by the dQ pass (rowsum(dO * O)) and read by the dK/dV pass. */
int rv_attn_bwd_nat(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const void* v, int64_t ld_v, const void* o, int64_t ld_o,
                    const void* dout, int64_t ld_do, const float* lse, float* delta, void* dq, int64_t ld_dq, void* dk, int64_t ld_dk,
                    void* dv, int64_t ld_dv, const int32_t* lens, const int32_t* cu_rows, int total_rows, int B, int H, int H_kv, int S,
                    int S_pad, int hd, int causal, float scale, void* workspace, int64_t workspace_bytes, const float* rope_cos_sin,
                    const int32_t* rope_positions, const void* zeros16, void* stream);

/* rv_transpose_bf16 for packed batches: batch b0 reads rows [cu_rows[b0], cu_rows[b0+1]) of `in` (R_max = longest). */
int rv_transpose_bf16_varlen(const void* in, int64_t in_ld, const int32_t* cu_rows, int64_t in_bs1, void* out, int64_t out_ld,
                             int64_t out_bs0, int64_t out_bs1, int R_max, int C, int R_pad, int nb0, int nb1, int perm32,
                             void* stream);
/* rv_rope_inplace with an explicit position per token row (packed batches: position = row - first row of its sample). */
int rv_rope_inplace_pos(void* x, int64_t ld, const float* cos_sin, const int32_t* positions, int rows, int heads, int hd,
                        int nsec, int dir, void* stream);

/* ---- MLP activations ------------------------------------------------------------------------------------------------
 * LlamaMLP (modeling_llama.py:226): act[r, f] = silu(gu[r, f]) * gu[r, F + f]   (gu = fused gate|up output). */
int rv_swiglu_fwd(const void* gu, int64_t ld_gu, void* act, int64_t ld_act, int rows, int F, void* stream);
int rv_swiglu_bwd(const void* dact, int64_t ld_dact, const void* gu, int64_t ld_gu, void* dgu, int64_t ld_dgu, int rows,
                  int F, void* stream);
/* Inverted dropout with a counter-based mask: y[i] = keep(seed, i) ? x[i] / (1 - p) : 0; keep: 16 bits of a splitmix64 value shared by the
 * four elements i >> 2, compared with round(p * 2^16) (p is honoured to 1.5e-5).
 * The same (seed, p) regenerates the mask, so backward applies the same call to the gradient (lora_dropout). */
int rv_dropout_bf16(const void* x, void* y, int64_t n, float p, uint64_t seed, void* stream);
/* y += dropout(x) with the same mask as rv_dropout_bf16(p, seed): the adapter branch of a LoRA layer's input gradient,
 * dx += dropout'(dt A), in one pass (peft LoraLayer: lora_dropout is applied to the layer input, so its adjoint masks dt A). */
int rv_dropout_add_bf16(const void* x, void* y, int64_t n, float p, uint64_t seed, void* stream);
/* LoRA down-projection with the adapter's input dropout inside: T[M, R] = alpha / (1 - p) * mask(seed) o X[M, K] * A[R, K]^T
 * = lora_A(lora_dropout(x)) * (alpha / r) of a peft LoraLayer (reference wiring train/train.py:1515-1532, defaults :152-157).
 * The mask is that of rv_dropout_bf16(X as M * K contiguous elements, p, seed) -- backward re-creates dropout(X) with that call --
 * and is applied to the operand fragments in registers: one pass over X instead of three.  K % 64 == 0, R <= 64, R % 4 == 0; with p > 0 X
 * must be contiguous (ldx == K: the mask indexes it as M * K elements); p = 0: the plain skinny product at HBM speed, any ldx % 8 == 0
 * (also used for dT = alpha * dY B, the adapters' backward, with B^T as the row-major operand). */
/* dx[M, N] (+)= dropout'(alpha * dT[M, K] op(A)): the adapter branch of a LoRA layer's input gradient with the forward's dropout mask
 * (that of rv_dropout_bf16 over M * N elements) applied to the accumulators in the GEMM epilogue.  trans_b: A stored [K, N] (lora_A [r, in]).
 * accumulate != 0: added to dx.  N % 8 == 0. */
int rv_gemm_dropout_add_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K, int trans_b,
                             float alpha, float p, uint64_t seed, int accumulate, const void* zeros16, void* stream);
int rv_lora_down_bf16(const void* X, int64_t ldx, const void* A, int64_t lda, void* T, int64_t ldt, int M, int R, int K, float alpha,
                      float p, uint64_t seed, const void* zeros16, void* stream);
/* gA[R, K] (+)= 1 / (1 - p) * dT[M, R]^T mask_p(X)[M, K]: the gradient of a LoRA adapter's A matrix (the adjoint of lora_A(lora_dropout(x)),
 * reference wiring train/train.py:1515-1532) with the forward's dropout mask -- that of rv_dropout_bf16(X as M * K contiguous elements, p, seed) --
 * re-created in registers: X is read once and dropout(X) never reaches HBM.  dT is the (alpha / r)-scaled gradient of the adapter's inner
 * activation.  R <= 64, R % 8 == 0, K % 8 == 0, 16-byte aligned X and dT; p > 0 needs ldx == K.  accumulate != 0: added to gA.  workspace: fp32
 * scratch for the token-slice partial sums, at least R * K * 4 bytes (deterministic reduction: no atomics). */
int rv_lora_a_grad_bf16(const void* dT, int64_t ldt, const void* X, int64_t ldx, void* gA, int64_t ldg, int M, int R, int K, float p, uint64_t seed,
                        int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* torch.nn.GELU (erf) of the mm_projector (multimodal_projector/builder.py:44) and its derivative. */
int rv_gelu_fwd(const void* x, void* y, int64_t n, void* stream);
int rv_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);

/* ---- loss ----------------------------------------------------------------------------------------------------------
 * LlamaForCausalLM loss (modeling_llama.py:1323-1337): logits.float(), CE with ignore_index -100.
 * labels[r] is the ALREADY SHIFTED target of row r.  loss_rows[r] = -log softmax(logits[r])[label] (0 if ignored).
 * If dlogits != NULL: dlogits[r] = (softmax - onehot) * inv_count (0 rows if ignored).  In-place use (dlogits == logits, same
 * ld) is supported: the target logit is read before any store of the row.  A label >= V is treated like ignore_index (it
 * never indexes the row); callers reject such labels on the host (radvlm_amd.engine does).
 * V may be any size; rows are ld >= ceil8(V) wide, the pad columns are ignored on read and get zero gradient. */
int rv_cross_entropy(const void* logits, int64_t ld, const int64_t* labels, float* loss_rows, void* dlogits,
                     int64_t ld_d, int rows, int V, float inv_count, void* stream);
/* out[0] = scale * sum(in[0..n))  (deterministic, single block). */
int rv_sum_f32(const float* in, int64_t n, float scale, float* out, void* stream);
/* The GRPO token loss (TRL GRPOTrainer._compute_loss, token level) on the rows rv_cross_entropy takes: bf16 logits, rows of ld >=
 * ceil8(V) columns, labels[r] the already shifted target (outside [0, V): an ignored row).  Per live row, in fp32, with lse and the
 * softmax p computed by the statements of rv_cross_entropy:
 *   logp = z[y] - lse;  r = exp(logp - old_logp[r])  (old_logp == NULL: r = 1 exactly);  rc = min(max(r, 1 - eps_low), 1 + eps_high)
 *   act  = (r A <= rc A);  loss = -min(r A, rc A);  beta > 0: q = ref_logp[r] - logp, kl = exp(q) - q - 1, loss += beta kl  (else kl = 0)
 *   g    = gweight[r] (A r [act])  -  gweight[r] beta (1 - exp(q))  when beta > 0;   dlogits[r][j] = (p[j] - [j == y]) * g
 * stats: five fp32 planes of `rows` entries each -- logp, loss, lweight[r] * loss, kl, clip code (0 active; 1: r < 1 - eps_low and
 * A < 0; 2: r > 1 + eps_high and A > 0).  An ignored row writes zeros to all of them and to its dlogits row and reads none of its
 * per-row floats.  dlogits may be the logits buffer (the target logit is read before any store), another buffer with its own ld_d, or
 * NULL (statistics only).  Pad columns are read as -inf and written as 0.
 * Bit promises: logp == -loss_rows of rv_cross_entropy on the same logits; with adv = 1, old_logp = NULL, beta = 0 and gweight = c
 * the dlogits are those of rv_cross_entropy with inv_count = c.
 * Refused (RV_ERR_ARG, nothing launched): a null logits / labels / adv / lweight / gweight / stats, rows < 1, V < 1, ld or ld_d not a
 * multiple of 8 or below ceil8(V), logits or dlogits not 16-byte aligned, eps_low / eps_high / beta negative or NaN, beta > 0 without
 * ref_logp.  Non-finite adv / old_logp / ref_logp on a live row are outside the contract. */
int rv_policy_loss_bf16(const void* logits, int64_t ld, const int64_t* labels, const float* adv, const float* lweight,
                        const float* gweight, const float* old_logp, const float* ref_logp, float eps_low, float eps_high, float beta,
                        float* stats, void* dlogits, int64_t ld_d, int rows, int V, void* stream);
/* Knowledge distillation (csrc/distill.hip): the generalised Jensen-Shannon divergence of TRL's GKDTrainer.generalized_jsd_loss between
 * a student row z and a teacher row u over the whole vocabulary, on the rows rv_cross_entropy takes (bf16, ld / ld_t >= ceil8(V)
 * columns).  teacher_row: int32 [rows], student row -> teacher row, -1 for none (the row is then ignored); NULL: row r <-> row r.
 * labels[r] only says whether row r is scored: outside [0, V) the row is ignored -- zeros in its four statistics and its dlogits row,
 * none of its floats is read.  Per live row, in fp32, with it = 1 / temperature formed once on the host and each logit multiplied by it
 * as it is read:
 *   s = it z - lse(it z);  lt = it u - lse(it u);  p = exp(s);  t = exp(lt);  d = lt - s      (lse: rv_cross_entropy's statements)
 *   beta == 0 (forward KL):  L = sum_j t_j d_j;                     dL/dz_j = (p_j - t_j) it
 *   beta == 1 (reverse KL):  L = sum_j p_j r_j, r_j = -d_j;         dL/dz_j = p_j (r_j - L) it
 *   0 < beta < 1:  r_j = -log((1 - beta) + beta exp(d_j)), evaluated without the exponential of a positive number;
 *                  KL_S = sum_j p_j r_j;  KL_T = sum_j t_j (d_j + r_j);  L = beta KL_T + (1 - beta) KL_S;
 *                  dL/dz_j = (1 - beta) p_j (r_j - KL_S) it      (the terms through the mixture cancel)
 * The end points are TRL's special cases, not the limits of the middle formula (which tends to 0 at both ends).  No tau^2 factor.
 * dlogits[r][j] = gweight[r] dL/dz_j (the product gweight[r] it is formed once per row) and zeros in the pad columns up to
 * ceil8(V).  dlogits may be the logits buffer (a thread overwrites only vectors it alone reads), another buffer with its own
 * ld_d, or NULL (statistics only).  Pad columns are never summed.
 * stats: four fp32 planes of `rows` entries -- jsd = L, lweight[r] * L, kl_teacher, kl_student (beta 0: L, ., L, 0; beta 1: L, ., 0, L).
 * One workgroup per row; every sum is taken per thread in ascending column order, then across lanes, then across waves 0..3: no
 * atomics, and a row's bits depend on the row pair and the scalars alone -- not on rows, the grid, teacher_row or the buffer form.
 * Bit promises: at temperature 1 the student's lse and p are rv_cross_entropy's; so with beta = 0, temperature = 1 and a teacher row
 * whose label logit is so far above the rest (200) that every other t_j underflows to 0, jsd == loss_rows of rv_cross_entropy and,
 * with gweight = c, dlogits == its dlogits with inv_count = c.  A teacher row equal to the student row gives jsd == 0 and a zero
 * gradient row at beta 0 and 1.
 * Finite logits only; the result stays finite for |d| up to the range of the logits themselves.
 * Refused (RV_ERR_ARG, nothing launched): a null logits / teacher / labels / lweight / gweight / stats, rows < 1, V < 1, ld, ld_t or
 * ld_d not a multiple of 8 or below ceil8(V), logits, teacher or dlogits not 16-byte aligned, beta outside [0, 1] or NaN, temperature
 * <= 0 or not finite. */
int rv_distill_loss_bf16(const void* logits, int64_t ld, const void* teacher, int64_t ld_t, const int32_t* teacher_row,
                         const int64_t* labels, const float* lweight, const float* gweight, float beta, float temperature, float* stats,
                         void* dlogits, int64_t ld_d, int rows, int V, void* stream);

/* ---- DPO preference training (csrc/preference.hip) -------------------------------------------------------------------
 * The sequence-level part of the DPO loss, between two calls of rv_policy_loss_bf16: (A) with dlogits = NULL gives the logp plane,
 * rv_dpo_pairs_f64 turns it into one gradient coefficient per scored token, (C) with adv = those coefficients writes dlogits.
 * Scored order: the scored tokens of sequence 0, then of sequence 1, ...; sequence b owns [seg_off[b], seg_off[b + 1]).  Scored token j
 * lives in row j of logp / coef (row_idx == NULL: the gathered head) or in row row_idx[j] (the all-rows head).  `rows` is the length
 * of logp and coef; a token whose row lies outside [0, rows) contributes nothing and is not written.
 *
 * THE SUM ORDER (fp64, a promise): 64 accumulators start at +0.0; element j of the sequence (j = 0, 1, ... in scored order) is added
 * to accumulator j mod 64, ascending in j; then for o = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l xor o] for all l at once; the sum
 * is acc[0].  It depends on the sequence's own length alone -- not on the batch, the layout, row_idx or the other sequences -- and an
 * empty sequence sums to +0.0.  No atomics.
 *
 * sums[b] = the sum of sequence b, b < B. */
int rv_seq_logp_sums_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, double* sums, int B, int rows, void* stream);
/* P pairs as 2 P sequences: sequence p is prompt + chosen, sequence P + p prompt + rejected (seg_off has 2 P + 1 entries).  One
 * workgroup per pair; the two sums are rv_seq_logp_sums_f64's, bit for bit.  With n the scored tokens of a sequence, in fp64, one
 * rounding per operation (no fused multiply-adds):
 *   pi = sum  (loss_type 2, ipo: sum / n);   rho = rho[sequence], 0 when rho == NULL (reference-free);   s = 1  (ipo: 1 / n)
 *   u = (pi_c - pi_r) - (rho_c - rho_r);   h = beta u;   logsig(x) = -(max(-x, 0) + log1p(exp(-|x|)));   sig(x) = {1, e}[x < 0] / (1 + e), e = exp(-|x|)
 *   0 sigmoid: loss = -(1 - eps) logsig(h) - eps logsig(-h);   dl = beta (eps sig(h) - (1 - eps) sig(-h))
 *   1 hinge:   loss = max(0, 1 - h);                           dl = 1 - h > 0 ? -beta : 0            (eps is not used)
 *   2 ipo:     loss = (u - 1 / (2 beta))^2;                    dl = 2 (u - 1 / (2 beta))
 *   k = alpha_over_P dl;   coef of every chosen scored token = fp32(gamma_over_Nc - k s_c), of every rejected one = fp32(k s_r)
 * (one fp64 value rounded once: A = -dL/dlogp_token of L below).  Rows of coef that hold no scored token are not touched.
 * planes: seven fp64 planes of P entries -- pi_c, pi_r, h, loss, beta (pi_c - rho_c), beta (pi_r - rho_r), the chosen sum (pi_c
 * unless ipo).  batch (fp64 [3], written by a one-wave kernel in the same fixed order over the pairs, after the pair kernel):
 *   batch[0] = L = alpha_over_P sum_p loss_p - gamma_over_Nc sum_p chosen_sum_p;   batch[1] = alpha_over_P sum_p loss_p;
 *   batch[2] = -sum_p chosen_sum_p / N_c, N_c = seg_off[P] - seg_off[0].
 * Refused (RV_ERR_ARG, nothing launched): a null logp / seg_off / planes / batch / coef, P < 1, rows < 1, beta not finite or <= 0,
 * label_smoothing outside [0, 0.5), a loss_type other than 0, 1, 2, ipo with label_smoothing != 0, a NaN alpha_over_P or gamma_over_Nc. */
int rv_dpo_pairs_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, const double* rho, int P, int loss_type, double beta,
                     double label_smoothing, double alpha_over_P, double gamma_over_Nc, double* planes, double* batch, float* coef,
                     int rows, void* stream);
/* GRPO with sequence-level importance ratios (GSPO; TRL importance_sampling_level="sequence"), launch (B) between the same two sweeps:
 * B sequences in scored order (seg_off has B + 1 entries, row_idx as above), one workgroup per sequence.  lweight, gweight, old_logp
 * (NULL: on-policy) and ref_logp (NULL unless beta > 0) are the fp32 per-row arrays rv_policy_loss_bf16 takes, adv_seq fp32 [B] one
 * advantage per sequence.  With n the scored tokens of sequence b and A = adv_seq[b], in fp64 on the fp32 inputs, one rounding per
 * operation (no fused multiply-adds), every sum over the sequence's tokens in THE SUM ORDER:
 *   m = sum_j (logp_j - old_j) / n  (each difference formed in fp64; old_logp == NULL or n == 0: m = +0);   s = exp(m), exactly 1 when m == 0
 *   sc = min(max(s, 1 - eps_low), 1 + eps_high);   act = (s A <= sc A);   l = -(act ? s A : sc A)  (n == 0: l = 0)
 *   beta > 0: q_j = ref_j - logp_j, kl_j = expm1(q_j) - q_j  (else kl_j = 0);   W_l = sum_j lweight_j, W_g = sum_j gweight_j
 *   coef_j = fp32(([act] s A) (W_g / n) + (gweight_j beta) expm1(q_j))  (beta == 0: the first product alone);   kl_j is stored as fp32(kl_j)
 * coef_j = -dL/dlogp_j of L below with gweight in lweight's place: sweep (C) with adv = coef, lweight = gweight = 1, no old or reference
 * log-probs and beta = 0 writes dlogits = (p - onehot) coef.  coef and kl are written at scored rows only.
 * planes: five fp64 planes of B entries -- m, s, l, the clip code (0 active; 1: s < 1 - eps_low and A < 0; 2: s > 1 + eps_high and
 * A > 0), sum_j lweight_j kl_j.  batch (fp64 [2], written by a one-wave kernel, the sums over the sequences in THE SUM ORDER, after
 * the sequence kernel):   batch[1] = beta sum_b planes[4][b];   batch[0] = L = sum_b (W_l,b l_b) + batch[1].
 * An empty sequence writes m = +0, s = 1, l = 0, code 0 and touches no row.
 * Bit promise: with old_logp NULL or equal to logp, beta == 0 or ref_logp equal to logp, and gweight constant inside each sequence,
 * coef_j == gweight_j * adv_seq[b] as fp32 multiplies them -- the coefficient of rv_policy_loss_bf16 at r = 1 (n < 2^29 copies of one
 * fp32 value sum exactly in fp64, the division by n is exact, and one rounding of the exact 48-bit product is the fp32 product).
 * Refused (RV_ERR_ARG, nothing launched): a null logp / seg_off / adv_seq / lweight / gweight / planes / batch / coef / kl, B < 1,
 * rows < 1, eps_low / eps_high / beta negative or NaN, beta > 0 without ref_logp. */
int rv_gspo_seqs_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, const float* adv_seq, const float* lweight,
                     const float* gweight, const float* old_logp, const float* ref_logp, double eps_low, double eps_high, double beta,
                     double* planes, double* batch, float* coef, float* kl, int B, int rows, void* stream);

/* ---- embedding splice ---------------------------------------------------------------------------------------------
 * prepare_inputs_labels_for_multimodal steps (vi)-(viii), llava_arch.py:449-531, as one gather:
 * dst[r] = idx[r] >= 0 ? table_a[idx[r]] : (idx[r] == -1 ? 0 : table_b[-idx[r] - 2]).  (exact-zero pad rows) */
int rv_gather_rows(void* dst, int64_t ld_dst, const void* table_a, int64_t ld_a, const void* table_b, int64_t ld_b,
                   const int32_t* idx, int rows, int d, void* stream);
/* Embedding gradient without atomics: for segment s, out[out_row[s]] = sum_{j in [off[s], off[s+1])} src[pos[j]]. */
int rv_segment_sum_rows(const void* src, int64_t ld_src, const int32_t* seg_off, const int32_t* pos,
                        const int32_t* out_row, int nseg, void* out, int64_t ld_out, int d, void* stream);

/* Weighted form: out[out_row[s]] = sum_j w[j] * src[pos[j]].  Forward and adjoint of the anyres_max bilinear
 * down-sampling nn.functional.interpolate(mode="bilinear") at llava_arch.py:381-392 (4 taps per output row; the
 * adjoint's CSR is the transposed tap list, built on the host), deterministic (no atomics). */
int rv_weighted_segment_sum_rows(const void* src, int64_t ld_src, const int32_t* seg_off, const int32_t* pos,
                                 const float* w, const int32_t* out_row, int nseg, void* out, int64_t ld_out, int d,
                                 void* stream);

/* 'maxpool2x2' patch merge (nn.functional.max_pool2d(grid, 2), llava_arch.py:375-379): out[out_row[s]] = elementwise max of the
 * four rows src[idx4[4s..4s+3]] (window scan order; `which` keeps the winning slot per element); backward routes the gradient
 * of every pooled row to the winning source element and zero to the other three (windows do not overlap: no atomics). */
int rv_max4_rows_fwd(const void* src, int64_t ld_src, const int32_t* idx4, const int32_t* out_row, int n, void* out, int64_t ld_out,
                     uint8_t* which, int d, void* stream);
int rv_max4_rows_bwd(const void* dout, int64_t ld_dout, const int32_t* idx4, const int32_t* dout_row, int n, const uint8_t* which,
                     void* dsrc, int64_t ld_dsrc, int d, void* stream);

/* Device-side image normalisation and tiling (the host image path of train/train.py:1060-1099 + mm_utils.py:243-293 ends in
 * processor.preprocess: rescale 1/255, (x - mean) / std, HWC -> CHW, per tile): n uint8 canvases [gh*tile, gw*tile, 3] (HOST memory is
 * not accepted: device pointers only) -> bf16 [n*gh*gw, 3, tile, tile], tiles in row-major grid order (divide_to_patches, mm_utils.py:191-210).
 * mode 0: CLIPImageProcessor arithmetic (float32(u8) / 255), mode 1: SigLipImageProcessor (float64(u8) * factor -> float32); mean3 / std3
 * are HOST arrays of 3 floats (passed by value).  Bit-identical to normalising on the host in fp32 and casting on the device; the upload
 * is a quarter of the fp32 bytes. */
int rv_normalize_tiles_u8(const uint8_t* img, void* out, int n, int gh, int gw, int tile, int mode, double factor, const float* mean3,
                          const float* std3, void* stream);
/* ---- CLIP embeddings -----------------------------------------------------------------------------------------------
 * HF:modeling_clip.py:202-218: patches of pix [n,3,H,W] (bf16) -> rows [n*gh*gw, Kp], k = c*p*p + i*p + j (zero
 * padded to Kp); then out[n, 0] = cls + pos[0], out[n, 1+i] = patch_out[n, i] + pos[1+i]. */
int rv_im2col_patches(const void* pix, void* out, int n, int H, int W, int p, int Kp, void* stream);
int rv_clip_embed(const void* patch_out, const void* cls, const void* pos, void* out, int n, int P, int d, void* stream);
/* SigLipVisionEmbeddings (siglip_encoder.py:169-174): x[n, i] += pos[i] in place (no class token; the conv bias rides the
 * patch GEMM).  rv_im2col_patches accepts H, W that are not multiples of p ('valid' conv: trailing pixels unused). */
int rv_add_pos_rows(void* x, const void* pos, int n, int P, int d, void* stream);

/* ---- optimizer / misc ----------------------------------------------------------------------------------------------
 * torch.optim.AdamW step (optim="adamw_torch", train/train.py:140) on a flat slice: fp32 master/m/v, bf16 params and
 * grads; grad is multiplied by *gscale (device scalar, e.g. the clip coefficient) if gscale != NULL. */
int rv_adamw(void* p_bf16, float* master, const void* g_bf16, float* m, float* v, int64_t n, float lr, float b1,
             float b2, float eps, float wd, float bc1, float bc2, const float* gscale, void* stream);
/* 8-bit AdamW state (optim="adamw_bnb_8bit", train/llava_trainer.py:416-431; csrc/adam8.hip): block-wise dynamic quantisation of the two
 * moments, 256 elements per block counted from a tensor's first element, one fp32 absmax per block, the codebooks of
 * csrc/adam8_codebook.h.  The rule is tests/adam8_ref.py and the kernels match it bit for bit.  kind 0: signed table (exp_avg, absmax =
 * max |x|); kind 1: unsigned table (exp_avg_sq, absmax = max x) with the guard "a value > 0 never takes code 0".
 * quantise: codes[n] and absmax[ceil(n / 256)] of one tensor x[n]; dequantise: x[i] = table[codes[i]] * absmax[i / 256]. */
int rv_adam8_quantize_f32(const float* x, int64_t n, uint8_t* codes, float* absmax, int kind, void* stream);
int rv_adam8_dequantize_f32(const uint8_t* codes, const float* absmax, int64_t n, int kind, float* x, void* stream);
/* rv_adamw on a slice whose moments are 8-bit: per element dequantise m and v, the update of rv_adamw (the same device function),
 * master and the bf16 parameter from the unquantised new moments, then the block maxima and the new codes.  Bit-identical to
 * rv_adam8_dequantize_f32 -> rv_adamw -> rv_adam8_quantize_f32 per tensor.  table: device int64 [3, ntensors] = each tensor's first
 * element in p / master / g, its length (> 0), its first block (0 for the first; tensor t owns ceil(length / 256) blocks, consecutive).
 * Block b's codes are bytes [256 b, 256 b + 256) of codes_m / codes_v (nblocks * 256 bytes each; a short last block leaves its
 * remaining bytes untouched), its scales absmax_m[b] / absmax_v[b].  One launch for the whole slice. */
int rv_adamw8(void* p_bf16, float* master, const void* g_bf16, uint8_t* codes_m, uint8_t* codes_v, float* absmax_m, float* absmax_v,
              const int64_t* table, int ntensors, int64_t nblocks, float lr, float b1, float b2, float eps, float wd, float bc1,
              float bc2, const float* gscale, void* stream);
/* NF4 frozen decoder base of a LoRA run (QLoRA: --bits 4 --quant_type nf4; csrc/nf4.hip).  A block is 64 consecutive elements of one tensor
 * counted from its first element (the last may be short), one fp32 absmax = max |x| per block (an all-zero block divides by 1), the
 * sixteen levels of csrc/nf4_codebook.h, two codes per byte with element 2j in the high nibble (an odd length leaves the last low nibble
 * 0).  The rule is tests/nf4_ref.py and the kernels match it bit for bit.
 * quantise: codes[ceil(n / 2)] and absmax[ceil(n / 64)] of one bf16 tensor x[n]; code = the number of fp32 midpoints strictly below
 * fp32(x) / absmax. */
int rv_nf4_quantize_bf16(const void* x_bf16, int64_t n, uint8_t* codes, float* absmax, void* stream);
/* One launch dequantises every tensor of a table into dst: dst[first destination + i] = bf16(level[code_i] * absmax of i's block), one fp32
 * multiply and one rounding.  table: device int64 [6, ntensors] = each tensor's first chunk (0 for the first; a tensor owns ceil(length /
 * 2048) consecutive chunks, nchunks in all), first code byte in `codes`, first absmax entry, length (> 0), first element in dst, first
 * second-level scale.  Two modes.  absmax != NULL: plain fp32 absmax[first absmax entry + block].  absmax == NULL (double quantisation):
 * the block's absmax is fp32(signed8[absmax_codes[first absmax entry + block]] * scale2[first scale + block / 256]) + offset[tensor], the
 * signed table of csrc/adam8_codebook.h.  The destinations of the tensors need not be adjacent; nothing outside them is written.  Code
 * bytes at a 4-byte and destinations at a 16-byte aligned address take vector accesses, anything else masked narrow ones. */
int rv_nf4_dequant_bf16(const uint8_t* codes, const float* absmax, const uint8_t* absmax_codes, const float* scale2, const float* offset,
                        const int64_t* table, int ntensors, int64_t nchunks, void* dst_bf16, void* stream);
/* partial[blk] = sum of squares of the block's slice (fp32); finish with rv_clip_coef. */
int rv_sumsq_partial_bf16(const void* g, int64_t n, float* partial, int nblk, void* stream);
/* norm = sqrt(sum partial); out[0] = norm, out[1] = min(1, max_norm / (norm + 1e-6))  (torch clip_grad_norm_). */
int rv_clip_coef(const float* partial, int nblk, float max_norm, float* out2, void* stream);
int rv_cast_f32_to_bf16(const float* in, void* out, int64_t n, void* stream);
int rv_cast_bf16_to_f32(const void* in, float* out, int64_t n, void* stream);
/* y[i] = a[i] + b[i] (bf16). */
int rv_add_bf16(const void* a, const void* b, void* y, int64_t n, void* stream);

/* ---- decode (generate(): one new token per sequence, radvlm_amd/csrc/gemv.hip and decode.hip) ----------------------------
 * The reference decodes through HF generate on inputs_embeds (llava_llama.py generate() -> HF:generation/utils.py greedy search with
 * a DynamicCache); these entry points are its per-token arithmetic: the projections at M = batch rows, attention of one query row
 * against the cache, the cache update, the greedy logits processors and the greedy argmax. */
/* Skinny NT GEMM (gemv.hip, with its two quantised forms below): Y[M,N] = X[M,K] W[N,K]^T (+ bias[N]) (+ residual[M,N]) for
 * 1 <= M <= 32 (fp32 accumulation; bf16 Y, or fp32 Y with out_f32 for the lm_head scores).  Weights are streamed once (16-byte nontemporal loads); the K range is split over workgroups when
 * N alone gives too few of them (rv_gemv_split(N, K) slices, combined in slice order by a second launch through `workspace`, which
 * needs split * M * N * 4 bytes when split > 1).  The reduction order is a function of (N, K): row r's result is bit-identical for
 * every M.  K % 8 == 0, ldx % 8 == 0, ldw % 8 == 0. */
int rv_gemv_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, void* Y, int64_t ldy, const void* bias, const void* residual,
                 int64_t ldr, int M, int N, int K, int out_f32, void* workspace, int64_t ws_bytes, void* stream);
/* Number of K slices rv_gemv_bf16 uses for an [N, K] weight (host function, no launch). */
int rv_gemv_split(int N, int K);
/* Weight-only int8 decoding (reference: load_pretrained_model(load_8bit=True), model/builder.py:27-31, bitsandbytes row-wise int8
 * with lm_head left in 16 bits).  For a bf16 row w of K entries: s = max|w| / 127 (fp32 IEEE division; 1 for a zero row),
 * q = clamp(rint(float(w) / s), -127, 127) (IEEE division, round half to even), W^ = bf16_rne(float(q) * s).  One pass over
 * W[N, K] (rows of ldw elements; a row slice of the fused q|k|v or gate|up store is fine) writes W^ over W, s to scale[N] and q to
 * packed[N][ldp] (int8; ldp = rv_w8_row_bytes(K) bytes).  The packed layout is private to this entry and rv_gemv_w8_bf16: 64 bytes
 * per pair of 32-deep K steps, the 8 weights of steps 2j and 2j + 1 that one MFMA lane group reads side by side, zero padding past K.
 * Quantising W^ again does not give W^ back: call it once.  Non-finite weights are outside the contract.  K % 8 == 0, ldw % 8 == 0. */
int rv_quantize_rows_w8_bf16(void* W, int64_t ldw, void* packed, int64_t ldp, float* scale, int N, int K, void* stream);
/* Bytes of one packed row for K input features (host function, no launch). */
int64_t rv_w8_row_bytes(int K);
/* rv_gemv_bf16 with the weight given as (packed, scale) of rv_quantize_rows_w8_bf16: the bf16 operand bf16_rne(float(q) * s) is rebuilt
 * in registers, the K split, the k-to-lane assignment and the accumulation order are rv_gemv_bf16's, so Y is bit-identical to
 * rv_gemv_bf16 on W^ for every M.  Half the weight bytes per call.  Same workspace rule. */
int rv_gemv_w8_bf16(const void* X, int64_t ldx, const void* packed, int64_t ldp, const float* scale, void* Y, int64_t ldy,
                    const void* bias, const void* residual, int64_t ldr, int M, int N, int K, int out_f32, void* workspace,
                    int64_t ws_bytes, void* stream);
/* Weight-only MXFP4 decoding (reference: load_pretrained_model(load_4bit=True), model/builder.py; here OCP Microscaling FP4, E2M1
 * elements with one E8M0 scale per block of 32 consecutive k).  For each block of a bf16 row (the last
 * block is shorter when K % 32 != 0; only its existing entries count):
 *     amax = max |w|    e = floor(log2(amax)) - 2 (0 for an all-zero block)    a = |w| / 2^e
 *     code = nearest of {0, .5, 1, 1.5, 2, 3, 4, 6} (codes 0..7), ties to the even code, a > 6 saturates to code 7
 *     W^ = sign(w) * value[code] * 2^e (exactly a bf16 number; code 0 gives +0.0)    nibble = sign << 3 | code (0 for code 0)
 * One pass over W[N, K] (rows of ldw elements; a row slice of the fused q|k|v or gate|up store is fine) writes W^ over W, the nibbles to
 * packed[N][ldp] (ldp = rv_w4_row_bytes(K)) and the scale bytes e + 127 to scales[N][lds] (uint8, lds = rv_w4_scale_row_bytes(K)).
 * The layout is private to this entry and rv_gemv_w4_bf16: 64 bytes per four 32-deep K steps, the 8 weights of each of the four steps
 * that one MFMA lane group reads side by side; padding past K is nibble 0 and scale byte 127.  Lossy (about 12 % relative Frobenius
 * error on Gaussian rows); block maxima outside [2^-120, 2^120] and non-finite weights are outside the contract.  K % 8 == 0,
 * ldw % 8 == 0. */
int rv_quantize_rows_mxfp4_bf16(void* W, int64_t ldw, void* packed, int64_t ldp, void* scales, int64_t lds, int N, int K, void* stream);
/* Bytes of one packed nibble row / of one scale row for K input features (host functions, no launch). */
int64_t rv_w4_row_bytes(int K);
int64_t rv_w4_scale_row_bytes(int K);
/* rv_gemv_bf16 with the weight given as (packed, scales) of rv_quantize_rows_mxfp4_bf16: the bf16 operand W^ is rebuilt in registers,
 * the K split, the k-to-lane assignment and the accumulation order are rv_gemv_bf16's, so Y is bit-identical to rv_gemv_bf16 on W^ for
 * every M <= 32.  0.27x the weight bytes per call.  Same workspace rule; ldp and lds must be the layout's. */
int rv_gemv_w4_bf16(const void* X, int64_t ldx, const void* packed, int64_t ldp, const void* scales, int64_t lds, void* Y, int64_t ldy,
                    const void* bias, const void* residual, int64_t ldr, int M, int N, int K, int out_f32, void* workspace,
                    int64_t ws_bytes, void* stream);
/* Decoding with live LoRA adapters (the down-projection in lora_decode.hip, the fused product in gemv.hip; reference: a peft LoraLayer in eval mode, y = W x + (alpha / r) B A x, which the
 * reference only ever evaluates merged).  The two calls a fused projection takes at M <= 32 rows; the arithmetic is that of the
 * training path's adapted linear at dropout 0: t rounded once to bf16, already scaled, then one fp32 sum and one store for y. */
/* T[M, j r .. (j + 1) r) = bf16(scale * X[M, K] A_j[r, K]^T) for the n_mod <= 3 adapters A0, A1, A2 that share the input X (q|k|v,
 * gate|up); each A_j has its own base pointer (rows of lda elements).  K is split over workgroups in rv_lora_down_split(r, K)
 * slices, summed in slice order through `workspace` (split * M * n_mod * r * 4 bytes when split > 1) by a second launch; no atomics,
 * a row's bits do not depend on M.  1 <= M <= 32, r % 8 == 0, 8 <= r <= 64, K % 8 == 0, ldx % 8 == 0, lda % 8 == 0, X and A_j
 * 16-byte aligned, ldt >= n_mod * r. */
int rv_lora_down_rows_bf16(const void* X, int64_t ldx, const void* A0, const void* A1, const void* A2, int64_t lda, int n_mod, void* T,
                           int64_t ldt, int M, int r, int K, float scale, void* workspace, int64_t ws_bytes, void* stream);
/* Number of K slices rv_lora_down_rows_bf16 uses (host function, no launch). */
int rv_lora_down_split(int r, int K);
/* Y[M, N] = X[M, K] W[N, K]^T + T_j B_j^T (+ bias[N]) (+ residual[M, N]), bf16 Y, 1 <= M <= 32: rv_gemv_bf16 with the adapter riding it
 * (an instantiation of rv_gemv_bf16's kernel, behind the same launch routine and split-K combine).
 * Module j < n_mod owns the columns [col0_j, col1_j) of Y, reads its t from columns [toff_j, toff_j + r) of T[M, ldt] and its
 * B_j[col1_j - col0_j, r] from its own pointer (rows of ldb elements); ranges ascend and do not overlap, col0_j is a multiple of 64
 * and col1_j is a multiple of 64 or N; columns outside every range get no adapter.  The W part takes rv_gemv_bf16's K split
 * (rv_gemv_split(N, K)), k-to-lane assignment, step order, four-wave reduction, combine and epilogue; the adapter's ceil(r / 32)
 * steps follow all W steps of the one accumulator that takes them, so with B = 0 every bit of Y is rv_gemv_bf16's.  r as above,
 * K % 8 == 0, ldx, ldw, ldt, ldb, toff_j multiples of 8, X, W, T, B_j 16-byte aligned.  Workspace as rv_gemv_bf16. */
int rv_gemv_lora_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* T, int64_t ldt, int r, int n_mod, const void* B0,
                      int col0_0, int col1_0, int toff0, const void* B1, int col0_1, int col1_1, int toff1, const void* B2, int col0_2,
                      int col1_2, int toff2, int64_t ldb, void* Y, int64_t ldy, const void* bias, const void* residual, int64_t ldr, int M,
                      int N, int K, void* workspace, int64_t ws_bytes, void* stream);
/* Decode attention (flash-decoding, decode.hip; the kernel body, the partial layout, the combine and the launcher that the six
 * other rv_attn_decode_* / rv_attn_extend_* entry points below share with it or with each other are csrc/attn_split.h): for every sequence b and q head h, softmax(scale * q[b,h] K^T) V over the cached keys
 * [0, kv_len[b]) of kv head h / (H / Hkv), hd in {64, 128}, up to 8 q heads per kv head (GQA), fp32 softmax and accumulation.
 * cache: bf16 [B][L_max][ld_c] (sequence stride bs_c), K of kv head g at columns g*hd, V at v_off + g*hd.  q: [B, H*hd] rows (ld_q);
 * out: bf16 [B, H*hd] rows (ld_o).  Keys are split into chunks of `chunk` rows (a multiple of 16 for hd 128, of 32 for hd 64,
 * <= 512) over workgroups; each writes (o, m, l) partials to `part` (B * H * ceil(L_max / chunk) * (hd + 2) floats) and a second
 * launch merges a sequence's chunks in chunk order.  kv_len is an int32 device array, values <= L_max (0: the row is all zeros).
 * ld_q < H*hd or ld_o < H*hd is refused (RV_ERR_ARG), as in rv_attn_extend_bf16. */
int rv_attn_decode_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len,
                        int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk,
                        float scale, void* stream);
/* Decode attention probabilities (attn_probs.hip; reference: output_attentions in modeling_llama.py:352-382, attn_weights =
 * softmax(Q K^T / sqrt(hd) + mask) in fp32): for every sequence b and q head h the normalised fp32 row softmax(scale * q[b,h] K^T) over
 * the cached keys [0, n_b), n_b = min(kv_len[b], L_max, L_out), of kv head h / (H / Hkv).  q, cache, ld_c, bs_c, kv_len, L_max, H, Hkv,
 * hd as for rv_attn_decode_bf16; V is never read.  L_out <= L_max is the number of columns the caller wants (pass L_out >= every
 * kv_len[b] for the distribution over all of a row's keys).  probs: fp32 [B][H][ld_p], ld_p >= L_out, or null; mean: fp32 [B][ld_m],
 * ld_m >= L_out, the mean over the H heads added in head order 0 .. H-1 then divided by H, or null; not both null.  Columns
 * [n_b, L_out) are written as 0.0f (kv_len[b] <= 0: the whole row), columns >= L_out are not touched.  A key at or past n_b is never
 * loaded.  ws: fp32 scratch of rv_attn_decode_probs_ws_bytes(B, H, L_out) bytes (the scaled scores and (max, sum) per (row, head)),
 * contents arbitrary, not to be shared by launches that can overlap.  No atomics, every reduction in a fixed order that is a function
 * of n_b alone: row b has the same bits alone and in any batch, and for every L_out >= n_b.  RV_ERR_ARG before any launch for a null
 * q / cache / kv_len / ws, both outputs null, hd not 64 or 128, H % Hkv, H / Hkv > 8, ld_q / ld_c / bs_c not multiples of 8 or too
 * small, ld_p / ld_m < L_out, L_out > L_max, B > 65535 and a short workspace. */
int rv_attn_decode_probs_f32(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, const int32_t* kv_len, int L_max,
                             int L_out, void* probs, int64_t ld_p, void* mean, int64_t ld_m, void* ws, int64_t ws_bytes, int B, int H,
                             int Hkv, int hd, float scale, void* stream);
int64_t rv_attn_decode_probs_ws_bytes(int B, int H, int L_out);
/* SnapKV prompt-cache compression (kvpress.hip; reference: none -- the reference decodes with HF's uncompressed DynamicCache,
 * transformers/cache_utils.py; the rule is Li et al. 2024, "SnapKV: LLM Knows What You Are Looking for Before Generation", restated in
 * tests/kvpress_ref.py).  Sequence b has P_b = cu[b+1] - cu[b] rows in the packed q|k|v product of the prompt pass; its last w rows are
 * the observation window, the n_b = P_b - w rows before it the prefix.  flags: int32 [B] or null; a sequence with flags[b] == 0 is
 * skipped by all three.  No atomics; every reduction runs in an order that is a function of the sequence's own P_b, w and H / Hkv, so a
 * sequence has the same bits alone and in any batch.
 * rv_kv_votes_f32: votes[b][g][j] (fp32 [B][Hkv][ld_v], j < n_b) = the sum over the H / Hkv query heads h of kv head g and the w window
 * rows t of softmax(scale * q[h, n_b + t] K_g^T)[j], each row's fp32 softmax over its causal keys [0, n_b + t].  q / k: the post-RoPE
 * bf16 rows (row strides ld_q / ld_k, head h at columns h*hd), hd in {64, 128}, H / Hkv <= 8, 1 <= w <= 64; max_P >= every P_b sizes
 * the grid.  Q K^T runs on v_mfma_f32_16x16x32_bf16 with each 128-key chunk (fixed in absolute position) staged once in LDS for all
 * w * H / Hkv query rows; a first pass writes per-(row, chunk) max and sum, merged in chunk order, a second recomputes the scores and
 * adds exp(s - m) / l.  V is never read; a key at or past P_b is never loaded, a key past a row's causal limit gets an exact-zero
 * weight; columns [n_b, ld_v) are not touched, and a sequence with n_b < 1 is skipped.  ws: rv_kv_votes_ws_bytes(B, H, Hkv, w, max_P)
 * bytes, contents arbitrary.
 * rv_kv_select_i32: keep[b][g][0..N) (int32 [B][Hkv][N]) = the N - w prefix positions with the largest
 * pooled[j] = max(votes[max(0, j - k/2) .. min(n_b - 1, j + k/2)]), ties to the lower position, in ascending order, then the window
 * positions n_b .. P_b - 1.  Votes must be non-negative (they order as their bit patterns: a radix select, one bit per sweep).  Only
 * sequences with P_b > N are written.  ws: rv_kv_select_ws_bytes(B, Hkv, ld_v) bytes.
 * rv_kv_gather_bf16: for every sequence with P_b > N, slot s < N and kv head g, the K (columns g*hd) and V (columns v_off + g*hd) of
 * row cu[b] + keep[b][g][s] of kv (row stride ld_kv) are copied to row seq[b] * L_max + s of cache (row stride ld_c, n_rows
 * sequences of L_max rows); nothing else is written, and an entry of keep outside [0, P_b) or a seq[b] outside [0, n_rows) writes
 * nothing.
 * RV_ERR_ARG before any launch: the conditions of rv_attn_decode_probs_f32 on pointers, B, H, Hkv, hd and strides, and w outside
 * [1, 64], max_P <= w, ld_v < max_P - w, N <= w, k even or outside [1, 63], N > L_max, a short workspace. */
int rv_kv_votes_f32(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const int32_t* cu, const int32_t* flags, int max_P, void* votes,
                    int64_t ld_v, void* ws, int64_t ws_bytes, int B, int H, int Hkv, int hd, int w, float scale, void* stream);
int64_t rv_kv_votes_ws_bytes(int B, int H, int Hkv, int w, int max_P);
int rv_kv_select_i32(const void* votes, int64_t ld_v, const int32_t* cu, const int32_t* flags, void* keep, void* ws, int64_t ws_bytes, int B,
                     int Hkv, int N, int w, int k, void* stream);
int64_t rv_kv_select_ws_bytes(int B, int Hkv, int64_t ld_v);
int rv_kv_gather_bf16(const void* kv, int64_t ld_kv, int v_off, const int32_t* cu, const int32_t* flags, const int32_t* keep,
                      const int32_t* seq, void* cache, int64_t ld_c, int L_max, int n_rows, int B, int Hkv, int hd, int N, void* stream);
/* Extend attention (the prompt pass of a continued generation, over a reused KV cache): sequence b has n_b = cu_q[b+1] - cu_q[b] >= 1
 * new query rows q[cu_q[b] .. cu_q[b+1]) at positions r[b] .. r[b] + n_b - 1, whose K|V rows are already in the cache; query i attends
 * causally to the keys [0, r[b] + i] of kv head h / (H / Hkv).  hd in {64, 128}, up to 8 q heads per kv head, fp32 softmax and
 * accumulation, bf16 MFMA for Q K^T and P V.  cache / q / out as for rv_attn_decode_bf16 (q and out: [M, H*hd] rows, M = cu_q[B]);
 * cu_q (B + 1 entries) and r (B entries) are int32 device arrays with r[b] + n_b <= L_max; max_q >= every n_b.  Keys are split into
 * chunks of `chunk` positions (a multiple of 64) fixed in absolute key position; each workgroup (chunk, kv head, tile of query rows
 * of one sequence) writes (o, m, l) partials to `part` (M * H * ceil(L_max / chunk) * (hd + 2) floats) and a second launch merges a
 * row's chunks in chunk order: a row's result is bit-identical whatever else shares the launch, the other rows of its own sequence
 * included (a row of an n-row call has the bits of the same query sent alone as a one-row call at its position).  Cache positions at
 * or past r[b] + n_b are never loaded and may hold anything (NaN included), and the combine reads only partial slots some workgroup
 * wrote, so `part` needs no initialisation.  A key INSIDE the suffix that a row may not see (positions r[b] + i + 1 .. r[b] + n_b - 1)
 * is not skipped: a workgroup stages the keys up to its tile's last row (tiles of 64 / 32 / 16 rows for 1 / 2 / >= 3 q heads per kv
 * head, counted from the sequence's first new row) and gives such a key an exact-zero weight, so the suffix's own K|V rows must be
 * finite: a non-finite K|V row at position j makes non-finite, beside the rows that see it, the earlier rows of j's own tile whose
 * position lies in j's chunk (0 * inf); every other row keeps its bits. */
int rv_attn_extend_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* cu_q,
                        const int32_t* r, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int M, int max_q,
                        int H, int Hkv, int hd, int chunk, float scale, void* stream);
/* KV cache append: cache[b][pos[b]][0:width] = src[b][0:width] (bf16; rows of the post-RoPE k|v columns of the qkv product);
 * pos is an int32 device array, slots outside [0, L_max) are skipped.  width % 8 == 0.  ld_src < width or ld_c < width is refused
 * (RV_ERR_ARG). */
int rv_kv_append_bf16(const void* src, int64_t ld_src, void* cache, int64_t ld_c, int64_t bs_c, const int32_t* pos, int L_max, int B,
                      int width, void* stream);
/* Greedy token choice: out[r] (int64) = argmax over the first n columns of fp32 row r (torch.argmax: lowest index among equal
 * maxima, NaN counts as the maximum); columns >= n (vocabulary pad rows of the lm_head) are never read. */
int rv_argmax_rows_f32(const float* x, int64_t ld, int rows, int n, int64_t* out, void* stream);
/* Greedy logits processors fused with the argmax (HF: GenerationMixin._get_logits_processor, generation/logits_process.py, run on the
 * scores of each greedy step): in place on fp32 row r (first n columns, n <= 262144), in HF's order,
 *   RepetitionPenaltyLogitsProcessor   every DISTINCT token of the row's history: x < 0 ? x * p : x / p (IEEE fp32; p = 1: off);
 *   NoRepeatNGramLogitsProcessor       ngram > 0, t >= ngram: every window i <= t - ngram whose first ngram - 1 tokens equal the last
 *                                      ngram - 1 generated ones bans its last token (ngram = 1 bans every generated token);
 *   NoBadWordsLogitsProcessor          multi-token sequences, CSR (bad_tok, bad_off[n_bad + 1]): a sequence of length L is checked
 *                                      when t >= L; if its first L - 1 tokens equal the last L - 1 generated ones, its last token is banned;
 *   ban[0 .. n_ban)                    ids banned on every row this step, composed by the caller: SuppressTokens, SuppressTokensAtBegin
 *                                      (t == 0), MinLength / MinNewTokensLength (EOS while t < the minimum), one-token bad words;
 * a banned entry becomes -inf; then out[r] = argmax of the processed row (rv_argmax_rows_f32's semantics).  hist: int32 [rows, >= t]
 * rows of ld_hist, the t tokens generated so far (pads of finished rows included, the prompt excluded: HF's input_ids of inputs_embeds
 * generation).  Ids outside [0, n) are ignored.  Only entries a processor touches are written.  Rows are independent (no atomics to
 * global memory).  Differs from HF in one case: HF ADDS -inf for a bad word, so a +inf / NaN entry there becomes NaN; here it becomes -inf. */
int rv_logits_process_argmax_f32(float* x, int64_t ld, int rows, int n, const int32_t* hist, int64_t ld_hist, int t, float rep_penalty,
                                 int ngram, const int32_t* ban, int n_ban, const int32_t* bad_tok, const int32_t* bad_off, int n_bad,
                                 int64_t* out, void* stream);
/* The same processors for rows at different steps (continuous batching, generate_batch): row r is at step t[r] with EOS minimum
 * min_new[r] (int32 device arrays of `rows` entries, as slot[]); its history is hist[slot[r]][0 .. t[r]) of an int32 [hist_rows,
 * hist_cols] array of row stride ld_hist (hist may be NULL with hist_rows = 0: no history), so a history row stays with its KV-cache
 * slot.  The ban lists are passed apart and composed per row: ban_always on every row (suppress_tokens, one-token bad words), ban_begin
 * where t[r] == 0, ban_eos where t[r] < min_new[r].  Penalty, n-gram and multi-token bad words as rv_logits_process_argmax_f32; with
 * every t[r] equal (and the lists composed as that entry's ban) the processed rows and out[] are bit-identical to it.  logprob (fp32
 * [rows] or NULL): logprob[r] = processed[out[r]] - logsumexp(processed row), from a running max and rescaled sum kept in the same
 * sweep and merged in a fixed order (the row is read once).  One workgroup per row, no global atomics: a row's result does not depend
 * on the other rows of the launch.  History reads are clamped to [0, hist_cols) and a slot outside [0, hist_rows) reads none. */
int rv_logits_process_argmax_rows_f32(float* x, int64_t ld, int rows, int n, const int32_t* hist, int64_t ld_hist, int hist_rows,
                                      int hist_cols, const int32_t* slot, const int32_t* t, const int32_t* min_new, float rep_penalty,
                                      int ngram, const int32_t* ban_always, int n_always, const int32_t* ban_begin, int n_begin,
                                      const int32_t* ban_eos, int n_eos, const int32_t* bad_tok, const int32_t* bad_off, int n_bad,
                                      int64_t* out, float* logprob, void* stream);

/* Seeded sampling (generate(do_sample=True, seed=...); HF: GenerationMixin._sample with do_sample=True, the warpers of
 * generation/logits_process.py in HF's order, then softmax and one draw).  Per fp32 row r (first n columns, n <= 262144; the greedy
 * processors above run first when one is active), with x the row as it comes in:
 *   TemperatureLogitsWarper  s_i = x_i / temperature (IEEE fp32 division; temperature > 0);
 *   TopKLogitsWarper         top_k > 0: v = the k'-th largest s, k' = min(top_k, n); s_i < v is removed, every tie with v stays (0: off);
 *   TopPLogitsWarper         top_p < 1: p = softmax(s) over what remains; i is removed iff sum{p_j : s_j <= s_i} <= 1 - top_p.  The
 *                            maximum always stays.  Among EQUAL scores at the cut HF's sort order is unspecified: here all of them stay;
 *   MinPLogitsWarper         min_p > 0: i is removed iff p_i < min_p * max_j p_j, evaluated as fl(s_i - max s) < fl(log(min_p));
 *   draw                     q = softmax over the kept set, u = (b + 0.5) * 2^-24 with b the top 24 bits of splitmix64(t[r] *
 *                            0xD1342543DE82EF95 + splitmix64(seed[r] * 1000003)) (portable_rng._stream(seed, 0, t + 1)[t] >> 40; the
 *                            kernel holds u as the integer 2 b + 1 over 2^25, never as a float); out[r] = the lowest id i with sum{q_j : j <= i, j kept} > u, the sum in TOKEN-ID order.
 * seed (uint64) and t (int32, the row's own step) are device arrays of `rows` entries.  write_scores != 0: the row is overwritten with
 * the warped scores, s_i (bit-equal to the fp32 quotient) where kept and -inf where removed (HF's output_scores under sampling);
 * write_scores == 0: the row is only read.  logprob (fp32 [rows] or NULL): log q[out[r]].  A row that holds a NaN or +inf, or no finite
 * entry, cannot be sampled: out[r] = -1, logprob[r] = NaN, and the row is left as it is.
 * A fixed number of workgroups (8) share a row, each with a fixed run of its tiles; every sweep is a launch, and the partial maxima and
 * integer histograms of one launch are merged in a fixed order by the next.  No sort, no float atomics, no global atomics: probabilities enter every sum as 64-bit fixed point, rne(exp(s_i - max s) * 2^40),
 * added as integers, so the token, the written scores and logprob of a row are the same bits on every launch, for every `rows` and
 * whatever the other rows hold.  depth = 1: the one fp32 addition a term of the CDF sum passes through is the fma that applies the
 * rounding residual of s_i - max s to its exponential; the sum itself is integer.  A normalised partial sum is within
 * (depth + 4) * 2^-23 of exact arithmetic on the fp32 s (csrc/sample.hip derives it).  Two sweeps of the row with every warper off,
 * four more for top-k, four more for top-p; one launch per sweep and one for the draw.  ws: device scratch of ws_bytes >=
 * rv_sample_ws_bytes(rows) bytes, 8-byte aligned, contents arbitrary; it must not be shared by launches that can overlap. */
int rv_sample_rows_f32(float* x, int64_t ld, int rows, int n, const uint64_t* seed, const int32_t* t, float temperature, int top_k,
                       float top_p, float min_p, int write_scores, int64_t* out, float* logprob, void* ws, int64_t ws_bytes, void* stream);
/* Host function: the bytes of scratch rv_sample_rows_f32 needs for `rows` rows. */
int64_t rv_sample_ws_bytes(int rows);
/* Host function: the 24 bits b of the draw above for (seed, t), the same code the kernel runs. */
uint32_t rv_sample_uniform24(uint64_t seed, int32_t t);
/* rv_sample_rows_f32 drawing from another stream: b is the top 24 bits of portable_rng._stream(seed, tag, t + 1)[t], that is
 * splitmix64(t * 0xD1342543DE82EF95 + splitmix64(seed * 1000003 + tag)), tag >= 0.  The same kernels; tag 0 is rv_sample_rows_f32 bit
 * for bit (it calls this entry).  Assisted sampling draws the draft model's tokens with tag 2, see rv_spec_accept_rows_f32. */
int rv_sample_rows_tagged_f32(float* x, int64_t ld, int rows, int n, const uint64_t* seed, const int32_t* t, int32_t tag, float temperature,
                              int top_k, float top_p, float min_p, int write_scores, int64_t* out, float* logprob, void* ws,
                              int64_t ws_bytes, void* stream);
/* Host function: rv_sample_uniform24 for the stream `tag`. */
uint32_t rv_sample_uniform24_tagged(uint64_t seed, int32_t tag, int32_t t);

/* ---- speculative sampling (generate(assistant_model=..., do_sample=True), radvlm_amd/csrc/spec.hip) ---------------------------------
 * The accept / resample step of assisted generation under sampling (HF: generation/utils.py _speculative_sampling; Leviathan et al.
 * 2023).  Group g holds R target rows p[g * R + i, :n] and R - 1 draft rows q[g * (R - 1) + i, :n], fp32 warped scores as
 * rv_sample_rows_f32(write_scores = 1) leaves them (finite where kept, -inf where removed), and the R - 1 drafted ids draft[g, i]
 * (int32).  P_i / Q_i: the softmax over the finite entries of p-row / q-row i.  For i = 0 .. R - 2 and x = draft[g, i]:
 *   draft i is accepted iff 0 <= x < n, P_i(x) > 0 and u_a * Q_i(x) <= P_i(x);
 *   n_accept[g] = a = the drafts accepted before the first one that is not;
 *   a < R - 1: token[g] is drawn from r(j) ~ max(0, P_a(j) - Q_a(j)), and from P_a when r is identically 0;  a = R - 1: from P_{R-1};
 *   either way it is the lowest id j whose cumulative sum in TOKEN-ID order exceeds u_r times the total (the sampler's draw rule);
 *   logprob[g] = log P_a(token[g]), under the target's distribution.
 * u_a of draft i is the uniform (2 b + 1) / 2^25 of rv_sample_uniform24_tagged(seed[g], 1, t0[g] + i), u_r that of (seed[g], 0,
 * t0[g] + a): t0 (int32 [groups]) is the step of row 0, seed uint64 [groups].  The draft model's own draws use tag 2
 * (rv_sample_rows_tagged_f32): three distinct streams, since a draft's draw and its accept test must be independent.  R = 1 (no
 * drafts; q and draft may be NULL) is the plain draw from P_0 with tag 0.
 * A p-row or q-row on the path (rows 0 .. a) that holds a NaN or +inf, or no finite entry, ends it: n_accept[g] = the drafts accepted
 * before that row, token[g] = -1, logprob[g] = NaN.  Columns >= n are never read; rows need 4-byte alignment only.
 * Exact cases: bitwise equal p-row i and q-row i accept draft i for every seed (both sides of the test are then one double times u_a <
 * 1 and times 1); a draft with p = -inf is never accepted.  Elsewhere an accept test or a draw may differ from exact arithmetic on the
 * fp32 scores only inside a band of delta = 2^-25, relative to the larger side: for a test the sides are u_a * Q_i(x) and P_i(x); for a
 * draw at id j they are sum{P : ids <= j} + u_r * sum{Q} and sum{Q : ids <= j} + u_r * sum{P} over the ids with P > Q (Q = 0 for a draw
 * from P).  Derivation (csrc/spec.hip): exp in float64; a row's normaliser Z = sum rne(exp(s_j - max s) * 2^44) as a 64-bit integer,
 * within n * 2^-45 <= 2^-27 of exact; float64 products and sums over <= 263,168 terms add < 2^-34.  delta is below rv_sample_rows_f32's
 * (depth + 4) * 2^-23.
 * One workgroup per row for max and Z, then one per group: thread k adds the weights of its fixed run of ids in id order, one thread
 * adds the 1024 run sums in order and walks the run that holds the target.  No float atomics, no global atomics: n_accept, token and
 * logprob of a group are the same bits on every launch, for every `groups` and whatever the other groups hold.  ws: device scratch of
 * ws_bytes >= rv_spec_ws_bytes(groups, R) bytes, 8-byte aligned, contents arbitrary.  RV_ERR_ARG: a null pointer, R outside 1 .. 32, n
 * outside 1 .. 262144, ld_p < n or ld_q < n, a short or misaligned ws. */
int rv_spec_accept_rows_f32(const float* p, int64_t ld_p, const float* q, int64_t ld_q, const int32_t* draft, const uint64_t* seed,
                            const int32_t* t0, int groups, int R, int n, int32_t* n_accept, int64_t* token, float* logprob, void* ws,
                            int64_t ws_bytes, void* stream);
/* Host function: the bytes of scratch rv_spec_accept_rows_f32 needs. */
int64_t rv_spec_ws_bytes(int groups, int R);

/* ---- beam search (generate_beams(), radvlm_amd/csrc/beam.hip) ----------------------------------------------------------------------
 * The reference reaches beam search through HF generate(num_beams=...) (finetuning/llava/eval/model_vqa.py --num_beams ->
 * HF:generation/utils.py _beam_search), which reorders the whole KV cache by the chosen parents after every token.  Here the cache is
 * never reordered: every beam appends to its own cache row and attention follows the beam's ancestry through a table. */
/* rv_attn_decode_bf16 with a per-key row lookup: key position j of query row r (rows of them, one q row and one kv_len each) is read,
 * at that same position j, from cache row  j < prefix_len[r] ? prefix_row[r] : tail_src[r * ld_t + (j - prefix_len[r])].
 * prefix_row, prefix_len (int32 [rows]) and tail_src (int32 rows of ld_t, tail_cols valid columns; NULL with tail_cols = 0) are device
 * arrays.  cache holds cache_rows rows of bs_c elements; every looked-up row is clamped into [0, cache_rows), a negative prefix_len
 * counts as 0 and a tail position >= tail_cols reads prefix_row[r], so no table content makes the kernel read outside the cache.
 * Entries for positions >= kv_len[r] are never read.  Chunking is by absolute key position with the same `chunk`, the per-chunk
 * arithmetic and the combine are rv_attn_decode_bf16's: out is BIT-IDENTICAL to rv_attn_decode_bf16 on the cache materialised by that
 * gather, for hd 64 and 128, up to 8 q heads per kv head and kv_len 0 .. L_max.  The lookup is resolved per chunk into LDS; the K / V
 * loads stay 16 bytes per lane.  part: rows * H * ceil(L_max / chunk) * (hd + 2) floats.  ld_q < H*hd or ld_o < H*hd is refused
 * (RV_ERR_ARG), as there. */
int rv_attn_decode_beam_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len,
                             int L_max, const int32_t* prefix_row, const int32_t* prefix_len, const int32_t* tail_src, int64_t ld_t,
                             int tail_cols, int cache_rows, void* out, int64_t ld_o, void* part, int64_t part_bytes, int rows, int H,
                             int Hkv, int hd, int chunk, float scale, void* stream);
/* HF _beam_search's nn.functional.log_softmax(logits, dim=-1) on the fp32 scores, in place on the first n columns (n <= 262144) of
 * each row: x_i <- fl(fl(x_i - m) - L), m = max x, L = fl32(log(sum exp(x_i - m))), the sum in fp64 in a fixed order (per thread in
 * index order, lanes by xor butterfly, waves 0..3).  One workgroup per row: a row's bits depend on neither `rows` nor the other rows.
 * Columns >= n are never touched.  -inf entries stay -inf; a row with a NaN, a +inf or no finite entry becomes NaN throughout, as in
 * torch.  |result - exact| <= 2^-24 (2 |result| + 4 ln n + 3) on a finite row (csrc/beam.hip derives it). */
int rv_log_softmax_rows_f32(float* x, int64_t ld, int rows, int n, void* stream);
/* HF _get_top_k_continuations' torch.topk over the accumulated log-probs: for each of `groups` prompts, over its nb consecutive rows
 * r of x (row g * nb + r, first n columns), v(r, i) = fl(x[r][i] + score[g * nb + r]) (one fp32 add) and out_v / out_i [groups, K]
 * are the K best candidates as (v, flat index r * n + i), ordered by v descending, then flat index ascending, NaN ranking highest
 * (rv_argmax_rows_f32's rule).  The order is total where torch leaves ties open, so the output is the same bits for any grid.
 * 1 <= nb <= 16, 1 <= K <= min(64, nb * n), n <= 262144.  Slices of the candidates are reduced to their K best by K rounds of a
 * workgroup argmax and merged by a second launch: no sort of a row, no float atomics, no global atomics.  ws: device scratch of
 * ws_bytes >= rv_beam_topk_ws_bytes(groups, nb, n, K), contents arbitrary; not to be shared by launches that can overlap. */
int rv_beam_topk_f32(const float* x, int64_t ld, int groups, int nb, int n, const float* score, int K, float* out_v, int32_t* out_i,
                     void* ws, int64_t ws_bytes, void* stream);
/* Host function: the bytes of scratch rv_beam_topk_f32 needs. */
int64_t rv_beam_topk_ws_bytes(int groups, int nb, int n, int K);

/* ---- classifier-free guidance (generate(guidance_scale=), radvlm_amd/csrc/cfg.hip) ---------------------------------------------------
 * HF reaches it through generate(guidance_scale=g, negative_prompt_ids=...) (HF:generation/logits_process.py
 * UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__), with a second forward pass per token for the unconditional logits.  Here
 * the unconditional sequence is one more row of the same decode step, and this kernel combines the two raw fp32 logits rows. */
/* For each of `rows` row pairs and every column j < n (n <= 262144): with lc / lu the bits rv_log_softmax_rows_f32 gives row r of c / u,
 *     c[r][j] <- fl(fl(g * fl(lc - lu)) + lu)
 * three separately rounded fp32 operations in torch's order (no fma contraction).  c: raw conditional logits, rows of ld_c floats,
 * overwritten; u: raw unconditional logits, rows of ld_u floats, never written; the two must not overlap.  Columns >= n of both are
 * never touched.  No atomics and a fixed reduction order: a row's bits depend on that row pair and on g alone, not on `rows`, the launch
 * structure or the other rows.  Non-finite logits are outside the contract.
 * ws NULL: one launch, one workgroup per pair.  ws given (device scratch of ws_bytes >= rv_cfg_guide_ws_bytes(rows), 4-byte aligned,
 * contents arbitrary, not to be shared by launches that can overlap): the row statistics by one launch, the elementwise part by a
 * second one that spreads every row over many workgroups -- the same bits, faster on few long rows.
 * |result - exact| <= (1 + 2^-20) (|g| E(lc) + |1 - g| E(lu) + |fl32(g) - g| |lc - lu| + 2^-24 (2 |g| |lc - lu| + |exact|)) with
 * E(l) = 2^-24 (2 |l| + 4 ln n + 3), against exact arithmetic on the fp32 inputs and the real g (csrc/cfg.hip derives it).
 * n < 1, rows < 1, ld_c < n, ld_u < n, a null c or u, a short or misaligned ws are refused (RV_ERR_ARG). */
int rv_cfg_guide_rows_f32(float* c, int64_t ld_c, const float* u, int64_t ld_u, int rows, int n, float g, void* ws, int64_t ws_bytes,
                          void* stream);
/* Host function: the bytes of scratch the two-launch form of rv_cfg_guide_rows_f32 needs. */
int64_t rv_cfg_guide_ws_bytes(int rows);

/* ---- DoLa, decoding by contrasting layers (generate(dola_layers=), radvlm_amd/csrc/dola.hip) -----------------------------------------
 * HF reaches it through generate(dola_layers=...) (transformers 4.43 - 4.5x: _dola_decoding, _dola_select_contrast,
 * _relative_top_filter).  Here the candidate layers' hidden states of the current token go through lm_head as further rows of the
 * decode step, and this kernel turns the 1 + n_layers raw fp32 logits rows of a sequence into the contrasted score row. */
/* For each of `rows` rows: f's row r (rows of ld_f floats, the last layer's raw logits, overwritten) against the n_layers candidate
 * rows c + k * stride_c_layer + r * ld_c (0 <= k < n_layers <= 16, never written, not overlapping f), first n columns (n <= 262144).
 * With lf / lq_k the bits rv_log_softmax_rows_f32 gives the rows:
 *   n_layers > 1: J_k = 0.5 * mean_v M ((log M - lf) + (log M - lq_k)), M = (exp(lf) + exp(lq_k)) / 2 (the Jensen-Shannon divergence;
 *   fp32 terms with the fast exp / log, a term with M < FLT_MIN counting as 0, summed in fp64 in a fixed order), and
 *   chosen[r] = argmax_k J_k, an exact tie going to the lower k; n_layers == 1: chosen[r] = 0 and no divergence is computed.
 *   f[r][v] <- -inf where lf_v < fl(max(lf) + log_rt), else fl(lf_v - lb_v), lb the chosen row's log-softmax: one fp32 rounding on
 *   the log-softmax kernel's bits, so given chosen[r] the row is bit for bit what torch computes from rv_log_softmax_rows_f32's rows.
 * log_rt: fl32(ln relative_top), from the host.  chosen: int32 [rows].  jsd: fp32 [rows][n_layers] receiving J (0 for n_layers == 1),
 * or NULL.  Columns >= n are never touched.  No atomics and a fixed reduction order: a row's f, chosen and jsd bits depend on that
 * row's 1 + n_layers rows alone, not on `rows`, the grid or the other rows.  Non-finite logits are outside the contract but cannot
 * fault (chosen stays below n_layers).  ws: device scratch of ws_bytes >= rv_dola_ws_bytes(rows, n_layers), 8-byte aligned, contents
 * arbitrary, not to be shared by launches that can overlap.
 * With u = 2^-24, E(l) = u (2 |l| + 4 ln n + 3), X(l) = u (|l| + 2), A = 2 log M - lf - lq, Ab = |log M - lf| + |log M - lq|, T = M A:
 *   |J^_k - J_k| <= (1 + 2^-10) (0.5 / n) sum_v B_v + u |J_k| + 2^-100,
 *   B_v = |p A / 2 + (p - q) / 2| E(lf) + |q A / 2 + (q - p) / 2| E(lq) + (|A| + 2) ((p X(lf) + q X(lq)) / 2 + u M) + 8 u M |log M|
 *         + 2 u M Ab + u |T|
 * against exact arithmetic on the fp32 inputs (csrc/dola.hip derives it).
 * A null f, c, chosen or ws, rows < 1, n_layers < 1 or > 16, n < 1 or > 262144, ld_f < n, ld_c < n, a short or misaligned ws are
 * refused (RV_ERR_ARG). */
int rv_dola_contrast_rows_f32(float* f, int64_t ld_f, const float* c, int64_t ld_c, int64_t stride_c_layer, int rows, int n_layers, int n,
                              float log_rt, int32_t* chosen, float* jsd, void* ws, int64_t ws_bytes, void* stream);
/* Host function: the bytes of scratch rv_dola_contrast_rows_f32 needs. */
int64_t rv_dola_ws_bytes(int rows, int n_layers);

/* ---- constrained decoding (generate(constraint=), radvlm_amd/csrc/constrain.hip, radvlm_amd/constraints.py) -------------------------
 * HF reaches it through generate(prefix_allowed_tokens_fn=...): PrefixConstrainedLogitsProcessor adds a mask of 0 / -inf after
 * MinNewTokensLength and before SuppressTokens.  Every processor of rv_logits_process_argmax*_f32 other than the repetition penalty
 * only writes -inf and the penalty maps -inf to -inf, so masking the raw row first and running the fused kernel unchanged gives HF's
 * row.  Two differences: an allowed -0.0 keeps its sign (HF's `+ 0.0` makes it +0.0), and a banned NaN / +inf becomes -inf where HF
 * keeps the NaN (the deviation the bad-words processor documents).  Here the allowed sets come from a deterministic automaton over
 * token ids instead of a Python callback per row and step. */
/* The automaton in CSR form: edge_off int32 [n_states + 1], edge_tok int32 [n_edges] strictly ascending within a state, edge_next
 * int32 [n_edges] in [-1, n_states).  state: int32 [state_rows]; a value s >= 0 is live (allowed ids edge_tok[edge_off[s] ..
 * edge_off[s + 1])), -1 is free, -2 and every other value outside [0, n_states) is dead.
 * For each of `rows` rows of x (fp32, rows of ld floats, first n columns, n <= 262144), with si = slot ? slot[r] : r (slot: int32
 * [rows] of distinct entries, or NULL) and s = state[si]:
 *   advance  tok != NULL (int64 [rows]: the token chosen from the row's previous step): a live s becomes the edge_next of the edge
 *            (s, tok[r]) -- -2 when s has no such edge, or when tok[r] is no int32 -- a negative s stays, and state[si] <- s.
 *            tok == NULL (the first step after a prompt pass or an admission): s is used as it is and state is not written.
 *   mask     s == -1: the row is not accessed.  Dead: x[r][0 .. n) <- -inf.  Live: every column of [0, n) that is not an allowed id
 *            <- -inf; allowed columns are neither read nor written (NaN payloads and -0.0 stay).  Edge ids outside [0, n) are ignored.
 * The kernel loads no element of x; columns >= n are never written.  One launch, one workgroup per row, no global atomics: a row's
 * bits and its new state depend on its own state, token and edge run alone.  Tables that break the rules above cannot fault (run
 * bounds are clamped into [0, n_edges]); a slot outside [0, state_rows) makes the row dead and writes no state.
 * A null x, state or table, rows < 1, n < 1 or > 262144, ld < n, state_rows < 1, slot == NULL with rows > state_rows, n_states < 1
 * and n_edges < 1 are refused (RV_ERR_ARG). */
int rv_constrain_rows_f32(float* x, int64_t ld, int rows, int n, int32_t* state, int state_rows, const int32_t* slot, const int64_t* tok,
                          const int32_t* edge_off, const int32_t* edge_tok, const int32_t* edge_next, int n_states, int n_edges,
                          void* stream);

/* ---- prompt-lookup decoding (generate(prompt_lookup_num_tokens=), radvlm_amd/csrc/lookup.hip) ----------------------------------------
 * The reference reaches it through HF generate(prompt_lookup_num_tokens=k) (HF:generation/candidate_generator.py
 * PromptLookupCandidateGenerator -> _assisted_decoding): k tokens drafted from n-gram repeats of the sequence are verified by one
 * forward pass of k + 1 rows.  Here that pass is a decode step of R = k + 1 rows on one cache row (LlavaEngine.verify_step). */
/* rv_attn_decode_bf16 for R consecutive query rows per sequence: query row b * R + i (0 <= i < R, 1 <= R <= 32) attends the keys
 * [0, min(kv_len0[b] + i, L_max)) of sequence b (kv_len0: int32 [B], device), whose own K|V rows are in the cache already.  hd 64 or
 * 128, up to 8 q heads per kv head, `chunk` as there; part: B * R * H * ceil(L_max / chunk) * (hd + 2) floats.  A workgroup takes a
 * chunk of one kv head for a group of rows (16 / (H / Hkv) of them) and loads and converts each K and V fragment once for the group;
 * a key a row may not see is skipped, never multiplied by zero, so positions at or past a row's key count may hold anything (NaN
 * included).  Chunking by absolute key position, the key-to-lane assignment, each lane's summation order, the shuffle trees, the
 * wave 0..3 merge and the combine's chunk order are rv_attn_decode_bf16's: every row of out is BIT-IDENTICAL to rv_attn_decode_bf16
 * run on that row alone with kv_len = kv_len0[b] + i.  No global atomics.  R outside 1 .. 32, a short `part`, ld_q < H*hd or
 * ld_o < H*hd are refused (RV_ERR_ARG), as there. */
int rv_attn_decode_verify_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len0,
                               int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int R, int H, int Hkv, int hd,
                               int chunk, float scale, void* stream);

/* ---- int8 KV cache (generate(kv_cache_dtype="int8"), radvlm_amd/csrc/kvq.hip) --------------------------------------------------------
 * The reference has no quantised cache (HF's QuantizedCache is the nearest relative); the rule is rv_quantize_rows_w8_bf16's, per group.
 * One group = the hd values of one kv head of K, or of V, at one cached position:
 *     amax = max |x|    s = amax / 127 (1 for an all-zero group)    q = clamp(rint(float(x) / s), -127, 127)    x^ = bf16_rne(float(q) * s)
 * IEEE fp32 division, round half to even; non-finite inputs are outside the contract.  Per decoder layer the cache is two tensors of
 * flat rows (flat row = b * L_max + position, consecutive): q8 int8 rows of ld_q bytes with the columns of the bf16 cache (K of kv
 * head g at g*hd, V at Hkv*hd + g*hd), and s fp32 rows of ld_s floats (column g: K head g; column Hkv + g: V head g). */
/* Quantises M source rows of 2*Hkv*hd bf16 values (rows of ld_src elements: the k|v columns of a q|k|v product) into the flat cache rows
 * rows[0 .. M) (int64, device); a row outside [0, cache_rows) is skipped.  xhat (optional, NULL to skip): a bf16 cache of the bf16 layout
 * (rows of ld_x) that receives x^ in the same flat rows.  q8 and s are given together or both NULL (then xhat alone is written).
 * hd 64 or 128; ld_src, ld_q, ld_x multiples of 8 and >= 2*Hkv*hd, ld_s >= 2*Hkv (RV_ERR_ARG otherwise).  No atomics: a group is
 * reduced by an xor butterfly inside one wave (max is order-free).  Two source rows naming one cache row race. */
int rv_kv_quantize_rows_bf16(const void* src, int64_t ld_src, void* q8, int64_t ld_q, float* s, int64_t ld_s, void* xhat, int64_t ld_x,
                             const int64_t* rows, int64_t cache_rows, int M, int Hkv, int hd, void* stream);
/* The same arithmetic addressed like rv_kv_append_bf16: source row b goes to flat row b * L_max + pos[b] (pos int32 [B], device); a
 * position outside [0, L_max) is skipped. */
int rv_kv_append_q8_bf16(const void* src, int64_t ld_src, void* q8, int64_t ld_q, float* s, int64_t ld_s, void* xhat, int64_t ld_x,
                         const int32_t* pos, int L_max, int B, int Hkv, int hd, void* stream);
/* rv_attn_decode_bf16 over the int8 cache: cache_q8 int8 [B][L_max][ld_c] (sequence stride bs_c, V at column v_off + g*hd), cache_s
 * fp32 [B][L_max][ld_s] (sequence stride bs_s, V scales at column vs_off + g).  A lane loads 8 bytes and its group's scale and rebuilds
 * bf16_rne(float(q) * s) in registers; the assignment of (key row, 8-element slice) to (wave, lane), each lane's key order, the xor
 * butterflies, the wave-order sum, `part` and the combine are rv_attn_decode_bf16's, so out is BIT-IDENTICAL to rv_attn_decode_bf16 on
 * the dequantised cache at the same `chunk`, for every kv_len.  Keys at or past kv_len[b] are never loaded: bytes and scales there may
 * hold anything (-128, NaN).  Same limits and refusals: hd 64 or 128, H / Hkv <= 8, chunk <= 512 and a multiple of 16 (hd 128) or 32
 * (hd 64), part of B * H * ceil(L_max / chunk) * (hd + 2) floats, ld_q / ld_o >= H*hd. */
int rv_attn_decode_kv8_bf16(const void* q, int64_t ld_q, const void* cache_q8, int64_t ld_c, int64_t bs_c, int v_off, const float* cache_s,
                            int64_t ld_s, int64_t bs_s, int vs_off, const int32_t* kv_len, int L_max, void* out, int64_t ld_o, void* part,
                            int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk, float scale, void* stream);

/* ---- shared prompt prefixes (generate_batch(share_prefix=True), radvlm_amd/csrc/prefix.hip) ------------------------------------------
 * The reference evaluates a split one request at a time (HF generate() per sample), so each question about a radiograph pays for the
 * image's keys again; HF has no counterpart.  Here the requests of one generate_batch() call that begin with the same prompt records
 * keep bit-equal K|V at those positions of their own cache rows (copied, LlavaEngine / BatchScheduler), and this entry reads them once. */
/* rv_attn_decode_bf16 for rows grouped in tiles.  c0: int32 [B] (device), row b's shared chunk count; tile: int32 [B][16] (device),
 * tile[b][0] == b when row b leads a tile, whose rows are then tile[b][0 .. 16 / (H / Hkv)) up to the first -1; any other row has
 * tile[b][0] != b.  Workgroup (chunk c, kv head, row b) with c >= c0[b] is rv_attn_decode_bf16's.  With c < c0[b] it returns at once
 * unless b leads its tile; a leading workgroup loads and converts the chunk's K and V fragments once, from row b, and uses each for up
 * to 16 (row, q head) queries of its tile, writing every row's partial in the plain `part` layout; one combine per row with the row's
 * own kv_len.  CONTRACT: when every row of a tile has c0 equal to its leader's, holds at least c0 * chunk keys and holds K|V equal to
 * the leader's at positions below c0 * chunk, every row of out is BIT-IDENTICAL to rv_attn_decode_bf16 on the same cache at the same
 * `chunk` (key-to-lane assignment, each lane's summation order, the shuffle trees, the wave 0..3 merge and the combine are that
 * kernel's; a key a row may not see is skipped, never multiplied by zero).  c0 all zero: rv_attn_decode_bf16 on every row.  The table
 * is not trusted for bounds: entries outside [0, B) end a tile's list, and a query never sees a position at or past its row's kv_len
 * or the leader's, so rows past kv_len may hold anything (NaN included); a table that breaks the contract gives wrong values in the
 * rows it names, never an access outside q / cache / part.  Limits and refusals are rv_attn_decode_bf16's (hd 64 or 128, H / Hkv <= 8,
 * chunk <= 512 and a multiple of 16 (hd 128) or 32 (hd 64), part of B * H * ceil(L_max / chunk) * (hd + 2) floats).  No atomics. */
int rv_attn_decode_shared_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len,
                               const int32_t* c0, const int32_t* tile, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes,
                               int B, int H, int Hkv, int hd, int chunk, float scale, void* stream);

/* ---- scoring candidate answers (model.score(), radvlm_amd/csrc/score.hip) -----------------------------------------------------------
 * The reference's abnormality_classification task (radvlm/evaluation/evaluate_instructions.py) generates free text per finding and
 * string-matches it; lm-evaluation-harness's loglikelihood (and HF compute_transition_scores) instead reads log p(answer | prompt) off
 * one forward per (prompt + answer).  Here a prompt is prefilled once and every candidate answer runs only its own rows, reading the
 * prompt's keys in place. */
/* rv_attn_extend_bf16 with two key sources.  Sequence b has n_b = cu_q[b+1] - cu_q[b] >= 0 query rows at positions prefix_len[b] + i,
 * and query i attends causally to the keys [0, prefix_len[b] + i]: key j < prefix_len[b] is position j of row prefix_row[b] of
 * `prefix` (bf16 [P_rows][P_max][ld_p], row stride bs_p), key j >= prefix_len[b] is position j - prefix_len[b] of row b of `tail`
 * (bf16 [B][T_max][ld_t], row stride bs_t; the n_b tail rows are already written).  Both use the KV cache's column layout (K of kv
 * head g at g*hd, V at v_off + g*hd).  cu_q (B + 1), prefix_row and prefix_len (B) are int32 device arrays; max_q >= every n_b and
 * max_q <= T_max.  The work split, the 64-key stages, the online softmax, the partials and the combine are rv_attn_extend_bf16's and
 * the chunk grid is fixed in absolute key positions (only the address a staged key is loaded from is chosen per key): out is
 * BIT-IDENTICAL to rv_attn_extend_bf16 with r = prefix_len and the same `chunk` on the cache materialised as
 * prefix[prefix_row[b], :prefix_len[b]] ++ tail[b, :n_b], for hd 64 and 128 and up to 8 q heads per kv head.  Keys at or past
 * prefix_len[b] + n_b are never loaded: prefix positions >= prefix_len[b] and tail positions >= n_b may hold anything (NaN included).
 * A tail row that a query may not see (a later row of the same sequence) is staged with its tile and gets an exact-zero weight, as in
 * rv_attn_extend_bf16: the n_b tail rows must be finite.  A sequence
 * with n_b == 0 writes nothing.  A sequence whose prefix_row[b] is outside [0, P_rows) or whose prefix_len[b] is outside [0, P_max]
 * is not read at all and its rows of out are zeros.  part: M * H * ceil((P_max + T_max) / chunk) * (hd + 2) floats.  Refusals
 * (RV_ERR_ARG) as rv_attn_extend_bf16's, and a null prefix_row / prefix_len, P_rows <= 0, P_max <= 0, T_max <= 0, max_q > T_max. */
int rv_attn_extend_prefix_bf16(const void* q, int64_t ld_q, const void* prefix, int64_t ld_p, int64_t bs_p, int P_rows, int P_max,
                               const void* tail, int64_t ld_t, int64_t bs_t, int T_max, int v_off, const int32_t* cu_q,
                               const int32_t* prefix_row, const int32_t* prefix_len, void* out, int64_t ld_o, void* part,
                               int64_t part_bytes, int B, int M, int max_q, int H, int Hkv, int hd, int chunk, float scale, void* stream);
/* The log-prob of one given token per row, and the row's argmax: output row r reads row s = src_row ? src_row[r] : r of the fp32
 * logits x (x_rows rows of ld floats, first n columns, n <= 262144) and gets
 *     logprob[r] = fl(fl(x[s][target[r]] - m) - L),
 * (m, L) by the statements rv_log_softmax_rows_f32 runs (csrc/log_softmax.h), so the value is the bits that entry leaves at that
 * column; x is never written.  target[r] < 0 (an ignored position, e.g. -100): 0.0f.  target[r] >= n: NaN.  s outside [0, x_rows):
 * NaN, argmax[r] = -1, and no row is read.  A row with a NaN, a +inf or no finite entry gives NaN, as there; a -inf target in a finite
 * row gives -inf.  argmax (int64 [rows], or NULL to skip) follows rv_argmax_rows_f32's rule (lowest index among equal maxima, NaN
 * above everything) and is written whatever the target.  src_row (int32 [rows], or NULL) lets several outputs share one row, e.g. the
 * candidates that continue one prompt.  Columns >= n are never read.  One workgroup per output row, no atomics: a row's bits depend on
 * neither `rows` nor the other rows. */
int rv_token_logprob_rows_f32(const float* x, int64_t ld, int x_rows, int n, const int32_t* src_row, const int32_t* target, int rows,
                              float* logprob, int64_t* argmax, void* stream);

/* LoRA merge (peft merge_and_unload): W[N,K] <- bf16_rne(float(W) + scale * sum_j B[n,j] A[j,k]) in place, 1 <= r <= 256.  The sum runs in
 * fp32 on MFMA in a fixed order (r zero-padded to a multiple of 32) and is rounded once: the same inputs give the same bits for any
 * grid and any placement of W.  W: bf16 rows of ldw elements (a row slice of a fused q|k|v or gate|up store is fine), 16-byte aligned,
 * K % 8 == 0, ldw % 8 == 0.  B: bf16 [N, r] rows of ldb; A: bf16 [r, K] rows of lda.  No workspace. */
int rv_lora_merge_bf16(void* W, int64_t ldw, const void* B, int64_t ldb, const void* A, int64_t lda, int N, int K, int r, float scale,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif

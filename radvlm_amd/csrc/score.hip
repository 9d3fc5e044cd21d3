// Scoring candidate answers for gfx950 (model.score(), LlavaEngine.score_tails): the log-likelihood of token sequences the caller
// already has, after a prompt that many candidates share.
//
// rv_attn_extend_prefix_bf16 is extend.hip's attention with two key sources.  Query i of sequence b sits at position prefix_len[b] + i
// and sees the keys [0, prefix_len[b] + i]: key j < prefix_len[b] is position j of row prefix_row[b] of a prefix cache (the prompt,
// prefilled once, read in place by every candidate that continues it), key j >= prefix_len[b] is position j - prefix_len[b] of row b of
// a tail cache (the candidate's own rows, already written).  The work split, the 64-key LDS stages, the MFMA operand layouts, the online
// softmax, the per-chunk partials and the combine are extend.hip's own (attn_split.h), and the chunk grid is fixed in absolute key positions;
// only the address a staged key is loaded from differs, chosen per key, so a stage may straddle prefix_len[b].  out is therefore
// BIT-IDENTICAL to rv_attn_extend_bf16 with r = prefix_len on the cache materialised as prefix[prefix_row[b], :prefix_len[b]] ++
// tail[b, :n_b], and a row's bits depend on its own sequence only.
//
// rv_token_logprob_rows_f32 turns fp32 logits rows into the log-prob of one given token per row, plus the row's argmax, without writing
// the log-softmax of the row: the statistics (m, L) are log_softmax.h's statements, so the value is the bits rv_log_softmax_rows_f32
// leaves at that column.
// Reference call sites are listed in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "log_softmax.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// a sequence whose prefix_row / prefix_len lie outside the prefix cache is not run: its blocks return before any read, and the combine
// writes zeros for its rows
DEVINL bool xp_valid(int prow, int plen, int P_rows, int P_max) { return prow >= 0 && prow < P_rows && plen >= 0 && plen <= P_max; }

// attn_split.h's MFMA body with each key from its own source, so a stage may straddle prefix_len[b]
template <int HD>
__global__ __launch_bounds__(256) void attn_extend_prefix_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ prefix,
                                                                 long ld_p, long bs_p, const bf16* __restrict__ tail, long ld_t, long bs_t,
                                                                 int v_off, const int* __restrict__ cu_q, const int* __restrict__ prow_,
                                                                 const int* __restrict__ plen_, int P_rows, int P_max, int T_max,
                                                                 float* __restrict__ part, int H, int Hkv, int chunk, int nch, int tiles,
                                                                 float scale) {
    const int b = blockIdx.z / tiles;
    const int q_beg = cu_q[b], n_b = min(cu_q[b + 1] - q_beg, T_max);
    const int prow = prow_[b], r0 = plen_[b];
    if (!xp_valid(prow, r0, P_rows, P_max)) return;
    const bf16* pb = prefix + (long)prow * bs_p + blockIdx.y * HD;     // key j < r0: position j
    const bf16* tb = tail + (long)b * bs_t + blockIdx.y * HD;          // key j >= r0: position j - r0
    // no bound on the keys beyond the causal one: r0 <= P_max and n_b <= T_max keep them inside both caches
    attn_extend_body<HD>(q, ld_q, [=](int j) { return j < r0 ? pb + (long)j * ld_p : tb + (long)(j - r0) * ld_t; }, v_off, q_beg, n_b, r0,
                         0x7fffffff, part, H, Hkv, chunk, nch, tiles, scale);
}

// extend's rows (RowsExtend) at r = prefix_len; the rows of a sequence the attention kernel refused (or past T_max) are zeros
struct RowsExtendPrefix {
    const int *cu_q, *prow_, *plen_;
    int P_rows, P_max, T_max, B;
    DEVINL int operator()(int row, int nch, int chunk) const {
        const int b = xt_seq(cu_q, B, row);
        const int i = row - cu_q[b];
        if (!xp_valid(prow_[b], plen_[b], P_rows, P_max) || i < 0 || i >= T_max) return 0;
        return min((plen_[b] + i) / chunk + 1, nch);
    }
};

// ------------------------------------------------------------------------------------------------ token log-prob of a row
// One workgroup per output row r, which reads row s = src_row ? src_row[r] : r of x: (m, L) by log_softmax.h's statements, then
// logprob[r] = fl(fl(x[s, target[r]] - m) - L), rv_log_softmax_rows_f32's value at that column.  The argmax is a sweep of its own
// (common.h's am_better: NaN ranks highest there and is ignored by the maximum, so the two cannot share one).
__global__ __launch_bounds__(256) void token_logprob_rows_kernel(const float* __restrict__ x, long ld, int x_rows, int n,
                                                                 const int* __restrict__ src_row, const int* __restrict__ target,
                                                                 float* __restrict__ logprob, int64_t* __restrict__ argmax) {
    __shared__ float redm[4];
    __shared__ double reds[4];
    __shared__ float bc[2];
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int s = src_row ? src_row[r] : r;
    if (s < 0 || s >= x_rows) {                      // uniform over the workgroup: no barrier is skipped by part of it
        if (tid == 0) {
            logprob[r] = NAN;
            if (argmax) argmax[r] = -1;
        }
        return;
    }
    const float* row = x + (long)s * ld;
    if (argmax) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < n; j += 256) {
            const float v = row[j];
            if (am_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (am_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane_id() == 0) { rv[wave_id()] = bv; ri[wave_id()] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k)
                if (am_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
            argmax[r] = bi;
        }
    }
    const int t = target[r];
    if (t < 0) {                                     // ignored position (-100): uniform over the workgroup
        if (tid == 0) logprob[r] = 0.f;
        return;
    }
    const float m = ls_row_max(row, n, redm);
    const float L = ls_block_logsum(ls_thread_sum(row, n, m), reds, bc);
    if (tid == 0) logprob[r] = t < n ? (row[t] - m) - L : NAN;
}

}  // namespace

extern "C" int rv_attn_extend_prefix_bf16(const void* q, int64_t ld_q, const void* prefix, int64_t ld_p, int64_t bs_p, int P_rows, int P_max,
                                          const void* tail, int64_t ld_t, int64_t bs_t, int T_max, int v_off, const int32_t* cu_q,
                                          const int32_t* prefix_row, const int32_t* prefix_len, void* out, int64_t ld_o, void* part,
                                          int64_t part_bytes, int B, int M, int max_q, int H, int Hkv, int hd, int chunk, float scale,
                                          void* stream) {
    const int tiles = xt_tiles(B, max_q, H, Hkv);
    const bool ok = cu_q && prefix_row && prefix_len && tiles > 0 && max_q <= M && P_rows > 0 && P_max > 0 && T_max > 0 && max_q <= T_max &&
                    chunk % XT_KT == 0 && split_cache_ok(prefix, ld_p, bs_p, v_off, Hkv, hd, P_max) &&
                    split_cache_ok(tail, ld_t, bs_t, v_off, Hkv, hd, T_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, M, H, Hkv, hd, (int64_t)P_max + T_max, chunk, stream,
                             RowsExtendPrefix{cu_q, prefix_row, prefix_len, P_rows, P_max, T_max, B}, [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_extend_prefix_kernel<hd_c()>, dim3(nch, Hkv, B * tiles), dim3(256), 0, ST, (const bf16*)q,
                                                    (long)ld_q, (const bf16*)prefix, (long)ld_p, (long)bs_p, (const bf16*)tail, (long)ld_t,
                                                    (long)bs_t, v_off, cu_q, prefix_row, prefix_len, P_rows, P_max, T_max, (float*)part, H, Hkv,
                                                    chunk, nch, tiles, scale);
                             });
}

extern "C" int rv_token_logprob_rows_f32(const float* x, int64_t ld, int x_rows, int n, const int32_t* src_row, const int32_t* target,
                                         int rows, float* logprob, int64_t* argmax, void* stream) {
    if (!x || !target || !logprob || x_rows <= 0 || rows <= 0 || n <= 0 || n > 262144 || ld < n) return RV_ERR_ARG;
    hipLaunchKernelGGL(token_logprob_rows_kernel, dim3(rows), dim3(256), 0, ST, x, (long)ld, x_rows, n, src_row, target, logprob, argmax);
    return rv_check_launch();
}

// Decode-time kernels for gfx950: flash-decoding attention of one query row per (sequence, q head) against a KV cache, the cache
// append, and the row argmax of greedy decoding with its logits processors.
// Reductions use a fixed order that depends on the problem shape only (a sequence's own kv_len) -- never on other rows or on
// timing -- and no float atomics: a row's result is bit-identical whatever else shares its launch.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ decode attention
// Block (chunk c, kv head kh, sequence b): keys [c*chunk, min((c+1)*chunk, kv_len[b])) of the sequence's own cache row, through
// attn_split.h's register-q body.  Writes the chunk's partial; attn_split_combine_kernel merges the chunks.
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                          long bs_c, int v_off, const int* __restrict__ kv_len, int L_max, float* __restrict__ part,
                                                          int H, int Hkv, int chunk, float scale) {
    const int c = blockIdx.x, b = blockIdx.z;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int len = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len) return;                     // the combine reads chunks < ceil(len / chunk) only
    const int j1 = min(j0 + chunk, len);
    attn_decode_body<HD>(q, ld_q, cache + (long)b * bs_c, ld_c, v_off, [](int) { return 0L; }, j0, j1, part, H, G, nch, scale);
}

// ------------------------------------------------------------------------------------------------ cache append
// cache[b][pos[b]][0:width] = src[b][0:width]; slots outside [0, L_max) are not written
__global__ void kv_append_kernel(const bf16* __restrict__ src, long ld_src, bf16* __restrict__ cache, long ld_c, long bs_c,
                                 const int* __restrict__ pos, int L_max, int width) {
    const int b = blockIdx.x;
    const int p = pos[b];
    if (p < 0 || p >= L_max) return;
    for (int e = threadIdx.x * 8; e < width; e += blockDim.x * 8)
        *(bf16x8*)(cache + (long)b * bs_c + (long)p * ld_c + e) = *(const bf16x8*)(src + (long)b * ld_src + e);
}

// ------------------------------------------------------------------------------------------------ row argmax
// torch.argmax semantics over the first n columns (common.h's am_better): the lowest index among equal maxima, NaN above everything
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, long ld, int n, int64_t* __restrict__ out) {
    __shared__ float rv[4];
    __shared__ int ri[4];
    const float* row = x + (long)blockIdx.x * ld;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < n; j += 256) {
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
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k)
            if (am_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
        out[blockIdx.x] = bi;
    }
}

// ------------------------------------------------------------------------------------------------ greedy logits processors + argmax
// HF's greedy logits processors (repetition penalty, no-repeat n-gram, bad words, min length / min new tokens, suppress, begin-suppress)
// fused with the row argmax above.  One workgroup per row.  Phase 1 walks the row's generated tokens h[0..t) and sets two LDS bitmaps
// with LDS atomicOr: `pen` (one bit per distinct history token: the penalty lands once per token, as HF's gather -> scatter does) and
// `ban` (n-gram continuations, bad-word continuations whose prefix ends h, the host-composed static list).  Phase 2 reads the row once,
// applies x < 0 ? x * p : x / p on `pen` bits (IEEE fp32 division: no reciprocal) and then -inf on `ban` bits, writes back only the
// touched entries and feeds the fixed-order argmax.  Ids outside [0, n) set no bit.  The bitmaps are dynamic LDS, n / 4 bytes.
// One difference from HF: HF adds -inf for a bad word (so +inf / NaN become NaN), here a bad word sets -inf like every other ban.
constexpr int LP_MAX_N = 262144;                // 2 x 32 KB of bitmap: Qwen2's 152,064 plus resize_token_embeddings growth
constexpr int LP_U = 8;

DEVINL void lp_set(unsigned* bm, int tok, int n) {
    if (tok >= 0 && tok < n) atomicOr(&bm[tok >> 5], 1u << (tok & 31));
}

__global__ __launch_bounds__(256) void logits_process_argmax_kernel(float* __restrict__ x, long ld, int n, const int32_t* __restrict__ hist,
                                                                    long ld_hist, int t, float pen_p, int ngram, const int32_t* __restrict__ ban,
                                                                    int n_ban, const int32_t* __restrict__ bad_tok,
                                                                    const int32_t* __restrict__ bad_off, int n_bad, int64_t* __restrict__ out) {
    extern __shared__ unsigned lp_bits[];
    const int words = (n + 31) >> 5;
    unsigned* pen = lp_bits;
    unsigned* bnd = lp_bits + words;
    float* row = x + (long)blockIdx.x * ld;
    const int32_t* h = hist + (long)blockIdx.x * ld_hist;
    const int tid = threadIdx.x;
    for (int w = tid; w < 2 * words; w += 256) lp_bits[w] = 0u;
    __syncthreads();
    if (pen_p != 1.0f)
        for (int i = tid; i < t; i += 256) lp_set(pen, h[i], n);
    if (ngram > 0 && t >= ngram) {
        // window i (i <= t - ngram) bans its last token when its first ngram - 1 tokens equal the last ngram - 1 generated ones
        for (int i = tid; i <= t - ngram; i += 256) {
            bool eq = true;
            for (int k = 0; k < ngram - 1 && eq; ++k) eq = h[i + k] == h[t - ngram + 1 + k];
            if (eq) lp_set(bnd, h[i + ngram - 1], n);
        }
    }
    for (int j = tid; j < n_ban; j += 256) lp_set(bnd, ban[j], n);
    for (int s = tid; s < n_bad; s += 256) {
        const int o = bad_off[s], L = bad_off[s + 1] - o;
        if (L < 2 || t < L) continue;            // HF skips a sequence longer than the generated tokens (t >= L, not L - 1)
        bool eq = true;
        for (int k = 0; k < L - 1 && eq; ++k) eq = bad_tok[o + k] == h[t - L + 1 + k];
        if (eq) lp_set(bnd, bad_tok[o + L - 1], n);
    }
    __syncthreads();
    // LP_U independent loads in flight per thread: one workgroup streams the whole row, so the sweep is latency-bound without them
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j0 = tid; j0 < n; j0 += 256 * LP_U) {
        float vs[LP_U];
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
            const int j = j0 + u * 256;
            vs[u] = j < n ? row[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
            const int j = j0 + u * 256;
            if (j >= n) break;
            float v = vs[u];
            const unsigned m = 1u << (j & 31);
            const bool pj = pen[j >> 5] & m, bj = bnd[j >> 5] & m;
            if (pj) v = v < 0.f ? v * pen_p : v / pen_p;
            if (bj) v = -INFINITY;
            if (pj || bj) row[j] = v;
            if (am_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (am_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    __syncthreads();                             // every bitmap read is done: the reduction scratch reuses the bitmap's first words
    float* rv = (float*)lp_bits;
    int* ri = (int*)(lp_bits + 4);
    if (lane_id() == 0) { rv[wave_id()] = bv; ri[wave_id()] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k)
            if (am_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
        out[blockIdx.x] = bi;
    }
}

// The same processors for rows that sit at different steps (continuous batching): row r has its own step t[r] and EOS minimum
// min_new[r], and its history is hist[slot[r], 0 .. t[r]), so a history row stays with its KV-cache slot.  The ban lists come apart:
// `always` (suppress_tokens, one-token bad words), `begin` (t[r] == 0) and `eos` (t[r] < min_new[r]); each row composes its own.
// The phases are those of logits_process_argmax_kernel, so at equal t the processed row and token are the same bits.  LOGP: the same
// sweep also keeps a running (max, sum of exp(x - max)) per thread -- per batch of LP_U loads: the batch maximum, one rescale, then
// LP_U independent exponentials summed in order, so no exp waits on the previous one -- merged in a fixed order (lanes by xor
// butterfly, then waves 0..3), and logprob[r] = (x[tok] - max) - log(sum): the log-softmax of the processed row at the chosen token,
// the row read once.
DEVINL void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    if (M == -INFINITY) return;                  // both empty
    s = s * expf(m - M) + os * expf(om - M);
    m = M;
}

template <bool LOGP>
__global__ __launch_bounds__(256) void logits_process_argmax_rows_kernel(
    float* __restrict__ x, long ld, int n, const int32_t* __restrict__ hist, long ld_hist, int hist_rows, int hist_cols,
    const int32_t* __restrict__ slot, const int32_t* __restrict__ tv, const int32_t* __restrict__ min_new, float pen_p, int ngram,
    const int32_t* __restrict__ ban_a, int n_a, const int32_t* __restrict__ ban_b, int n_b, const int32_t* __restrict__ ban_e, int n_e,
    const int32_t* __restrict__ bad_tok, const int32_t* __restrict__ bad_off, int n_bad, int64_t* __restrict__ out,
    float* __restrict__ logprob) {
    extern __shared__ unsigned lp_bits[];
    const int words = (n + 31) >> 5;
    unsigned* pen = lp_bits;
    unsigned* bnd = lp_bits + words;
    float* row = x + (long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    const int t = tv[blockIdx.x], s = slot[blockIdx.x];
    // history reads stay inside hist[0 .. hist_rows) x [0 .. hist_cols) whatever the caller passed: a slot out of range reads none
    const int th = (hist && s >= 0 && s < hist_rows) ? min(max(t, 0), hist_cols) : 0;
    const int32_t* h = th > 0 ? hist + (long)s * ld_hist : nullptr;
    for (int w = tid; w < 2 * words; w += 256) lp_bits[w] = 0u;
    __syncthreads();
    if (pen_p != 1.0f)
        for (int i = tid; i < th; i += 256) lp_set(pen, h[i], n);
    if (ngram > 0 && th >= ngram) {
        for (int i = tid; i <= th - ngram; i += 256) {
            bool eq = true;
            for (int k = 0; k < ngram - 1 && eq; ++k) eq = h[i + k] == h[th - ngram + 1 + k];
            if (eq) lp_set(bnd, h[i + ngram - 1], n);
        }
    }
    for (int j = tid; j < n_a; j += 256) lp_set(bnd, ban_a[j], n);
    if (t == 0)
        for (int j = tid; j < n_b; j += 256) lp_set(bnd, ban_b[j], n);
    if (t < min_new[blockIdx.x])
        for (int j = tid; j < n_e; j += 256) lp_set(bnd, ban_e[j], n);
    for (int q = tid; q < n_bad; q += 256) {
        const int o = bad_off[q], L = bad_off[q + 1] - o;
        if (L < 2 || th < L) continue;
        bool eq = true;
        for (int k = 0; k < L - 1 && eq; ++k) eq = bad_tok[o + k] == h[th - L + 1 + k];
        if (eq) lp_set(bnd, bad_tok[o + L - 1], n);
    }
    __syncthreads();
    float bv = -INFINITY, lm = -INFINITY, ls = 0.f;
    int bi = 0x7fffffff;
    for (int j0 = tid; j0 < n; j0 += 256 * LP_U) {
        float vs[LP_U];
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
            const int j = j0 + u * 256;
            vs[u] = j < n ? row[j] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
            const int j = j0 + u * 256;
            if (j >= n) break;
            float v = vs[u];
            const unsigned m = 1u << (j & 31);
            const bool pj = pen[j >> 5] & m, bj = bnd[j >> 5] & m;
            if (pj) v = v < 0.f ? v * pen_p : v / pen_p;
            if (bj) v = -INFINITY;
            if (pj || bj) row[j] = v;
            if (am_better(v, j, bv, bi)) { bv = v; bi = j; }
            vs[u] = v;
        }
        if (LOGP) {
            float mb = lm;
#pragma unroll
            for (int u = 0; u < LP_U; ++u) mb = fmaxf(mb, vs[u]);
            if (mb != -INFINITY) {
                float acc = 0.f;
#pragma unroll
                for (int u = 0; u < LP_U; ++u) acc += __expf(vs[u] - mb);
                ls = ls * __expf(lm - mb) + acc;
                lm = mb;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (am_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        if (LOGP) {
            const float om = __shfl_xor(lm, o, 64), os = __shfl_xor(ls, o, 64);
            lse_merge(lm, ls, om, os);
        }
    }
    __syncthreads();                             // every bitmap read is done: the reduction scratch reuses the bitmap's first words
    float* rv = (float*)lp_bits;
    int* ri = (int*)(lp_bits + 4);
    float* rm = (float*)(lp_bits + 8);
    float* rs = (float*)(lp_bits + 12);
    if (lane_id() == 0) {
        rv[wave_id()] = bv;
        ri[wave_id()] = bi;
        if (LOGP) { rm[wave_id()] = lm; rs[wave_id()] = ls; }
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            if (am_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
            if (LOGP) lse_merge(lm, ls, rm[k], rs[k]);
        }
        out[blockIdx.x] = bi;
        if (LOGP) logprob[blockIdx.x] = (bv - lm) - logf(ls);
    }
}

}  // namespace

extern "C" int rv_attn_decode_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len,
                                   int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk,
                                   float scale, void* stream) {
    return attn_split_launch(kv_len && ad_chunk_ok(chunk, hd) && split_cache_ok(cache, ld_c, bs_c, v_off, Hkv, hd, L_max), q, ld_q, out, ld_o,
                             part, part_bytes, B, H, Hkv, hd, L_max, chunk, stream, RowsKvLen{kv_len, L_max}, [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_decode_kernel<hd_c()>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q,
                                                    (const bf16*)cache, (long)ld_c, (long)bs_c, v_off, kv_len, L_max, (float*)part, H, Hkv, chunk,
                                                    scale);
                             });
}

extern "C" int rv_kv_append_bf16(const void* src, int64_t ld_src, void* cache, int64_t ld_c, int64_t bs_c, const int32_t* pos, int L_max, int B,
                                 int width, void* stream) {
    if (!src || !cache || !pos || B <= 0 || width <= 0 || (width & 7) || (ld_src & 7) || (ld_c & 7) || (bs_c & 7) || ld_src < width ||
        ld_c < width || bs_c < (int64_t)L_max * ld_c)
        return RV_ERR_ARG;
    hipLaunchKernelGGL(kv_append_kernel, dim3(B), dim3(256), 0, ST, (const bf16*)src, (long)ld_src, (bf16*)cache, (long)ld_c, (long)bs_c, pos,
                       L_max, width);
    return rv_check_launch();
}

extern "C" int rv_argmax_rows_f32(const float* x, int64_t ld, int rows, int n, int64_t* out, void* stream) {
    if (!x || !out || rows <= 0 || n <= 0 || ld < n) return RV_ERR_ARG;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3(rows), dim3(256), 0, ST, x, (long)ld, n, out);
    return rv_check_launch();
}

extern "C" int rv_logits_process_argmax_f32(float* x, int64_t ld, int rows, int n, const int32_t* hist, int64_t ld_hist, int t, float rep_penalty,
                                            int ngram, const int32_t* ban, int n_ban, const int32_t* bad_tok, const int32_t* bad_off, int n_bad,
                                            int64_t* out, void* stream) {
    if (!x || !out || rows <= 0 || n <= 0 || n > LP_MAX_N || ld < n || t < 0 || (t > 0 && (!hist || ld_hist < t)) || !(rep_penalty > 0.f) ||
        ngram < 0 || n_ban < 0 || (n_ban > 0 && !ban) || n_bad < 0 || (n_bad > 0 && (!bad_tok || !bad_off)))
        return RV_ERR_ARG;
    const size_t lds = (size_t)2 * ((n + 31) / 32) * sizeof(unsigned);     // >= 32 bytes (the reduction scratch) for every n >= 1
    hipLaunchKernelGGL(logits_process_argmax_kernel, dim3(rows), dim3(256), lds < 32 ? 32 : lds, ST, x, (long)ld, n, hist, (long)ld_hist, t,
                       rep_penalty, ngram, ban, n_ban, bad_tok, bad_off, n_bad, out);
    return rv_check_launch();
}

extern "C" int rv_logits_process_argmax_rows_f32(float* x, int64_t ld, int rows, int n, const int32_t* hist, int64_t ld_hist, int hist_rows,
                                                 int hist_cols, const int32_t* slot, const int32_t* t, const int32_t* min_new,
                                                 float rep_penalty, int ngram, const int32_t* ban_always, int n_always,
                                                 const int32_t* ban_begin, int n_begin, const int32_t* ban_eos, int n_eos,
                                                 const int32_t* bad_tok, const int32_t* bad_off, int n_bad, int64_t* out, float* logprob,
                                                 void* stream) {
    if (!x || !out || !slot || !t || !min_new || rows <= 0 || n <= 0 || n > LP_MAX_N || ld < n || hist_rows < 0 || hist_cols < 0 ||
        (hist_rows > 0 && hist_cols > 0 && (!hist || ld_hist < hist_cols)) || !(rep_penalty > 0.f) || ngram < 0 || n_always < 0 ||
        (n_always > 0 && !ban_always) || n_begin < 0 || (n_begin > 0 && !ban_begin) || n_eos < 0 || (n_eos > 0 && !ban_eos) ||
        n_bad < 0 || (n_bad > 0 && (!bad_tok || !bad_off)))
        return RV_ERR_ARG;
    if (hist_rows == 0 || hist_cols == 0) hist = nullptr;
    const size_t lds = (size_t)2 * ((n + 31) / 32) * sizeof(unsigned);     // the reduction scratch needs 64 bytes
    if (logprob)
        hipLaunchKernelGGL(logits_process_argmax_rows_kernel<true>, dim3(rows), dim3(256), lds < 64 ? 64 : lds, ST, x, (long)ld, n, hist,
                           (long)ld_hist, hist_rows, hist_cols, slot, t, min_new, rep_penalty, ngram, ban_always, n_always, ban_begin,
                           n_begin, ban_eos, n_eos, bad_tok, bad_off, n_bad, out, logprob);
    else
        hipLaunchKernelGGL(logits_process_argmax_rows_kernel<false>, dim3(rows), dim3(256), lds < 64 ? 64 : lds, ST, x, (long)ld, n, hist,
                           (long)ld_hist, hist_rows, hist_cols, slot, t, min_new, rep_penalty, ngram, ban_always, n_always, ban_begin,
                           n_begin, ban_eos, n_eos, bad_tok, bad_off, n_bad, out, logprob);
    return rv_check_launch();
}

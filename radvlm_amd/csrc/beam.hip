// Beam-search kernels for gfx950: decode attention that follows a beam's ancestry through the KV cache instead of reordering it, the
// in-place fp32 log-softmax of the score rows, and the top-K over the num_beams * vocab candidates of each prompt.
// As in decode.hip every reduction runs in a fixed order that depends on the problem shape only and there are no global or float
// atomics: a row's (a prompt's) result is bit-identical whatever else shares the launch.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "log_softmax.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ beam decode attention
// decode.hip's attn_decode_kernel with one change: key position j of query row b is read from cache row src(b, j) instead of row b,
//   src(b, j) = j < prefix_len[b] ? prefix_row[b] : tail_src[b][j - prefix_len[b]],   clamped into [0, cache_rows).
// The chunk's source rows are resolved once into LDS (one coalesced int32 read of the table per chunk; a chunk inside the prefix reads
// no table at all), so the K and V loads stay what they are there: LPR lanes read one 16-byte slice each of a key row, and the lookup
// only changes the row base the slices hang from.  Scores, chunk statistics, P V and the combine are that kernel's own -- both run
// attn_split.h's attn_decode_body -- which is what makes the output bit-identical to it on the gathered cache.
template <int HD>
__global__ __launch_bounds__(256) void attn_decode_beam_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                               long bs_c, int v_off, const int* __restrict__ kv_len, int L_max,
                                                               const int* __restrict__ prefix_row, const int* __restrict__ prefix_len,
                                                               const int* __restrict__ tail_src, long ld_t, int tail_cols, int cache_rows,
                                                               float* __restrict__ part, int H, int Hkv, int chunk, float scale) {
    __shared__ int srow[AD_CHUNK_MAX];
    const int c = blockIdx.x, b = blockIdx.z;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int len = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len) return;                     // the combine reads chunks < ceil(len / chunk) only
    const int j1 = min(j0 + chunk, len), n = j1 - j0;
    // source rows of the chunk's keys; an entry past tail_cols cannot be looked up and falls back to the prefix row
    {
        const int plen = max(prefix_len[b], 0);
        const int prow = min(max(prefix_row[b], 0), cache_rows - 1);
        for (int jj = threadIdx.x; jj < n; jj += 256) {
            const int tpos = j0 + jj - plen;
            int r = prow;
            if (tpos >= 0 && tpos < tail_cols) r = min(max(tail_src[(long)b * ld_t + tpos], 0), cache_rows - 1);
            srow[jj] = r;
        }
    }
    __syncthreads();
    attn_decode_body<HD>(q, ld_q, cache, ld_c, v_off, [&](int jj) { return (long)srow[jj] * bs_c; }, j0, j1, part, H, G, nch, scale);
}

// ------------------------------------------------------------------------------------------------ row log-softmax
// In place on the first n columns of fp32 row r: x_i <- fl(fl(x_i - m) - L), m = max x, L = fl32(log(S)), S = sum exp(x_i - m).
// One workgroup per row, three sweeps (the second and third hit the cache): the maximum (exact, order-free); the sum, every term
// __expf(fl(x_i - m)) widened to fp64 and added per thread in index order, then lanes by xor butterfly, then waves 0..3 -- a fixed
// order, so a row's bits depend on the row alone; the write.  L is computed once (thread 0, fp64 log) and broadcast through LDS.
//
// Error against exact arithmetic on the fp32 inputs, u = 2^-24, for a row of finite entries (-inf entries stay -inf exactly):
//   d_i = fl(x_i - m) is within u |d_i| of x_i - m, which moves exp by a relative u |d_i|;
//   __expf(d) = v_exp_f32(fl(d * log2(e))): the rounded product and the rounded constant shift the exponent by at most 1.5 u |d| (in
//     base e), the instruction itself is good to 1 ulp = 2 u; results below 2^-126 flush to 0, an absolute 2^-126 each;
//   so term i carries a relative error of at most (3 |d_i| + 3) u, second-order terms included;
//   the fp64 sum of <= 262144 fp32 terms adds a relative 2^-35, nothing beside u;
//   S >= 1 (the maximum's own term is exactly 1), and with p = softmax(x): sum p_i |d_i| = H(p) - ln S <= ln n, so S carries a relative
//     error of at most (3 ln n + 3) u, which is the absolute error of ln S; rounding it to fp32 adds u |L|, and |L| <= ln n;
//   the last subtraction rounds once more: u |out_i|; and |d_i| <= |out_i| because L >= 0.
// Together |out_i - exact_i| <= u (2 |out_i| + 4 ln n + 3): 3.2e-6 + 1.2e-7 |out_i| at n = 262144.  It stays under the 1e-5 the
// logprobs of generate_batch are tested to while |out_i| <= 57; a log-prob further down than that is resolved to 2 ulp of itself.
// The statistics (m, L) are the device functions of log_softmax.h, which rv_cfg_guide_rows_f32 (cfg.hip) shares to get the same bits.
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(float* __restrict__ x, long ld, int n) {
    __shared__ float redm[4];
    __shared__ double reds[4];
    __shared__ float bc[2];
    float* row = x + (long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    const float m = ls_row_max(row, n, redm);
    const float L = ls_block_logsum(ls_thread_sum(row, n, m), reds, bc);
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vs[LS_U];
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
            const int j = j0 + u * 256;
            vs[u] = j < n ? row[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
            const int j = j0 + u * 256;
            if (j < n) row[j] = (vs[u] - m) - L;
        }
    }
}

// ------------------------------------------------------------------------------------------------ grouped top-K
// Candidates of group g: v(r, i) = fl(x[g * nb + r][i] + score[g * nb + r]) at flat index r * n + i.  The order is total: NaN first,
// then the larger value, then the lower flat index (rv_argmax_rows_f32's rule extended by the index), so "the K best" is one list.
// Stage 1: a workgroup holds a fixed slice of TK_SLICE consecutive flat indices in registers and selects its K best by K rounds of a
// block argmax over "what ranks after the previous winner"; it writes them, best first, to scratch.  Stage 2: one workgroup per group
// runs the same K rounds over the nblk * K survivors.  A slice with fewer than K candidates pads with sentinels that rank after every
// real candidate.  No sort of a row and no atomics; the result is a function of the group's values only.
constexpr int TK_PER = 16;
constexpr int TK_SLICE = 256 * TK_PER;
constexpr int TK_NONE = 0x7fffffff;

// best of the workgroup's candidates (bv, bi), known to every thread on return; `rv`/`ri` are 2 x 4 LDS words, `par` flips per call
DEVINL void tk_block_best(float& bv, int& bi, float (*rv)[4], int (*ri)[4], int par) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (am_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane_id() == 0) { rv[par][wave_id()] = bv; ri[par][wave_id()] = bi; }
    __syncthreads();
    bv = rv[par][0];
    bi = ri[par][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (am_better(rv[par][k], ri[par][k], bv, bi)) { bv = rv[par][k]; bi = ri[par][k]; }
}

__global__ __launch_bounds__(256) void beam_topk_slices_kernel(const float* __restrict__ x, long ld, int n, int nb,
                                                               const float* __restrict__ score, int K, float* __restrict__ sv,
                                                               int* __restrict__ si) {
    __shared__ float rv[2][4];
    __shared__ int ri[2][4];
    const int blk = blockIdx.x, g = blockIdx.y, nblk = gridDim.x;
    const long total = (long)nb * n;
    float v[TK_PER];
    int id[TK_PER];
#pragma unroll
    for (int e = 0; e < TK_PER; ++e) {
        const long f = (long)blk * TK_SLICE + e * 256 + threadIdx.x;
        v[e] = -INFINITY;
        id[e] = TK_NONE;
        if (f < total) {
            const int r = (int)(f / n), i = (int)(f - (long)r * n);
            v[e] = x[((long)g * nb + r) * ld + i] + score[g * nb + r];
            id[e] = (int)f;
        }
    }
    float pv = 0.f;
    int pi = -1;                                 // nothing selected yet: every candidate is eligible
    float* ov = sv + ((long)g * nblk + blk) * K;
    int* oi = si + ((long)g * nblk + blk) * K;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = TK_NONE;
#pragma unroll
        for (int e = 0; e < TK_PER; ++e) {
            const bool after = pi < 0 || am_better(pv, pi, v[e], id[e]);
            if (after && am_better(v[e], id[e], bv, bi)) { bv = v[e]; bi = id[e]; }
        }
        tk_block_best(bv, bi, rv, ri, k & 1);
        if (threadIdx.x == 0) { ov[k] = bv; oi[k] = bi; }
        pv = bv;
        pi = bi;
        if (bi == TK_NONE) {                     // the slice is exhausted: the rest are sentinels too
            for (int kk = k + 1 + threadIdx.x; kk < K; kk += 256) { ov[kk] = -INFINITY; oi[kk] = TK_NONE; }
            break;
        }
    }
}

__global__ __launch_bounds__(256) void beam_topk_merge_kernel(const float* __restrict__ sv, const int* __restrict__ si, int cand, int K,
                                                              float* __restrict__ out_v, int* __restrict__ out_i) {
    __shared__ float rv[2][4];
    __shared__ int ri[2][4];
    const int g = blockIdx.x;
    const float* cv = sv + (long)g * cand;
    const int* ci = si + (long)g * cand;
    float pv = 0.f;
    int pi = -1;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = TK_NONE;
        for (int e = threadIdx.x; e < cand; e += 256) {
            const float v = cv[e];
            const int i = ci[e];
            const bool after = pi < 0 || am_better(pv, pi, v, i);
            if (after && am_better(v, i, bv, bi)) { bv = v; bi = i; }
        }
        tk_block_best(bv, bi, rv, ri, k & 1);
        if (threadIdx.x == 0) { out_v[(long)g * K + k] = bv; out_i[(long)g * K + k] = bi; }
        pv = bv;
        pi = bi;
    }
}

}  // namespace

extern "C" int rv_attn_decode_beam_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off,
                                        const int32_t* kv_len, int L_max, const int32_t* prefix_row, const int32_t* prefix_len,
                                        const int32_t* tail_src, int64_t ld_t, int tail_cols, int cache_rows, void* out, int64_t ld_o,
                                        void* part, int64_t part_bytes, int rows, int H, int Hkv, int hd, int chunk, float scale,
                                        void* stream) {
    const bool ok = kv_len && prefix_row && prefix_len && cache_rows > 0 && tail_cols >= 0 && (tail_cols == 0 || (tail_src && ld_t >= tail_cols)) &&
                    ad_chunk_ok(chunk, hd) && split_cache_ok(cache, ld_c, bs_c, v_off, Hkv, hd, L_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, rows, H, Hkv, hd, L_max, chunk, stream, RowsKvLen{kv_len, L_max},
                             [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_decode_beam_kernel<hd_c()>, dim3(nch, Hkv, rows), dim3(256), 0, ST, (const bf16*)q,
                                                    (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c, v_off, kv_len, L_max, prefix_row,
                                                    prefix_len, tail_src, (long)ld_t, tail_cols, cache_rows, (float*)part, H, Hkv, chunk, scale);
                             });
}

extern "C" int rv_log_softmax_rows_f32(float* x, int64_t ld, int rows, int n, void* stream) {
    if (!x || rows <= 0 || n <= 0 || n > 262144 || ld < n) return RV_ERR_ARG;
    hipLaunchKernelGGL(log_softmax_rows_kernel, dim3(rows), dim3(256), 0, ST, x, (long)ld, n);
    return rv_check_launch();
}

extern "C" int64_t rv_beam_topk_ws_bytes(int groups, int nb, int n, int K) {
    if (groups <= 0 || nb <= 0 || n <= 0 || K <= 0) return 0;
    return (int64_t)groups * cdiv((long)nb * n, TK_SLICE) * K * 8;
}

extern "C" int rv_beam_topk_f32(const float* x, int64_t ld, int groups, int nb, int n, const float* score, int K, float* out_v,
                                int32_t* out_i, void* ws, int64_t ws_bytes, void* stream) {
    if (!x || !score || !out_v || !out_i || !ws || groups <= 0 || nb < 1 || nb > 16 || n <= 0 || n > 262144 || ld < n || K < 1 || K > 64 ||
        K > (long)nb * n || ws_bytes < rv_beam_topk_ws_bytes(groups, nb, n, K))
        return RV_ERR_ARG;
    const int nblk = (int)cdiv((long)nb * n, TK_SLICE);
    float* sv = (float*)ws;
    int* si = (int*)ws + (long)groups * nblk * K;
    hipLaunchKernelGGL(beam_topk_slices_kernel, dim3(nblk, groups), dim3(256), 0, ST, x, (long)ld, n, nb, score, K, sv, si);
    hipLaunchKernelGGL(beam_topk_merge_kernel, dim3(groups), dim3(256), 0, ST, (const float*)sv, (const int*)si, nblk * K, K, out_v, out_i);
    return rv_check_launch();
}

// Beam-search kernels for gfx950: decode attention that follows a beam's ancestry through the KV cache instead of reordering it, the
// in-place fp32 log-softmax of the score rows, and the top-K over the num_beams * vocab candidates of each prompt.
// As in decode.hip every reduction runs in a fixed order that depends on the problem shape only and there are no global or float
// atomics: a row's (a prompt's) result is bit-identical whatever else shares the launch.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
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
// only changes the row base the slices hang from.  Scores, chunk statistics, P V and the combine are that kernel's statement for
// statement, which is what makes the output bit-identical to it on the gathered cache.
constexpr int AD_GMAX = 8;
constexpr int AD_CHUNK_MAX = 512;

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_beam_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                               long bs_c, int v_off, const int* __restrict__ kv_len, int L_max,
                                                               const int* __restrict__ prefix_row, const int* __restrict__ prefix_len,
                                                               const int* __restrict__ tail_src, long ld_t, int tail_cols, int cache_rows,
                                                               float* __restrict__ part, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    __shared__ float sc[AD_GMAX][AD_CHUNK_MAX];
    __shared__ float ored[4][AD_GMAX][HD];
    __shared__ float mstat[AD_GMAX];
    __shared__ int srow[AD_CHUNK_MAX];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int len = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len) return;                     // the combine reads chunks < ceil(len / chunk) only
    const int j1 = min(j0 + chunk, len), n = j1 - j0;
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
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
    const bf16* kbase = cache + kh * HD + li * 8;
    const bf16* vbase = kbase + v_off;
    float qv[AD_GMAX][8];
#pragma unroll
    for (int g = 0; g < AD_GMAX; ++g) {
        if (g < G) {
            const bf16x8 t = *(const bf16x8*)(q + (long)b * ld_q + (kh * G + g) * HD + li * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) qv[g][i] = bf2f(t[i]);
        }
    }
    // scores
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        const bool ok = j < j1;
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)srow[j - j0] * bs_c + (long)j * ld_c) : zero8();
#pragma unroll
        for (int g = 0; g < AD_GMAX; ++g) {
            if (g < G) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d += qv[g][i] * bf2f(kt[i]);
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
                if (ok && li == 0) sc[g][j - j0] = d * scale;
            }
        }
    }
    __syncthreads();
    // chunk softmax statistics: wave w owns heads w and w + 4
    for (int g = w; g < G; g += 4) {
        float m = -INFINITY;
        for (int j = lane; j < n; j += 64) m = fmaxf(m, sc[g][j]);
        m = wave_max(m);
        float l = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float p = expf(sc[g][j] - m);
            sc[g][j] = p;
            l += p;
        }
        l = wave_sum(l);
        if (lane == 0) {
            mstat[g] = m;
            float* pp = part + (((long)b * H + kh * G + g) * nch + c) * (HD + 2);
            pp[HD] = m;
            pp[HD + 1] = l;
        }
    }
    __syncthreads();
    // P V
    float acc[AD_GMAX][8];
#pragma unroll
    for (int g = 0; g < AD_GMAX; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[g][i] = 0.f;
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        if (j < j1) {
            const bf16x8 vt = *(const bf16x8*)(vbase + (long)srow[j - j0] * bs_c + (long)j * ld_c);
#pragma unroll
            for (int g = 0; g < AD_GMAX; ++g) {
                if (g < G) {
                    const float p = sc[g][j - j0];
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[g][i] += p * bf2f(vt[i]);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < AD_GMAX; ++g) {
        if (g < G) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a = acc[g][i];
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
                if (lr == 0) ored[w][g][li * 8 + i] = a;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < G * HD; idx += 256) {
        const int g = idx / HD, dd = idx % HD;
        float o = ored[0][g][dd];
        o += ored[1][g][dd];
        o += ored[2][g][dd];
        o += ored[3][g][dd];
        part[(((long)b * H + kh * G + g) * nch + c) * (HD + 2) + dd] = o;
    }
}

// decode.hip's attn_decode_combine_kernel: one block of HD threads per (row, q head), chunks merged in chunk order
template <int HD>
__global__ __launch_bounds__(HD) void attn_decode_beam_combine_kernel(const float* __restrict__ part, const int* __restrict__ kv_len, int L_max,
                                                                      bf16* __restrict__ out, long ld_o, int H, int nch, int chunk) {
    const int bh = blockIdx.x, b = bh / H, h = bh % H, dd = threadIdx.x;
    const int len = min(kv_len[b], L_max);
    const int nc = min((len + chunk - 1) / chunk, nch);
    const float* pp = part + (long)bh * nch * (HD + 2);
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, pp[c * (HD + 2) + HD]);
    float L = 0.f, o = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float e = expf(pp[c * (HD + 2) + HD] - M);
        L += pp[c * (HD + 2) + HD + 1] * e;
        o += pp[c * (HD + 2) + dd] * e;
    }
    out[(long)b * ld_o + h * HD + dd] = f2bf(nc > 0 ? o / L : 0.f);
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

DEVINL bool tk_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// best of the workgroup's candidates (bv, bi), known to every thread on return; `rv`/`ri` are 2 x 4 LDS words, `par` flips per call
DEVINL void tk_block_best(float& bv, int& bi, float (*rv)[4], int (*ri)[4], int par) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane_id() == 0) { rv[par][wave_id()] = bv; ri[par][wave_id()] = bi; }
    __syncthreads();
    bv = rv[par][0];
    bi = ri[par][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (tk_better(rv[par][k], ri[par][k], bv, bi)) { bv = rv[par][k]; bi = ri[par][k]; }
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
            const bool after = pi < 0 || tk_better(pv, pi, v[e], id[e]);
            if (after && tk_better(v[e], id[e], bv, bi)) { bv = v[e]; bi = id[e]; }
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
            const bool after = pi < 0 || tk_better(pv, pi, v, i);
            if (after && tk_better(v, i, bv, bi)) { bv = v; bi = i; }
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
    if (!q || !cache || !kv_len || !prefix_row || !prefix_len || !out || !part || rows <= 0 || cache_rows <= 0 || Hkv <= 0 || H % Hkv ||
        H / Hkv > AD_GMAX || (hd != 64 && hd != 128) || L_max <= 0 || chunk <= 0 || chunk > AD_CHUNK_MAX || chunk % (hd == 128 ? 16 : 32) ||
        (ld_q & 7) || (ld_c & 7) || (bs_c & 7) || (v_off & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd ||
        ld_c < v_off + (int64_t)Hkv * hd || bs_c < (int64_t)L_max * ld_c || tail_cols < 0 || (tail_cols > 0 && (!tail_src || ld_t < tail_cols)))
        return RV_ERR_ARG;
    const int nch = (L_max + chunk - 1) / chunk;
    if (part_bytes < (int64_t)rows * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const dim3 grid(nch, Hkv, rows);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_decode_beam_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len, L_max, prefix_row, prefix_len, tail_src, (long)ld_t, tail_cols, cache_rows, (float*)part, H,
                           Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_beam_combine_kernel<128>, dim3(rows * H), dim3(128), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_decode_beam_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len, L_max, prefix_row, prefix_len, tail_src, (long)ld_t, tail_cols, cache_rows, (float*)part, H,
                           Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_beam_combine_kernel<64>, dim3(rows * H), dim3(64), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    }
    return rv_check_launch();
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

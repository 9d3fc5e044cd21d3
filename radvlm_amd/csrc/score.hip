// Scoring candidate answers for gfx950 (model.score(), LlavaEngine.score_tails): the log-likelihood of token sequences the caller
// already has, after a prompt that many candidates share.
//
// rv_attn_extend_prefix_bf16 is extend.hip's attention with two key sources.  Query i of sequence b sits at position prefix_len[b] + i
// and sees the keys [0, prefix_len[b] + i]: key j < prefix_len[b] is position j of row prefix_row[b] of a prefix cache (the prompt,
// prefilled once, read in place by every candidate that continues it), key j >= prefix_len[b] is position j - prefix_len[b] of row b of
// a tail cache (the candidate's own rows, already written).  The work split, the 64-key LDS stages, the MFMA operand layouts, the online
// softmax, the per-chunk partials and the combine are extend.hip's statements, and the chunk grid is fixed in absolute key positions;
// only the address a staged key is loaded from differs, chosen per key, so a stage may straddle prefix_len[b].  out is therefore
// BIT-IDENTICAL to rv_attn_extend_bf16 with r = prefix_len on the cache materialised as prefix[prefix_row[b], :prefix_len[b]] ++
// tail[b, :n_b], and a row's bits depend on its own sequence only.
//
// rv_token_logprob_rows_f32 turns fp32 logits rows into the log-prob of one given token per row, plus the row's argmax, without writing
// the log-softmax of the row: the statistics (m, L) are log_softmax.h's statements, so the value is the bits rv_log_softmax_rows_f32
// leaves at that column.
// Reference call sites are listed in include/radvlm_hip.h.
#include "common.h"
#include "log_softmax.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

constexpr int XT_KT = 64;        // keys per LDS stage
constexpr int XT_GMAX = 8;       // query heads per kv head
constexpr int XT_MAXRT = 2;      // 16-row MFMA row tiles per wave (row tiles per block <= 8, 4 waves)
constexpr int XT_KPAD = 8;       // LDS row padding (bf16 elements)

// query sub-tiles of 16 rows per block: enough (query, head) row tiles for the 4 waves, at most 8 (a function of G alone)
DEVINL __host__ int xt_qs(int G) { return G >= 4 ? 1 : 4 / G; }

// a sequence whose prefix_row / prefix_len lie outside the prefix cache is not run: its blocks return before any read, and the combine
// writes zeros for its rows
DEVINL bool xp_valid(int prow, int plen, int P_rows, int P_max) { return prow >= 0 && prow < P_rows && plen >= 0 && plen <= P_max; }

// MFMA 16x16x32 (common.h): S = Q K^T with A = Q rows (lane l: row l&15, dims 8(l>>4)..+7 of k-step kk) and B = K^T (lane l: key l&15,
// same dims); P V with A = P (lane l: row l&15, keys 8(l>>4)..+7 of the 32-key step) and B = V (lane l: dim l&15 of the 16-dim tile, same
// keys), read from a transposed LDS image of V.  C/D: lane l, reg r holds [row 4(l>>4) + r][col l&15].
template <int HD>
__global__ __launch_bounds__(256) void attn_extend_prefix_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ prefix,
                                                                 long ld_p, long bs_p, const bf16* __restrict__ tail, long ld_t, long bs_t,
                                                                 int v_off, const int* __restrict__ cu_q, const int* __restrict__ prow_,
                                                                 const int* __restrict__ plen_, int P_rows, int P_max, int T_max,
                                                                 float* __restrict__ part, int H, int Hkv, int chunk, int nch, int tiles,
                                                                 float scale) {
    constexpr int KS = HD / 32;         // k-steps of Q K^T
    constexpr int DT = HD / 16;         // 16-wide output dim tiles
    __shared__ __attribute__((aligned(16))) bf16 Ks[XT_KT][HD + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Vt[HD][XT_KT + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Ps[4][XT_MAXRT][16][XT_KT + XT_KPAD];
    const int c = blockIdx.x, kh = blockIdx.y;
    const int b = blockIdx.z / tiles, t = blockIdx.z % tiles;
    const int G = H / Hkv, QS = xt_qs(G), QT = 16 * QS, R = QS * G;
    const int q_beg = cu_q[b], n_b = min(cu_q[b + 1] - q_beg, T_max);
    const int prow = prow_[b], r0 = plen_[b];
    if (!xp_valid(prow, r0, P_rows, P_max)) return;
    const int i0 = t * QT;
    if (i0 >= n_b) return;
    const int i_last = min(n_b, i0 + QT) - 1;
    const int j0 = c * chunk;
    const int j1 = min(j0 + chunk, r0 + i_last + 1);           // r0 <= P_max and i_last < T_max bound it
    if (j0 >= j1) return;
    const int lane = lane_id(), w = wave_id();
    const int lc = lane & 15, lh = lane >> 4;
    const bf16* pb = prefix + (long)prow * bs_p + kh * HD;     // key j < r0: position j
    const bf16* tb = tail + (long)b * bs_t + kh * HD;          // key j >= r0: position j - r0

    // Q fragments, running statistics and accumulators of this wave's row tiles (rt = w + 4k: sub-tile rt / G, head rt % G)
    bf16x8 qf[XT_MAXRT][KS];
    f32x4 o[XT_MAXRT][DT];
    float m[XT_MAXRT][4], l[XT_MAXRT][4];
#pragma unroll
    for (int k = 0; k < XT_MAXRT; ++k) {
        const int rt = w + 4 * k;
        const int s = rt / (G > 0 ? G : 1), g = rt % G;
        const int i = i0 + s * 16 + lc;
        const bool ok = rt < R && i < n_b;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
            qf[k][kk] = ok ? *(const bf16x8*)(q + (long)(q_beg + i) * ld_q + (kh * G + g) * HD + kk * 32 + lh * 8) : zero8();
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[k][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) { m[k][r] = -INFINITY; l[k][r] = 0.f; }
    }

    for (int kb = j0; kb < j1; kb += XT_KT) {
        // stage K [key][dim] and V^T [dim][key], each key from its own source; keys >= j1 read as zeros (a masked p is exactly 0, and
        // 0 * 0 adds nothing)
        for (int e = threadIdx.x; e < XT_KT * HD / 8; e += 256) {
            const int key = e / (HD / 8), d8 = (e % (HD / 8)) * 8;
            const int j = kb + key;
            bf16x8 kv = zero8(), vv = zero8();
            if (j < j1) {
                const bf16* src = j < r0 ? pb + (long)j * ld_p : tb + (long)(j - r0) * ld_t;
                kv = *(const bf16x8*)(src + d8);
                vv = *(const bf16x8*)(src + v_off + d8);
            }
            *(bf16x8*)&Ks[key][d8] = kv;
#pragma unroll
            for (int x = 0; x < 8; ++x) Vt[d8 + x][key] = vv[x];
        }
        __syncthreads();
        // S = Q K^T, mask, online softmax; P (bf16) to this wave's LDS tile
#pragma unroll
        for (int k = 0; k < XT_MAXRT; ++k) {
            const int rt = w + 4 * k;
            if (rt >= R) continue;
            const int s = rt / G;
            f32x4 sc[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                sc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const bf16x8 kf = *(const bf16x8*)&Ks[n * 16 + lc][kk * 32 + lh * 8];
                    sc[n] = mfma16(qf[k][kk], kf, sc[n]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + s * 16 + lh * 4 + r;
                const int lim = (i < n_b) ? r0 + i : -1;            // last key this row sees; rows past the sequence see none
                float mx = -INFINITY;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int j = kb + n * 16 + lc;
                    const float v = (j <= lim && j < j1) ? sc[n][r] * scale : -INFINITY;
                    sc[n][r] = v;
                    mx = fmaxf(mx, v);
                }
#pragma unroll
                for (int x = 1; x < 16; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x, 64));
                const float mn = fmaxf(m[k][r], mx);
                const float mu = mn == -INFINITY ? 0.f : mn;
                const float alpha = expf(m[k][r] - mu);
                m[k][r] = mn;
                float ps = 0.f;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float p = expf(sc[n][r] - mu);
                    sc[n][r] = p;
                    ps += p;
                }
                l[k][r] = l[k][r] * alpha + ps;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[k][dt][r] *= alpha;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ps[w][k][lh * 4 + r][n * 16 + lc] = f2bf(sc[n][r]);
        }
        __syncthreads();
        // O += P V
#pragma unroll
        for (int k = 0; k < XT_MAXRT; ++k) {
            const int rt = w + 4 * k;
            if (rt >= R) continue;
#pragma unroll
            for (int kk = 0; kk < XT_KT / 32; ++kk) {
                const bf16x8 pf = *(const bf16x8*)&Ps[w][k][lc][kk * 32 + lh * 8];
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const bf16x8 vf = *(const bf16x8*)&Vt[dt * 16 + lc][kk * 32 + lh * 8];
                    o[k][dt] = mfma16(pf, vf, o[k][dt]);
                }
            }
        }
        __syncthreads();
    }
    // partials of the rows that own this chunk (c <= pos / chunk): part[(row * H + h) * nch + c][HD + 2]
#pragma unroll
    for (int k = 0; k < XT_MAXRT; ++k) {
        const int rt = w + 4 * k;
        if (rt >= R) continue;
        const int s = rt / G, g = rt % G, h = kh * G + g;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float lr = l[k][r];
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) lr += __shfl_xor(lr, x, 64);
            const int i = i0 + s * 16 + lh * 4 + r;
            if (i >= n_b || c > (r0 + i) / chunk) continue;
            float* pp = part + (((long)(q_beg + i) * H + h) * nch + c) * (HD + 2);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) pp[dt * 16 + lc] = o[k][dt][r];
            if (lc == 0) {
                pp[HD] = m[k][r];
                pp[HD + 1] = lr;
            }
        }
    }
}

// one block of HD threads per (query row, q head): the row's chunks 0 .. pos / chunk merged in chunk order, bf16 out [M, H*HD]; the
// rows of a sequence the attention kernel refused (or past T_max) are zeros
template <int HD>
__global__ __launch_bounds__(HD) void attn_extend_prefix_combine_kernel(const float* __restrict__ part, const int* __restrict__ cu_q,
                                                                        const int* __restrict__ prow_, const int* __restrict__ plen_,
                                                                        int P_rows, int P_max, int T_max, int B, bf16* __restrict__ out,
                                                                        long ld_o, int H, int nch, int chunk) {
    const int mh = blockIdx.x, row = mh / H, h = mh % H, dd = threadIdx.x;
    int b = 0;
    while (b + 1 < B && cu_q[b + 1] <= row) ++b;
    const int i = row - cu_q[b];
    if (!xp_valid(prow_[b], plen_[b], P_rows, P_max) || i < 0 || i >= T_max) {
        out[(long)row * ld_o + h * HD + dd] = f2bf(0.f);
        return;
    }
    const int pos = plen_[b] + i;
    const int nc = min(pos / chunk + 1, nch);
    const float* pp = part + (long)mh * nch * (HD + 2);
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, pp[c * (HD + 2) + HD]);
    float L = 0.f, o = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float e = expf(pp[c * (HD + 2) + HD] - M);
        L += pp[c * (HD + 2) + HD + 1] * e;
        o += pp[c * (HD + 2) + dd] * e;
    }
    out[(long)row * ld_o + h * HD + dd] = f2bf(o / L);
}

// ------------------------------------------------------------------------------------------------ token log-prob of a row
// torch.argmax semantics over the first n columns: the lowest index among equal maxima, NaN above everything (rv_argmax_rows_f32's rule)
DEVINL bool tl_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// One workgroup per output row r, which reads row s = src_row ? src_row[r] : r of x: (m, L) by log_softmax.h's statements, then
// logprob[r] = fl(fl(x[s, target[r]] - m) - L), rv_log_softmax_rows_f32's value at that column.  The argmax is a sweep of its own
// (NaN ranks highest there and is ignored by the maximum, so the two cannot share one).
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
            if (tl_better(v, j, bv, bi)) { bv = v; bi = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (tl_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane_id() == 0) { rv[wave_id()] = bv; ri[wave_id()] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 4; ++k)
                if (tl_better(rv[k], ri[k], bv, bi)) { bv = rv[k]; bi = ri[k]; }
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
    if (!q || !prefix || !tail || !cu_q || !prefix_row || !prefix_len || !out || !part || B <= 0 || M <= 0 || max_q <= 0 || max_q > M ||
        Hkv <= 0 || H % Hkv || H / Hkv > XT_GMAX || (hd != 64 && hd != 128) || P_rows <= 0 || P_max <= 0 || T_max <= 0 || max_q > T_max ||
        chunk <= 0 || chunk % XT_KT || (ld_q & 7) || (ld_p & 7) || (bs_p & 7) || (ld_t & 7) || (bs_t & 7) || (v_off & 7) ||
        ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || ld_p < v_off + (int64_t)Hkv * hd || ld_t < v_off + (int64_t)Hkv * hd ||
        bs_p < (int64_t)P_max * ld_p || bs_t < (int64_t)T_max * ld_t)
        return RV_ERR_ARG;
    const int64_t L_max = (int64_t)P_max + T_max;
    if (L_max > 0x7fffffff) return RV_ERR_ARG;
    const int nch = (int)((L_max + chunk - 1) / chunk);
    if (part_bytes < (int64_t)M * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const int QT = 16 * xt_qs(H / Hkv);
    const int tiles = (max_q + QT - 1) / QT;
    if ((int64_t)B * tiles > 65535) return RV_ERR_ARG;
    const dim3 grid(nch, Hkv, B * tiles);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_extend_prefix_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)prefix, (long)ld_p,
                           (long)bs_p, (const bf16*)tail, (long)ld_t, (long)bs_t, v_off, cu_q, prefix_row, prefix_len, P_rows, P_max, T_max,
                           (float*)part, H, Hkv, chunk, nch, tiles, scale);
        hipLaunchKernelGGL(attn_extend_prefix_combine_kernel<128>, dim3(M * H), dim3(128), 0, ST, (const float*)part, cu_q, prefix_row,
                           prefix_len, P_rows, P_max, T_max, B, (bf16*)out, (long)ld_o, H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_extend_prefix_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)prefix, (long)ld_p,
                           (long)bs_p, (const bf16*)tail, (long)ld_t, (long)bs_t, v_off, cu_q, prefix_row, prefix_len, P_rows, P_max, T_max,
                           (float*)part, H, Hkv, chunk, nch, tiles, scale);
        hipLaunchKernelGGL(attn_extend_prefix_combine_kernel<64>, dim3(M * H), dim3(64), 0, ST, (const float*)part, cu_q, prefix_row,
                           prefix_len, P_rows, P_max, T_max, B, (bf16*)out, (long)ld_o, H, nch, chunk);
    }
    return rv_check_launch();
}

extern "C" int rv_token_logprob_rows_f32(const float* x, int64_t ld, int x_rows, int n, const int32_t* src_row, const int32_t* target,
                                         int rows, float* logprob, int64_t* argmax, void* stream) {
    if (!x || !target || !logprob || x_rows <= 0 || rows <= 0 || n <= 0 || n > 262144 || ld < n) return RV_ERR_ARG;
    hipLaunchKernelGGL(token_logprob_rows_kernel, dim3(rows), dim3(256), 0, ST, x, (long)ld, x_rows, n, src_row, target, logprob, argmax);
    return rv_check_launch();
}

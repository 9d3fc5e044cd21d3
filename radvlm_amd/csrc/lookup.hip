// Prompt-lookup (speculative) decoding kernel for gfx950: decode attention of R consecutive query rows of one sequence -- the last
// emitted token and R - 1 drafted ones, row i seeing the keys [0, kv_len0 + i) -- with every K / V fragment of a chunk loaded and
// converted once for a whole group of rows.  As in decode.hip every reduction runs in a fixed order that depends on the row's own key
// count only and there are no global or float atomics: a row's result is bit-identical to rv_attn_decode_bf16 on that row alone.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ verify decode attention
// decode.hip's attn_decode_kernel for a staircase of rows.  Block (chunk c, kv head kh, sequence b x row group): a "query" is one
// (row, q head of kv head kh) pair, up to AV_NQ = 16 of them per block (rows per group = 16 / G: 16 rows of an MHA model, 2 of a G = 7
// or 8 one), query nq = (row - first row) * G + g.  Query nq sees the chunk's first nr[nq] keys, nr = min(j0 + chunk, len_row) - j0 with
// len_row = min(kv_len0[b] + row, L_max); only the last one or two chunks differ between the rows of a group.
// What keeps a row's bits those of attn_decode_kernel at kv_len = kv_len0[b] + row:
//   - key j sits on the same lane (wave w, lane row lr) whatever j1 is, so a lane walks ITS keys in the same ascending order and simply
//     stops earlier for a shorter row: a key the row may not see is skipped (never multiplied by zero; a stale row may hold NaN);
//   - the score of (query, key) does not depend on j1 at all: the 8 products in element order, the xor tree over the LPR lanes, * scale;
//   - m, l: one wave per query, lane-strided over j < nr in ascending order, wave_max / wave_sum -- which wave runs a query is immaterial;
//   - P V: acc += p * v per lane in its key order, the xor tree over the lane rows, waves 0..3 added in order; the combine is that
//     kernel's with the row's own key count.
// The q rows live in LDS as fp32 (the score loop reads them as broadcasts); the P V accumulators are the register budget: 16 x 8 floats.
constexpr int AD_GMAX = 8;
constexpr int AD_CHUNK_MAX = 512;
constexpr int AV_NQ = 16;
constexpr int AV_RMAX = 32;

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_verify_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                                 long bs_c, int v_off, const int* __restrict__ kv_len0, int L_max,
                                                                 float* __restrict__ part, int R, int rpg, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    constexpr int BUF = AV_NQ * AD_CHUNK_MAX > 4 * AV_NQ * HD ? AV_NQ * AD_CHUNK_MAX : 4 * AV_NQ * HD;
    __shared__ float buf[BUF];                  // sc[AV_NQ][chunk] through the P V loop, then ored[4][AV_NQ][HD]
    __shared__ float qs[AV_NQ][HD];
    __shared__ int nrs[AV_NQ];
    const int c = blockIdx.x, kh = blockIdx.y;
    const int ngrp = (R + rpg - 1) / rpg;
    const int b = blockIdx.z / ngrp, r0 = (blockIdx.z % ngrp) * rpg;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int rows = min(rpg, R - r0), NQ = rows * G;
    const int kv0 = kv_len0[b];
    const int j0 = c * chunk;
    const int len_max = min(kv0 + r0 + rows - 1, L_max);          // the group's last row sees the most keys
    if (j0 >= len_max) return;                  // no row of the group reaches this chunk; the combine reads a row's own chunks only
    const int j1 = min(j0 + chunk, len_max);
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + li * 8;
    const bf16* vbase = kbase + v_off;
    if (threadIdx.x < AV_NQ) {
        const int nq = threadIdx.x;
        int n = 0;
        if (nq < NQ) n = min(max(min(j0 + chunk, min(kv0 + r0 + nq / G, L_max)) - j0, 0), chunk);
        nrs[nq] = n;
    }
    for (int idx = threadIdx.x; idx < NQ * LPR; idx += 256) {
        const int nq = idx / LPR, s = idx % LPR;
        const bf16x8 t = *(const bf16x8*)(q + ((long)b * R + r0 + nq / G) * ld_q + (kh * G + nq % G) * HD + s * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qs[nq][s * 8 + i] = bf2f(t[i]);
    }
    __syncthreads();
    int nr[AV_NQ];
#pragma unroll
    for (int nq = 0; nq < AV_NQ; ++nq) nr[nq] = __builtin_amdgcn_readfirstlane(nrs[nq]);
    // scores
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        const bool ok = j < j1;
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)j * ld_c) : zero8();
        float kf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = bf2f(kt[i]);
#pragma unroll
        for (int nq = 0; nq < AV_NQ; ++nq) {
            if (nr[nq] > 0) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d += qs[nq][li * 8 + i] * kf[i];
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
                if (j - j0 < nr[nq] && li == 0) buf[nq * chunk + (j - j0)] = d * scale;
            }
        }
    }
    __syncthreads();
    // chunk softmax statistics: wave w owns queries w, w + 4, ...
    for (int nq = w; nq < NQ; nq += 4) {
        const int n = nrs[nq];
        if (n <= 0) continue;
        float* s = buf + nq * chunk;
        float m = -INFINITY;
        for (int j = lane; j < n; j += 64) m = fmaxf(m, s[j]);
        m = wave_max(m);
        float l = 0.f;
        for (int j = lane; j < n; j += 64) {
            const float p = expf(s[j] - m);
            s[j] = p;
            l += p;
        }
        l = wave_sum(l);
        if (lane == 0) {
            float* pp = part + ((((long)b * R + r0 + nq / G) * H + kh * G + nq % G) * nch + c) * (HD + 2);
            pp[HD] = m;
            pp[HD + 1] = l;
        }
    }
    __syncthreads();
    // P V
    float acc[AV_NQ][8];
#pragma unroll
    for (int nq = 0; nq < AV_NQ; ++nq)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[nq][i] = 0.f;
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        if (j < j1) {
            const bf16x8 vt = *(const bf16x8*)(vbase + (long)j * ld_c);
            float vf[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) vf[i] = bf2f(vt[i]);
#pragma unroll
            for (int nq = 0; nq < AV_NQ; ++nq) {
                if (j - j0 < nr[nq]) {
                    const float p = buf[nq * chunk + (j - j0)];
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[nq][i] += p * vf[i];
                }
            }
        }
    }
    __syncthreads();                            // every read of the scores is done: the wave partials reuse their space
#pragma unroll
    for (int nq = 0; nq < AV_NQ; ++nq) {
        if (nr[nq] > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a = acc[nq][i];
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
                if (lr == 0) buf[(w * AV_NQ + nq) * HD + li * 8 + i] = a;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NQ * HD; idx += 256) {
        const int nq = idx / HD, dd = idx % HD;
        if (nrs[nq] <= 0) continue;
        float o = buf[(0 * AV_NQ + nq) * HD + dd];
        o += buf[(1 * AV_NQ + nq) * HD + dd];
        o += buf[(2 * AV_NQ + nq) * HD + dd];
        o += buf[(3 * AV_NQ + nq) * HD + dd];
        part[((((long)b * R + r0 + nq / G) * H + kh * G + nq % G) * nch + c) * (HD + 2) + dd] = o;
    }
}

// decode.hip's attn_decode_combine_kernel with the row's own key count: one block of HD threads per (query row, q head)
template <int HD>
__global__ __launch_bounds__(HD) void attn_decode_verify_combine_kernel(const float* __restrict__ part, const int* __restrict__ kv_len0, int L_max,
                                                                        bf16* __restrict__ out, long ld_o, int R, int H, int nch, int chunk) {
    const int bh = blockIdx.x, row = bh / H, h = bh % H, dd = threadIdx.x;
    const int len = min(kv_len0[row / R] + row % R, L_max);
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
    out[(long)row * ld_o + h * HD + dd] = f2bf(nc > 0 ? o / L : 0.f);
}

}  // namespace

extern "C" int rv_attn_decode_verify_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off,
                                          const int32_t* kv_len0, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B,
                                          int R, int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    if (!q || !cache || !kv_len0 || !out || !part || B <= 0 || R < 1 || R > AV_RMAX || Hkv <= 0 || H % Hkv || H / Hkv > AD_GMAX ||
        (hd != 64 && hd != 128) || L_max <= 0 || chunk <= 0 || chunk > AD_CHUNK_MAX || chunk % (hd == 128 ? 16 : 32) || (ld_q & 7) ||
        (ld_c & 7) || (bs_c & 7) || (v_off & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || ld_c < v_off + (int64_t)Hkv * hd ||
        bs_c < (int64_t)L_max * ld_c)
        return RV_ERR_ARG;
    const int nch = (L_max + chunk - 1) / chunk;
    if (part_bytes < (int64_t)B * R * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const int rpg = AV_NQ / (H / Hkv);          // rows per block: G <= 8, so at least 2
    const int ngrp = (R + rpg - 1) / rpg;
    const dim3 grid(nch, Hkv, B * ngrp);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_decode_verify_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len0, L_max, (float*)part, R, rpg, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_verify_combine_kernel<128>, dim3(B * R * H), dim3(128), 0, ST, (const float*)part, kv_len0, L_max,
                           (bf16*)out, (long)ld_o, R, H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_decode_verify_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len0, L_max, (float*)part, R, rpg, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_verify_combine_kernel<64>, dim3(B * R * H), dim3(64), 0, ST, (const float*)part, kv_len0, L_max,
                           (bf16*)out, (long)ld_o, R, H, nch, chunk);
    }
    return rv_check_launch();
}

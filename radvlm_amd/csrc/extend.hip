// Extend attention for gfx950: the prompt pass of a continued generate() call, causal attention of the uncached suffix rows of each
// sequence against that sequence's KV cache (the reused prefix plus the suffix's own rows, already written).  Query i of sequence b sits
// at position r[b] + i and attends to the keys [0, r[b] + i].
//
// Work split, flash-decoding style: block (chunk c, kv head kh, query tile z) takes the keys [c*chunk, (c+1)*chunk) of one tile of
// XT_QS * 16 query rows of one sequence times the G = H / Hkv query heads of kv head kh, so every K / V tile staged in LDS feeds all of
// them; chunks past the tile's last key are skipped.  Each block writes the (unnormalised o, running max m, sum l) of its rows per chunk;
// extend_combine_kernel merges a row's chunks in chunk order.  Tiles start at each sequence's first suffix row and the chunk grid is
// fixed in absolute key positions, so a row's result depends on its own sequence only: bit-identical alone or in any batch.
// Reference call sites are listed in include/radvlm_hip.h.
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

constexpr int XT_KT = 64;        // keys per LDS stage
constexpr int XT_GMAX = 8;       // query heads per kv head
constexpr int XT_MAXRT = 2;      // 16-row MFMA row tiles per wave (row tiles per block <= 8, 4 waves)
constexpr int XT_KPAD = 8;       // LDS row padding (bf16 elements)

// query sub-tiles of 16 rows per block: enough (query, head) row tiles for the 4 waves, at most 8 (a function of G alone)
DEVINL __host__ int xt_qs(int G) { return G >= 4 ? 1 : 4 / G; }

// MFMA 16x16x32 (common.h): S = Q K^T with A = Q rows (lane l: row l&15, dims 8(l>>4)..+7 of k-step kk) and B = K^T (lane l: key l&15,
// same dims); P V with A = P (lane l: row l&15, keys 8(l>>4)..+7 of the 32-key step) and B = V (lane l: dim l&15 of the 16-dim tile, same
// keys), read from a transposed LDS image of V.  C/D: lane l, reg r holds [row 4(l>>4) + r][col l&15].
template <int HD>
__global__ __launch_bounds__(256) void attn_extend_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                          long bs_c, int v_off, const int* __restrict__ cu_q, const int* __restrict__ rr,
                                                          int L_max, float* __restrict__ part, int H, int Hkv, int chunk, int nch, int tiles,
                                                          float scale) {
    constexpr int KS = HD / 32;         // k-steps of Q K^T
    constexpr int DT = HD / 16;         // 16-wide output dim tiles
    __shared__ __attribute__((aligned(16))) bf16 Ks[XT_KT][HD + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Vt[HD][XT_KT + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Ps[4][XT_MAXRT][16][XT_KT + XT_KPAD];
    const int c = blockIdx.x, kh = blockIdx.y;
    const int b = blockIdx.z / tiles, t = blockIdx.z % tiles;
    const int G = H / Hkv, QS = xt_qs(G), QT = 16 * QS, R = QS * G;
    const int q_beg = cu_q[b], n_b = cu_q[b + 1] - q_beg, r0 = rr[b];
    const int i0 = t * QT;
    if (i0 >= n_b) return;
    const int i_last = min(n_b, i0 + QT) - 1;
    const int j0 = c * chunk;
    const int j1 = min(min(j0 + chunk, r0 + i_last + 1), L_max);
    if (j0 >= j1) return;
    const int lane = lane_id(), w = wave_id();
    const int lc = lane & 15, lh = lane >> 4;
    const bf16* cb = cache + (long)b * bs_c + kh * HD;

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
        // stage K [key][dim] and V^T [dim][key]; keys >= j1 read as zeros (a masked p is exactly 0, and 0 * 0 adds nothing)
        for (int e = threadIdx.x; e < XT_KT * HD / 8; e += 256) {
            const int key = e / (HD / 8), d8 = (e % (HD / 8)) * 8;
            const int j = kb + key;
            bf16x8 kv = zero8(), vv = zero8();
            if (j < j1) {
                kv = *(const bf16x8*)(cb + (long)j * ld_c + d8);
                vv = *(const bf16x8*)(cb + (long)j * ld_c + v_off + d8);
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

// one block of HD threads per (query row, q head): the row's chunks 0 .. pos / chunk merged in chunk order, bf16 out [M, H*HD]
template <int HD>
__global__ __launch_bounds__(HD) void attn_extend_combine_kernel(const float* __restrict__ part, const int* __restrict__ cu_q,
                                                                 const int* __restrict__ rr, int B, bf16* __restrict__ out, long ld_o, int H,
                                                                 int nch, int chunk) {
    const int mh = blockIdx.x, row = mh / H, h = mh % H, dd = threadIdx.x;
    int b = 0;
    while (b + 1 < B && cu_q[b + 1] <= row) ++b;
    const int pos = rr[b] + row - cu_q[b];
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

}  // namespace

extern "C" int rv_attn_extend_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* cu_q,
                                   const int32_t* r, int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int M, int max_q,
                                   int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    if (!q || !cache || !cu_q || !r || !out || !part || B <= 0 || M <= 0 || max_q <= 0 || max_q > M || Hkv <= 0 || H % Hkv ||
        H / Hkv > XT_GMAX || (hd != 64 && hd != 128) || L_max <= 0 || chunk <= 0 || chunk % XT_KT || (ld_q & 7) || (ld_c & 7) || (bs_c & 7) ||
        (v_off & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || ld_c < v_off + (int64_t)Hkv * hd || bs_c < (int64_t)L_max * ld_c)
        return RV_ERR_ARG;
    const int nch = (L_max + chunk - 1) / chunk;
    if (part_bytes < (int64_t)M * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const int QT = 16 * xt_qs(H / Hkv);
    const int tiles = (max_q + QT - 1) / QT;
    if ((int64_t)B * tiles > 65535) return RV_ERR_ARG;
    const dim3 grid(nch, Hkv, B * tiles);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_extend_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c,
                           v_off, cu_q, r, L_max, (float*)part, H, Hkv, chunk, nch, tiles, scale);
        hipLaunchKernelGGL(attn_extend_combine_kernel<128>, dim3(M * H), dim3(128), 0, ST, (const float*)part, cu_q, r, B, (bf16*)out, (long)ld_o,
                           H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_extend_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c,
                           v_off, cu_q, r, L_max, (float*)part, H, Hkv, chunk, nch, tiles, scale);
        hipLaunchKernelGGL(attn_extend_combine_kernel<64>, dim3(M * H), dim3(64), 0, ST, (const float*)part, cu_q, r, B, (bf16*)out, (long)ld_o,
                           H, nch, chunk);
    }
    return rv_check_launch();
}

// Shared-prefix decode attention for gfx950: rv_attn_decode_bf16 for a batch in which groups of cache rows ("tiles") hold bit-equal K|V
// at their first c0 * chunk positions -- the requests of one generate_batch() call that begin with the same image and system prompt.
// A shared chunk's K / V fragments are loaded and converted once, from the tile's first row, for every (row, q head) query of the tile;
// a chunk at or past c0 is the plain kernel's work on the row alone.  As in decode.hip every reduction runs in a fixed order that depends
// on the row's own key count only and there are no global or float atomics: a row's result is bit-identical to rv_attn_decode_bf16 on
// the same cache.  Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ shared-prefix decode attention
// decode.hip's attn_decode_kernel restated the way lookup.hip restates it for a staircase.  Block (chunk c, kv head kh, row b), grid
// (nch, Hkv, B) as there.  A "query" is one (row, q head of kv head kh) pair, up to AS_NQ = 16 of them per block:
//   c >= c0[b]: the block's rows are {b}, its G queries the plain kernel's;
//   c <  c0[b]: the block returns at once unless b leads its tile (tile[b][0] == b); a leading block's rows are tile[b][0 .. 16 / G)
//               up to the first -1, query nq = t * G + g for the tile's t-th row, and every K / V fragment is read from row b.
// Query nq sees the chunk's first nr[nq] keys, nr = min(j0 + chunk, len_row) - j0 with len_row = min(kv_len[row], L_max), in a shared
// chunk capped by the leading row's own count: a position at or past a row's kv_len (its own or the leader's) never reaches an output,
// whatever the table says.  Rows outside [0, B) end the list.  Under the contract (every row of a tile holds c0 * chunk keys or more)
// nr is `chunk` for every query of a shared chunk.
// What keeps a row's bits those of attn_decode_kernel (the list of lookup.hip):
//   - key j sits on the same lane (wave w, lane row lr), so a lane walks ITS keys in the same ascending order; a key the row may not
//     see is skipped (never multiplied by zero; a stale row may hold NaN);
//   - the score of (query, key): the 8 products in element order, the xor tree over the LPR lanes, * scale;
//   - m, l: one wave per query, lane-strided over j < nr in ascending order, wave_max / wave_sum -- which wave runs a query is immaterial;
//   - P V: acc += p * v per lane in its key order, the xor tree over the lane rows, waves 0..3 added in order; the combine is that
//     kernel's.  The K / V bits come from the leading row instead of the row's own: equal by the contract.
// The q rows live in LDS as fp32 (the score loop reads them as broadcasts); the P V accumulators are the register budget: 16 x 8 floats.
constexpr int AD_GMAX = 8;
constexpr int AD_CHUNK_MAX = 512;
constexpr int AS_NQ = 16;
constexpr int AS_TILE = 16;                     // columns of the tile table

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_shared_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                                 long bs_c, int v_off, const int* __restrict__ kv_len,
                                                                 const int* __restrict__ c0v, const int* __restrict__ tile, int L_max,
                                                                 float* __restrict__ part, int B, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    constexpr int BUF = AS_NQ * AD_CHUNK_MAX > 4 * AS_NQ * HD ? AS_NQ * AD_CHUNK_MAX : 4 * AS_NQ * HD;
    __shared__ float buf[BUF];                  // sc[AS_NQ][chunk] through the P V loop, then ored[4][AS_NQ][HD]
    __shared__ float qs[AS_NQ][HD];
    __shared__ int nrs[AS_NQ];
    __shared__ int rws[AS_NQ];                  // cache / q / part row of each query, -1: none
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int G = H / Hkv, rpt = AS_NQ / G;
    const int nch = gridDim.x;
    const bool shared = c < c0v[b];
    if (shared && tile[(long)b * AS_TILE] != b) return;           // the tile's leading block writes this row's partial
    const int len_b = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len_b) return;                    // as the plain kernel; a shared chunk holds at most the leading row's keys
    const int j1 = min(j0 + chunk, len_b);
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + li * 8;
    const bf16* vbase = kbase + v_off;
    if (threadIdx.x < AS_NQ) {
        const int nq = threadIdx.x, t = nq / G;
        int row = -1;
        if (t == 0) {
            row = b;
        } else if (shared && t < rpt) {
            row = b;                            // walk the list: a -1 or an out-of-range entry ends it
            for (int k = 1; k <= t && row >= 0; ++k) {
                const int e = tile[(long)b * AS_TILE + k];
                row = (e >= 0 && e < B) ? e : -1;
            }
        }
        int n = 0;
        if (row >= 0 && nq < rpt * G) n = min(max(min(j1, min(kv_len[row], L_max)) - j0, 0), chunk);
        nrs[nq] = n;
        rws[nq] = n > 0 ? row : -1;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < AS_NQ * LPR; idx += 256) {
        const int nq = idx / LPR, s = idx % LPR;
        const int row = rws[nq];
        if (row < 0) continue;
        const bf16x8 t = *(const bf16x8*)(q + (long)row * ld_q + (kh * G + nq % G) * HD + s * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) qs[nq][s * 8 + i] = bf2f(t[i]);
    }
    __syncthreads();
    int nr[AS_NQ];
#pragma unroll
    for (int nq = 0; nq < AS_NQ; ++nq) nr[nq] = __builtin_amdgcn_readfirstlane(nrs[nq]);
    // scores
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        const bool ok = j < j1;
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)j * ld_c) : zero8();
        float kf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = bf2f(kt[i]);
#pragma unroll
        for (int nq = 0; nq < AS_NQ; ++nq) {
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
    for (int nq = w; nq < AS_NQ; nq += 4) {
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
            float* pp = part + (((long)rws[nq] * H + kh * G + nq % G) * nch + c) * (HD + 2);
            pp[HD] = m;
            pp[HD + 1] = l;
        }
    }
    __syncthreads();
    // P V
    float acc[AS_NQ][8];
#pragma unroll
    for (int nq = 0; nq < AS_NQ; ++nq)
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
            for (int nq = 0; nq < AS_NQ; ++nq) {
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
    for (int nq = 0; nq < AS_NQ; ++nq) {
        if (nr[nq] > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a = acc[nq][i];
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
                if (lr == 0) buf[(w * AS_NQ + nq) * HD + li * 8 + i] = a;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < AS_NQ * HD; idx += 256) {
        const int nq = idx / HD, dd = idx % HD;
        if (nrs[nq] <= 0) continue;
        float o = buf[(0 * AS_NQ + nq) * HD + dd];
        o += buf[(1 * AS_NQ + nq) * HD + dd];
        o += buf[(2 * AS_NQ + nq) * HD + dd];
        o += buf[(3 * AS_NQ + nq) * HD + dd];
        part[(((long)rws[nq] * H + kh * G + nq % G) * nch + c) * (HD + 2) + dd] = o;
    }
}

// decode.hip's attn_decode_combine_kernel, statement for statement: one block of HD threads per (row, q head), the row's own kv_len
template <int HD>
__global__ __launch_bounds__(HD) void attn_decode_shared_combine_kernel(const float* __restrict__ part, const int* __restrict__ kv_len, int L_max,
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

}  // namespace

extern "C" int rv_attn_decode_shared_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off,
                                          const int32_t* kv_len, const int32_t* c0, const int32_t* tile, int L_max, void* out, int64_t ld_o,
                                          void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk, float scale, void* stream) {
    if (!q || !cache || !kv_len || !c0 || !tile || !out || !part || B <= 0 || Hkv <= 0 || H % Hkv || H / Hkv > AD_GMAX ||
        (hd != 64 && hd != 128) || L_max <= 0 || chunk <= 0 || chunk > AD_CHUNK_MAX || chunk % (hd == 128 ? 16 : 32) || (ld_q & 7) ||
        (ld_c & 7) || (bs_c & 7) || (v_off & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || ld_c < v_off + (int64_t)Hkv * hd ||
        bs_c < (int64_t)L_max * ld_c)
        return RV_ERR_ARG;
    const int nch = (L_max + chunk - 1) / chunk;
    if (part_bytes < (int64_t)B * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const dim3 grid(nch, Hkv, B);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_decode_shared_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len, c0, tile, L_max, (float*)part, B, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_shared_combine_kernel<128>, dim3(B * H), dim3(128), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_decode_shared_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c,
                           (long)bs_c, v_off, kv_len, c0, tile, L_max, (float*)part, B, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_shared_combine_kernel<64>, dim3(B * H), dim3(64), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    }
    return rv_check_launch();
}

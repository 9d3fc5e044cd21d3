// Decode attention probabilities for gfx950: rv_attn_decode_probs_f32, the normalised softmax(scale * q K^T) rows that the split-KV
// decode family (attn_split.h) never materialises -- it keeps (o, m, l) partials only.  One query row per (sequence, q head) against
// the sequence's bf16 KV cache, rv_attn_decode_bf16's operands; V is never read.  Three launches over a caller-provided workspace:
//   (a) scores      grid (key chunk, kv head, row): s[b, h, j] = fl(dot(q[b, h], K[b, j]) * scale) on the register-q layout of
//                   attn_decode_body (HD/8 lanes per key row, one 16-byte K load each, the G heads of a kv head share it);
//   (b) statistics  one workgroup per (row, head): m = max_j s, l = sum_j expf(s - m);
//   (c) finalize    grid (tile of key positions, row): heads in order 0 .. H-1, p = expf(s - m_h) / l_h to `probs`, their mean in
//                   head order to `mean`; columns [n, L_out) are written as 0.0f.
// No atomics.  A score depends on its (q row, key) alone: 8 products in element order per lane, the xor tree over the HD/8 lanes.  The
// statistics walk thread-strided in ascending j, then the xor tree of a wave, then waves 0..3 in order: a function of the row's own
// key count.  So a row's bits do not depend on B, on the grid, on L_out beyond its keys, or on AP_CHUNK (which is therefore no
// argument).  A key at or past n = min(kv_len[b], L_max, L_out) is never loaded.
#include "attn_split.h"

namespace {

constexpr int AP_CHUNK = 256;       // keys per score workgroup and positions per finalize workgroup

DEVINL int ap_keys(const int* __restrict__ kv_len, int b, int L_max, int L_out) { return min(min(kv_len[b], L_max), L_out); }

// ws: s[B * H][L_out], then (m, l)[B * H]
DEVINL float* ap_stats(float* ws, long BH, int L_out) { return ws + BH * L_out; }

template <int HD>
__global__ __launch_bounds__(256) void attn_probs_score_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                               long bs_c, const int* __restrict__ kv_len, int L_max, int L_out,
                                                               float* __restrict__ ws, int H, int G, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int n = ap_keys(kv_len, b, L_max, L_out);
    const int j0 = c * AP_CHUNK;
    if (j0 >= n) return;
    const int j1 = min(j0 + AP_CHUNK, n);
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + li * 8;
    float qv[AD_GMAX][8];
#pragma unroll
    for (int g = 0; g < AD_GMAX; ++g) {
        if (g < G) {
            const bf16x8 t = *(const bf16x8*)(q + (long)b * ld_q + (kh * G + g) * HD + li * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) qv[g][i] = bf2f(t[i]);
        }
    }
    float* srow = ws + ((long)b * H + kh * G) * L_out;
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        const bool ok = j < j1;
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)j * ld_c) : zero8();
#pragma unroll
        for (int g = 0; g < AD_GMAX; ++g) {
            if (g < G) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) d += qv[g][i] * bf2f(kt[i]);
#pragma unroll
                for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
                if (ok && li == 0) srow[(long)g * L_out + j] = d * scale;
            }
        }
    }
}

__global__ __launch_bounds__(256) void attn_probs_stats_kernel(const int* __restrict__ kv_len, int L_max, int L_out, float* __restrict__ ws,
                                                               int H, long BH) {
    __shared__ float red[4];
    const long rh = blockIdx.x;
    const int b = (int)(rh / H);
    const int n = ap_keys(kv_len, b, L_max, L_out);
    if (n <= 0) return;
    const float* s = ws + rh * L_out;
    float m = -INFINITY;
    for (int j = threadIdx.x; j < n; j += 256) m = fmaxf(m, s[j]);
    m = wave_max(m);
    if (lane_id() == 0) red[wave_id()] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float l = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) l += expf(s[j] - m);
    l = block_sum<4>(l, red);
    if (threadIdx.x == 0) {
        float* st = ap_stats(ws, BH, L_out) + rh * 2;
        st[0] = m;
        st[1] = l;
    }
}

__global__ __launch_bounds__(AP_CHUNK) void attn_probs_finalize_kernel(const int* __restrict__ kv_len, int L_max, int L_out,
                                                                       const float* __restrict__ ws, float* __restrict__ probs, long ld_p,
                                                                       float* __restrict__ mean, long ld_m, int H, long BH) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * AP_CHUNK + threadIdx.x;
    if (j >= L_out) return;
    const int n = ap_keys(kv_len, b, L_max, L_out);
    const float* st = ws + BH * L_out + (long)b * H * 2;
    const float* s = ws + (long)b * H * L_out + j;
    float* pr = probs ? probs + (long)b * H * ld_p + j : nullptr;
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
        float p = 0.f;
        if (j < n) p = expf(s[(long)h * L_out] - st[2 * h]) / st[2 * h + 1];
        if (pr) pr[(long)h * ld_p] = p;
        acc += p;
    }
    if (mean) mean[(long)b * ld_m + j] = j < n ? acc / (float)H : 0.f;
}

}  // namespace

extern "C" int64_t rv_attn_decode_probs_ws_bytes(int B, int H, int L_out) {
    if (B <= 0 || H <= 0 || L_out <= 0) return 0;
    return ((int64_t)B * H * L_out + (int64_t)B * H * 2) * 4;
}

extern "C" int rv_attn_decode_probs_f32(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, const int32_t* kv_len,
                                        int L_max, int L_out, void* probs, int64_t ld_p, void* mean, int64_t ld_m, void* ws, int64_t ws_bytes,
                                        int B, int H, int Hkv, int hd, float scale, void* stream) {
    if (!q || !kv_len || !ws || (!probs && !mean) || B <= 0 || B > 65535 || Hkv <= 0 || Hkv > 65535 || H <= 0 || H % Hkv ||
        H / Hkv > AD_GMAX || (hd != 64 && hd != 128) || L_max <= 0 || L_out <= 0 || L_out > L_max || (ld_q & 7) || ld_q < (int64_t)H * hd ||
        !split_cache_ok(cache, ld_c, bs_c, 0, Hkv, hd, L_max) || (probs && ld_p < L_out) || (mean && ld_m < L_out) ||
        ws_bytes < rv_attn_decode_probs_ws_bytes(B, H, L_out))
        return RV_ERR_ARG;
    const int G = H / Hkv;
    const long BH = (long)B * H;
    const unsigned nch = cdiv(L_out, AP_CHUNK);
    if (hd == 128)
        hipLaunchKernelGGL(attn_probs_score_kernel<128>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache,
                           (long)ld_c, (long)bs_c, kv_len, L_max, L_out, (float*)ws, H, G, scale);
    else
        hipLaunchKernelGGL(attn_probs_score_kernel<64>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache,
                           (long)ld_c, (long)bs_c, kv_len, L_max, L_out, (float*)ws, H, G, scale);
    hipLaunchKernelGGL(attn_probs_stats_kernel, dim3((unsigned)BH), dim3(256), 0, ST, kv_len, L_max, L_out, (float*)ws, H, BH);
    hipLaunchKernelGGL(attn_probs_finalize_kernel, dim3(nch, B), dim3(AP_CHUNK), 0, ST, kv_len, L_max, L_out, (const float*)ws, (float*)probs,
                       (long)ld_p, (float*)mean, (long)ld_m, H, BH);
    return rv_check_launch();
}

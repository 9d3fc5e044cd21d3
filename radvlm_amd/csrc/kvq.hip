// int8 KV cache kernels for gfx950: the quantising cache write (prefill rows by a row list, decode rows by position) and decode
// attention over the quantised cache.  One group = the hd values of one kv head of K, or of V, at one cached position:
//     amax = max |x|      s = amax / 127 (1 for an all-zero group)      q = clamp(rint(x / s), -127, 127)      x^ = bf16_rne(float(q) * s)
// (IEEE fp32 division, round half to even; rv_quantize_rows_w8_bf16's rule per group).  The attention kernel rebuilds x^ in registers and
// is decode.hip's attn_decode_kernel otherwise -- the same (key row, 8-element slice) per (wave, lane), the same xor butterflies, wave-order
// sum and chunk combine -- so its output is bit-identical to rv_attn_decode_bf16 on the dequantised cache.  No atomics; every reduction
// runs in a fixed order.  Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "attn_split.h"
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ quantising cache write
// Block (x: 256-lane slice of a row, y: source row m).  A lane owns 8 consecutive values; the HD / 8 lanes of a group sit side by side in
// one wave (HD / 8 divides 64), so the group maximum is an xor butterfly over them -- max is order-free and there is nothing to add.
// The destination is the flat cache row rows[m] (prefill), or m * L_max + pos[m] (decode append); a row outside the cache is skipped.
template <int HD>
__global__ __launch_bounds__(256) void kv_quantize_kernel(const bf16* __restrict__ src, long ld_src, signed char* __restrict__ Q, long ld_q,
                                                          float* __restrict__ S, long ld_s, bf16* __restrict__ X, long ld_x,
                                                          const int64_t* __restrict__ rows, const int* __restrict__ pos, int L_max,
                                                          long cache_rows, int width) {
    constexpr int LPR = HD / 8;
    const int m = blockIdx.y;
    long flat;
    if (rows) {
        flat = rows[m];
        if (flat < 0 || flat >= cache_rows) return;
    } else {
        const int p = pos[m];
        if (p < 0 || p >= L_max) return;
        flat = (long)m * L_max + p;
    }
    const int e = (blockIdx.x * 256 + threadIdx.x) * 8;
    const bool in = e < width;                   // width % HD == 0: the lanes of a group are all in or all out
    bf16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (bf16)0.f;
    if (in) t = *(const bf16x8*)(src + (long)m * ld_src + e);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(t[i])));
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    if (!in) return;
    const float s = amax > 0.f ? amax / 127.f : 1.f;
    bf16x8 o;
    unsigned lo = 0u, hi = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float q = fminf(fmaxf(rintf(bf2f(t[i]) / s), -127.f), 127.f);
        o[i] = f2bf(q * s);
        const unsigned b = (unsigned)(int)q & 0xffu;
        if (i < 4) lo |= b << (8 * i);
        else hi |= b << (8 * (i - 4));
    }
    if (Q) {
        *(u32x2*)(Q + flat * ld_q + e) = u32x2{lo, hi};
        if ((threadIdx.x & (LPR - 1)) == 0) S[flat * ld_s + e / HD] = s;
    }
    if (X) *(bf16x8*)(X + flat * ld_x + e) = o;
}

// ------------------------------------------------------------------------------------------------ decode attention, int8 cache
// decode.hip's attn_decode_kernel with the K / V fragment rebuilt from 8 bytes and the group's scale.  What keeps the bits:
//   - key j sits on wave w, lane row lr as there (j = jb + w * RPW + lr, jb in steps of RPB), and a lane walks its keys in ascending order;
//   - a score is the 8 products in element order, the xor tree over the LPR lanes, * scale; m / l: one wave per head, lane-strided;
//   - P V: acc += p * v per lane in its key order, the xor tree over the lane rows, waves 0..3 added in order; the same combine.
// AK_U key rows are loaded before the first is used (8-byte loads need more of them in flight than the 16-byte ones of the bf16 kernel);
// they are consumed in ascending order, so nothing above changes.  A key at or past kv_len is never loaded: its bytes and scale may be
// anything.
constexpr int AK_U = 4;

DEVINL void dq8f(u32x2 r, float s, float* out) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        out[i] = bf2f(f2bf((float)(int)(signed char)(r.x >> (8 * i)) * s));
        out[4 + i] = bf2f(f2bf((float)(int)(signed char)(r.y >> (8 * i)) * s));
    }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16* __restrict__ q, long ld_q, const signed char* __restrict__ cq,
                                                              long ld_c, long bs_c, int v_off, const float* __restrict__ cs, long ld_s,
                                                              long bs_s, int vs_off, const int* __restrict__ kv_len, int L_max,
                                                              float* __restrict__ part, int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    __shared__ float sc[AD_GMAX][AD_CHUNK_MAX];
    __shared__ float ored[4][AD_GMAX][HD];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int len = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len) return;                     // the combine reads chunks < ceil(len / chunk) only
    const int j1 = min(j0 + chunk, len), n = j1 - j0;
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const signed char* kbase = cq + (long)b * bs_c + kh * HD + li * 8;
    const signed char* vbase = kbase + v_off;
    const float* ksb = cs + (long)b * bs_s + kh;
    const float* vsb = ksb + vs_off;
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
    for (int jb = j0; jb < j1; jb += RPB * AK_U) {
        u32x2 kr[AK_U];
        float ks[AK_U];
#pragma unroll
        for (int u = 0; u < AK_U; ++u) {
            const int j = jb + u * RPB + w * RPW + lr;
            const bool ok = j < j1;
            kr[u] = ok ? *(const u32x2*)(kbase + (long)j * ld_c) : u32x2{0u, 0u};
            ks[u] = ok ? ksb[(long)j * ld_s] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < AK_U; ++u) {
            if (jb + u * RPB >= j1) break;     // block-uniform: the bf16 kernel's loop ends here too
            const int j = jb + u * RPB + w * RPW + lr;
            const bool ok = j < j1;
            float kt[8];
            dq8f(kr[u], ks[u], kt);
#pragma unroll
            for (int g = 0; g < AD_GMAX; ++g) {
                if (g < G) {
                    float d = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) d += qv[g][i] * kt[i];
#pragma unroll
                    for (int o = 1; o < LPR; o <<= 1) d += __shfl_xor(d, o, 64);
                    if (ok && li == 0) sc[g][j - j0] = d * scale;
                }
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
    for (int jb = j0; jb < j1; jb += RPB * AK_U) {
        u32x2 vr[AK_U];
        float vs[AK_U];
#pragma unroll
        for (int u = 0; u < AK_U; ++u) {
            const int j = jb + u * RPB + w * RPW + lr;
            const bool ok = j < j1;
            vr[u] = ok ? *(const u32x2*)(vbase + (long)j * ld_c) : u32x2{0u, 0u};
            vs[u] = ok ? vsb[(long)j * ld_s] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < AK_U; ++u) {
            const int j = jb + u * RPB + w * RPW + lr;
            if (j < j1) {
                float vt[8];
                dq8f(vr[u], vs[u], vt);
#pragma unroll
                for (int g = 0; g < AD_GMAX; ++g) {
                    if (g < G) {
                        const float p = sc[g][j - j0];
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[g][i] += p * vt[i];
                    }
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

int kv_quantize_launch(const void* src, int64_t ld_src, void* q8, int64_t ld_q, float* s, int64_t ld_s, void* xhat, int64_t ld_x,
                       const int64_t* rows, const int32_t* pos, int L_max, int64_t cache_rows, int M, int Hkv, int hd, void* stream) {
    const int64_t width = 2 * (int64_t)Hkv * hd;
    if (!src || (!rows && !pos) || (!q8 != !s) || (!q8 && !xhat) || M <= 0 || Hkv <= 0 || (hd != 64 && hd != 128) || L_max <= 0 ||
        cache_rows <= 0 || (ld_src & 7) || ld_src < width || (q8 && ((ld_q & 7) || ld_q < width || ld_s < 2 * Hkv)) ||
        (xhat && ((ld_x & 7) || ld_x < width)) || M > 65535)
        return RV_ERR_ARG;
    const dim3 grid(cdiv(width / 8, 256), M);
    if (hd == 128)
        hipLaunchKernelGGL(kv_quantize_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)src, (long)ld_src, (signed char*)q8, (long)ld_q, s,
                           (long)ld_s, (bf16*)xhat, (long)ld_x, rows, pos, L_max, (long)cache_rows, (int)width);
    else
        hipLaunchKernelGGL(kv_quantize_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)src, (long)ld_src, (signed char*)q8, (long)ld_q, s,
                           (long)ld_s, (bf16*)xhat, (long)ld_x, rows, pos, L_max, (long)cache_rows, (int)width);
    return rv_check_launch();
}

}  // namespace

extern "C" int rv_kv_quantize_rows_bf16(const void* src, int64_t ld_src, void* q8, int64_t ld_q, float* s, int64_t ld_s, void* xhat,
                                        int64_t ld_x, const int64_t* rows, int64_t cache_rows, int M, int Hkv, int hd, void* stream) {
    if (!rows) return RV_ERR_ARG;
    // the launch takes up to 65,535 source rows (grid.y): a longer prefill goes in slices
    for (int m0 = 0; m0 < M; m0 += 65535) {
        const int mm = M - m0 < 65535 ? M - m0 : 65535;
        const int rc = kv_quantize_launch((const char*)src + (int64_t)m0 * ld_src * 2, ld_src, q8, ld_q, s, ld_s, xhat, ld_x, rows + m0, nullptr, 1,
                                          cache_rows, mm, Hkv, hd, stream);
        if (rc != RV_OK) return rc;
    }
    return M > 0 ? RV_OK : RV_ERR_ARG;
}

extern "C" int rv_kv_append_q8_bf16(const void* src, int64_t ld_src, void* q8, int64_t ld_q, float* s, int64_t ld_s, void* xhat, int64_t ld_x,
                                    const int32_t* pos, int L_max, int B, int Hkv, int hd, void* stream) {
    if (!pos) return RV_ERR_ARG;
    return kv_quantize_launch(src, ld_src, q8, ld_q, s, ld_s, xhat, ld_x, nullptr, pos, L_max, (int64_t)B * L_max, B, Hkv, hd, stream);
}

extern "C" int rv_attn_decode_kv8_bf16(const void* q, int64_t ld_q, const void* cache_q8, int64_t ld_c, int64_t bs_c, int v_off,
                                       const float* cache_s, int64_t ld_s, int64_t bs_s, int vs_off, const int32_t* kv_len, int L_max, void* out,
                                       int64_t ld_o, void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk, float scale,
                                       void* stream) {
    const bool ok = kv_len && cache_s && v_off >= 0 && vs_off >= 0 && ld_s >= vs_off + (int64_t)Hkv && bs_s >= (int64_t)L_max * ld_s &&
                    ad_chunk_ok(chunk, hd) && split_cache_ok(cache_q8, ld_c, bs_c, v_off, Hkv, hd, L_max);
    return attn_split_launch(ok, q, ld_q, out, ld_o, part, part_bytes, B, H, Hkv, hd, L_max, chunk, stream, RowsKvLen{kv_len, L_max},
                             [&](auto hd_c, int nch) {
                                 hipLaunchKernelGGL(attn_decode_kv8_kernel<hd_c()>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q,
                                                    (const signed char*)cache_q8, (long)ld_c, (long)bs_c, v_off, cache_s, (long)ld_s, (long)bs_s,
                                                    vs_off, kv_len, L_max, (float*)part, H, Hkv, chunk, scale);
                             });
}

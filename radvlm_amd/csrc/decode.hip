// Decode-time kernels for gfx950: the skinny NT GEMM of one generated token per sequence (M = batch, 1..32 rows), flash-decoding
// attention of one query row per (sequence, q head) against a KV cache, the cache append and the row argmax of greedy decoding.
// Reductions use a fixed order that depends on the problem shape only (N, K; a sequence's own kv_len) -- never on M, on other rows or
// on timing -- and no atomics: a row's result is bit-identical whatever else shares its launch.
// Reference call sites are listed per entry point in include/radvlm_hip.h.
#include "common.h"
#include "radvlm_hip.h"

#include <math.h>

namespace {

#define ST ((hipStream_t)stream)

DEVINL bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (bf16)0.f;
    return z;
}

// weights are read once per token by exactly one CU: nontemporal (MI355X_MICROARCH "nt-weights")
DEVINL bf16x8 ld_nt(const bf16* p) { return __builtin_nontemporal_load((const bf16x8*)p); }

// ------------------------------------------------------------------------------------------------ skinny NT GEMM
// Y[M,N] = X[M,K] W[N,K]^T (+ bias) (+ residual), M <= 32.  Block: 4 waves, 64 output columns (four 16-column MFMA tiles); the K steps
// (32 deep) of the block's K range are split into 4 contiguous runs, one per wave.  Weights go straight from HBM to VGPRs (dwordx4, nt),
// U steps in flight per wave; the X rows (<= 64 KB, L2-resident) are loaded beside them.  MT = row tiles of 16 (rows >= M read zeros).
// MFMA 16x16x32: A = X rows (lane l: row l&15, k 8*(l>>4)..+7), B = W rows (lane l: column l&15, same k) -> D[row][col].
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int GV_COLS = 64;
constexpr int GV_U = 4;

// W8: the weight operand is int8 with one fp32 scale per row (rv_quantize_rows_w8_bf16's packed rows) and the bf16 fragment
// bf16_rne(float(q) * s) is rebuilt in registers.  Same K steps per wave, same k-to-lane assignment per MFMA and every accumulator
// takes its steps in ascending order, so the result is bit-identical to the bf16 kernel on the dequantised weight.  Packed row:
// 64 bytes per PAIR of K steps; lane group kg's 16 bytes hold its 8 weights of step 2j, then its 8 of step 2j + 1 (one dwordx4 nt
// load feeds two MFMA steps); a trailing odd step and ragged K are zero-padded in the packed row.
// Step pairs in flight per wave.  2 (the bf16 kernel's four K steps per iteration at half its bytes) against 4 (its bytes in flight at twice
// the K per iteration) were both built and timed per decoder shape on one box (DESIGN.md 5b "8-bit decoder weights"; the records of both
// builds are in profiles/decode_ab_gemv.jsonl, mode w8, field `build`).  2 is the default: it needs fewer registers than the bf16 kernel
// (96 / 128 against 112 / 146, VGPR + AGPR), 4 needs 144 / 192 and leaves 3 / 2 waves per SIMD.  build.sh out.so -DRV_GV8_P=4 rebuilds
// the other.
#ifndef RV_GV8_P
#define RV_GV8_P 2
#endif
constexpr int GV8_P = RV_GV8_P;

DEVINL bf16x8 dq8(unsigned lo, unsigned hi, float s) {
    bf16x8 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = f2bf((float)(int)(signed char)(lo >> (8 * i)) * s);
        r[4 + i] = f2bf((float)(int)(signed char)(hi >> (8 * i)) * s);
    }
    return r;
}

// The scale pointer is a trailing parameter pack, empty for bf16.  It exists for one reason: the bf16 instantiation keeps the parent
// kernel's exact parameter list, and with it the parent's device code instruction for instruction (an extra pointer, or the body moved
// into an inlined helper, changed its register allocation).  W8 = "a scale was passed".
DEVINL const float* gv_scale() { return nullptr; }
DEVINL const float* gv_scale(const float* p) { return p; }

template <int MT, typename... S>
__global__ __launch_bounds__(256) void gemv_kernel(const bf16* __restrict__ X, long ldx, const bf16* __restrict__ W, long ldw, int M, int N,
                                                   int K, int split, float* __restrict__ part, void* __restrict__ Y, long ldy,
                                                   const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr, int out_f32,
                                                   S... scale_arg) {
    constexpr bool W8 = sizeof...(S) == 1;
    __shared__ float red[4][MT * 16][GV_COLS];
    const int lane = lane_id(), w = wave_id();
    const int c = lane & 15, kg = lane >> 4;
    const int n0 = blockIdx.x * GV_COLS;
    const int sidx = blockIdx.y;
    const int ks = (K + 31) / 32;
    const int unit = sidx * 4 + w, units = split * 4;
    const int s0 = (int)((long)ks * unit / units), s1 = (int)((long)ks * (unit + 1) / units);
    const bf16* wp[4];
    bool n_ok[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int n = n0 + ct * 16 + c;
        n_ok[ct] = n < N;
        if constexpr (W8)                                           // packed rows of ldw bytes, 16 bytes per lane group and step pair
            wp[ct] = (const bf16*)((const char*)W + (long)(n_ok[ct] ? n : 0) * ldw + kg * 16);
        else
            wp[ct] = W + (long)(n_ok[ct] ? n : 0) * ldw + kg * 8;
    }
    const bf16* xp[MT];
    bool m_ok[MT];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt) {
        const int m = rt * 16 + c;
        m_ok[rt] = m < M;
        xp[rt] = X + (long)(m_ok[rt] ? m : 0) * ldx + kg * 8;
    }
    f32x4 acc[MT][4];
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (W8) {
        const float* __restrict__ wscale = gv_scale(scale_arg...);
        float sc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sc[ct] = n_ok[ct] ? wscale[n0 + ct * 16 + c] : 0.f;
        int st = s0;
        if ((st & 1) && st < s1) {                                  // the wave's range starts inside a pair: its second half alone
            const int k = st * 32;
            const bool kin = k + kg * 8 < K;
            u32x2 wq[4];
            bf16x8 xf[MT];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                wq[ct] = (kin && n_ok[ct]) ? __builtin_nontemporal_load((const u32x2*)((const char*)wp[ct] + (long)(st >> 1) * 64 + 8))
                                           : u32x2{0u, 0u};
#pragma unroll
            for (int rt = 0; rt < MT; ++rt) xf[rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const bf16x8 wf = dq8(wq[ct].x, wq[ct].y, sc[ct]);
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[rt], wf, acc[rt][ct]);
            }
            ++st;
        }
        for (; st < s1; st += 2 * GV8_P) {
            u32x4 wq[GV8_P][4];
            bf16x8 xf[2 * GV8_P][MT];
#pragma unroll
            for (int p = 0; p < GV8_P; ++p) {
                const bool pin = st + 2 * p < s1;                   // a pair's 64 bytes exist whenever its first step does
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    wq[p][ct] = (pin && n_ok[ct])
                                    ? __builtin_nontemporal_load((const u32x4*)((const char*)wp[ct] + (long)((st >> 1) + p) * 64))
                                    : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = (st + 2 * p + h) * 32;
                    const bool kin = (st + 2 * p + h) < s1 && k + kg * 8 < K;
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) xf[2 * p + h][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
                }
            }
#pragma unroll
            for (int p = 0; p < GV8_P; ++p) {
                const bool hin = st + 2 * p + 1 < s1;               // the pair's second step may belong to the next wave: zeros then
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const bf16x8 w0 = dq8(wq[p][ct].x, wq[p][ct].y, sc[ct]);
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[2 * p][rt], w0, acc[rt][ct]);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const bf16x8 w1 = dq8(hin ? wq[p][ct].z : 0u, hin ? wq[p][ct].w : 0u, sc[ct]);
#pragma unroll
                    for (int rt = 0; rt < MT; ++rt) acc[rt][ct] = mfma16(xf[2 * p + 1][rt], w1, acc[rt][ct]);
                }
            }
        }
    } else {
        for (int st = s0; st < s1; st += GV_U) {
            bf16x8 wf[GV_U][4], xf[GV_U][MT];
#pragma unroll
            for (int u = 0; u < GV_U; ++u) {
                const int k = (st + u) * 32;
                const bool kin = (st + u) < s1 && k + kg * 8 < K;       // K % 8 == 0: a lane's 8 elements are all in or all out
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) wf[u][ct] = (kin && n_ok[ct]) ? ld_nt(wp[ct] + k) : zero8();
#pragma unroll
                for (int rt = 0; rt < MT; ++rt) xf[u][rt] = (kin && m_ok[rt]) ? *(const bf16x8*)(xp[rt] + k) : zero8();
            }
#pragma unroll
            for (int u = 0; u < GV_U; ++u)
#pragma unroll
                for (int rt = 0; rt < MT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = mfma16(xf[u][rt], wf[u][ct], acc[rt][ct]);
        }
    }
#pragma unroll
    for (int rt = 0; rt < MT; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[w][rt * 16 + 4 * kg + r][ct * 16 + c] = acc[rt][ct][r];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 16 * GV_COLS; idx += 256) {
        const int m = idx / GV_COLS, col = idx % GV_COLS, n = n0 + col;
        if (m >= M || n >= N) continue;
        float v = red[0][m][col];
        v += red[1][m][col];
        v += red[2][m][col];
        v += red[3][m][col];
        if (split > 1) {
            part[((long)sidx * M + m) * N + n] = v;
            continue;
        }
        if (bias) v += bf2f(bias[n]);
        if (R) v += bf2f(R[(long)m * ldr + n]);
        if (out_f32)
            ((float*)Y)[(long)m * ldy + n] = v;
        else
            ((bf16*)Y)[(long)m * ldy + n] = f2bf(v);
    }
}

// split-K combine: the K-slices summed in slice order, then bias / residual / store (same epilogue as above)
__global__ void gemv_combine_kernel(const float* __restrict__ part, int split, int M, int N, void* __restrict__ Y, long ldy,
                                    const bf16* __restrict__ bias, const bf16* __restrict__ R, long ldr, int out_f32) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)M * N) return;
    const int m = (int)(tid / N), n = (int)(tid % N);
    float v = part[tid];
    for (int s = 1; s < split; ++s) v += part[(long)s * M * N + tid];
    if (bias) v += bf2f(bias[n]);
    if (R) v += bf2f(R[(long)m * ldr + n]);
    if (out_f32)
        ((float*)Y)[(long)m * ldy + n] = v;
    else
        ((bf16*)Y)[(long)m * ldy + n] = f2bf(v);
}

// ------------------------------------------------------------------------------------------------ int8 row quantisation
// One workgroup per weight row: absmax, s = amax / 127 (1 for a zero row), q = clamp(rint(w / s)), W <- bf16_rne(float(q) * s) in place,
// q into the packed row gemv_kernel's int8 instantiation reads.  IEEE division and rint (round half to even); max is order-free, no
// atomics.  The in-place write is race-free because (a) every load of pass 1 is consumed before the __syncthreads() after the wave
// reduction, which all threads pass before any thread writes, and (b) in pass 2 the map g -> k is a bijection onto the row's 8-element
// groups, so each group is read and written by one thread only (not the thread that read it in pass 1: the barrier orders those).
__global__ __launch_bounds__(256) void quantize_rows_w8_kernel(bf16* __restrict__ W, long ldw, signed char* __restrict__ Q, long ldq,
                                                               float* __restrict__ scale, int K) {
    __shared__ float red[4];
    bf16* row = W + (long)blockIdx.x * ldw;
    signed char* qrow = Q + (long)blockIdx.x * ldq;
    float amax = 0.f;
    for (int k = threadIdx.x * 8; k < K; k += 256 * 8) {
        const bf16x8 t = *(const bf16x8*)(row + k);
#pragma unroll
        for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(bf2f(t[i])));
    }
    amax = wave_max(amax);
    if (lane_id() == 0) red[wave_id()] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = amax > 0.f ? amax / 127.f : 1.f;
    if (threadIdx.x == 0) scale[blockIdx.x] = s;
    // packed group g (8 bytes): pair g / 8, lane group (g % 8) / 2, half g % 2 -> k = (2 * pair + half) * 32 + 8 * group
    for (int g = threadIdx.x; g < ldq / 8; g += 256) {
        const int k = (2 * (g >> 3) + (g & 1)) * 32 + ((g & 7) >> 1) * 8;
        unsigned lo = 0u, hi = 0u;
        if (k < K) {
            const bf16x8 t = *(const bf16x8*)(row + k);
            bf16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float q = fminf(fmaxf(rintf(bf2f(t[i]) / s), -127.f), 127.f);
                o[i] = f2bf(q * s);
                const unsigned b = (unsigned)(int)q & 0xffu;
                if (i < 4) lo |= b << (8 * i);
                else hi |= b << (8 * (i - 4));
            }
            *(bf16x8*)(row + k) = o;
        }
        *(u32x2*)(qrow + (long)g * 8) = u32x2{lo, hi};
    }
}

// ------------------------------------------------------------------------------------------------ decode attention
// Block (chunk c, kv head kh, sequence b): keys [c*chunk, min((c+1)*chunk, kv_len[b])) for the G = H / Hkv query heads of kv head kh,
// which share every K / V read.  LPR = HD/8 lanes read one 16-byte slice each of a key row; a wave covers 64/LPR rows per step.
// Writes the chunk's (unnormalised o, running max m, sum l) to part[b][h][c][HD + 2]; attn_decode_combine_kernel merges the chunks.
constexpr int AD_GMAX = 8;
constexpr int AD_CHUNK_MAX = 512;

template <int HD>
__global__ __launch_bounds__(256) void attn_decode_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ cache, long ld_c,
                                                          long bs_c, int v_off, const int* __restrict__ kv_len, int L_max, float* __restrict__ part,
                                                          int H, int Hkv, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    __shared__ float sc[AD_GMAX][AD_CHUNK_MAX];
    __shared__ float ored[4][AD_GMAX][HD];
    __shared__ float mstat[AD_GMAX];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int G = H / Hkv;
    const int nch = gridDim.x;
    const int len = min(kv_len[b], L_max);
    const int j0 = c * chunk;
    if (j0 >= len) return;                     // the combine reads chunks < ceil(len / chunk) only
    const int j1 = min(j0 + chunk, len), n = j1 - j0;
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const bf16* kbase = cache + (long)b * bs_c + kh * HD + li * 8;
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
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)j * ld_c) : zero8();
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
            const bf16x8 vt = *(const bf16x8*)(vbase + (long)j * ld_c);
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

// one block of HD threads per (sequence, q head): chunks merged in chunk order, bf16 out [B, H*HD]
template <int HD>
__global__ __launch_bounds__(HD) void attn_decode_combine_kernel(const float* __restrict__ part, const int* __restrict__ kv_len, int L_max,
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
// torch.argmax semantics over the first n columns: the lowest index among equal maxima, NaN above everything
DEVINL bool am_better(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

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

inline unsigned cdiv(long a, long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

extern "C" int rv_gemv_split(int N, int K) {
    // K slices per column block: enough blocks for >= 2 per CU on 256 CUs, every wave keeps >= 2 of its 32-deep K steps.  A function of
    // (N, K) only, so a row's reduction order never depends on M.
    const long nb = (N + GV_COLS - 1) / GV_COLS, ks = (K + 31) / 32;
    int split = 1;
    while (nb * split < 512 && split < 16 && ks >= (long)split * 2 * 4 * 2) split *= 2;
    return split;
}

extern "C" int rv_gemv_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, void* Y, int64_t ldy, const void* bias, const void* residual,
                            int64_t ldr, int M, int N, int K, int out_f32, void* workspace, int64_t ws_bytes, void* stream) {
    if (!X || !W || !Y || M < 1 || M > 32 || N <= 0 || K <= 0 || (K & 7) || (ldx & 7) || (ldw & 7) || ldx < K || ldw < K || ldy < N ||
        (residual && ldr < N))
        return RV_ERR_ARG;
    const int split = rv_gemv_split(N, K);
    float* part = nullptr;
    if (split > 1) {
        if (!workspace || ws_bytes < (int64_t)split * M * N * 4) return RV_ERR_ARG;
        part = (float*)workspace;
    }
    const dim3 grid(cdiv(N, GV_COLS), split);
    if (M <= 16)
        hipLaunchKernelGGL(gemv_kernel<1>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W, (long)ldw, M, N, K, split, part, Y,
                           (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
    else
        hipLaunchKernelGGL(gemv_kernel<2>, grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)W, (long)ldw, M, N, K, split, part, Y,
                           (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
    if (split > 1)
        hipLaunchKernelGGL(gemv_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, ST, (const float*)part, split, M, N, Y, (long)ldy,
                           (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
    return rv_check_launch();
}

extern "C" int64_t rv_w8_row_bytes(int K) { return (((int64_t)K + 31) / 32 + 1) / 2 * 64; }

extern "C" int rv_quantize_rows_w8_bf16(void* W, int64_t ldw, void* packed, int64_t ldp, float* scale, int N, int K, void* stream) {
    if (!W || !packed || !scale || N <= 0 || K <= 0 || (K & 7) || (ldw & 7) || ldw < K || ldp != rv_w8_row_bytes(K)) return RV_ERR_ARG;
    hipLaunchKernelGGL(quantize_rows_w8_kernel, dim3(N), dim3(256), 0, ST, (bf16*)W, (long)ldw, (signed char*)packed, (long)ldp, scale, K);
    return rv_check_launch();
}

extern "C" int rv_gemv_w8_bf16(const void* X, int64_t ldx, const void* packed, int64_t ldp, const float* scale, void* Y, int64_t ldy,
                               const void* bias, const void* residual, int64_t ldr, int M, int N, int K, int out_f32, void* workspace,
                               int64_t ws_bytes, void* stream) {
    if (!X || !packed || !scale || !Y || M < 1 || M > 32 || N <= 0 || K <= 0 || (K & 7) || (ldx & 7) || ldx < K || ldp != rv_w8_row_bytes(K) ||
        ldy < N || (residual && ldr < N))
        return RV_ERR_ARG;
    const int split = rv_gemv_split(N, K);
    float* part = nullptr;
    if (split > 1) {
        if (!workspace || ws_bytes < (int64_t)split * M * N * 4) return RV_ERR_ARG;
        part = (float*)workspace;
    }
    const dim3 grid(cdiv(N, GV_COLS), split);
    if (M <= 16)
        hipLaunchKernelGGL((gemv_kernel<1, const float*>), grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)packed, (long)ldp, M, N, K,
                           split, part, Y, (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32, scale);
    else
        hipLaunchKernelGGL((gemv_kernel<2, const float*>), grid, dim3(256), 0, ST, (const bf16*)X, (long)ldx, (const bf16*)packed, (long)ldp, M, N, K,
                           split, part, Y, (long)ldy, (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32, scale);
    if (split > 1)
        hipLaunchKernelGGL(gemv_combine_kernel, dim3(cdiv((long)M * N, 256)), dim3(256), 0, ST, (const float*)part, split, M, N, Y, (long)ldy,
                           (const bf16*)bias, (const bf16*)residual, (long)ldr, out_f32);
    return rv_check_launch();
}

extern "C" int rv_attn_decode_bf16(const void* q, int64_t ld_q, const void* cache, int64_t ld_c, int64_t bs_c, int v_off, const int32_t* kv_len,
                                   int L_max, void* out, int64_t ld_o, void* part, int64_t part_bytes, int B, int H, int Hkv, int hd, int chunk,
                                   float scale, void* stream) {
    if (!q || !cache || !kv_len || !out || !part || B <= 0 || Hkv <= 0 || H % Hkv || H / Hkv > AD_GMAX || (hd != 64 && hd != 128) ||
        L_max <= 0 || chunk <= 0 || chunk > AD_CHUNK_MAX || chunk % (hd == 128 ? 16 : 32) || (ld_q & 7) || (ld_c & 7) || (bs_c & 7) ||
        (v_off & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || ld_c < v_off + (int64_t)Hkv * hd || bs_c < (int64_t)L_max * ld_c)
        return RV_ERR_ARG;
    const int nch = (L_max + chunk - 1) / chunk;
    if (part_bytes < (int64_t)B * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    const dim3 grid(nch, Hkv, B);
    if (hd == 128) {
        hipLaunchKernelGGL(attn_decode_kernel<128>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c,
                           v_off, kv_len, L_max, (float*)part, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(B * H), dim3(128), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    } else {
        hipLaunchKernelGGL(attn_decode_kernel<64>, grid, dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)cache, (long)ld_c, (long)bs_c,
                           v_off, kv_len, L_max, (float*)part, H, Hkv, chunk, scale);
        hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(B * H), dim3(64), 0, ST, (const float*)part, kv_len, L_max, (bf16*)out,
                           (long)ld_o, H, nch, chunk);
    }
    return rv_check_launch();
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

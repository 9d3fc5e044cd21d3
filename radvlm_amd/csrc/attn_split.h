// What the seven split-KV cache attention entry points share (flash-decoding style: a block per key chunk writes a partial, a second
// launch merges a row's chunks): rv_attn_decode_bf16 (decode.hip), _beam (beam.hip), _kv8 (kvq.hip), _verify (lookup.hip), _shared
// (prefix.hip), rv_attn_extend_bf16 (extend.hip) and _extend_prefix (score.hip).  Every one of them promises the bits of
// rv_attn_decode_bf16 or rv_attn_extend_bf16 on the same keys, so what is the same statement in two of them is written here once:
//   - the partial layout, the chunk merge and the one combine kernel (all seven);
//   - the register-q body of decode and beam;
//   - the 16-query LDS-q body of verify and shared;
//   - the MFMA body of extend and extend_prefix;
//   - the host routine: argument conditions, nch, the partial buffer's size, the hd dispatch, the combine launch.
// Deliberately not shared: the register-q and the LDS-q body stay two bodies, the int8 kernel keeps its own body (no body is templated
// over the cache format), and each kernel keeps its own prologue.
#pragma once
#include "common.h"

#include <math.h>

#include <type_traits>

constexpr int AD_GMAX = 8;          // query heads per kv head
constexpr int AD_CHUNK_MAX = 512;   // keys per chunk of the decode family (their scores live in LDS)
constexpr int AD_NQ = 16;           // (row, q head) queries per block of the LDS-q body
constexpr int XT_KT = 64;           // extend family: keys per LDS stage
constexpr int XT_GMAX = 8;          // extend family: query heads per kv head
constexpr int XT_MAXRT = 2;         // 16-row MFMA row tiles per wave (row tiles per block <= 8, 4 waves)
constexpr int XT_KPAD = 8;          // LDS row padding (bf16 elements)

// query sub-tiles of 16 rows per extend block: enough (query, head) row tiles for the 4 waves, at most 8 (a function of G alone)
DEVINL __host__ int xt_qs(int G) { return G >= 4 ? 1 : 4 / G; }

// ------------------------------------------------------------------------------------------------ partials and their merge
// part[(row * H + h) * nch + c][HD + 2]: the chunk's unnormalised o[HD], then its running max m, then its sum l
template <int HD>
DEVINL float* split_slot(float* part, long rh, int nch, int c) {
    return part + (rh * nch + c) * (HD + 2);
}

// element dd of a (row, head)'s output from its first nc slots pp: chunks merged in chunk order
template <int HD>
DEVINL float split_merge(const float* pp, int nc, int dd) {
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, pp[c * (HD + 2) + HD]);
    float L = 0.f, o = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float e = expf(pp[c * (HD + 2) + HD] - M);
        L += pp[c * (HD + 2) + HD + 1] * e;
        o += pp[c * (HD + 2) + dd] * e;
    }
    return o / L;
}

// A Rows functor tells the combine how many chunks partial row r owns; none: the row's output is zeros.

// one kv_len per row: decode, beam, kv8, shared
struct RowsKvLen {
    const int* kv_len;
    int L_max;
    DEVINL int operator()(int r, int nch, int chunk) const {
        const int len = min(kv_len[r], L_max);
        return min((len + chunk - 1) / chunk, nch);
    }
};

// verify's staircase: row r = b * R + i sees kv_len0[b] + i keys
struct RowsStair {
    const int* kv_len0;
    int L_max, R;
    DEVINL int operator()(int r, int nch, int chunk) const {
        const int len = min(kv_len0[r / R] + r % R, L_max);
        return min((len + chunk - 1) / chunk, nch);
    }
};

// one block of HD threads per (partial row, q head), bf16 out [rows, H*HD]
template <int HD, class Rows>
__global__ __launch_bounds__(HD) void attn_split_combine_kernel(const float* __restrict__ part, Rows rows, bf16* __restrict__ out, long ld_o,
                                                                int H, int nch, int chunk) {
    const int bh = blockIdx.x, row = bh / H, h = bh % H, dd = threadIdx.x;
    const int nc = rows(row, nch, chunk);
    const float v = split_merge<HD>(part + (long)bh * nch * (HD + 2), nc, dd);
    out[(long)row * ld_o + h * HD + dd] = f2bf(nc > 0 ? v : 0.f);
}

// ------------------------------------------------------------------------------------------------ (a) register-q body: decode, beam
// Block (chunk c, kv head kh, row b) = blockIdx: keys [j0, j1) for the G = H / Hkv query heads of kv head kh, which share every K / V
// read.  LPR = HD/8 lanes read one 16-byte slice each of a key row; a wave covers 64/LPR rows per step.  Writes the chunk's partial of
// every head.
// kb: the cache row that holds every key, or the cache itself when krow(jj), an element offset, picks the row of the chunk's jj-th key
// (beam's ancestry lookup).  The kernel has returned already for a chunk with no keys (j0 >= j1).
template <int HD, class KeyRow>
DEVINL void attn_decode_body(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ kb, long ld_c, int v_off, KeyRow krow, int j0,
                             int j1, float* __restrict__ part, int H, int G, int nch, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    __shared__ float sc[AD_GMAX][AD_CHUNK_MAX];
    __shared__ float ored[4][AD_GMAX][HD];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int n = j1 - j0;
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    const bf16* kbase = kb + kh * HD + li * 8;
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
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + krow(j - j0) + (long)j * ld_c) : zero8();
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
            float* pp = split_slot<HD>(part, (long)b * H + kh * G + g, nch, c);
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
            const bf16x8 vt = *(const bf16x8*)(vbase + krow(j - j0) + (long)j * ld_c);
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
        split_slot<HD>(part, (long)b * H + kh * G + g, nch, c)[dd] = o;
    }
}

// ------------------------------------------------------------------------------------------------ (b) LDS-q body: verify, shared
// Block (chunk c, kv head kh) = blockIdx.x / .y, up to AD_NQ (row, q head of kv head kh) queries.  The kernel's prologue has filled
// nrs[nq] (query nq sees the chunk's first nrs[nq] keys; 0: no such query) and qs[nq] (its q row as fp32), and orow(nq) names the row
// its partial belongs to; queries >= NQ are not looked at by the statistics and the final store.  kbase / vbase: the lane's slice of
// the K / V row at position 0 of the cache row every query reads.  What keeps a query's bits those of attn_decode_body:
//   - key j sits on the same lane (wave w, lane row lr) whatever j1 is, so a lane walks ITS keys in the same ascending order and simply
//     stops earlier for a shorter row: a key the row may not see is skipped (never multiplied by zero; a stale row may hold NaN);
//   - the score of (query, key) does not depend on j1 at all: the 8 products in element order, the xor tree over the LPR lanes, * scale;
//   - m, l: one wave per query, lane-strided over j < nr in ascending order, wave_max / wave_sum -- which wave runs a query is immaterial;
//   - P V: acc += p * v per lane in its key order, the xor tree over the lane rows, waves 0..3 added in order.
// The score loop reads the q rows as LDS broadcasts; the P V accumulators are the register budget: 16 x 8 floats.
template <int HD>
constexpr int AD_NQ_BUF = AD_NQ * AD_CHUNK_MAX > 4 * AD_NQ * HD ? AD_NQ * AD_CHUNK_MAX : 4 * AD_NQ * HD;

template <int HD, class OutRow>
DEVINL void attn_decode_nq_body(const bf16* kbase, const bf16* vbase, long ld_c, float* buf, const float (*qs)[HD], const int* nrs, int NQ,
                                OutRow orow, int j0, int j1, float* __restrict__ part, int H, int G, int chunk, float scale) {
    constexpr int LPR = HD / 8, RPW = 64 / LPR, RPB = 4 * RPW;
    const int c = blockIdx.x, kh = blockIdx.y, nch = gridDim.x;
    const int lane = lane_id(), w = wave_id();
    const int li = lane % LPR, lr = lane / LPR;
    int nr[AD_NQ];
#pragma unroll
    for (int nq = 0; nq < AD_NQ; ++nq) nr[nq] = __builtin_amdgcn_readfirstlane(nrs[nq]);
    // scores
    for (int jb = j0; jb < j1; jb += RPB) {
        const int j = jb + w * RPW + lr;
        const bool ok = j < j1;
        const bf16x8 kt = ok ? *(const bf16x8*)(kbase + (long)j * ld_c) : zero8();
        float kf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kf[i] = bf2f(kt[i]);
#pragma unroll
        for (int nq = 0; nq < AD_NQ; ++nq) {
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
            float* pp = split_slot<HD>(part, orow(nq) * H + kh * G + nq % G, nch, c);
            pp[HD] = m;
            pp[HD + 1] = l;
        }
    }
    __syncthreads();
    // P V
    float acc[AD_NQ][8];
#pragma unroll
    for (int nq = 0; nq < AD_NQ; ++nq)
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
            for (int nq = 0; nq < AD_NQ; ++nq) {
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
    for (int nq = 0; nq < AD_NQ; ++nq) {
        if (nr[nq] > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float a = acc[nq][i];
#pragma unroll
                for (int o = LPR; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
                if (lr == 0) buf[(w * AD_NQ + nq) * HD + li * 8 + i] = a;
            }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < NQ * HD; idx += 256) {
        const int nq = idx / HD, dd = idx % HD;
        if (nrs[nq] <= 0) continue;
        float o = buf[(0 * AD_NQ + nq) * HD + dd];
        o += buf[(1 * AD_NQ + nq) * HD + dd];
        o += buf[(2 * AD_NQ + nq) * HD + dd];
        o += buf[(3 * AD_NQ + nq) * HD + dd];
        split_slot<HD>(part, orow(nq) * H + kh * G + nq % G, nch, c)[dd] = o;
    }
}

// ------------------------------------------------------------------------------------------------ (c) MFMA body: extend, extend_prefix
// Block (chunk c, kv head kh, query tile t = blockIdx.z % tiles) of a sequence whose q_beg (first query row), n_b (query rows), r0
// (position of the first) the kernel has worked out: the keys [c*chunk, (c+1)*chunk) below j_end for one tile of xt_qs * 16 query rows
// times the G query heads of kv head kh, so every K / V tile staged in LDS feeds all of them; chunks past the tile's last key are
// skipped.  Query i sits at position r0 + i and sees the keys [0, r0 + i]; ksrc(j) is the K row of key j at kv head kh (V at + v_off).
// MFMA 16x16x32 (common.h): S = Q K^T with A = Q rows (lane l: row l&15, dims 8(l>>4)..+7 of k-step kk) and B = K^T (lane l: key l&15,
// same dims); P V with A = P (lane l: row l&15, keys 8(l>>4)..+7 of the 32-key step) and B = V (lane l: dim l&15 of the 16-dim tile, same
// keys), read from a transposed LDS image of V.  C/D: lane l, reg r holds [row 4(l>>4) + r][col l&15].
template <int HD, class KeySrc>
DEVINL void attn_extend_body(const bf16* __restrict__ q, long ld_q, KeySrc ksrc, int v_off, int q_beg, int n_b, int r0, int j_end,
                             float* __restrict__ part, int H, int Hkv, int chunk, int nch, int tiles, float scale) {
    constexpr int KS = HD / 32;         // k-steps of Q K^T
    constexpr int DT = HD / 16;         // 16-wide output dim tiles
    __shared__ __attribute__((aligned(16))) bf16 Ks[XT_KT][HD + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Vt[HD][XT_KT + XT_KPAD];
    __shared__ __attribute__((aligned(16))) bf16 Ps[4][XT_MAXRT][16][XT_KT + XT_KPAD];
    const int c = blockIdx.x, kh = blockIdx.y, t = blockIdx.z % tiles;
    const int G = H / Hkv, QS = xt_qs(G), QT = 16 * QS, R = QS * G;
    const int i0 = t * QT;
    if (i0 >= n_b) return;
    const int i_last = min(n_b, i0 + QT) - 1;
    const int j0 = c * chunk;
    const int j1 = min(min(j0 + chunk, r0 + i_last + 1), j_end);
    if (j0 >= j1) return;
    const int lane = lane_id(), w = wave_id();
    const int lc = lane & 15, lh = lane >> 4;

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
                const bf16* src = ksrc(j);
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
    // partials of the rows that own this chunk (c <= pos / chunk)
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
            float* pp = split_slot<HD>(part, (long)(q_beg + i) * H + h, nch, c);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) pp[dt * 16 + lc] = o[k][dt][r];
            if (lc == 0) {
                pp[HD] = m[k][r];
                pp[HD + 1] = lr;
            }
        }
    }
}

// the sequence of extend query row `row`: cu_q[b] <= row < cu_q[b + 1]
DEVINL int xt_seq(const int* __restrict__ cu_q, int B, int row) {
    int b = 0;
    while (b + 1 < B && cu_q[b + 1] <= row) ++b;
    return b;
}

// extend: row `row` of sequence b sits at position rr[b] + row - cu_q[b] and owns the chunks 0 .. pos / chunk
struct RowsExtend {
    const int *cu_q, *rr;
    int B;
    DEVINL int operator()(int row, int nch, int chunk) const {
        const int b = xt_seq(cu_q, B, row);
        const int pos = rr[b] + row - cu_q[b];
        return min(pos / chunk + 1, nch);
    }
};

// ------------------------------------------------------------------------------------------------ host
// a bf16 / int8 cache [rows, L_max, ld_c] with K of kv head g at columns g*hd and V at v_off + g*hd
static inline bool split_cache_ok(const void* cache, int64_t ld_c, int64_t bs_c, int v_off, int Hkv, int hd, int64_t L_max) {
    return cache && !(ld_c & 7) && !(bs_c & 7) && !(v_off & 7) && ld_c >= v_off + (int64_t)Hkv * hd && bs_c >= L_max * ld_c;
}

// the decode family keeps a chunk's scores in LDS and walks it in steps of 4 * 64 / (hd / 8) keys
static inline bool ad_chunk_ok(int chunk, int hd) { return chunk <= AD_CHUNK_MAX && chunk % (hd == 128 ? 16 : 32) == 0; }

// query tiles per sequence of the extend family's grid (nch, Hkv, B * tiles); 0: no such grid, the launcher refuses
static inline int xt_tiles(int B, int max_q, int H, int Hkv) {
    if (B <= 0 || max_q <= 0 || Hkv <= 0 || H < Hkv) return 0;
    const int QT = 16 * xt_qs(H / Hkv);
    const int tiles = (max_q + QT - 1) / QT;
    return (int64_t)B * tiles > 65535 ? 0 : tiles;
}

// Every entry point's launcher.  `ok` is the entry point's own verdict on what only it takes (its caches, index arrays, chunk
// granularity); launch(hd_c, nch) starts its kernel for HD = hd_c() on a grid of nch chunks; `rows` tells the combine about each of the
// n_rows partial rows.  The partial buffer holds n_rows * H * nch slots of hd + 2 floats.
template <class Rows, class Launch>
int attn_split_launch(bool ok, const void* q, int64_t ld_q, void* out, int64_t ld_o, void* part, int64_t part_bytes, int64_t n_rows, int H,
                      int Hkv, int hd, int64_t L_max, int chunk, void* stream, Rows rows, Launch launch) {
    if (!q || !out || !part || n_rows <= 0 || Hkv <= 0 || H % Hkv || H / Hkv > AD_GMAX || (hd != 64 && hd != 128) || L_max <= 0 ||
        L_max > 0x7fffffff || chunk <= 0 || (ld_q & 7) || ld_q < (int64_t)H * hd || ld_o < (int64_t)H * hd || !ok)
        return RV_ERR_ARG;
    const int nch = (int)((L_max + chunk - 1) / chunk);
    if (part_bytes < n_rows * H * nch * (hd + 2) * 4) return RV_ERR_ARG;
    auto run = [&](auto hd_c) {
        constexpr int HD = decltype(hd_c)::value;
        launch(hd_c, nch);
        hipLaunchKernelGGL((attn_split_combine_kernel<HD, Rows>), dim3((unsigned)(n_rows * H)), dim3(HD), 0, ST, (const float*)part, rows,
                           (bf16*)out, (long)ld_o, H, nch, chunk);
    };
    if (hd == 128)
        run(std::integral_constant<int, 128>());
    else
        run(std::integral_constant<int, 64>());
    return rv_check_launch();
}

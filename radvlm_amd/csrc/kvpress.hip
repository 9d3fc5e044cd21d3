// SnapKV prompt-cache compression for gfx950 (Li et al., 2024): rv_kv_votes_f32, rv_kv_select_i32, rv_kv_gather_bf16.  The rule is
// stated once more in tests/kvpress_ref.py (numpy, fp64 sums).  Sequence b has P = cu[b+1] - cu[b] prompt rows; its last w rows are the
// observation window, the n = P - w rows before it the prefix.
//
// (1) votes[b][g][j], j < n: the sum over the G = H / Hkv query heads of kv head g and the w window rows t of
//     softmax_j'(scale * q[h, n + t] . k[j'])[j], row t's softmax over its causal keys [0, n + t], fp32.  Three launches:
//       (a) statistics  grid (key chunk, kv head, sequence), 4 waves.  The chunk's KP_CHUNK = 128 keys -- fixed in absolute position --
//                       are staged once in LDS for all R = w * G <= 512 query rows (row r = head * w + t).  Wave v takes the 16-row
//                       tiles v, v + 4, ...: Q K^T on v_mfma_f32_16x16x32_bf16 (the operand maps of common.h), the causal mask, the
//                       chunk's max m and l = sum exp(s - m) per row to the workspace.
//       (b) merge       one thread per row: M = max_c m_c, L = sum_c l_c * exp(m_c - M), chunks in ascending order.
//       (c) votes       the grid of (a) over the chunks below n: the same staging and the same MFMA sequence give the same scores;
//                       p = exp(s - M) / L is added per lane over the wave's tiles in ascending order and registers 0..3, then the
//                       xor tree over the four 16-lane groups, then waves 0..3 in order through LDS.
//     No atomics; every order above is a function of the sequence's own P, w, G: a sequence has the same bits alone and in any
//     batch.  A key at or past P is never loaded (its LDS row is zeros); a key in (n + t, P) is loaded and gets an exact-zero weight
//     (its score is -inf before the exponential).  V is never read.  Columns [n, ld_v) of votes are not touched.
// (2) keep[b][g][0..N): pooled[j] = max(votes[max(0, j - k/2) .. min(n - 1, j + k/2)]); the N - w prefix positions with the largest
//     pooled value, ties to the lower position, in ascending position order; then the window positions n .. P - 1.  One workgroup
//     per (kv head, sequence).  Non-negative floats order as their bit patterns, so the (N - w)-th largest key is found by a radix
//     select from the top bit down, one bit per sweep, counted with wave ballots and integer adds in LDS -- no atomics, no O(n^2) rank
//     count -- and the kept positions are written by one ordered pass of ballot prefix counts.
// (3) gather: cache row seq[b] * L_max + s takes, in kv head g's K and V columns, the K|V of prompt row keep[b][g][s].
// Sequences with flags[b] == 0 (flags may be null: all are taken) are skipped by every kernel; select and gather also skip P <= N.
#include "common.h"

#include <math.h>

#include <type_traits>

namespace {

constexpr int KP_CHUNK = 128;       // keys per workgroup of the vote kernels
constexpr int KP_NT = KP_CHUNK / 16;
constexpr int KP_WMAX = 64;         // window rows
constexpr int KP_GMAX = 8;          // query heads per kv head
constexpr int KP_KPAD = 8;          // LDS row padding (bf16 elements)

// the chunk's K rows [key][dim] into LDS; keys at or past P read as zeros
template <int HD>
DEVINL void kp_stage(bf16 (*Ks)[HD + KP_KPAD], const bf16* __restrict__ kb, long ld_k, int j0, int P) {
    for (int e = threadIdx.x; e < KP_CHUNK * HD / 8; e += 256) {
        const int key = e / (HD / 8), d8 = (e % (HD / 8)) * 8;
        const int j = j0 + key;
        *(bf16x8*)&Ks[key][d8] = j < P ? *(const bf16x8*)(kb + (long)j * ld_k + d8) : zero8();
    }
}

// S = Q K^T of row tile rt against the staged chunk: sc[nt][reg] = score of row rt * 16 + 4 (lane >> 4) + reg, key nt * 16 + (lane & 15).
// Both vote kernels call this, so they see the same bits.
template <int HD>
DEVINL void kp_scores(f32x4 (&sc)[KP_NT], const bf16 (*Ks)[HD + KP_KPAD], const bf16* __restrict__ qb, long ld_q, int rt, int R, int w,
                      int lc, int lh) {
    constexpr int KS = HD / 32;
    const int r = rt * 16 + lc;
    bf16x8 qf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
        qf[kk] = r < R ? *(const bf16x8*)(qb + (long)(r % w) * ld_q + (r / w) * HD + kk * 32 + lh * 8) : zero8();
#pragma unroll
    for (int nt = 0; nt < KP_NT; ++nt) {
        sc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) sc[nt] = mfma16(qf[kk], *(const bf16x8*)&Ks[nt * 16 + lc][kk * 32 + lh * 8], sc[nt]);
    }
}

struct KpSeq {
    int q_beg, P, n;
};
DEVINL KpSeq kp_seq(const int* __restrict__ cu, int b, int w) {
    const int q_beg = cu[b], P = cu[b + 1] - q_beg;
    return KpSeq{q_beg, P, P - w};
}

// ws: (m, l)[B * Hkv][nch][R], then (M, L)[B * Hkv][R]
DEVINL float* kp_chunk_stats(float* ws, long bg, int nch, int c, int R) { return ws + ((bg * nch + c) * R) * 2; }
DEVINL float* kp_row_stats(float* ws, long BG, long bg, int nch, int R) { return ws + (BG * nch * R + bg * R) * 2; }

template <int HD>
__global__ __launch_bounds__(256) void kv_vote_stats_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ k, long ld_k,
                                                            const int* __restrict__ cu, const int* __restrict__ flags,
                                                            float* __restrict__ ws, int Hkv, int G, int w, int nch, float scale) {
    __shared__ __attribute__((aligned(16))) bf16 Ks[KP_CHUNK][HD + KP_KPAD];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    if (flags && !flags[b]) return;
    const KpSeq s = kp_seq(cu, b, w);
    const int j0 = c * KP_CHUNK;
    if (s.n < 1 || j0 >= s.P) return;
    const int lane = lane_id(), wv = wave_id(), lc = lane & 15, lh = lane >> 4;
    const int R = w * G, NT = (R + 15) / 16;
    kp_stage<HD>(Ks, k + (long)s.q_beg * ld_k + kh * HD, ld_k, j0, s.P);
    __syncthreads();
    const bf16* qb = q + (long)(s.q_beg + s.n) * ld_q + (long)kh * G * HD;
    float* st = kp_chunk_stats(ws, (long)b * Hkv + kh, nch, c, R);
    for (int rt = wv; rt < NT; rt += 4) {
        f32x4 sc[KP_NT];
        kp_scores<HD>(sc, Ks, qb, ld_q, rt, R, w, lc, lh);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = rt * 16 + lh * 4 + reg;
            const int lim = r < R ? s.n + r % w : -1;               // the last key the row sees (< P); padding rows see none
            float mx = -INFINITY;
#pragma unroll
            for (int nt = 0; nt < KP_NT; ++nt) {
                const float v = j0 + nt * 16 + lc <= lim ? sc[nt][reg] * scale : -INFINITY;
                sc[nt][reg] = v;
                mx = fmaxf(mx, v);
            }
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x, 64));
            const float mu = mx == -INFINITY ? 0.f : mx;
            float ps = 0.f;
#pragma unroll
            for (int nt = 0; nt < KP_NT; ++nt) ps += expf(sc[nt][reg] - mu);
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) ps += __shfl_xor(ps, x, 64);
            if (r < R && lc == 0) {
                st[2 * r] = mx;
                st[2 * r + 1] = ps;
            }
        }
    }
}

__global__ __launch_bounds__(256) void kv_vote_merge_kernel(const int* __restrict__ cu, const int* __restrict__ flags, float* __restrict__ ws,
                                                            long BG, int Hkv, int G, int w, int nch) {
    const int r = blockIdx.x * 256 + threadIdx.x, kh = blockIdx.y, b = blockIdx.z;
    const int R = w * G;
    if (r >= R || (flags && !flags[b])) return;
    const KpSeq s = kp_seq(cu, b, w);
    if (s.n < 1) return;
    const int nc = min((s.P + KP_CHUNK - 1) / KP_CHUNK, nch);
    const long bg = (long)b * Hkv + kh;
    float M = -INFINITY;
    for (int c = 0; c < nc; ++c) M = fmaxf(M, kp_chunk_stats(ws, bg, nch, c, R)[2 * r]);
    float L = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float* st = kp_chunk_stats(ws, bg, nch, c, R);
        L += st[2 * r + 1] * expf(st[2 * r] - M);
    }
    float* fin = kp_row_stats(ws, BG, bg, nch, R);
    fin[2 * r] = M;
    fin[2 * r + 1] = L;
}

template <int HD>
__global__ __launch_bounds__(256) void kv_vote_sum_kernel(const bf16* __restrict__ q, long ld_q, const bf16* __restrict__ k, long ld_k,
                                                          const int* __restrict__ cu, const int* __restrict__ flags,
                                                          const float* __restrict__ ws, float* __restrict__ votes, long ld_v, long BG, int Hkv,
                                                          int G, int w, int nch, float scale) {
    __shared__ __attribute__((aligned(16))) bf16 Ks[KP_CHUNK][HD + KP_KPAD];
    __shared__ float part[4][KP_CHUNK];
    const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
    if (flags && !flags[b]) return;
    const KpSeq s = kp_seq(cu, b, w);
    const int j0 = c * KP_CHUNK;
    if (s.n < 1 || j0 >= s.n) return;
    const int lane = lane_id(), wv = wave_id(), lc = lane & 15, lh = lane >> 4;
    const int R = w * G, NT = (R + 15) / 16;
    kp_stage<HD>(Ks, k + (long)s.q_beg * ld_k + kh * HD, ld_k, j0, s.P);
    __syncthreads();
    const bf16* qb = q + (long)(s.q_beg + s.n) * ld_q + (long)kh * G * HD;
    const long bg = (long)b * Hkv + kh;
    const float* fin = kp_row_stats(const_cast<float*>(ws), BG, bg, nch, R);
    float acc[KP_NT];
#pragma unroll
    for (int nt = 0; nt < KP_NT; ++nt) acc[nt] = 0.f;
    for (int rt = wv; rt < NT; rt += 4) {
        f32x4 sc[KP_NT];
        kp_scores<HD>(sc, Ks, qb, ld_q, rt, R, w, lc, lh);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = rt * 16 + lh * 4 + reg;
            const bool ok = r < R;                                  // every real row sees every prefix key: no mask below n
            const float M = ok ? fin[2 * r] : 0.f, L = ok ? fin[2 * r + 1] : 1.f;
#pragma unroll
            for (int nt = 0; nt < KP_NT; ++nt) acc[nt] += ok ? expf(sc[nt][reg] * scale - M) / L : 0.f;
        }
    }
#pragma unroll
    for (int nt = 0; nt < KP_NT; ++nt) {
        acc[nt] += __shfl_xor(acc[nt], 16, 64);
        acc[nt] += __shfl_xor(acc[nt], 32, 64);
        if (lh == 0) part[wv][nt * 16 + lc] = acc[nt];
    }
    __syncthreads();
    const int j = j0 + threadIdx.x;
    if (threadIdx.x < KP_CHUNK && j < s.n && j < ld_v)
        votes[bg * ld_v + j] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ select
// a vote as a sort key: the bit pattern of a non-negative float; a negative value (the votes never are) counts as 0
DEVINL unsigned kp_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? 0u : u;
}

// keys >= x among pk[0, n): thread-strided counts, ballots are not needed for a sum of ints -- the xor tree, then waves 0..3
DEVINL int kp_count_ge(const unsigned* __restrict__ pk, int n, unsigned x, int* red) {
    int cnt = 0;
    for (int j = threadIdx.x; j < n; j += 256) cnt += pk[j] >= x ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = cnt;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void kv_select_kernel(const float* __restrict__ votes, long ld_v, const int* __restrict__ cu,
                                                        const int* __restrict__ flags, unsigned* __restrict__ ws, int* __restrict__ keep,
                                                        int Hkv, int N, int w, int k) {
    __shared__ int red[4];
    __shared__ int wsum[4][2];
    const int kh = blockIdx.x, b = blockIdx.y;
    if (flags && !flags[b]) return;
    const KpSeq s = kp_seq(cu, b, w);
    if (s.P <= N || s.n > ld_v) return;                             // not compressed; or a vote row shorter than the prefix
    const int n = s.n, m = N - w;                                   // 1 <= m < n
    const long bg = (long)b * Hkv + kh;
    const float* v = votes + bg * ld_v;
    unsigned* pk = ws + bg * ld_v;
    int* out = keep + bg * N;
    const int half = k / 2;
    for (int j = threadIdx.x; j < n; j += 256) {
        unsigned mx = kp_key(v[j]);
        for (int d = 1; d <= half; ++d) {
            if (j - d >= 0) mx = max(mx, kp_key(v[j - d]));
            if (j + d < n) mx = max(mx, kp_key(v[j + d]));
        }
        pk[j] = mx;
    }
    __syncthreads();                                                // the workgroup reads its own global writes below
    // T: the m-th largest key = the largest x with count(key >= x) >= m, built from the top bit down (bit 31 is never set)
    unsigned T = 0;
    for (int bit = 30; bit >= 0; --bit) {
        const unsigned cand = T | (1u << bit);
        if (kp_count_ge(pk, n, cand, red) >= m) T = cand;
    }
    const int take_eq = m - kp_count_ge(pk, n, T + 1u, red);        // how many keys equal to T are kept: the lowest positions
    // ordered pass: position j goes to slot (#greater before j) + min(#equal before j, take_eq)
    const int lane = lane_id(), wv = wave_id();
    const unsigned long long below = (1ull << lane) - 1ull;
    int base_g = 0, base_e = 0;
    for (int jb = 0; jb < n; jb += 256) {
        const int j = jb + threadIdx.x;
        const unsigned key = j < n ? pk[j] : 0u;
        const bool gt = j < n && key > T, eq = j < n && key == T;
        const unsigned long long bgm = __ballot(gt), bem = __ballot(eq);
        __syncthreads();
        if (lane == 0) {
            wsum[wv][0] = __popcll(bgm);
            wsum[wv][1] = __popcll(bem);
        }
        __syncthreads();
        int og = base_g, oe = base_e, tg = 0, te = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (x < wv) {
                og += wsum[x][0];
                oe += wsum[x][1];
            }
            tg += wsum[x][0];
            te += wsum[x][1];
        }
        const int ng = og + __popcll(bgm & below), ne = oe + __popcll(bem & below);
        if (gt || (eq && ne < take_eq)) {
            const int slot = ng + min(ne, take_eq);
            if (slot < m) out[slot] = j;
        }
        base_g += tg;
        base_e += te;
    }
    for (int t = threadIdx.x; t < w; t += 256) out[m + t] = n + t;
}

// ------------------------------------------------------------------------------------------------ gather
__global__ __launch_bounds__(256) void kv_gather_kernel(const bf16* __restrict__ kv, long ld_kv, int v_off, const int* __restrict__ cu,
                                                        const int* __restrict__ flags, const int* __restrict__ keep,
                                                        const int* __restrict__ seq, bf16* __restrict__ cache, long ld_c, int L_max,
                                                        int n_rows, int Hkv, int HD, int N) {
    const int sl = blockIdx.x, b = blockIdx.y;
    if (flags && !flags[b]) return;
    const int q_beg = cu[b], P = cu[b + 1] - q_beg;
    const int row = seq[b];
    if (P <= N || row < 0 || row >= n_rows) return;
    bf16* dst = cache + ((long)row * L_max + sl) * ld_c;
    const int per = Hkv * (HD / 8);
    for (int e = threadIdx.x; e < 2 * per; e += 256) {
        const int vpart = e / per, g = (e % per) / (HD / 8), d8 = (e % (HD / 8)) * 8;
        const int j = keep[((long)b * Hkv + g) * N + sl];
        if (j < 0 || j >= P) continue;                             // never a row of another sequence
        const int col = vpart * v_off + g * HD + d8;
        *(bf16x8*)(dst + col) = *(const bf16x8*)(kv + (long)(q_beg + j) * ld_kv + col);
    }
}

static inline bool kp_common_ok(const void* cu, int B, int Hkv, int hd) {
    return cu && B > 0 && B <= 65535 && Hkv > 0 && Hkv <= 65535 && (hd == 64 || hd == 128);
}

}  // namespace

extern "C" int64_t rv_kv_votes_ws_bytes(int B, int H, int Hkv, int w, int max_P) {
    if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || w <= 0 || max_P <= 0) return 0;
    const int64_t R = (int64_t)w * (H / Hkv), nch = (max_P + KP_CHUNK - 1) / KP_CHUNK;
    return (int64_t)B * Hkv * R * (nch + 1) * 2 * 4;
}

extern "C" int rv_kv_votes_f32(const void* q, int64_t ld_q, const void* k, int64_t ld_k, const int32_t* cu, const int32_t* flags, int max_P,
                               void* votes, int64_t ld_v, void* ws, int64_t ws_bytes, int B, int H, int Hkv, int hd, int w, float scale,
                               void* stream) {
    if (!q || !k || !votes || !ws || !kp_common_ok(cu, B, Hkv, hd) || H <= 0 || H % Hkv || H / Hkv > KP_GMAX || w < 1 || w > KP_WMAX ||
        max_P <= w || (ld_q & 7) || ld_q < (int64_t)H * hd || (ld_k & 7) || ld_k < (int64_t)Hkv * hd || !aligned16(q) || !aligned16(k) ||
        ld_v < max_P - w || ws_bytes < rv_kv_votes_ws_bytes(B, H, Hkv, w, max_P))
        return RV_ERR_ARG;
    const int G = H / Hkv, R = w * G;
    const int nch = (max_P + KP_CHUNK - 1) / KP_CHUNK, nchv = (max_P - w + KP_CHUNK - 1) / KP_CHUNK;
    const long BG = (long)B * Hkv;
    auto run = [&](auto hd_c) {
        constexpr int HD = decltype(hd_c)::value;
        hipLaunchKernelGGL(kv_vote_stats_kernel<HD>, dim3(nch, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)k,
                           (long)ld_k, cu, flags, (float*)ws, Hkv, G, w, nch, scale);
        hipLaunchKernelGGL(kv_vote_merge_kernel, dim3(cdiv(R, 256), Hkv, B), dim3(256), 0, ST, cu, flags, (float*)ws, BG, Hkv, G, w, nch);
        hipLaunchKernelGGL(kv_vote_sum_kernel<HD>, dim3(nchv, Hkv, B), dim3(256), 0, ST, (const bf16*)q, (long)ld_q, (const bf16*)k,
                           (long)ld_k, cu, flags, (const float*)ws, (float*)votes, (long)ld_v, BG, Hkv, G, w, nch, scale);
    };
    if (hd == 128)
        run(std::integral_constant<int, 128>());
    else
        run(std::integral_constant<int, 64>());
    return rv_check_launch();
}

extern "C" int64_t rv_kv_select_ws_bytes(int B, int Hkv, int64_t ld_v) {
    if (B <= 0 || Hkv <= 0 || ld_v <= 0) return 0;
    return (int64_t)B * Hkv * ld_v * 4;
}

extern "C" int rv_kv_select_i32(const void* votes, int64_t ld_v, const int32_t* cu, const int32_t* flags, void* keep, void* ws,
                                int64_t ws_bytes, int B, int Hkv, int N, int w, int k, void* stream) {
    if (!votes || !keep || !ws || !cu || B <= 0 || B > 65535 || Hkv <= 0 || Hkv > 65535 || w < 1 || w > KP_WMAX || N <= w || k < 1 ||
        k > 63 || !(k & 1) || ld_v <= 0 || ws_bytes < rv_kv_select_ws_bytes(B, Hkv, ld_v))
        return RV_ERR_ARG;
    hipLaunchKernelGGL(kv_select_kernel, dim3(Hkv, B), dim3(256), 0, ST, (const float*)votes, (long)ld_v, cu, flags, (unsigned*)ws,
                       (int*)keep, Hkv, N, w, k);
    return rv_check_launch();
}

extern "C" int rv_kv_gather_bf16(const void* kv, int64_t ld_kv, int v_off, const int32_t* cu, const int32_t* flags, const int32_t* keep,
                                 const int32_t* seq, void* cache, int64_t ld_c, int L_max, int n_rows, int B, int Hkv, int hd, int N,
                                 void* stream) {
    if (!kv || !keep || !seq || !cache || !kp_common_ok(cu, B, Hkv, hd) || N < 2 || N > L_max || n_rows <= 0 || (v_off & 7) ||
        v_off < (int64_t)Hkv * hd || (ld_kv & 7) || ld_kv < v_off + (int64_t)Hkv * hd || (ld_c & 7) || ld_c < v_off + (int64_t)Hkv * hd ||
        !aligned16(kv) || !aligned16(cache))
        return RV_ERR_ARG;
    hipLaunchKernelGGL(kv_gather_kernel, dim3(N, B), dim3(256), 0, ST, (const bf16*)kv, (long)ld_kv, v_off, cu, flags, keep, seq,
                       (bf16*)cache, (long)ld_c, L_max, n_rows, Hkv, hd, N);
    return rv_check_launch();
}

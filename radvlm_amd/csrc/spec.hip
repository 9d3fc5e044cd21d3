// Speculative sampling's accept / resample step (generate(assistant_model=..., do_sample=True, seed=...); HF: _speculative_sampling,
// Leviathan et al. 2023).  Semantics and the band: include/radvlm_hip.h, rv_spec_accept_rows_f32.
//
// Two launches, and the workgroups of one launch never meet:
//   stats   one workgroup per score row (R target rows and R - 1 draft rows per group): the row's maximum m and whether it is usable
//           (no NaN, no +inf, a finite entry), then Z = sum of rne(exp(s_i - m) * 2^44) over the row as a 64-bit integer, so Z does
//           not depend on the order in which the 1024 threads arrive (<= 2^44 * 262,144 = 2^62).  Both go to the caller's workspace.
//   decide  one workgroup per group.  Every thread walks the drafts (the values are uniform): draft i with id x is accepted iff
//           e_p > 0 and fl(fl(e_q * Zp) * u_a) <= fl(e_p * Zq), e_. = exp(s(x) - m) in float64 of the target's / the draft's row i.
//           Bitwise equal rows give e_p == e_q and Zp == Zq, the two products are then the same double X, and fl(X * u) <= X for
//           u < 1: such a draft is accepted for every seed.  Then the draw at row a = n_accept, with weights w_j = max(0, fl(e_p(j) *
//           Zq) - fl(e_q(j) * Zp)) (the residual; a < R - 1) or w_j = e_p(j) (the bonus row, or a residual that is identically 0).
//           Thread k owns the ids [k * c, (k + 1) * c), c = ceil(n / 1024), and adds their weights in id order; thread 0 adds the 1024
//           chunk sums in chunk order, finds the chunk that holds u_r * S and walks that chunk again in id order.  Every sum is float64
//           in an order fixed by n alone: a group's outputs are the same bits on every launch and whatever the other groups hold.
// No float atomics, no global atomics, no integer wider than 64 bits.  Columns >= n are never read; rows need no alignment.
//
// The band.  Against exact arithmetic on the fp32 scores: exp() in float64 is within 2^-52 relative; a term of Z is rounded by at most
// 1/2 in units of 2^-44 of the row's largest term, so Z (>= 2^44) is within n * 2^-45 <= 2^-27 relative; a product and the multiplication
// by u add 2^-53 each.  The two sides of an accept test, u * Q(x) * (Zp Zq) and P(x) * (Zp Zq), are therefore each within 2^-27 + 2^-50
// relative, and the test can differ from the exact one only where the sides are within delta = 2^-25 of the larger one.  A residual
// draw compares A = sum{P_j : j <= i, P_j > Q_j} + u_r * sum{Q_j : P_j > Q_j} with B = sum{Q_j : j <= i, P_j > Q_j} + u_r * sum{P_j :
// P_j > Q_j}: sums of non-negative terms that each carry the 2^-27 + 2^-50 above, added in float64 over at most 262,144 + 1024 terms
// (<= 2^-34 relative): again it can differ only where |A - B| <= delta * max(A, B).  The draw from P is the case Q = 0.  delta = 2^-25 is
// below the sampler's (depth + 4) * 2^-23.
#include "common.h"
#include "radvlm_hip.h"
#include "sample_rng.h"

#include <math.h>

typedef unsigned long long u64;

namespace {

constexpr int SP_MAX_N = 262144, SP_MAX_R = 32;
constexpr int SP_T = 1024, SP_W = SP_T / 64;
constexpr int SP_ROW_WORDS = 2;                  // per score row in the workspace: (bits of m | unusable << 32), Z
constexpr double SP_FIX = 17592186044416.0;      // 2^44
enum { SP_TAG_DRAW = 0, SP_TAG_ACCEPT = 1 };     // the streams of the resample / bonus draw and of the accept tests

// one rounded product: never contracted into an fma with a neighbouring add, so that equal factors give equal products
DEVINL double sp_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
DEVINL double sp_exp(float s, float m) { return s > -INFINITY ? exp((double)s - (double)m) : 0.0; }

DEVINL u64 sp_shfl_xor64(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}

struct SpRow {
    float m;
    bool bad;
    double Z;
};
DEVINL SpRow sp_row_load(const u64* w) {
    SpRow r;
    r.m = __uint_as_float((unsigned)w[0]);
    r.bad = (w[0] >> 32) != 0;
    r.Z = (double)w[1];
    return r;
}

// row k of group g: the target's rows 0 .. R - 1, then the draft's rows 0 .. R - 2
__global__ __launch_bounds__(SP_T) void spec_stats_kernel(const float* __restrict__ p, long ld_p, const float* __restrict__ q, long ld_q,
                                                          int R, int n, u64* __restrict__ ws) {
    __shared__ float red_m[SP_W];
    __shared__ int red_b[SP_W];
    __shared__ u64 red_z[SP_W];
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int per = 2 * R - 1, g = blockIdx.x / per, k = blockIdx.x % per;
    const float* row = k < R ? p + ((long)g * R + k) * ld_p : q + ((long)g * (R - 1) + (k - R)) * ld_q;
    u64* out = ws + (long)blockIdx.x * SP_ROW_WORDS;

    float m = -INFINITY;
    int bad = 0;
    for (int i = tid; i < n; i += SP_T) {
        const float v = row[i];
        bad |= (v != v) | (v == INFINITY);
        m = fmaxf(m, v);
    }
    m = wave_max(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
    if (lane == 0) { red_m[w] = m; red_b[w] = bad; }
    __syncthreads();
    for (int j = 0; j < SP_W; ++j) {
        m = fmaxf(m, red_m[j]);
        bad |= red_b[j];
    }
    if (bad || !(m > -INFINITY)) {               // NaN, +inf or no finite entry: block-uniform
        if (tid == 0) {
            out[0] = 1ull << 32;
            out[1] = 0;
        }
        return;
    }
    u64 z = 0;
    for (int i = tid; i < n; i += SP_T) z += __double2ull_rn(sp_exp(row[i], m) * SP_FIX);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) z += sp_shfl_xor64(z, o);
    if (lane == 0) red_z[w] = z;
    __syncthreads();
    if (tid == 0) {
        z = 0;
        for (int j = 0; j < SP_W; ++j) z += red_z[j];
        out[0] = (u64)__float_as_uint(m);
        out[1] = z;
    }
}

// the weight of id j in the draw at a row: the residual max(0, P_j - Q_j) up to the factor Zp * Zq, or P_j up to Zp
DEVINL double sp_weight(bool resid, const float* prow, const float* qrow, int j, const SpRow& P, const SpRow& Q) {
#pragma clang fp contract(off)
    const double ep = sp_exp(prow[j], P.m);
    if (!resid) return ep;
    const double d = sp_mul(ep, Q.Z) - sp_mul(sp_exp(qrow[j], Q.m), P.Z);
    return d > 0.0 ? d : 0.0;
}

__global__ __launch_bounds__(SP_T) void spec_decide_kernel(const float* __restrict__ p, long ld_p, const float* __restrict__ q, long ld_q,
                                                           const int32_t* __restrict__ draft, const uint64_t* __restrict__ seed,
                                                           const int32_t* __restrict__ t0, int R, int n, const u64* __restrict__ ws,
                                                           int32_t* __restrict__ n_accept, int64_t* __restrict__ token,
                                                           float* __restrict__ logprob) {
    __shared__ double csum[SP_T];
    __shared__ double shS;
    const int tid = threadIdx.x, g = blockIdx.x;
    const u64* wr = ws + (long)g * (2 * R - 1) * SP_ROW_WORDS;
    const float* pg = p + (long)g * R * ld_p;
    const float* qg = q + (long)g * (R - 1) * ld_q;          // never dereferenced when R == 1
    const uint64_t sd = seed[g];
    const int t = t0[g];

    // the accept tests: every thread computes the same values
    int a = 0;
    for (; a < R - 1; ++a) {
        const SpRow P = sp_row_load(wr + a * SP_ROW_WORDS), Q = sp_row_load(wr + (R + a) * SP_ROW_WORDS);
        if (P.bad || Q.bad) break;
        const int x = draft[(long)g * (R - 1) + a];
        if (x < 0 || x >= n) break;
        const double ep = sp_exp(pg[(long)a * ld_p + x], P.m), eq = sp_exp(qg[(long)a * ld_q + x], Q.m);
        if (!(ep > 0.0)) break;
        const double u = (double)(2ull * sm_uniform24(sd, SP_TAG_ACCEPT, t + a) + 1ull) * 0x1p-25;
        if (!(sp_mul(sp_mul(eq, P.Z), u) <= sp_mul(ep, Q.Z))) break;
    }
    const SpRow P = sp_row_load(wr + a * SP_ROW_WORDS);
    SpRow Q = P;
    bool resid = a < R - 1;
    if (resid) Q = sp_row_load(wr + (R + a) * SP_ROW_WORDS);
    if (P.bad || Q.bad) {                        // an unusable row on the path: the sampler's mark
        if (tid == 0) {
            n_accept[g] = a;
            token[g] = -1;
            logprob[g] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    const float* prow = pg + (long)a * ld_p;
    const float* qrow = resid ? qg + (long)a * ld_q : prow;

    const int chunk = (n + SP_T - 1) / SP_T;
    const int lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    double S;
    for (;;) {
        double s = 0.0;
        for (int j = lo; j < hi; ++j) s += sp_weight(resid, prow, qrow, j, P, Q);
        csum[tid] = s;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int k = 0; k < SP_T; ++k) tot += csum[k];
            shS = tot;
        }
        __syncthreads();
        S = shS;
        if (S > 0.0 || !resid) break;
        resid = false;                           // P <= Q everywhere it matters: HF falls back to P
    }
    if (tid != 0) return;
    int64_t tok = -1;
    if (S > 0.0) {
        const double target = (double)(2ull * sm_uniform24(sd, SP_TAG_DRAW, t + a) + 1ull) * 0x1p-25 * S;
        // the chunk that holds the target; a sum that rounding left at or below it ends in the last chunk with any weight
        int sel = -1, last = -1;
        double acc = 0.0, last_base = 0.0;
        for (int k = 0; k < SP_T; ++k) {
            if (!(csum[k] > 0.0)) continue;
            last = k;
            last_base = acc;
            if (acc + csum[k] > target) { sel = k; break; }
            acc += csum[k];
        }
        if (sel < 0) { sel = last; acc = last_base; }
        const int c0 = sel * chunk, c1 = c0 + chunk < n ? c0 + chunk : n;
        int lastj = -1;
        for (int j = c0; j < c1; ++j) {
            const double wgt = sp_weight(resid, prow, qrow, j, P, Q);
            if (!(wgt > 0.0)) continue;
            lastj = j;
            acc += wgt;
            if (acc > target) break;
        }
        tok = lastj;
    }
    n_accept[g] = a;
    token[g] = tok;
    float lp = __uint_as_float(0x7fc00000u);
    if (tok >= 0) lp = (float)(((double)prow[tok] - (double)P.m) - (log(P.Z) - 44.0 * 0.69314718055994530942));
    logprob[g] = lp;
}

}  // namespace

extern "C" int64_t rv_spec_ws_bytes(int groups, int R) {
    return groups > 0 && R >= 1 && R <= SP_MAX_R ? (int64_t)groups * (2 * R - 1) * SP_ROW_WORDS * 8 : 0;
}

extern "C" int rv_spec_accept_rows_f32(const float* p, int64_t ld_p, const float* q, int64_t ld_q, const int32_t* draft, const uint64_t* seed,
                                       const int32_t* t0, int groups, int R, int n, int32_t* n_accept, int64_t* token, float* logprob,
                                       void* ws, int64_t ws_bytes, void* stream) {
    if (!p || !seed || !t0 || !n_accept || !token || !logprob || groups <= 0 || R < 1 || R > SP_MAX_R || n <= 0 || n > SP_MAX_N || ld_p < n ||
        (reinterpret_cast<uintptr_t>(p) & 3u) || !ws || (reinterpret_cast<uintptr_t>(ws) & 7u) || ws_bytes < rv_spec_ws_bytes(groups, R))
        return RV_ERR_ARG;
    if (R > 1 && (!q || !draft || ld_q < n || (reinterpret_cast<uintptr_t>(q) & 3u))) return RV_ERR_ARG;
    hipLaunchKernelGGL(spec_stats_kernel, dim3(groups * (2 * R - 1)), dim3(SP_T), 0, ST, p, (long)ld_p, q, (long)ld_q, R, n, (u64*)ws);
    hipLaunchKernelGGL(spec_decide_kernel, dim3(groups), dim3(SP_T), 0, ST, p, (long)ld_p, q, (long)ld_q, draft, seed, t0, R, n,
                       (const u64*)ws, n_accept, token, logprob);
    return rv_check_launch();
}

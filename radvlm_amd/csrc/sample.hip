// Seeded sampling of one token per fp32 score row (generate(do_sample=True, seed=...)): HF's warpers temperature -> top-k -> top-p ->
// min-p, then one counter-based draw.  Semantics: include/radvlm_hip.h, rv_sample_rows_f32.
//
// A row is shared by SM_G = 8 workgroups of 16 waves, each with a fixed run of the row's 256-entry tiles, and every sweep below is
// a launch of its own: the workgroups of a row meet only at launch boundaries.  Each leaves its partial result (a maximum, 256 integer
// bins) in a slot of its own in the caller's workspace, and every workgroup of the next launch merges the 8 partials in the order
// g = 0 .. 7.  No sort, no float atomics, no global atomics, no float sum whose order could vary: a row's token, written scores and
// logprob are the same bits on every launch and whatever else shares the launch.
//
//   s_i = x_i / T (IEEE fp32 division), key_i = the order-preserving uint32 image of s_i (-0 counted as +0).  Every warper becomes a
//   threshold: entry i is kept iff key_i >= K and s_i - m >= log(min_p), m = max s.
//   sweep 1          max key; NaN anywhere, m = +inf or m = -inf: the row is unusable, out = -1, nothing else runs.
//   top-k (4 sweeps) radix select, 8 bits per sweep from the top: integer LDS histograms (16 interleaved copies per bin, so the lanes of
//                    a wave that hit one bin spread over 16 banks), the smallest key with #{key <= it} > n - k.  Exact.
//   top-p (4 sweeps) the same descent over the entries top-k left, each weighted with its mass in 64-bit fixed point,
//                    f_i = rne(exp(s_i - m) * 2^40): integer LDS adds, so a bin's mass does not depend on the order of arrival.  The
//                    first sweep's bins also give Z = sum f; the threshold is the smallest key with sum{f_j : key_j <= it} > (1 - top_p) Z,
//                    so equal scores at the cut are all kept.
//   last sweep       kept entries' f summed per 256-entry tile in id order (a wave reduction of integers); with write_scores the warped
//                    row is written (s_i or -inf).  Then a launch of one wave per row scans the <= 1025 tile sums, finds the tile that holds
//                    floor(u * Z_kept) and scans that tile again: the token is the lowest id whose inclusive integer sum exceeds it.
//   A warper that is off (top_k = 0 or >= n, top_p = 1, min_p = 0) costs no sweep: 2 sweeps at least, 10 with everything on, and one more launch for the draw.
//
// depth = 1.  The CDF sum itself is integer: no fp32 addition, whatever the length of the row.  The one fp32 addition a term passes
// through is the fma that applies the rounding residual of s_i - m to exp(): d = fl(s - m), r = (s - m) - d exactly (TwoSum),
// e = fma(expf(d), r, expf(d)).  Error of a normalised partial sum C / Z against exact arithmetic on the fp32 s: each term carries
// <= 2^-23 (expf, <= 1 ulp) + 2^-24 (the fma) relative, which enters C and Z alike (<= 3 * 2^-23 on the quotient), and the fixed-point
// rounding is <= 2^-41 per term, <= 2^-23 of Z (>= 2^40) over 262,144 terms, in C and in Z: <= 5 * 2^-23 = (depth + 4) * 2^-23.
#include "common.h"
#include "radvlm_hip.h"
#include "sample_rng.h"

#include <math.h>

typedef unsigned long long u64;

namespace {

constexpr int SM_MAX_N = 262144;                 // as the logits-processor kernels
constexpr int SM_G = 8;                          // workgroups that share a row
constexpr int SM_T = 1024, SM_W = SM_T / 64;
constexpr int SM_U = 4;                          // tiles a wave has in flight: few workgroups stream the row, so a sweep is latency-bound
constexpr int SM_TILE = 256;                     // entries per tile: one float4 per lane
constexpr int SM_REP = 16;                       // interleaved copies of each histogram bin
constexpr int SM_PER_LANE = 17;                  // tile sums a lane of the last scan owns
constexpr int SM_TILES_CAP = 64 * SM_PER_LANE;   // >= (SM_MAX_N + 3 + 255) / 256 = 1025

DEVINL unsigned sm_key(float s) {
    const unsigned u = __float_as_uint(s + 0.0f);                // -0 -> +0: equal scores get equal keys
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVINL float sm_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// exp(s - m) for d = fl(s - m) > -inf, with the subtraction's rounding residual applied; err returns the residual
DEVINL float sm_exp(float s, float m, float d, float& err) {
    const float nm = -m, bb = d - s;
    err = (s - (d - bb)) + (nm - bb);
    const float e = expf(d);
    return fmaf(e, err, e);
}
DEVINL u64 sm_fix(float e) { return __float2ull_rn(e * 1099511627776.0f); }     // * 2^40

DEVINL u64 shfl64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
DEVINL u64 shfl_xor64(u64 v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}
DEVINL u64 shfl_up64(u64 v, int o) {
    const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}
DEVINL u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
    return v;
}
DEVINL u64 wave_scan64(u64 v) {                  // inclusive, lanes in order
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = shfl_up64(v, o);
        if (lane_id() >= o) v += t;
    }
    return v;
}

// A row seen through 16-byte loads: rowa is the row's address rounded down to 16 bytes, entry id sits at index id + a of it, the valid
// indices are [a, end).  Nothing outside them is read or written.
struct SmRow {
    const float* rowa;
    float* wrow;
    int a, end, ntiles, tlo, thi;                // this workgroup's tiles are [tlo, thi)
    float T;
};

// the four entries at indices i0 .. i0 + 3 (i0 % 4 == 0) divided by T; returns the mask of the valid ones
DEVINL unsigned sm_load4(const SmRow& R, int i0, float v[4]) {
    unsigned ok = 0;
    if (i0 >= R.a && i0 + 4 <= R.end) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(R.rowa + i0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        ok = 15u;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + c;
            const bool in = i >= R.a && i < R.end;
            v[c] = 0.f;
            if (in) v[c] = R.rowa[i];
            ok |= (in ? 1u : 0u) << c;
        }
    }
    if (R.T != 1.0f) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = v[c] / R.T;
    }
    return ok;
}

// f(tile, i0, v, ok) for every tile in [tlo, thi); wave w takes tiles tlo + w, tlo + w + 16, ...; the call is wave-uniform
template <class F>
DEVINL void sm_sweep(const SmRow& R, F&& f) {
    const int w = wave_id(), lane = lane_id();
    for (int t0 = R.tlo + w; t0 < R.thi; t0 += SM_W * SM_U) {
        float v[SM_U][4];
        unsigned ok[SM_U];
#pragma unroll
        for (int u = 0; u < SM_U; ++u) {
            const int tl = t0 + u * SM_W;
            ok[u] = 0;
            if (tl < R.thi) ok[u] = sm_load4(R, tl * SM_TILE + lane * 4, v[u]);
        }
#pragma unroll
        for (int u = 0; u < SM_U; ++u) {
            const int tl = t0 + u * SM_W;
            if (tl < R.thi) f(tl, tl * SM_TILE + lane * 4, v[u], ok[u]);
        }
    }
}

// What one launch does to its share of the row.  A launch first resolves what the launch before it left in the workspace.
enum { SM_NONE = 0, SM_MAX = 1, SM_KSEL = 2, SM_PSEL = 3, SM_FINAL = 4 };

// Per row, in 8-byte words: SM_SLOTS states of 4 words (the state launch p worked with sits in slot p), the SM_G partial maxima, two
// sets (launches alternate) of SM_G partial histograms of 256 bins, the tile sums.  Nothing of it needs to be zeroed: every word is
// written by one launch before a later one reads it.
constexpr int SM_SLOTS = 12;                     // >= 10 launches: max, 4 + 4 radix passes, the tile sums
constexpr int SM_WS_STATE = 0, SM_WS_MAXP = SM_WS_STATE + 4 * SM_SLOTS, SM_WS_HIST = SM_WS_MAXP + SM_G,
              SM_WS_TSUM = SM_WS_HIST + 2 * SM_G * 256, SM_WS_WORDS = SM_WS_TSUM + SM_TILES_CAP;

struct SmState {
    unsigned kmax, bad, prefix, K;
    u64 below, L;
};
DEVINL SmState sm_state_load(const u64* st) {
    SmState S;
    const u64 a = st[0], b = st[1];
    S.kmax = (unsigned)a; S.bad = (unsigned)(a >> 32); S.prefix = (unsigned)b; S.K = (unsigned)(b >> 32);
    S.below = st[2]; S.L = st[3];
    return S;
}
DEVINL void sm_state_store(u64* st, const SmState& S) {
    st[0] = (u64)S.kmax | ((u64)S.bad << 32);
    st[1] = (u64)S.prefix | ((u64)S.K << 32);
    st[2] = S.below;
    st[3] = S.L;
}
DEVINL void sm_row(SmRow& R, float* row, int n, float T) {
    R.a = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
    R.rowa = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(row) - 4u * (uintptr_t)R.a);
    R.wrow = reinterpret_cast<float*>(reinterpret_cast<uintptr_t>(row) - 4u * (uintptr_t)R.a);
    R.end = n + R.a;
    R.ntiles = (R.end + SM_TILE - 1) / SM_TILE;
    R.T = T;
    R.tlo = 0;
    R.thi = R.ntiles;
}

// One pass of the sampler over a row that SM_G workgroups share: workgroup g of a row owns a fixed run of its tiles.  The workgroups
// of a row meet only at launch boundaries: each leaves its partial result (a maximum, 256 integer bins) in a place of its own, and
// every workgroup of the next launch adds the SM_G partials in the order g = 0 .. SM_G - 1 (integers, so the order is a formality).
__global__ __launch_bounds__(SM_T) void sample_pass_kernel(float* x, long ld, int n, float T, int top_k, double frac, float min_p,
                                                           int write_scores, u64* __restrict__ ws, int p, int cur, int lvl, int prev,
                                                           int plvl) {
    __shared__ u64 hist[256 * SM_REP];
    __shared__ u64 tot[256];
    __shared__ SmState shS;
    __shared__ unsigned red_k[SM_W];
    __shared__ int red_b[SM_W];
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int r = blockIdx.x / SM_G, g = blockIdx.x % SM_G;
    u64* wr = ws + (long)r * SM_WS_WORDS;
    SmRow R;
    sm_row(R, x + (long)r * ld, n, T);
    const int chunk = (R.ntiles + SM_G - 1) / SM_G;
    R.tlo = g * chunk < R.ntiles ? g * chunk : R.ntiles;
    R.thi = R.tlo + chunk < R.ntiles ? R.tlo + chunk : R.ntiles;

    // resolve the launch before this one
    SmState S = {0u, 0u, 0u, 0u, 0ull, 0ull};
    if (p > 0) S = sm_state_load(wr + SM_WS_STATE + 4 * (p - 1));
    if (prev == SM_MAX) {
        for (int k = 0; k < SM_G; ++k) {
            const u64 v = wr[SM_WS_MAXP + k];
            S.kmax = (unsigned)v > S.kmax ? (unsigned)v : S.kmax;
            S.bad |= (unsigned)(v >> 32);
        }
    } else if (prev == SM_KSEL || prev == SM_PSEL) {
        const u64* part = wr + SM_WS_HIST + ((p - 1) & 1) * SM_G * 256;
        if (tid < 256) {
            u64 s = 0;
            for (int k = 0; k < SM_G; ++k) s += part[k * 256 + tid];
            tot[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            if (plvl == 0) {
                S.prefix = 0;
                S.below = 0;
                S.L = (u64)(n - top_k);
                if (prev == SM_PSEL) {
                    u64 Z = 0;
                    for (int b = 0; b < 256; ++b) Z += tot[b];
                    S.L = (u64)(frac * (double)Z);
                    if (Z > 0 && S.L >= Z) S.L = Z - 1;          // min_tokens_to_keep = 1: the maximum stays
                }
            }
            u64 acc = S.below;
            unsigned sel = 255;
            for (int b = 0; b < 256; ++b) {
                const u64 nx = acc + tot[b];
                if (nx > S.L) { sel = b; break; }
                acc = nx;
            }
            S.prefix = (S.prefix << 8) | sel;
            S.below = acc;
            if (plvl == 3) {                                     // the threshold of this warper; the later one can only raise it
                S.K = S.prefix > S.K ? S.prefix : S.K;
                S.prefix = 0;
            }
            shS = S;
        }
        __syncthreads();
        S = shS;
    }
    if (g == 0 && tid == 0) sm_state_store(wr + SM_WS_STATE + 4 * p, S);
    const float m = sm_unkey(S.kmax);
    if (cur != SM_MAX && (S.bad || !(fabsf(m) < INFINITY))) return;      // NaN, +inf or no finite entry: the draw writes -1

    if (cur == SM_MAX) {
        unsigned kmax = 0;
        int bad = 0;
        sm_sweep(R, [&](int, int, const float* v, unsigned ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((ok >> c) & 1u) {
                    bad |= v[c] != v[c];
                    const unsigned k = sm_key(v[c]);
                    kmax = k > kmax ? k : kmax;
                }
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned ok = __shfl_xor(kmax, o, 64);
            kmax = ok > kmax ? ok : kmax;
            bad |= __shfl_xor(bad, o, 64);
        }
        if (lane == 0) { red_k[w] = kmax; red_b[w] = bad; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < SM_W; ++k) {
                kmax = red_k[k] > kmax ? red_k[k] : kmax;
                bad |= red_b[k];
            }
            wr[SM_WS_MAXP + g] = (u64)kmax | ((u64)(bad ? 1u : 0u) << 32);
        }
    } else if (cur == SM_KSEL || cur == SM_PSEL) {
        // one level of the radix select, 8 bits from the top: the weight (1, or the fixed-point mass) of this workgroup's entries per bin
        const bool mass = cur == SM_PSEL;
        const int shift = 24 - 8 * lvl, rep = tid & (SM_REP - 1);
        const unsigned kmin = mass ? S.K : 0u, prefix = S.prefix;
        for (int i = tid; i < 256 * SM_REP; i += SM_T) hist[i] = 0;
        __syncthreads();
        sm_sweep(R, [&](int, int, const float* v, unsigned ok) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!((ok >> c) & 1u)) continue;
                const unsigned key = sm_key(v[c]);
                if (key < kmin) continue;
                if (lvl > 0 && (key >> (shift + 8)) != prefix) continue;
                u64 wgt = 1;
                if (mass) {
                    const float d = v[c] - m;
                    if (!(d > -INFINITY)) continue;
                    float err;
                    wgt = sm_fix(sm_exp(v[c], m, d, err));
                    if (wgt == 0) continue;
                }
                atomicAdd(&hist[((key >> shift) & 255u) * SM_REP + rep], wgt);
            }
        });
        __syncthreads();
        if (tid < 256) {
            u64 s = 0;
#pragma unroll
            for (int c = 0; c < SM_REP; ++c) s += hist[tid * SM_REP + c];
            wr[SM_WS_HIST + ((p & 1) * SM_G + g) * 256 + tid] = s;
        }
    } else {
        // SM_FINAL: kept mass per tile, the warped row
        const unsigned K = S.K > S.kmax ? S.kmax : S.K;          // the maximum is kept whatever happened above
        const float dmin = min_p > 0.f ? (float)log((double)min_p) : -INFINITY;
        sm_sweep(R, [&](int tl, int i0, const float* v, unsigned ok) {
            u64 s = 0;
            float o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                o[c] = -INFINITY;
                if (!((ok >> c) & 1u)) continue;
                const float d = v[c] - m;
                if (sm_key(v[c]) >= K && d >= dmin) {
                    o[c] = v[c];
                    if (d > -INFINITY) {
                        float err;
                        s += sm_fix(sm_exp(v[c], m, d, err));
                    }
                }
            }
            s = wave_sum64(s);
            if (lane == 0) wr[SM_WS_TSUM + tl] = s;
            if (write_scores) {
                if (ok == 15u) {
                    f32x4 q;
                    q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
                    *reinterpret_cast<f32x4*>(R.wrow + i0) = q;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if ((ok >> c) & 1u) R.wrow[i0 + c] = o[c];
                }
            }
        });
    }
}

// The draw: one wave per row over the tile sums the last pass left; pf is that pass's launch index
__global__ __launch_bounds__(64) void sample_draw_kernel(float* x, long ld, int n, const uint64_t* __restrict__ seed,
                                                         const int32_t* __restrict__ tv, float T, float min_p, int write_scores,
                                                         const u64* __restrict__ ws, int pf, int64_t* __restrict__ out,
                                                         float* __restrict__ logprob, uint64_t tag) {
    const int lane = lane_id();
    const u64* wr = ws + (long)blockIdx.x * SM_WS_WORDS;
    const u64* tsum = wr + SM_WS_TSUM;
    SmRow R;
    sm_row(R, x + (long)blockIdx.x * ld, n, T);
    const SmState S = sm_state_load(wr + SM_WS_STATE + 4 * pf);
    const float m = sm_unkey(S.kmax);
    if (S.bad || !(fabsf(m) < INFINITY)) {
        if (lane == 0) {
            out[blockIdx.x] = -1;
            if (logprob) logprob[blockIdx.x] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    const unsigned K = S.K > S.kmax ? S.kmax : S.K;
    // min-p: p_i < min_p * p_max  <=>  s_i - m < log(min_p); the compare is on fl(s_i - m), which is monotone in s_i
    const float dmin = min_p > 0.f ? (float)log((double)min_p) : -INFINITY;

    // lane l owns tile sums [l * per, (l + 1) * per)
    const int per = (R.ntiles + 63) / 64;
    u64 ls = 0;
    for (int j = 0; j < per; ++j) {
        const int tl = lane * per + j;
        if (tl < R.ntiles) ls += tsum[tl];
    }
    const u64 inc = wave_scan64(ls);
    const u64 Z = shfl64(inc, 63);
    const u64 r2 = 2ull * sm_uniform24(seed[blockIdx.x], tag, tv[blockIdx.x]) + 1ull;      // u = r2 * 2^-25
    const u64 target = (__umul64hi(r2, Z) << 39) | ((r2 * Z) >> 25);                   // floor(u * Z) < Z
    const bool mine = (inc - ls) <= target && target < inc;
    const u64 owner = __ballot(mine);
    if (owner == 0) {                            // Z == 0 cannot happen (the maximum has mass 2^40); never index with a lane of -1
        if (lane == 0) {
            out[blockIdx.x] = -1;
            if (logprob) logprob[blockIdx.x] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    int sel = 0;
    u64 base = 0;
    if (mine) {
        u64 acc = inc - ls;
        for (int j = 0; j < per; ++j) {
            const int tl = lane * per + j;
            if (tl >= R.ntiles) break;
            const u64 nx = acc + tsum[tl];
            if (nx > target) { sel = tl; break; }
            acc = nx;
        }
        base = acc;
    }
    const int src = __ffsll((long long)owner) - 1;
    sel = __shfl(sel, src, 64);
    base = shfl64(base, src);

    // the tile that holds the target, again; after write_scores it already holds s (or -inf where removed, which stays removed)
    if (write_scores) R.T = 1.0f;
    float v[4], dd[4], ee[4];
    u64 f[4];
    const int i0 = sel * SM_TILE + lane * 4;
    const unsigned ok = sm_load4(R, i0, v);
    u64 lsum = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f[c] = 0;
        dd[c] = ee[c] = 0.f;
        if (!((ok >> c) & 1u)) continue;
        const float d = v[c] - m;
        if (sm_key(v[c]) >= K && d >= dmin && d > -INFINITY) {
            f[c] = sm_fix(sm_exp(v[c], m, d, ee[c]));
            dd[c] = d;
        }
        lsum += f[c];
    }
    const u64 linc = base + wave_scan64(lsum);
    const u64 hit = __ballot(linc > target);
    if (hit == 0) {
        if (lane == 0) {
            out[blockIdx.x] = -1;
            if (logprob) logprob[blockIdx.x] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    if (lane == __ffsll((long long)hit) - 1) {
        u64 acc = linc - lsum;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc += f[c];
            if (acc > target) {
                out[blockIdx.x] = (int64_t)(i0 + c - R.a);
                if (logprob)
                    logprob[blockIdx.x] = (float)((double)dd[c] + (double)ee[c] - (log((double)Z) - 40.0 * 0.69314718055994530942));
                break;
            }
        }
    }
}

}  // namespace

extern "C" uint32_t rv_sample_uniform24(uint64_t seed, int32_t t) { return sm_uniform24(seed, 0, t); }
extern "C" uint32_t rv_sample_uniform24_tagged(uint64_t seed, int32_t tag, int32_t t) { return sm_uniform24(seed, (uint64_t)(int64_t)tag, t); }

extern "C" int64_t rv_sample_ws_bytes(int rows) { return rows > 0 ? (int64_t)rows * SM_WS_WORDS * 8 : 0; }

extern "C" int rv_sample_rows_tagged_f32(float* x, int64_t ld, int rows, int n, const uint64_t* seed, const int32_t* t, int32_t tag,
                                         float temperature, int top_k, float top_p, float min_p, int write_scores, int64_t* out,
                                         float* logprob, void* ws, int64_t ws_bytes, void* stream) {
    if (!x || !seed || !t || !out || rows <= 0 || n <= 0 || n > SM_MAX_N || ld < n || (reinterpret_cast<uintptr_t>(x) & 3u) || tag < 0 ||
        !(temperature > 0.f) || !(temperature < INFINITY) || top_k < 0 || !(top_p >= 0.f && top_p <= 1.f) || !(min_p >= 0.f && min_p <= 1.f) ||
        !ws || (reinterpret_cast<uintptr_t>(ws) & 7u) || ws_bytes < rv_sample_ws_bytes(rows))
        return RV_ERR_ARG;
    const double frac = 1.0 - (double)top_p;
    int p = 0, prev = SM_NONE, plvl = 0;
    auto pass = [&](int cur, int lvl) {
        hipLaunchKernelGGL(sample_pass_kernel, dim3(rows * SM_G), dim3(SM_T), 0, ST, x, (long)ld, n, temperature, top_k, frac, min_p,
                           write_scores, (u64*)ws, p, cur, lvl, prev, plvl);
        prev = cur;
        plvl = lvl;
        ++p;
    };
    pass(SM_MAX, 0);
    if (top_k > 0 && top_k < n)
        for (int l = 0; l < 4; ++l) pass(SM_KSEL, l);
    if (top_p < 1.0f)
        for (int l = 0; l < 4; ++l) pass(SM_PSEL, l);
    pass(SM_FINAL, 0);
    hipLaunchKernelGGL(sample_draw_kernel, dim3(rows), dim3(64), 0, ST, x, (long)ld, n, seed, t, temperature, min_p, write_scores,
                       (const u64*)ws, p - 1, out, logprob, (uint64_t)tag);
    return rv_check_launch();
}

extern "C" int rv_sample_rows_f32(float* x, int64_t ld, int rows, int n, const uint64_t* seed, const int32_t* t, float temperature, int top_k,
                                  float top_p, float min_p, int write_scores, int64_t* out, float* logprob, void* ws, int64_t ws_bytes,
                                  void* stream) {
    return rv_sample_rows_tagged_f32(x, ld, rows, n, seed, t, 0, temperature, top_k, top_p, min_p, write_scores, out, logprob, ws, ws_bytes,
                                     stream);
}

// DoLa ("decoding by contrasting layers", HF: _dola_decoding / _dola_select_contrast / _relative_top_filter) for gfx950: the kernel that
// turns the raw fp32 logits row f of the last layer and the rows c_1 .. c_N of N earlier layers (lm_head of their hidden states, no
// final norm) into the contrasted score row, in place on f.  With lf, lq_k the bits rv_log_softmax_rows_f32 gives the rows
// (log_softmax.h: the same statements), per row:
//   layer choice   N == 1: the only candidate.  Otherwise p = exp(lf), q = exp(lq_k), M = (p + q) / 2 and
//                      J_k = 0.5 * mean_v T_v,   T_v = M ((log M - lf) + (log M - lq_k))        (the Jensen-Shannon divergence)
//                  and the chosen candidate is argmax_k J_k, an exact tie going to the lower k.  Every row chooses for itself (HF
//                  averages J over the batch first; at one row the two agree).
//   contrast       thresh = fl(-Lf + log_rt)  (max lf = fl(0 - Lf) = -Lf, log_rt = fl32(ln relative_top) from the host);
//                  out_v = -inf where lf_v < thresh, else fl(lf_v - lb_v) with lb the chosen candidate's log-softmax: one rounding on
//                  the log-softmax kernel's bits, compiled under `#pragma clang fp contract(off)` like cfg.hip's statement (nothing
//                  here multiplies, but the pragma keeps it so).  The row maximum always survives the filter.
// T_v is written as M * ((log M - lf) + (log M - lq)), not xlogy(M, M) - M lf: the second form cancels.  It is evaluated in fp32 with
// __expf / __logf (v_exp_f32 / v_log_f32 inside) and a term with M below FLT_MIN counts as 0: the true term is below 2^-118 there,
// and nothing then rests on what the two instructions do with subnormals.  The sum over v is fp64 in a fixed order: per thread in index
// order, lanes by xor butterfly, waves 0..3, then the row's DL_PIECE-column pieces in piece order.  So J_k depends on the two rows
// alone -- not on `rows`, the grid or the other candidates -- and there are no atomics.  Non-finite logits are outside the contract;
// they cannot fault: `chosen` is always an index below n_layers (comparisons with NaN keep the lower index).
//
// Launch structure (one form, so there is nothing to keep bit-identical with): four launches,
//   stats    one workgroup per (layer, row), layer 0 = f: (m, L) by log_softmax.h's device functions into ws
//   jsd      one workgroup per (piece, candidate, row): the fp64 partial sum of T over DL_PIECE columns into ws       (N > 1 only)
//   select   one wave per row: the pieces added in piece order, J_k, the argmax; writes chosen and (optionally) jsd
//   contrast one workgroup per (DL_EW columns, row): the filter and the subtraction, f overwritten
// A 152,064-entry row swept by one workgroup is bound by one compute unit's load latency (cfg.hip measured that), hence the pieces.
//
// Error of J_k against exact arithmetic on the fp32 inputs, u = 2^-24, V = n, rows of finite entries.  Inputs: beam.hip derives
// |l^ - l| <= E(l) = u (2 |l| + 4 ln V + 3) for a computed log-softmax entry.  Instructions, as this build's ISA holds them: __expf is
// v_mul_f32 by log2(e) and v_exp_f32; __logf is v_log_f32 and the product with ln 2 carried in two parts through three fmas (plus a
// 2^32 prescale of inputs below FLT_MIN, which the guard above never lets through).  Taking the ISA manual's 1 ulp for v_exp_f32 and
// v_log_f32:
//   p^ = exp(l^ + e),  |e| <= X(l) = u (|l| + 2)                 the argument's product rounding (|l| u) and 1 ulp = 2u of the result
//   |log^ M^ - log M^| <= 4 u |log M|                              1 ulp of log2 (2u |log M|); the two-part product adds less than 2u
// Write T(lf, lq) = M A, A = (log M - lf) + (log M - lq), Ab = |log M - lf| + |log M - lq| >= |A|.  The computed term is the exact
// function at the computed inputs plus what the instructions add, so to first order
//   inputs        |dT/dlf| E(lf) + |dT/dlq| E(lq),   dT/dlf = (p / 2) A + (p - q) / 2,   dT/dlq = (q / 2) A + (q - p) / 2
//                 (the derivatives keep the cancellation between M and log M: both vanish where p = q)
//   dM   <= (p X(lf) + q X(lq)) / 2 + u M               the two exponentials, the sum's rounding (x 0.5 is exact)
//   dlogM <= dM / M + 4 u |log M|
//   dA   <= 2 dlogM + 2 u Ab                            the two subtractions (u Ab) and their sum (u |A| <= u Ab)
//   dT   <= |A| dM + M dA + u |T|                       the product's rounding
// so  B_v = |dT/dlf| E(lf) + |dT/dlq| E(lq) + (|A| + 2) ((p X(lf) + q X(lq)) / 2 + u M) + 8 u M |log M| + 2 u M Ab + u |T|
// and |J^_k - J_k| <= (1 + 2^-10) (0.5 / V) sum_v B_v + u |J_k| + 2^-100.
// The factor 1 + 2^-10 carries every product of two small quantities -- also E^2 M where the first derivatives vanish, which stays
// below 2^-10 u M while 2 |l| + 4 ln V + 3 <= 128 -- and the fp64 sum's roundings (V 2^-53 sum |T|); u |J_k| is the rounding of J to
// fp32 on output; 2^-100 covers the flushed terms (V <= 2^18 of them, each below 2^-118).  tests/dola_ref.py evaluates the bound from
// float64 values, per row and per candidate.
#include "common.h"
#include "log_softmax.h"
#include "radvlm_hip.h"

#include <float.h>

namespace {

constexpr int DL_MAX_LAYERS = 16;
constexpr int DL_MAX_N = 262144;
constexpr int DL_PIECE = 4096;                       // columns per workgroup of the jsd launch: two sweep steps of 256 * LS_U
constexpr int DL_MAX_PIECES = DL_MAX_N / DL_PIECE;   // 64: the stride of a (row, candidate)'s partial sums in ws
constexpr int DL_EW_U = 4;                           // elements per thread of the contrast launch
constexpr int DL_EW = 256 * DL_EW_U;                 // columns per workgroup

DEVINL float dl_term(float xf, float mf, float Lf, float xq, float mq, float Lq) {
#pragma clang fp contract(off)
    const float lf = (xf - mf) - Lf;                 // rv_log_softmax_rows_f32's value, two roundings
    const float lq = (xq - mq) - Lq;
    const float M = 0.5f * (__expf(lf) + __expf(lq));
    if (!(M >= FLT_MIN)) return 0.f;
    const float lm = __logf(M);
    return M * ((lm - lf) + (lm - lq));
}

DEVINL float dl_contrast(float xf, float mf, float Lf, float xb, float mb, float Lb, float thresh) {
#pragma clang fp contract(off)
    const float lf = (xf - mf) - Lf;
    const float lb = (xb - mb) - Lb;
    return lf < thresh ? -INFINITY : lf - lb;
}

DEVINL const float* dl_row(const float* f, long ld_f, const float* c, long ld_c, long stride_c, int layer, int r) {
    return layer == 0 ? f + (long)r * ld_f : c + (long)(layer - 1) * stride_c + (long)r * ld_c;
}

// stats: workgroup b takes row b % rows of layer b / rows (0: f, k: candidate k - 1); stat[2 * b] = m, stat[2 * b + 1] = L
__global__ __launch_bounds__(256) void dola_stats_kernel(const float* __restrict__ f, long ld_f, const float* __restrict__ c, long ld_c,
                                                         long stride_c, int rows, int n, float* __restrict__ stat) {
    __shared__ float redm[4];
    __shared__ double reds[4];
    __shared__ float bc[2];
    const int b = blockIdx.x;
    const float* row = dl_row(f, ld_f, c, ld_c, stride_c, b / rows, b % rows);
    const float m = ls_row_max(row, n, redm);
    const float L = ls_block_logsum(ls_thread_sum(row, n, m), reds, bc);
    if (threadIdx.x == 0) {
        stat[2 * b] = m;
        stat[2 * b + 1] = L;
    }
}

// jsd: blockIdx.x = piece, blockIdx.y = candidate k, blockIdx.z = row r; part[(r * n_layers + k) * DL_MAX_PIECES + piece] = sum of T
__global__ __launch_bounds__(256) void dola_jsd_kernel(const float* __restrict__ f, long ld_f, const float* __restrict__ c, long ld_c,
                                                       long stride_c, int rows, int n_layers, int n, const float* __restrict__ stat,
                                                       double* __restrict__ part) {
    __shared__ double reds[4];
    const int piece = blockIdx.x, k = blockIdx.y, r = blockIdx.z;
    const float* rf = f + (long)r * ld_f;
    const float* rq = c + (long)k * stride_c + (long)r * ld_c;
    const float mf = stat[2 * r], Lf = stat[2 * r + 1];
    const int sq = (k + 1) * rows + r;
    const float mq = stat[2 * sq], Lq = stat[2 * sq + 1];
    const int end = min(n, (piece + 1) * DL_PIECE);
    double s = 0.0;
    for (int j0 = piece * DL_PIECE + threadIdx.x; j0 < end; j0 += 256 * LS_U) {
        float vf[LS_U], vq[LS_U];
#pragma unroll
        for (int i = 0; i < LS_U; ++i) {
            const int j = j0 + i * 256;
            vf[i] = j < end ? rf[j] : 0.f;
            vq[i] = j < end ? rq[j] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < LS_U; ++i) {
            const int j = j0 + i * 256;
            if (j < end) s += (double)dl_term(vf[i], mf, Lf, vq[i], mq, Lq);
        }
    }
    s = wave_sum_f64(s);
    if (lane_id() == 0) reds[wave_id()] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = reds[0];
        t += reds[1];
        t += reds[2];
        t += reds[3];
        part[((long)r * n_layers + k) * DL_MAX_PIECES + piece] = t;
    }
}

// select: one wave per row; lane k < n_layers adds candidate k's pieces in piece order
__global__ __launch_bounds__(64) void dola_select_kernel(int n_layers, int n, int pieces, const double* __restrict__ part,
                                                         int* __restrict__ chosen, float* __restrict__ jsd) {
    __shared__ double J[DL_MAX_LAYERS];
    const int r = blockIdx.x, k = threadIdx.x;
    if (k < n_layers) {
        double s = 0.0;
        if (n_layers > 1) {
            const double* p = part + ((long)r * n_layers + k) * DL_MAX_PIECES;
            for (int i = 0; i < pieces; ++i) s += p[i];
        }
        J[k] = 0.5 * s / (double)n;
        if (jsd) jsd[(long)r * n_layers + k] = (float)J[k];
    }
    __syncthreads();
    if (k == 0) {
        int best = 0;
        for (int i = 1; i < n_layers; ++i)
            if (J[i] > J[best]) best = i;
        chosen[r] = best;
    }
}

// contrast: blockIdx.x cuts the row into DL_EW-column pieces, blockIdx.y is the row
__global__ __launch_bounds__(256) void dola_contrast_kernel(float* __restrict__ f, long ld_f, const float* __restrict__ c, long ld_c,
                                                            long stride_c, int rows, int n, float log_rt, const float* __restrict__ stat,
                                                            const int* __restrict__ chosen) {
    const int r = blockIdx.y;
    const int k = chosen[r];
    float* rf = f + (long)r * ld_f;
    const float* rb = c + (long)k * stride_c + (long)r * ld_c;
    const int sb = (k + 1) * rows + r;
    const float mf = stat[2 * r], Lf = stat[2 * r + 1], mb = stat[2 * sb], Lb = stat[2 * sb + 1];
    const float thresh = -Lf + log_rt;
    const int j0 = blockIdx.x * DL_EW + threadIdx.x;
    float vf[DL_EW_U], vb[DL_EW_U];
#pragma unroll
    for (int i = 0; i < DL_EW_U; ++i) {
        const int j = j0 + i * 256;
        vf[i] = j < n ? rf[j] : 0.f;
        vb[i] = j < n ? rb[j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < DL_EW_U; ++i) {
        const int j = j0 + i * 256;
        if (j < n) rf[j] = dl_contrast(vf[i], mf, Lf, vb[i], mb, Lb, thresh);
    }
}

}  // namespace

// the statistics of (1 + n_layers) * rows rows (two floats each), then DL_MAX_PIECES fp64 partial sums per (row, candidate)
extern "C" int64_t rv_dola_ws_bytes(int rows, int n_layers) {
    if (rows < 1 || n_layers < 1 || n_layers > DL_MAX_LAYERS) return 0;
    return (int64_t)rows * (1 + n_layers) * 8 + (int64_t)rows * n_layers * DL_MAX_PIECES * 8;
}

extern "C" int rv_dola_contrast_rows_f32(float* f, int64_t ld_f, const float* c, int64_t ld_c, int64_t stride_c_layer, int rows,
                                         int n_layers, int n, float log_rt, int32_t* chosen, float* jsd, void* ws, int64_t ws_bytes,
                                         void* stream) {
    if (!f || !c || !chosen || !ws || rows < 1 || rows > 65535 || n_layers < 1 || n_layers > DL_MAX_LAYERS || n < 1 || n > DL_MAX_N)
        return RV_ERR_ARG;
    if (ld_f < n || ld_c < n || (n_layers > 1 && stride_c_layer < ld_c)) return RV_ERR_ARG;
    if (ws_bytes < rv_dola_ws_bytes(rows, n_layers) || ((uintptr_t)ws & 7)) return RV_ERR_ARG;
    float* stat = (float*)ws;
    double* part = (double*)((char*)ws + (int64_t)rows * (1 + n_layers) * 8);
    const int pieces = (n + DL_PIECE - 1) / DL_PIECE;
    hipLaunchKernelGGL(dola_stats_kernel, dim3((1 + n_layers) * rows), dim3(256), 0, ST, (const float*)f, (long)ld_f, c, (long)ld_c,
                       (long)stride_c_layer, rows, n, stat);
    if (n_layers > 1)
        hipLaunchKernelGGL(dola_jsd_kernel, dim3(pieces, n_layers, rows), dim3(256), 0, ST, (const float*)f, (long)ld_f, c, (long)ld_c,
                           (long)stride_c_layer, rows, n_layers, n, (const float*)stat, part);
    hipLaunchKernelGGL(dola_select_kernel, dim3(rows), dim3(64), 0, ST, n_layers, n, pieces, (const double*)part, (int*)chosen, jsd);
    hipLaunchKernelGGL(dola_contrast_kernel, dim3((n + DL_EW - 1) / DL_EW, rows), dim3(256), 0, ST, f, (long)ld_f, c, (long)ld_c,
                       (long)stride_c_layer, rows, n, log_rt, (const float*)stat, (const int*)chosen);
    return rv_check_launch();
}

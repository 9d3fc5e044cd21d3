// Classifier-free guidance for gfx950: the kernel that turns the raw fp32 logits rows of the conditional and the unconditional branch
// of one decode step into the guided score row (HF: UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__),
//     out = g * (log_softmax(c) - log_softmax(u)) + log_softmax(u),
// in place on c.  With lc, lu the bits rv_log_softmax_rows_f32 gives the two rows (log_softmax.h: the same statements), every entry is
//     d = fl(lc - lu);  p = fl(g * d);  out = fl(p + lu)
// three separate roundings in torch's order.  hipcc contracts g * d + lu into one fma (one rounding) by default -- also when it is
// written with __fmul_rn / __fadd_rn, which this toolchain's headers define as plain * and + -- so the statement is compiled under
// `#pragma clang fp contract(off)` (cg_guide); the ISA then holds v_mul_f32 and v_add_f32 and no v_fmac_f32.  As everywhere in the
// decode path there are no atomics and every reduction has a fixed order: a row's bits depend on that row pair and on g alone, not on
// `rows`, the grid or the other rows.
// Non-finite logits are outside the contract (-inf - -inf is NaN where torch gives NaN too, but nothing is promised).
//
// Two launch structures give the same bits (the elementwise part has no reduction):
//   pair  (ws == NULL): one launch, one workgroup per row pair.  Three sweeps -- maximum, sum, write -- each over both rows at once,
//         so a thread keeps 2 * LS_U loads in flight; the second and third sweep hit the cache.
//   split (ws != NULL): the statistics (m, L) of the 2 * rows rows by one workgroup per row (two sweeps) into ws, then an elementwise
//         launch that cuts every row into CG_EW-column pieces over many workgroups.  At rows = 1 the write sweep then runs on ~150
//         compute units instead of one; a 152,064-entry row streamed by one workgroup is bound by one compute unit's load latency.
// DESIGN.md 5b "Classifier-free guidance" holds the A/B of the two and of the unfused baseline; ops.cfg_guide_rows takes the faster.
//
// Error against exact arithmetic on the fp32 inputs and the caller's real g, u = 2^-24, rows of finite entries.  beam.hip derives
// |l^ - l| <= E(l) = u (2 |l| + 4 ln n + 3) for a computed log-softmax entry l^.  Write g32 = fl32(g) (the kernel's, and torch's,
// scale), D = lc - lu and exact = g D + lu = g lc + (1 - g) lu.  The computed value is
//     out^ = ((g32 (lc^ - lu^)(1 + e1))(1 + e2) + lu^)(1 + e3),   |e_k| <= u,
// and to first order
//     out^ - exact = g (lc^ - lc) + (1 - g)(lu^ - lu)      the two log-softmax errors, weighted as exact weights them
//                  + (g32 - g) D                            the scale's rounding
//                  + g D (e1 + e2)                          the subtraction's and the product's rounding
//                  + exact e3                               the sum's rounding
// so  |out^ - exact| <= |g| E(lc) + |1 - g| E(lu) + |g32 - g| |D| + u (2 |g| |D| + |exact|).
// Every dropped term is a product of two of the small quantities above (e_k, E / |l|, |g32 - g| / |g|), at most 2^-20 of a kept term
// for |l| < 2^20 u^-1; the bound is stated with the factor (1 + 2^-20) to carry them.  For g = 1 it is E(lc) + u (2 |D| + |lc|): the
// kernel still rounds three times where HF returns log_softmax(c) directly, which is why generate() treats g = 1 as "off".
// tests/test_cfg_kernel_gpu.py evaluates the bound per entry against a float64 run of HF's processor.
#include "common.h"
#include "log_softmax.h"
#include "radvlm_hip.h"

namespace {

constexpr int CG_EW_U = 4;                   // elements per thread of the elementwise launch
constexpr int CG_EW = 256 * CG_EW_U;         // columns per workgroup

DEVINL float cg_guide(float xc, float mc, float Lc, float xu, float mu, float Lu, float g) {
#pragma clang fp contract(off)               // p + lu must not become fma(g, d, lu): see the head of this file
    const float lc = (xc - mc) - Lc;         // rv_log_softmax_rows_f32's value, two roundings
    const float lu = (xu - mu) - Lu;
    const float d = lc - lu;
    const float p = g * d;
    return p + lu;
}

// pair: one workgroup per row pair
__global__ __launch_bounds__(256) void cfg_guide_pair_kernel(float* __restrict__ c, long ld_c, const float* __restrict__ u, long ld_u, int n,
                                                             float g) {
    __shared__ float redm[2][4];
    __shared__ double reds[2][4];
    __shared__ float bc[2][2];
    float* rc = c + (long)blockIdx.x * ld_c;
    const float* ru = u + (long)blockIdx.x * ld_u;
    const int tid = threadIdx.x;
    // the maxima: both rows in one sweep (max is exact and order-free, so the sweep's shape does not matter)
    float mc = -INFINITY, mu = -INFINITY;
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vc[LS_U], vu[LS_U];
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            const int j = j0 + k * 256;
            vc[k] = j < n ? rc[j] : -INFINITY;
            vu[k] = j < n ? ru[j] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            mc = fmaxf(mc, vc[k]);
            mu = fmaxf(mu, vu[k]);
        }
    }
    mc = wave_max(mc);
    mu = wave_max(mu);
    if (lane_id() == 0) {
        redm[0][wave_id()] = mc;
        redm[1][wave_id()] = mu;
    }
    __syncthreads();
    mc = fmaxf(fmaxf(redm[0][0], redm[0][1]), fmaxf(redm[0][2], redm[0][3]));
    mu = fmaxf(fmaxf(redm[1][0], redm[1][1]), fmaxf(redm[1][2], redm[1][3]));
    // the sums: each row's terms in ls_thread_sum's order (index order per thread), the two rows interleaved
    double sc = 0.0, su = 0.0;
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vc[LS_U], vu[LS_U];
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            const int j = j0 + k * 256;
            vc[k] = j < n ? rc[j] : -INFINITY;
            vu[k] = j < n ? ru[j] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            const int j = j0 + k * 256;
            if (j < n) {
                sc += (double)__expf(vc[k] - mc);
                su += (double)__expf(vu[k] - mu);
            }
        }
    }
    const float Lc = ls_block_logsum(sc, reds[0], bc[0]);
    const float Lu = ls_block_logsum(su, reds[1], bc[1]);
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vc[LS_U], vu[LS_U];
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            const int j = j0 + k * 256;
            vc[k] = j < n ? rc[j] : 0.f;
            vu[k] = j < n ? __builtin_nontemporal_load(ru + j) : 0.f;      // u's last use
        }
#pragma unroll
        for (int k = 0; k < LS_U; ++k) {
            const int j = j0 + k * 256;
            if (j < n) rc[j] = cg_guide(vc[k], mc, Lc, vu[k], mu, Lu, g);
        }
    }
}

// split, first launch: workgroup b < rows takes c's row b, workgroup rows + b takes u's row b; stat[2 * blk] = m, stat[2 * blk + 1] = L
__global__ __launch_bounds__(256) void cfg_stats_kernel(const float* __restrict__ c, long ld_c, const float* __restrict__ u, long ld_u, int rows,
                                                        int n, float* __restrict__ stat) {
    __shared__ float redm[4];
    __shared__ double reds[4];
    __shared__ float bc[2];
    const int b = blockIdx.x;
    const float* row = b < rows ? c + (long)b * ld_c : u + (long)(b - rows) * ld_u;
    const float m = ls_row_max(row, n, redm);
    const float L = ls_block_logsum(ls_thread_sum(row, n, m), reds, bc);
    if (threadIdx.x == 0) {
        stat[2 * b] = m;
        stat[2 * b + 1] = L;
    }
}

// split, second launch: blockIdx.x cuts the row into CG_EW-column pieces, blockIdx.y is the row
__global__ __launch_bounds__(256) void cfg_guide_ew_kernel(float* __restrict__ c, long ld_c, const float* __restrict__ u, long ld_u, int rows,
                                                           int n, float g, const float* __restrict__ stat) {
    const int r = blockIdx.y;
    float* rc = c + (long)r * ld_c;
    const float* ru = u + (long)r * ld_u;
    const float mc = stat[2 * r], Lc = stat[2 * r + 1], mu = stat[2 * (rows + r)], Lu = stat[2 * (rows + r) + 1];
    const int j0 = blockIdx.x * CG_EW + threadIdx.x;
    float vc[CG_EW_U], vu[CG_EW_U];
#pragma unroll
    for (int k = 0; k < CG_EW_U; ++k) {
        const int j = j0 + k * 256;
        vc[k] = j < n ? rc[j] : 0.f;
        vu[k] = j < n ? __builtin_nontemporal_load(ru + j) : 0.f;          // u's last use
    }
#pragma unroll
    for (int k = 0; k < CG_EW_U; ++k) {
        const int j = j0 + k * 256;
        if (j < n) rc[j] = cg_guide(vc[k], mc, Lc, vu[k], mu, Lu, g);
    }
}

}  // namespace

extern "C" int64_t rv_cfg_guide_ws_bytes(int rows) { return rows > 0 ? (int64_t)rows * 16 : 0; }

extern "C" int rv_cfg_guide_rows_f32(float* c, int64_t ld_c, const float* u, int64_t ld_u, int rows, int n, float g, void* ws,
                                     int64_t ws_bytes, void* stream) {
    if (!c || !u || rows < 1 || rows > 65535 || n < 1 || n > 262144 || ld_c < n || ld_u < n) return RV_ERR_ARG;
    if (ws && (ws_bytes < rv_cfg_guide_ws_bytes(rows) || ((uintptr_t)ws & 3))) return RV_ERR_ARG;
    if (!ws) {
        hipLaunchKernelGGL(cfg_guide_pair_kernel, dim3(rows), dim3(256), 0, ST, c, (long)ld_c, u, (long)ld_u, n, g);
    } else {
        hipLaunchKernelGGL(cfg_stats_kernel, dim3(2 * rows), dim3(256), 0, ST, (const float*)c, (long)ld_c, u, (long)ld_u, rows, n, (float*)ws);
        hipLaunchKernelGGL(cfg_guide_ew_kernel, dim3((n + CG_EW - 1) / CG_EW, rows), dim3(256), 0, ST, c, (long)ld_c, u, (long)ld_u, rows, n, g,
                           (const float*)ws);
    }
    return rv_check_launch();
}

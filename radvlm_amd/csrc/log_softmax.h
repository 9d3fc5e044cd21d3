// The row statistics of the fp32 log-softmax, shared by rv_log_softmax_rows_f32 (beam.hip) and rv_cfg_guide_rows_f32 (cfg.hip): both
// must produce the same bits, so both run these statements.  A 256-thread workgroup owns the row.
//   m = max x (exact, order-free);  L = fl32(log(S)),  S = sum exp(x_i - m): every term __expf(fl(x_i - m)) widened to fp64 and added
//   per thread in index order, then lanes by xor butterfly, then waves 0..3 -- a fixed order, so (m, L) depend on the row alone.
// The log-softmax value is then fl(fl(x_i - m) - L).  beam.hip derives the error bound.
#pragma once
#include "common.h"

#include <math.h>

constexpr int LS_U = 8;           // loads a thread keeps in flight per sweep step

// the row maximum, known to every thread on return; redm: 4 floats of LDS
DEVINL float ls_row_max(const float* __restrict__ row, int n, float* redm) {
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vs[LS_U];
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
            const int j = j0 + u * 256;
            vs[u] = j < n ? row[j] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < LS_U; ++u) m = fmaxf(m, vs[u]);
    }
    m = wave_max(m);
    if (lane_id() == 0) redm[wave_id()] = m;
    __syncthreads();
    return fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
}

// this thread's share of S, its terms added in index order
DEVINL double ls_thread_sum(const float* __restrict__ row, int n, float m) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int j0 = tid; j0 < n; j0 += 256 * LS_U) {
        float vs[LS_U];
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
            const int j = j0 + u * 256;
            vs[u] = j < n ? row[j] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < LS_U; ++u) {
            const int j = j0 + u * 256;
            if (j < n) s += (double)__expf(vs[u] - m);
        }
    }
    return s;
}

// L from the threads' shares, known to every thread on return; reds: 4 doubles of LDS, bc: 1 float.  L is computed once (thread 0,
// fp64 log) and broadcast through LDS.
DEVINL float ls_block_logsum(double s, double* reds, float* bc) {
    s = wave_sum_f64(s);
    if (lane_id() == 0) reds[wave_id()] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = reds[0];
        t += reds[1];
        t += reds[2];
        t += reds[3];
        bc[0] = (float)log(t);
    }
    __syncthreads();
    return bc[0];
}

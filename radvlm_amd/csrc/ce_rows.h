// The row sweeps of the bf16 cross entropy, shared by cross_entropy_kernel (ops.hip), policy_loss_kernel (policy.hip) and
// distill_kernel (distill.hip): the policy loss is the cross entropy with a per-row gradient coefficient, the distillation loss at
// temperature 1 against a one-hot teacher is the cross entropy itself, and their lse, target log-prob and softmax p must carry the bits
// rv_cross_entropy computes, so all three kernels run these statements.  A CE_TPB-thread workgroup owns the row; 16-byte row vectors.
// V need not be a multiple of 8 (a vocabulary grown by a few special tokens): rows are padded to ld >= ceil8(V) columns, the pad
// columns are ignored on read (-inf) and their gradient is written as zero.
// In place (dlogits == logits) is the engine's call: a kernel reads its target logit BEFORE ce_row_lse, because other waves of the
// block start overwriting the row in ce_row_grad as soon as they pass ce_row_lse's barrier.
#pragma once
#include "common.h"

constexpr int CE_TPB = 256;

DEVINL void ld8(const bf16* p, float (&v)[8]) {
    const bf16x8 t = *(const bf16x8*)p;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(t[i]);
}
DEVINL void st8(bf16* p, const float (&v)[8]) {
    bf16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = f2bf(v[i]);
    *(bf16x8*)p = t;
}

// log(sum exp) of the row lr[0 .. V), known to every thread on return: a running (max, sum) per thread, then lanes, then waves 0..3.
// red: 8 floats of LDS.
// SCALED (distill.hip): the row is scale * lr, each logit multiplied once in fp32 as it is read (scale 1 gives the unscaled bits).
// An unscaled caller's code is unchanged.
template <bool SCALED = false>
DEVINL float ce_row_lse(const bf16* lr, int V, float* red, float scale = 1.f) {
    const int nvec = (V + 7) / 8;
    float m = -INFINITY, s = 0.f;
    for (int i = threadIdx.x; i < nvec; i += CE_TPB) {
        float v[8];
        ld8(lr + i * 8, v);
        if (SCALED) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= scale;
        }
        if (i * 8 + 8 > V) {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (i * 8 + j >= V) v[j] = -INFINITY;
        }
        float vm = v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) vm = fmaxf(vm, v[j]);
        const float mn = fmaxf(m, vm);
        // Nothing finite seen yet (masked logits: a run of -inf that is this thread's first vector): shift by 0, not by -inf, so that
        // every term is exp(-inf) = 0 and not exp(-inf - -inf) = NaN, which s would keep once m turns finite.
        const float sh = mn == -INFINITY ? 0.f : mn;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += __expf(v[j] - sh);
        s = s * __expf(m - sh) + a;
        m = mn;
    }
    // block combine of (m, s)
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
    if (lane_id() == 0) { red[threadIdx.x >> 6] = wm; red[4 + (threadIdx.x >> 6)] = s; }
    __syncthreads();
    const float gm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float gs = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) gs += (red[i] == -INFINITY) ? 0.f : red[4 + i] * __expf(red[i] - gm);
    return gm + __logf(gs);
}

// an ignored row's gradient: zeros over the row's ceil8(V) columns
DEVINL void ce_row_zero(bf16* dr, int V) {
    const int nvec = (V + 7) / 8;
    const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < nvec; i += CE_TPB) st8(dr + i * 8, z);
}

// dr = (softmax(lr) - onehot(label)) * coef, zeros in the pad columns
DEVINL void ce_row_grad(const bf16* lr, bf16* dr, int V, int64_t label, float lse, float coef) {
    const int nvec = (V + 7) / 8;
    for (int i = threadIdx.x; i < nvec; i += CE_TPB) {
        float v[8], o[8];
        ld8(lr + i * 8, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = __expf(v[j] - lse);
            o[j] = (i * 8 + j < V) ? (p - ((int64_t)(i * 8 + j) == label ? 1.f : 0.f)) * coef : 0.f;
        }
        st8(dr + i * 8, o);
    }
}

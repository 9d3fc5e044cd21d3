// The GRPO token loss (TRL's clipped policy-gradient objective with the k3 KL estimate) on bf16 logits rows: rv_policy_loss_bf16.
// It is cross_entropy_kernel (ops.hip) with a per-row gradient coefficient: the row sweeps below are that kernel's statements, word for
// word, so that lse, the target's log-prob and the softmax p carry the bits rv_cross_entropy computes (tests/test_policy_kernel_gpu.py
// pins both anchors).  One 256-thread workgroup per row, 16-byte row loads, no atomics.
#include "common.h"
#include "radvlm_hip.h"

namespace {

constexpr int TPB = 256;

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

// stats: five fp32 planes of `rows` entries -- logp, loss, lweight * loss, kl, clip code
__global__ __launch_bounds__(TPB) void policy_loss_kernel(const bf16* logits, long ld, const int64_t* labels, const float* adv,
                                                          const float* lweight, const float* gweight, const float* old_logp,
                                                          const float* ref_logp, float eps_low, float eps_high, float beta, float* stats,
                                                          bf16* dlogits, long ld_d, int rows, int V) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    const int64_t label = labels[row];
    const bf16* lr = logits + row * ld;
    const int nvec = (V + 7) / 8;
    // The target logit is read BEFORE any dlogits store: the engine calls this kernel in place (dlogits == logits), and other
    // waves of the block start overwriting the row as soon as they pass the barrier below.
    const float target = (label >= 0 && label < V) ? bf2f(lr[label]) : 0.f;
    if (label < 0 || label >= V) {  // an ignored row: zeros everywhere, none of its per-row floats is read
        if (threadIdx.x < 5) stats[threadIdx.x * (long)rows + row] = 0.f;
        if (dlogits) {
            const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = threadIdx.x; i < nvec; i += TPB) st8(dlogits + row * ld_d + i * 8, z);
        }
        return;
    }
    // ---- sweep 1: running (max, sum) -> lse, as cross_entropy_kernel
    float m = -INFINITY, s = 0.f;
    for (int i = threadIdx.x; i < nvec; i += TPB) {
        float v[8];
        ld8(lr + i * 8, v);
        if (i * 8 + 8 > V) {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (i * 8 + j >= V) v[j] = -INFINITY;
        }
        float vm = v[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) vm = fmaxf(vm, v[j]);
        const float mn = fmaxf(m, vm);
        const float sh = mn == -INFINITY ? 0.f : mn;     // nothing finite seen yet: shift by 0, not by -inf (no NaN from -inf - -inf)
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += __expf(v[j] - sh);
        s = s * __expf(m - sh) + a;
        m = mn;
    }
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
    if (lane_id() == 0) { red[threadIdx.x >> 6] = wm; red[4 + (threadIdx.x >> 6)] = s; }
    __syncthreads();
    const float gm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float gs = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) gs += (red[i] == -INFINITY) ? 0.f : red[4 + i] * __expf(red[i] - gm);
    const float lse = gm + __logf(gs);
    // ---- the row's scalars (every thread: they are uniform loads and a dozen flops)
    const float logp = -(lse - target);                  // the CE kernel's loss row, negated: its bits, -0.0 where lse == target
    const float A = adv[row], gw = gweight[row];
    const float r = old_logp ? __expf(logp - old_logp[row]) : 1.f;      // d = 0 gives exactly 1
    const float rc = fminf(fmaxf(r, 1.f - eps_low), 1.f + eps_high);
    const float ua = r * A, ca = rc * A;
    const bool act = ua <= ca;                           // the unclipped term is the minimum
    float loss = -(act ? ua : ca);
    float g = gw * (act ? ua : 0.f);
    float kl = 0.f;
    if (beta > 0.f) {                                    // the entry point has checked ref_logp
        const float q = ref_logp[row] - logp;
        const float em1 = expm1f(q);                     // exp(q) - 1 without the cancellation at small q
        kl = em1 - q;
        loss += beta * kl;
        g += gw * beta * em1;                            // - gw * beta * (1 - exp(q))
    }
    if (threadIdx.x == 0) {
        const float code = act ? 0.f : (A < 0.f && r < 1.f - eps_low) ? 1.f : (A > 0.f && r > 1.f + eps_high) ? 2.f : 0.f;
        stats[row] = logp;
        stats[(long)rows + row] = loss;
        stats[2 * (long)rows + row] = lweight[row] * loss;
        stats[3 * (long)rows + row] = kl;
        stats[4 * (long)rows + row] = code;
    }
    // ---- sweep 2: the gradient, as cross_entropy_kernel with inv_count = g
    if (dlogits) {
        for (int i = threadIdx.x; i < nvec; i += TPB) {
            float v[8], o[8];
            ld8(lr + i * 8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __expf(v[j] - lse);
                o[j] = (i * 8 + j < V) ? (p - ((int64_t)(i * 8 + j) == label ? 1.f : 0.f)) * g : 0.f;
            }
            st8(dlogits + row * ld_d + i * 8, o);
        }
    }
}

}  // namespace

extern "C" int rv_policy_loss_bf16(const void* logits, int64_t ld, const int64_t* labels, const float* adv, const float* lweight,
                                   const float* gweight, const float* old_logp, const float* ref_logp, float eps_low, float eps_high,
                                   float beta, float* stats, void* dlogits, int64_t ld_d, int rows, int V, void* stream) {
    if (!logits || !labels || !adv || !lweight || !gweight || !stats || rows <= 0 || V < 1) return RV_ERR_ARG;
    const int64_t v8 = ((int64_t)V + 7) & ~(int64_t)7;
    if ((ld & 7) || ld < v8 || (dlogits && ((ld_d & 7) || ld_d < v8))) return RV_ERR_ARG;
    if ((((uintptr_t)logits) | ((uintptr_t)dlogits)) & 15) return RV_ERR_ARG;      // 16-byte row vectors
    if (!(eps_low >= 0.f) || !(eps_high >= 0.f) || !(beta >= 0.f) || (beta > 0.f && !ref_logp)) return RV_ERR_ARG;
    hipLaunchKernelGGL(policy_loss_kernel, dim3(rows), dim3(TPB), 0, ST, (const bf16*)logits, (long)ld, labels, adv, lweight, gweight,
                       old_logp, ref_logp, eps_low, eps_high, beta, stats, (bf16*)dlogits, (long)ld_d, rows, V);
    return rv_check_launch();
}

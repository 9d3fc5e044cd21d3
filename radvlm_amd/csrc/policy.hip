// The GRPO token loss (TRL's clipped policy-gradient objective with the k3 KL estimate) on bf16 logits rows: rv_policy_loss_bf16.
// It is cross_entropy_kernel (ops.hip) with a per-row gradient coefficient: both kernels run the row sweeps of ce_rows.h, so lse, the
// target's log-prob and the softmax p carry the bits rv_cross_entropy computes (tests/test_policy_kernel_gpu.py pins both anchors).
// One 256-thread workgroup per row, 16-byte row loads, no atomics.
#include "ce_rows.h"
#include "common.h"
#include "radvlm_hip.h"

namespace {

// stats: five fp32 planes of `rows` entries -- logp, loss, lweight * loss, kl, clip code
__global__ __launch_bounds__(CE_TPB) void policy_loss_kernel(const bf16* logits, long ld, const int64_t* labels, const float* adv,
                                                             const float* lweight, const float* gweight, const float* old_logp,
                                                             const float* ref_logp, float eps_low, float eps_high, float beta, float* stats,
                                                             bf16* dlogits, long ld_d, int rows, int V) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    const int64_t label = labels[row];
    const bf16* lr = logits + row * ld;
    const float target = (label >= 0 && label < V) ? bf2f(lr[label]) : 0.f;     // before any dlogits store (ce_rows.h: in place)
    if (label < 0 || label >= V) {  // an ignored row: zeros everywhere, none of its per-row floats is read
        if (threadIdx.x < 5) stats[threadIdx.x * (long)rows + row] = 0.f;
        if (dlogits) ce_row_zero(dlogits + row * ld_d, V);
        return;
    }
    const float lse = ce_row_lse(lr, V, red);
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
    if (dlogits) ce_row_grad(lr, dlogits + row * ld_d, V, label, lse, g);
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
    hipLaunchKernelGGL(policy_loss_kernel, dim3(rows), dim3(CE_TPB), 0, ST, (const bf16*)logits, (long)ld, labels, adv, lweight, gweight,
                       old_logp, ref_logp, eps_low, eps_high, beta, stats, (bf16*)dlogits, (long)ld_d, rows, V);
    return rv_check_launch();
}

// Knowledge distillation on bf16 logits rows: rv_distill_loss_bf16, the generalised Jensen-Shannon divergence of TRL's GKDTrainer
// (generalized_jsd_loss) between a student row and a teacher row over the whole vocabulary, and its gradient with respect to the
// student's logits.  Two rows in, one gradient row out: the floor is 3 * rows * ld * 2 bytes of HBM traffic.
// One CE_TPB-thread workgroup owns a row pair; thread t owns the 16-byte vectors t, t + CE_TPB, ... of BOTH rows in EVERY sweep, so
//   * the student's log-sum-exp is ce_row_lse's (ce_rows.h) and carries rv_cross_entropy's bits at temperature 1,
//   * in place (dlogits == logits) needs no ordering between threads: a thread overwrites only vectors it alone reads,
//   * the later sweeps read the rows again from global memory (L2 / the memory-side cache where they still are).  A form that kept
//     both rows in LDS (128 KB at V = 32,000: one workgroup per compute unit) was built, gave identical bits and took twice the
//     time at every size it fits; it is not kept.
// Every sum is per thread ascending, then the xor butterfly of wave_sum, then waves 0..3 in order: no atomics, and a row's bits depend
// on the row pair and the scalars alone.
#include "ce_rows.h"
#include "common.h"
#include "radvlm_hip.h"

namespace {

enum { FWD_KL = 0, REV_KL = 1, JSD = 2 };

// r = s - log m = -log((1 - b) + b exp(d)) and dr = d + r = lt - log m, neither through exp of a positive number: for d > 0 the
// mixture is factored by exp(d), which also gives dr without the cancellation of d + r.
template <int MODE>
DEVINL void log_ratios(float d, float b, float& r, float& dr) {
    if (MODE == REV_KL) { r = -d; dr = 0.f; return; }
    if (d > 0.f) { dr = -__logf(b + (1.f - b) * __expf(-d)); r = dr - d; }
    else         { r = -__logf((1.f - b) + b * __expf(d)); dr = d + r; }
}

// stats: four fp32 planes of `rows` entries -- jsd, lweight * jsd, kl_teacher, kl_student
template <int MODE>
__global__ __launch_bounds__(CE_TPB) void distill_kernel(const bf16* logits, long ld, const bf16* teacher, long ld_t, const int32_t* teacher_row,
                                                         const int64_t* labels, const float* lweight, const float* gweight, float beta,
                                                         float inv_tau, float* stats, bf16* dlogits, long ld_d, int rows, int V) {
    __shared__ float red[8];
    const long row = blockIdx.x;
    const int64_t label = labels[row];
    const long trow = teacher_row ? (long)teacher_row[row] : row;
    if (label < 0 || label >= V || trow < 0) {  // an ignored row: zeros everywhere, none of its floats is read
        if (threadIdx.x < 4) stats[threadIdx.x * (long)rows + row] = 0.f;
        if (dlogits) ce_row_zero(dlogits + row * ld_d, V);
        return;
    }
    const int nvec = (V + 7) / 8;
    const bf16* zr = logits + row * ld;
    const bf16* ur = teacher + trow * ld_t;
    const float lse_s = ce_row_lse<true>(zr, V, red, inv_tau);
    __syncthreads();                                     // red is written again
    const float lse_t = ce_row_lse<true>(ur, V, red, inv_tau);
    const float gw = gweight[row] * inv_tau;
    bf16* dr_row = dlogits ? dlogits + row * ld_d : nullptr;
    float jsd, kl_t, kl_s;
    if (MODE == FWD_KL) {
        // L = sum t (lt - s), dL/dz = (p - t) / tau: one sweep.  A one-hot teacher has t = 1 or 0 exactly and this is ce_row_grad's row.
        float acc = 0.f;
        for (int i = threadIdx.x; i < nvec; i += CE_TPB) {
            float z[8], u[8], o[8];
            ld8(zr + i * 8, z);
            ld8(ur + i * 8, u);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float s = z[j] * inv_tau - lse_s, lt = u[j] * inv_tau - lse_t;
                const float p = __expf(s), t = __expf(lt);
                const bool in = i * 8 + j < V;
                acc += in ? t * (lt - s) : 0.f;
                o[j] = in ? (p - t) * gw : 0.f;
            }
            if (dr_row) st8(dr_row + i * 8, o);
        }
        jsd = kl_t = block_sum<CE_TPB / 64>(acc, red);
        kl_s = 0.f;
    } else {
        const float cg = (MODE == REV_KL ? 1.f : 1.f - beta) * gw;
        float a_s = 0.f, a_t = 0.f;
        for (int i = threadIdx.x; i < nvec; i += CE_TPB) {
            float z[8], u[8];
            ld8(zr + i * 8, z);
            ld8(ur + i * 8, u);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float s = z[j] * inv_tau - lse_s, lt = u[j] * inv_tau - lse_t;
                float r, dr;
                log_ratios<MODE>(lt - s, beta, r, dr);
                const bool in = i * 8 + j < V;
                a_s += in ? __expf(s) * r : 0.f;
                if (MODE == JSD) a_t += in ? __expf(lt) * dr : 0.f;
            }
        }
        kl_s = block_sum<CE_TPB / 64>(a_s, red);
        kl_t = MODE == JSD ? block_sum<CE_TPB / 64>(a_t, red) : 0.f;
        jsd = MODE == JSD ? beta * kl_t + (1.f - beta) * kl_s : kl_s;
        if (dr_row) {       // dL/dz = c p (r - KL_S) / tau, c = 1 - beta (reverse KL: 1); the terms through the mixture cancel
            for (int i = threadIdx.x; i < nvec; i += CE_TPB) {
                float z[8], u[8], o[8];
                ld8(zr + i * 8, z);
                ld8(ur + i * 8, u);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float s = z[j] * inv_tau - lse_s, lt = u[j] * inv_tau - lse_t;
                    float r, dr;
                    log_ratios<MODE>(lt - s, beta, r, dr);
                    o[j] = (i * 8 + j < V) ? __expf(s) * (r - kl_s) * cg : 0.f;
                }
                st8(dr_row + i * 8, o);
            }
        }
    }
    if (threadIdx.x == 0) {
        stats[row] = jsd;
        stats[(long)rows + row] = lweight[row] * jsd;
        stats[2 * (long)rows + row] = kl_t;
        stats[3 * (long)rows + row] = kl_s;
    }
}

}  // namespace

extern "C" int rv_distill_loss_bf16(const void* logits, int64_t ld, const void* teacher, int64_t ld_t, const int32_t* teacher_row,
                                    const int64_t* labels, const float* lweight, const float* gweight, float beta, float temperature,
                                    float* stats, void* dlogits, int64_t ld_d, int rows, int V, void* stream) {
    if (!logits || !teacher || !labels || !lweight || !gweight || !stats || rows <= 0 || V < 1) return RV_ERR_ARG;
    const int64_t v8 = ((int64_t)V + 7) & ~(int64_t)7;
    if ((ld & 7) || ld < v8 || (ld_t & 7) || ld_t < v8 || (dlogits && ((ld_d & 7) || ld_d < v8))) return RV_ERR_ARG;
    if ((((uintptr_t)logits) | ((uintptr_t)teacher) | ((uintptr_t)dlogits)) & 15) return RV_ERR_ARG;      // 16-byte row vectors
    if (!(beta >= 0.f && beta <= 1.f) || !(temperature > 0.f) || !(temperature <= 3.4028234e38f)) return RV_ERR_ARG;
    const float inv_tau = 1.f / temperature;
#define RV_DISTILL_GO(MODE)                                                                                                            \
    hipLaunchKernelGGL(distill_kernel<MODE>, dim3(rows), dim3(CE_TPB), 0, ST, (const bf16*)logits, (long)ld, (const bf16*)teacher,         \
                       (long)ld_t, teacher_row, labels, lweight, gweight, beta, inv_tau, stats, (bf16*)dlogits, (long)ld_d, rows, V)
    if (beta == 0.f) RV_DISTILL_GO(FWD_KL);
    else if (beta == 1.f) RV_DISTILL_GO(REV_KL);
    else RV_DISTILL_GO(JSD);
#undef RV_DISTILL_GO
    return rv_check_launch();
}

// The sequence-level part between the two sweeps of rv_policy_loss_bf16, for DPO and for GRPO with sequence-level importance ratios
// (GSPO): per-sequence sums of the scored tokens' log-probs (rv_seq_logp_sums_f64), the pairwise DPO loss (rv_dpo_pairs_f64) and the
// clipped sequence ratio (rv_gspo_seqs_f64), the last two with their per-token gradient coefficients.
// Everything here is fp64 on fp32 inputs, in a fixed order (include/radvlm_hip.h states it), without atomics and without a host
// round trip.  The arithmetic is written one rounding per operation: no contraction into fused multiply-adds, so that
// tests/preference_ref.py can restate it operation by operation.
#include "common.h"
#include "radvlm_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int PAIR_TPB = 128;          // wave 0 sums the chosen answer, wave 1 the rejected one; both write coefficients
constexpr int GSPO_TPB = 256;          // one wave per sum of the sequence (log-ratio, lweight, gweight, lweight * kl); all write coefficients
enum { LOSS_SIGMOID = 0, LOSS_HINGE = 1, LOSS_IPO = 2 };
enum { PL_PI_C = 0, PL_PI_R, PL_H, PL_LOSS, PL_REWARD_C, PL_REWARD_R, PL_SUM_C, N_PLANES };
enum { GP_M = 0, GP_S, GP_L, GP_CLIP, GP_WKL, N_GSPO_PLANES };

// Scored token j lives in row j (row_idx NULL) or row_idx[j]; a row outside [0, rows) is never touched.
DEVINL long row_of(const int32_t* row_idx, int j) { return row_idx ? (long)row_idx[j] : (long)j; }

// The sum of one sequence by one wave: lane l adds term(row) of elements l, l + 64, ... of [j0, j1) in ascending order to a +0.0
// accumulator, then the xor butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).  It depends on the sequence's own
// length alone.
template <class Term>
DEVINL double seq_sum_of(const int32_t* row_idx, int j0, int j1, int rows, Term term) {
    double a = 0.0;
    for (int j = j0 + lane_id(); j < j1; j += 64) {
        const long r = row_of(row_idx, j);
        if (r >= 0 && r < rows) a += term(r);
    }
    return wave_sum_f64(a);
}
DEVINL double seq_sum(const float* logp, const int32_t* row_idx, int j0, int j1, int rows) {
    return seq_sum_of(row_idx, j0, j1, rows, [=](long r) { return (double)logp[r]; });
}

__global__ __launch_bounds__(64) void seq_logp_sums_kernel(const float* logp, const int32_t* seg_off, const int32_t* row_idx, double* sums,
                                                           int rows) {
    const int b = blockIdx.x;
    const double s = seq_sum(logp, row_idx, seg_off[b], seg_off[b + 1], rows);
    if (threadIdx.x == 0) sums[b] = s;
}

DEVINL double log_sigmoid(double h) { return -(fmax(-h, 0.0) + log1p(exp(-fabs(h)))); }
DEVINL double sigmoid(double h) {
    const double e = exp(-fabs(h));
    return (h >= 0.0 ? 1.0 : e) / (1.0 + e);
}

__global__ __launch_bounds__(PAIR_TPB) void dpo_pairs_kernel(const float* logp, const int32_t* seg_off, const int32_t* row_idx,
                                                             const double* rho, int P, int loss_type, double beta, double eps, double a_P,
                                                             double g_N, double* planes, float* coef, int rows) {
    __shared__ double red[2];
    const int p = blockIdx.x, w = wave_id();
    const int c0 = seg_off[p], c1 = seg_off[p + 1], r0 = seg_off[P + p], r1 = seg_off[P + p + 1];
    const double mine = w == 0 ? seq_sum(logp, row_idx, c0, c1, rows) : seq_sum(logp, row_idx, r0, r1, rows);
    if (lane_id() == 0) red[w] = mine;
    __syncthreads();
    const double sum_c = red[0], sum_r = red[1];
    const int n_c = c1 - c0, n_r = r1 - r0;
    // every thread forms the pair's scalars: a few dozen uniform flops
    const bool ipo = loss_type == LOSS_IPO;
    const double s_c = ipo && n_c > 0 ? 1.0 / (double)n_c : 1.0, s_r = ipo && n_r > 0 ? 1.0 / (double)n_r : 1.0;
    const double pi_c = ipo && n_c > 0 ? sum_c / (double)n_c : sum_c, pi_r = ipo && n_r > 0 ? sum_r / (double)n_r : sum_r;
    const double rho_c = rho ? rho[p] : 0.0, rho_r = rho ? rho[P + p] : 0.0;
    const double u = (pi_c - pi_r) - (rho_c - rho_r);
    const double h = beta * u;
    double loss, dl_du;
    if (loss_type == LOSS_SIGMOID) {
        loss = -(1.0 - eps) * log_sigmoid(h) - eps * log_sigmoid(-h);
        dl_du = beta * (eps * sigmoid(h) - (1.0 - eps) * sigmoid(-h));
    } else if (loss_type == LOSS_HINGE) {
        const double t = 1.0 - h;
        loss = fmax(0.0, t);
        dl_du = t > 0.0 ? -beta : 0.0;
    } else {
        const double t = u - 1.0 / (2.0 * beta);
        loss = t * t;
        dl_du = 2.0 * t;
    }
    const double k = a_P * dl_du;
    const float A_c = (float)(g_N - k * s_c), A_r = (float)(k * s_r);
    if (threadIdx.x == 0) {
        planes[PL_PI_C * (long)P + p] = pi_c;
        planes[PL_PI_R * (long)P + p] = pi_r;
        planes[PL_H * (long)P + p] = h;
        planes[PL_LOSS * (long)P + p] = loss;
        planes[PL_REWARD_C * (long)P + p] = beta * (pi_c - rho_c);
        planes[PL_REWARD_R * (long)P + p] = beta * (pi_r - rho_r);
        planes[PL_SUM_C * (long)P + p] = sum_c;
    }
    for (int j = c0 + (int)threadIdx.x; j < c1; j += PAIR_TPB) {
        const long r = row_of(row_idx, j);
        if (r >= 0 && r < rows) coef[r] = A_c;
    }
    for (int j = r0 + (int)threadIdx.x; j < r1; j += PAIR_TPB) {
        const long r = row_of(row_idx, j);
        if (r >= 0 && r < rows) coef[r] = A_r;
    }
}

// batch[0] = L = a_P * sum(loss) - g_N * sum(sum_c), batch[1] = a_P * sum(loss), batch[2] = -sum(sum_c) / N_c: one wave, the sums over the
// pairs in seq_sum's order (lane l takes pairs l, l + 64, ...; the same butterfly).
__global__ __launch_bounds__(64) void dpo_batch_kernel(const double* planes, const int32_t* seg_off, int P, double a_P, double g_N,
                                                       double* batch) {
    double sl = 0.0, sc = 0.0;
    for (int p = lane_id(); p < P; p += 64) {
        sl += planes[PL_LOSS * (long)P + p];
        sc += planes[PL_SUM_C * (long)P + p];
    }
    sl = wave_sum_f64(sl);
    sc = wave_sum_f64(sc);
    if (threadIdx.x == 0) {
        const int n_c = seg_off[P] - seg_off[0];
        batch[0] = a_P * sl - g_N * sc;
        batch[1] = a_P * sl;
        batch[2] = n_c > 0 ? -sc / (double)n_c : 0.0;
    }
}

// GSPO's clipped sequence term: ua = s A, ca = clamp(s, 1 - eps_low, 1 + eps_high) A; the unclipped one is active when it is the minimum.
struct SeqClip { double ua, loss; bool act; };
DEVINL SeqClip seq_clip(double s, double A, double eps_low, double eps_high) {
    const double sc = fmin(fmax(s, 1.0 - eps_low), 1.0 + eps_high);
    const double ua = s * A, ca = sc * A;
    const bool act = ua <= ca;
    return {ua, -(act ? ua : ca), act};
}
// k3 of one token: q = ref - logp, em1 = expm1(q), kl = em1 - q
DEVINL double k3(const float* ref_logp, const float* logp, long r, double* em1) {
    const double q = (double)ref_logp[r] - (double)logp[r];
    *em1 = expm1(q);
    return *em1 - q;
}

__global__ __launch_bounds__(GSPO_TPB) void gspo_seqs_kernel(const float* logp, const int32_t* seg_off, const int32_t* row_idx,
                                                             const float* adv_seq, const float* lweight, const float* gweight,
                                                             const float* old_logp, const float* ref_logp, double eps_low, double eps_high,
                                                             double beta, int B, double* planes, float* coef, float* kl, int rows) {
    __shared__ double red[4];
    const int b = blockIdx.x, w = wave_id();
    const int j0 = seg_off[b], j1 = seg_off[b + 1], n = j1 - j0;
    double mine = 0.0;
    if (w == 0) {
        if (old_logp) mine = seq_sum_of(row_idx, j0, j1, rows, [=](long r) { return (double)logp[r] - (double)old_logp[r]; });
    } else if (w == 1) {
        mine = seq_sum_of(row_idx, j0, j1, rows, [=](long r) { return (double)lweight[r]; });
    } else if (w == 2) {
        mine = seq_sum_of(row_idx, j0, j1, rows, [=](long r) { return (double)gweight[r]; });
    } else if (beta > 0.0) {                                 // the entry point has checked ref_logp
        mine = seq_sum_of(row_idx, j0, j1, rows, [=](long r) {
            double em1;
            return (double)lweight[r] * k3(ref_logp, logp, r, &em1);
        });
    }
    if (lane_id() == 0) red[w] = mine;
    __syncthreads();
    // every thread forms the sequence's scalars: a few uniform flops
    const double m = n > 0 ? red[0] / (double)n : 0.0;
    const double s = m == 0.0 ? 1.0 : exp(m);                // on-policy is exactly 1, whatever the library's exp returns at 0
    const double A = (double)adv_seq[b];
    const SeqClip c = seq_clip(s, A, eps_low, eps_high);
    if (threadIdx.x == 0) {
        const double code = c.act ? 0.0 : (A < 0.0 && s < 1.0 - eps_low) ? 1.0 : (A > 0.0 && s > 1.0 + eps_high) ? 2.0 : 0.0;
        planes[GP_M * (long)B + b] = m;
        planes[GP_S * (long)B + b] = s;
        planes[GP_L * (long)B + b] = red[1];                 // the lweight sum, until gspo_batch_kernel has used it and writes l here
        planes[GP_CLIP * (long)B + b] = code;
        planes[GP_WKL * (long)B + b] = red[3];
    }
    if (n <= 0) return;
    const double pg = (c.act ? c.ua : 0.0) * (red[2] / (double)n);
    for (int j = j0 + (int)threadIdx.x; j < j1; j += GSPO_TPB) {
        const long r = row_of(row_idx, j);
        if (r < 0 || r >= rows) continue;
        double g = pg, k = 0.0;
        if (beta > 0.0) {
            double em1;
            k = k3(ref_logp, logp, r, &em1);
            g = pg + ((double)gweight[r] * beta) * em1;
        }
        coef[r] = (float)g;
        kl[r] = (float)k;
    }
}

// Plane l = -min(s A, sc A) (0 for an empty sequence); batch[1] = beta * sum_b plane_wkl, batch[0] = L = sum_b (lweight sum)_b l_b +
// batch[1]: one wave, the sums over the sequences in seq_sum's order, as dpo_batch_kernel.
__global__ __launch_bounds__(64) void gspo_batch_kernel(double* planes, const int32_t* seg_off, const float* adv_seq, int B, double eps_low,
                                                        double eps_high, double beta, double* batch) {
    double sl = 0.0, sk = 0.0;
    for (int b = lane_id(); b < B; b += 64) {
        const double W = planes[GP_L * (long)B + b];
        const double l = seg_off[b + 1] > seg_off[b] ? seq_clip(planes[GP_S * (long)B + b], (double)adv_seq[b], eps_low, eps_high).loss : 0.0;
        planes[GP_L * (long)B + b] = l;
        sl += W * l;
        sk += planes[GP_WKL * (long)B + b];
    }
    sl = wave_sum_f64(sl);
    sk = wave_sum_f64(sk);
    if (threadIdx.x == 0) {
        const double bk = beta * sk;
        batch[0] = sl + bk;
        batch[1] = bk;
    }
}

}  // namespace

extern "C" int rv_seq_logp_sums_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, double* sums, int B, int rows,
                                    void* stream) {
    if (!logp || !seg_off || !sums || B < 1 || rows < 1) return RV_ERR_ARG;
    hipLaunchKernelGGL(seq_logp_sums_kernel, dim3(B), dim3(64), 0, ST, logp, seg_off, row_idx, sums, rows);
    return rv_check_launch();
}

extern "C" int rv_dpo_pairs_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, const double* rho, int P, int loss_type,
                                double beta, double label_smoothing, double alpha_over_P, double gamma_over_Nc, double* planes,
                                double* batch, float* coef, int rows, void* stream) {
    if (!logp || !seg_off || !planes || !batch || !coef || P < 1 || rows < 1) return RV_ERR_ARG;
    if (!(beta > 0.0) || beta > 1.7976931348623157e308) return RV_ERR_ARG;                    // NaN, <= 0 or +inf
    if (!(label_smoothing >= 0.0 && label_smoothing < 0.5)) return RV_ERR_ARG;
    if (loss_type != LOSS_SIGMOID && loss_type != LOSS_HINGE && loss_type != LOSS_IPO) return RV_ERR_ARG;
    if (loss_type == LOSS_IPO && label_smoothing != 0.0) return RV_ERR_ARG;
    if (!(alpha_over_P == alpha_over_P) || !(gamma_over_Nc == gamma_over_Nc)) return RV_ERR_ARG;
    hipLaunchKernelGGL(dpo_pairs_kernel, dim3(P), dim3(PAIR_TPB), 0, ST, logp, seg_off, row_idx, rho, P, loss_type, beta, label_smoothing,
                       alpha_over_P, gamma_over_Nc, planes, coef, rows);
    hipLaunchKernelGGL(dpo_batch_kernel, dim3(1), dim3(64), 0, ST, (const double*)planes, seg_off, P, alpha_over_P, gamma_over_Nc, batch);
    return rv_check_launch();
}

extern "C" int rv_gspo_seqs_f64(const float* logp, const int32_t* seg_off, const int32_t* row_idx, const float* adv_seq, const float* lweight,
                                const float* gweight, const float* old_logp, const float* ref_logp, double eps_low, double eps_high,
                                double beta, double* planes, double* batch, float* coef, float* kl, int B, int rows, void* stream) {
    if (!logp || !seg_off || !adv_seq || !lweight || !gweight || !planes || !batch || !coef || !kl || B < 1 || rows < 1) return RV_ERR_ARG;
    if (!(eps_low >= 0.0) || !(eps_high >= 0.0) || !(beta >= 0.0) || (beta > 0.0 && !ref_logp)) return RV_ERR_ARG;
    hipLaunchKernelGGL(gspo_seqs_kernel, dim3(B), dim3(GSPO_TPB), 0, ST, logp, seg_off, row_idx, adv_seq, lweight, gweight, old_logp,
                       ref_logp, eps_low, eps_high, beta, B, planes, coef, kl, rows);
    hipLaunchKernelGGL(gspo_batch_kernel, dim3(1), dim3(64), 0, ST, planes, seg_off, adv_seq, B, eps_low, eps_high, beta, batch);
    return rv_check_launch();
}

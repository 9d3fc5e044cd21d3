"""float64 reference of rv_distill_loss_bf16 (radvlm_amd/csrc/distill.hip), in the style of policy_ref.py: plain torch on the CPU, on
the bf16 inputs the kernel reads.  The three modes are TRL's GKDTrainer.generalized_jsd_loss (tests/test_distill_host.py pins the
gradient to autograd on that formula written out literally):
  s = log_softmax(z / tau), lt = log_softmax(u / tau), p = exp(s), t = exp(lt), d = lt - s
  beta == 0:  L = sum t d                                   dL/dz = (p - t) / tau
  beta == 1:  L = sum p r, r = -d                           dL/dz = p (r - L) / tau
  else:       r = s - log m, m = (1 - beta) p + beta t;  KL_S = sum p r;  KL_T = sum t (d + r);  L = beta KL_T + (1 - beta) KL_S
                                                            dL/dz = (1 - beta) p (r - KL_S) / tau
log m is a logaddexp, so nothing overflows for any finite d.

Gates (derived, not fitted):
  gradient, per element, 2^-7 A + 1e-30 (rowops_ref.assert_close_elementwise):
      beta == 0:  A = |gw| / tau (p + t)                                                       -- the cross entropy's form
      else:       A = |gw| c / tau p (|r| + |KL_S| + 2^-12 Mag),   c = 1 - beta (1 at beta == 1)
                  Mag = max|z| / tau + max|u| / tau + |lse_s| + |lse_t| + 1 for the row: 2^-7 2^-12 Mag = 32 fp32 ulps of Mag of
                  absolute error on a log-ratio built from four fp32 quantities of that magnitude
  fp32 rows, 1e-4 max(1, sum_j |term_j|) (rowops_ref.assert_rows_close; the policy kernel's constant), the terms being those of the
  plane: scale (jsd), scale_t (kl_teacher), scale_s (kl_student).
"""
import math

import torch


BF16 = torch.bfloat16
ROWS = 9
NAN = float("nan")
WEIGHT = (0.1, 0.2, 0.3, 0.1, 0.05, 0.0, NAN, 0.25, 0.15)
GENERIC, SAME, NOISY, DOMINANT, ZERO_WEIGHT, IGNORED = 0, 1, 2, 3, 5, 6
GSCALE = 0.5


def make_inputs(V):
    """The kernel tests' nine row pairs (bf16 student [9, V], bf16 teacher [9, V], labels, fp32 lweight, fp32 gweight): N(0, 2) logits;
    row 1's teacher is the student, row 2's the student plus N(0, 0.02) noise (the cancellation in r), row 3 has a dominant teacher logit
    at one column and a dominant student logit at another, both 40 above the rest, row 5 has weight zero, row 6 is ignored and its
    floats are NaN."""
    g = torch.Generator().manual_seed(4100 + V)
    z = torch.randn(ROWS, V, generator=g) * 2.0
    u = torch.randn(ROWS, V, generator=g) * 2.0
    u[SAME] = z[SAME]
    u[NOISY] = z[NOISY] + torch.randn(V, generator=g) * 0.02
    u[DOMINANT, min(5, V - 1)] = u[DOMINANT].max() + 40
    z[DOMINANT, 2] = z[DOMINANT].max() + 40
    z, u = z.to(BF16), u.to(BF16)
    u[SAME] = z[SAME]
    labels = torch.tensor([0, V - 1, V // 2, V // 3, 0, V - 1, -100, V // 5, min(5, V - 1)])
    w = torch.tensor(WEIGHT, dtype=torch.float64)
    return z, u, labels, w.to(torch.float32), (w * GSCALE).to(torch.float32)


def _logmix(s, lt, beta):
    return torch.logaddexp(s + math.log1p(-beta), lt + math.log(beta))


def jsd_rows(z, u, beta, tau):
    """The differentiable core on float64 [rows, V] tensors: (L, KL_T, KL_S, parts) with parts = dict(s, lt, r, dr)."""
    s, lt = torch.log_softmax(z / tau, -1), torch.log_softmax(u / tau, -1)
    p, t, d = s.exp(), lt.exp(), lt - s
    zero = torch.zeros(z.shape[0], dtype=z.dtype)
    if beta == 0:
        L = (t * d).sum(-1)
        return L, L, zero, dict(s=s, lt=lt, r=-d, dr=d)
    if beta == 1:
        L = (p * -d).sum(-1)
        return L, zero, L, dict(s=s, lt=lt, r=-d, dr=torch.zeros_like(d))
    logm = _logmix(s, lt, beta)
    r, dr = s - logm, lt - logm
    kl_s, kl_t = (p * r).sum(-1), (t * dr).sum(-1)
    return beta * kl_t + (1 - beta) * kl_s, kl_t, kl_s, dict(s=s, lt=lt, r=r, dr=dr)


def distill_loss(logits, teacher, labels, V, lweight, gweight, beta, tau, teacher_row=None):
    """logits, teacher: bf16 (or any float) [rows, >= V]; labels int64 [rows] (outside [0, V): an ignored row); lweight, gweight: the
    fp32 per-row weights the kernel gets; teacher_row: None or int [rows] (-1: ignored).
    Returns a dict of float64 tensors: jsd, wloss, kl_teacher, kl_student [rows]; grad, A [rows, V]; scale, scale_t, scale_s [rows]."""
    z = logits.detach().cpu().double()[:, :V]
    u = teacher.detach().cpu().double()[:, :V]
    labels = torch.as_tensor(labels, dtype=torch.int64).cpu()
    rows = z.shape[0]
    live = (labels >= 0) & (labels < V)
    if teacher_row is not None:
        tr = torch.as_tensor(teacher_row, dtype=torch.int64).cpu()
        live = live & (tr >= 0)
        u = u[tr.clamp_min(0)]
    zl = torch.where(live[:, None], z, torch.zeros_like(z))          # an ignored row may hold anything
    ul = torch.where(live[:, None], u, torch.zeros_like(u))
    lw = torch.where(live, torch.as_tensor(lweight).cpu().double(), torch.zeros(rows, dtype=torch.float64))
    gw = torch.where(live, torch.as_tensor(gweight).cpu().double(), torch.zeros(rows, dtype=torch.float64))
    L, kl_t, kl_s, q = jsd_rows(zl, ul, beta, tau)
    p, t, r, dr = q["s"].exp(), q["lt"].exp(), q["r"], q["dr"]
    if beta == 0:
        grad = gw[:, None] * (p - t) / tau
        A = gw.abs()[:, None] / tau * (p + t)
        sc_t = (t * dr.abs()).sum(-1)
        sc_s = torch.zeros_like(sc_t)
        sc = sc_t
    else:
        c = 1.0 if beta == 1 else 1.0 - beta
        mag = (zl.abs().amax(-1) + ul.abs().amax(-1)) / tau + torch.logsumexp(zl / tau, -1).abs() + torch.logsumexp(ul / tau, -1).abs() + 1
        grad = gw[:, None] * c * p * (r - kl_s[:, None]) / tau
        A = gw.abs()[:, None] * c / tau * p * (r.abs() + kl_s.abs()[:, None] + 2.0 ** -12 * mag[:, None])
        sc_s = (p * r.abs()).sum(-1)
        sc_t = (t * dr.abs()).sum(-1) if beta != 1 else torch.zeros_like(sc_s)
        sc = sc_s if beta == 1 else beta * sc_t + (1 - beta) * sc_s
    m = live.double()
    one = torch.ones(rows, dtype=torch.float64)
    return dict(jsd=L * m, wloss=lw * L * m, kl_teacher=kl_t * m, kl_student=kl_s * m, grad=grad * m[:, None], A=A * m[:, None],
                scale=torch.maximum(one, sc * m), scale_t=torch.maximum(one, sc_t * m), scale_s=torch.maximum(one, sc_s * m), live=live)

"""float64 reference of rv_policy_loss_bf16 (radvlm_amd/csrc/policy.hip), in the style of rowops_ref.cross_entropy: plain torch on the CPU
on the bf16 logits.  tests/test_policy_host.py pins it to float64 autograd of the formula, tests/test_policy_kernel_gpu.py holds the kernel
to it.

The clip decision is a comparison, so a row whose ratio lies on a clip edge may legitimately fall either way in fp32 and in float64.  Such a
row is no test case: the reference ASSERTS that every live row keeps |r - (1 - eps_low)| and |r - (1 + eps_high)| above EDGE_MARGIN, and
rejects the input otherwise instead of tolerating a flipped result.
"""
import torch

from rowops_ref import _f64

EDGE_MARGIN = 1e-3


def _rows(a, n):
    return None if a is None else torch.as_tensor(a, dtype=torch.float64).reshape(n)


def policy_loss(logits, labels, V, adv, lweight, gweight, old_logp=None, ref_logp=None, eps_low=0.2, eps_high=0.2, beta=0.0):
    """Rows of logits[:, :V]; a label outside [0, V) marks an ignored row: zeros everywhere, its per-row floats (NaN allowed) unread.
    Returns a dict: logp, loss, wloss (= lweight * loss), kl, clip (0 / 1 / 2), ratio -- all [rows]; scale = max(1, |lse| + |target|), the
    row gate's magnitude; grad = (softmax - onehot) g and A = (softmax + onehot) |g|, both [rows, V]; g [rows]."""
    z = _f64(logits)[0][:, :V]
    n = z.shape[0]
    labels = torch.as_tensor(labels, dtype=torch.int64).cpu()
    live = (labels >= 0) & (labels < V)
    lab = torch.where(live, labels, torch.zeros_like(labels))
    zero = torch.zeros(n, dtype=torch.float64)
    pick = lambda a: torch.where(live, _rows(a, n), zero)          # an ignored row's floats are never read: NaN there must not spread
    A_, lw, gw = pick(adv), pick(lweight), pick(gweight)
    lse = torch.logsumexp(z, -1)
    target = z.gather(1, lab[:, None])[:, 0]
    logp = target - lse
    r = torch.ones(n, dtype=torch.float64) if old_logp is None else torch.exp(logp - pick(old_logp))
    r = torch.where(live, r, torch.ones_like(r))
    lo, hi = 1.0 - eps_low, 1.0 + eps_high
    if old_logp is not None:
        near = live & (((r - lo).abs() <= EDGE_MARGIN) | ((r - hi).abs() <= EDGE_MARGIN))
        assert not bool(near.any()), f"rows {near.nonzero()[:, 0].tolist()} sit within {EDGE_MARGIN} of a clip edge: not a test case"
    rc = r.clamp(lo, hi)
    ua, ca = r * A_, rc * A_
    act = ua <= ca
    loss = -torch.minimum(ua, ca)
    g = gw * torch.where(act, ua, zero)
    kl = zero.clone()
    if beta > 0:
        assert ref_logp is not None
        q = pick(ref_logp) - logp
        kl = torch.expm1(q) - q
        loss = loss + beta * kl
        g = g - gw * beta * (-torch.expm1(q))
    clip = torch.where(~act & (r < lo) & (A_ < 0), torch.ones(n), torch.where(~act & (r > hi) & (A_ > 0), torch.full((n,), 2.0), torch.zeros(n)))
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z).scatter_(1, lab[:, None], 1.0)
    lv = live.double()
    m = lambda t: torch.where(live, t, zero)
    return dict(logp=m(logp), loss=m(loss), wloss=m(lw * loss), kl=m(kl), clip=m(clip.double()), ratio=r,
                scale=torch.where(live, (lse.abs() + target.abs()).clamp_min(1.0), torch.ones_like(lse)),
                grad=(p - onehot) * (g * lv)[:, None], A=(p + onehot) * (g.abs() * lv)[:, None], g=m(g))

"""float64 numpy restatement of rv_gspo_seqs_f64 (radvlm_amd/csrc/preference.hip; include/radvlm_hip.h states it): GRPO with one
importance ratio per sequence.  The fixed-order sums are preference_ref.ordered_sum; every other operation is one float64 operation,
in the kernel's order.  tests/test_gspo_host.py pins it to torch autograd on the CPU.

The clip decision is a comparison, so a sequence whose ratio lies on a clip edge may legitimately fall either way.  Such a sequence is
no test case: as policy_ref does per row, the reference ASSERTS that every live sequence keeps |s - (1 - eps_low)| and
|s - (1 + eps_high)| above policy_ref.EDGE_MARGIN, and rejects the input otherwise.
"""
import math

import numpy as np

from policy_ref import EDGE_MARGIN
from preference_ref import ordered_sum


def gspo(logp, counts, adv_seq, lweight, gweight, old_logp=None, ref_logp=None, eps_low=0.2, eps_high=0.2, beta=0.0):
    """logp, lweight, gweight, old_logp, ref_logp: fp32-valued arrays of sum(counts) entries in scored order; counts: the B scored
    counts (0 allowed); adv_seq: B advantages.  Returns a dict of float64 arrays: m, s, l, clip, wkl, W_l [B]; coef and kl [n] (before
    the fp32 rounding); L and kl_loss."""
    f = lambda a: None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64).reshape(-1)
    x, lw, gw, old, ref = f(logp), f(lweight), f(gweight), f(old_logp), f(ref_logp)
    A_ = f(adv_seq)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    B, n_all = counts.size, int(counts.sum())
    assert B >= 1 and A_.size == B and all(a is None or a.size == n_all for a in (x, lw, gw, old, ref))
    assert eps_low >= 0 and eps_high >= 0 and beta >= 0 and (beta == 0 or ref is not None)
    off = np.concatenate([[0], np.cumsum(counts)])
    lo, hi = 1.0 - eps_low, 1.0 + eps_high
    out = {k: np.zeros(B) for k in ("m", "s", "l", "clip", "wkl", "W_l")}
    coef, kl = np.zeros(n_all), np.zeros(n_all)
    for b in range(B):
        j0, j1, n = int(off[b]), int(off[b + 1]), int(counts[b])
        A = float(A_[b])
        sum_d = ordered_sum(x[j0:j1] - old[j0:j1]) if old is not None else 0.0
        W_l, W_g = ordered_sum(lw[j0:j1]), ordered_sum(gw[j0:j1])
        em1 = np.zeros(n)
        if beta > 0:
            q = ref[j0:j1] - x[j0:j1]
            em1 = np.array([math.expm1(v) for v in q])
            kl[j0:j1] = em1 - q
        wkl = ordered_sum(lw[j0:j1] * kl[j0:j1]) if beta > 0 else 0.0
        m = sum_d / float(n) if n > 0 else 0.0
        s = 1.0 if m == 0.0 else math.exp(m)
        if n > 0 and old is not None:
            assert abs(s - lo) > EDGE_MARGIN and abs(s - hi) > EDGE_MARGIN, f"sequence {b} sits within {EDGE_MARGIN} of a clip edge: not a test case"
        sc = min(max(s, lo), hi)
        ua, ca = s * A, sc * A
        act = ua <= ca
        l = -(ua if act else ca) if n > 0 else 0.0
        code = 0.0 if act else 1.0 if (A < 0 and s < lo) else 2.0 if (A > 0 and s > hi) else 0.0
        if n > 0:
            pg = (ua if act else 0.0) * (W_g / float(n))
            coef[j0:j1] = pg + (gw[j0:j1] * beta) * em1 if beta > 0 else pg
        for k, v in (("m", m), ("s", s), ("l", l), ("clip", code), ("wkl", wkl), ("W_l", W_l)):
            out[k][b] = v
    kl_loss = beta * ordered_sum(out["wkl"])
    out.update(coef=coef, kl=kl, kl_loss=kl_loss, L=ordered_sum(out["W_l"] * out["l"]) + kl_loss)
    return out

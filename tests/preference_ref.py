"""float64 numpy restatement of the DPO objective of radvlm_amd/csrc/preference.hip (include/radvlm_hip.h states it): the fixed-order
sequence sums, the pair terms, the batch scalar and the per-token coefficient A = -dL/dlogp.  tests/test_preference_host.py pins it to
torch autograd on the CPU.  Every operation is one numpy float64 operation, in the kernel's order."""
import math

import numpy as np

LOSS_TYPES = ("sigmoid", "hinge", "ipo")


def ordered_sum(x):
    """The documented order: 64 accumulators at +0.0, element j into accumulator j mod 64 ascending, then the xor butterfly."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    acc = np.zeros(64, dtype=np.float64)
    for j0 in range(0, x.size, 64):
        part = x[j0:j0 + 64]
        acc[:part.size] = acc[:part.size] + part
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return float(acc[0])


def log_sigmoid(h):
    return -(max(-h, 0.0) + math.log1p(math.exp(-abs(h))))


def sigmoid(h):
    e = math.exp(-abs(h))
    return (1.0 if h >= 0 else e) / (1.0 + e)


def dpo(token_logps, counts, ref=None, beta=0.1, dpo_alpha=1.0, gamma=1.0, loss_type="sigmoid", label_smoothing=0.0):
    """token_logps: every scored token's logp in scored order (2 P sequences: P chosen, then P rejected); counts: 2 P scored counts;
    ref: the 2 P reference quantities the kernel subtracts (sums; means for "ipo") or None.  Returns a dict of float64 arrays:
    pi_c, pi_r, h, loss, reward_c, reward_r, sum_c [P]; coef [n] (float64, before the fp32 rounding); L, dpo_loss, sft_loss.
    Rejects hinge inputs within 1e-3 of the kink, so no case can flip between precisions."""
    assert loss_type in LOSS_TYPES and beta > 0 and 0 <= label_smoothing < 0.5 and not (loss_type == "ipo" and label_smoothing)
    x = np.asarray(token_logps, dtype=np.float64).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    P = counts.size // 2
    assert counts.size == 2 * P and P >= 1 and x.size == counts.sum() and (counts > 0).all()
    off = np.concatenate([[0], np.cumsum(counts)])
    sums = np.array([ordered_sum(x[off[b]:off[b + 1]]) for b in range(2 * P)])
    ipo, eps = loss_type == "ipo", float(label_smoothing)
    n = counts.astype(np.float64)
    pi = sums / n if ipo else sums
    s = 1.0 / n if ipo else np.ones(2 * P)
    rho = np.zeros(2 * P) if ref is None else np.asarray(ref, dtype=np.float64).reshape(-1)
    a_P, g_N = float(dpo_alpha) / P, float(gamma) / float(counts[:P].sum())
    out = {k: np.zeros(P) for k in ("pi_c", "pi_r", "h", "loss", "reward_c", "reward_r", "sum_c")}
    coef = np.zeros(x.size)
    for p in range(P):
        c, r = p, P + p
        u = (pi[c] - pi[r]) - (rho[c] - rho[r])
        h = beta * u
        if loss_type == "sigmoid":
            loss = -(1.0 - eps) * log_sigmoid(h) - eps * log_sigmoid(-h)
            dl = beta * (eps * sigmoid(h) - (1.0 - eps) * sigmoid(-h))
        elif loss_type == "hinge":
            t = 1.0 - h
            assert abs(t) >= 1e-3, "hinge: an input within 1e-3 of the kink"
            loss, dl = max(0.0, t), (-beta if t > 0 else 0.0)
        else:
            t = u - 1.0 / (2.0 * beta)
            loss, dl = t * t, 2.0 * t
        k = a_P * dl
        coef[off[c]:off[c + 1]] = g_N - k * s[c]
        coef[off[r]:off[r + 1]] = k * s[r]
        for name, v in (("pi_c", pi[c]), ("pi_r", pi[r]), ("h", h), ("loss", loss), ("reward_c", beta * (pi[c] - rho[c])),
                        ("reward_r", beta * (pi[r] - rho[r])), ("sum_c", sums[c])):
            out[name][p] = v
    sl, sc = ordered_sum(out["loss"]), ordered_sum(out["sum_c"])
    out.update(coef=coef, sums=sums, L=a_P * sl - g_N * sc, dpo_loss=a_P * sl, sft_loss=-sc / float(counts[:P].sum()))
    return out


def fp32_ulp(x):
    """The spacing of fp32 at |x| (np.spacing), with the floor 1e-30."""
    return np.maximum(np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64), 1e-30)


def gate_ratios(got, ref, beta, rho=None):
    """Worst ratio error / gate of each kernel gate (the gates of tests/test_preference_kernel_gpu.py): got and ref are dicts with
    pi_c, pi_r, h, loss, reward_c, reward_r [P] and coef [n]."""
    P = ref["h"].size
    rho = np.zeros(2 * P) if rho is None else np.asarray(rho, dtype=np.float64)
    scale = 4 * 2.0 ** -53 * beta * (np.abs(ref["pi_c"]) + np.abs(ref["pi_r"]) + np.abs(rho[:P]) + np.abs(rho[P:]))
    scale = np.maximum(scale, 5e-324)
    worst = {}
    for k in ("h", "reward_c", "reward_r"):
        worst[k] = float(np.max(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / scale))
    lg = 16 * 2.0 ** -52 * np.maximum(np.abs(ref["loss"]), 2.0 ** -1022)
    worst["loss"] = float(np.max(np.abs(np.asarray(got["loss"], dtype=np.float64) - ref["loss"]) / lg))
    want = ref["coef"].astype(np.float32)
    worst["coef"] = float(np.max(np.abs(np.asarray(got["coef"], dtype=np.float64) - want.astype(np.float64)) / fp32_ulp(want)))
    return worst

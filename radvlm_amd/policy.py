"""Host planning of GRPO training (numpy only): group advantages, token weights, batch assembly, sampling seeds and the record
of per-token terms the engine hands to rv_policy_loss_bf16.  The definitions are TRL's GRPOTrainer's.

Scored tokens of sample b: the positions of its SPLICED row whose shifted target is not -100, ascending.  Every per-token array of
this module is given in that order -- one 1-D array per sample, or their concatenation -- which is the order of the labelled rows in
LlavaEngine.forward, so it survives the image splice, packing, left padding and the labelled-rows gather.
"""
from dataclasses import dataclass

import numpy as np

SCALE_REWARDS = ("group", "batch", "none")
LOSS_TYPES = ("grpo", "dapo", "bnpo", "dr_grpo")


def group_advantages(rewards, num_generations, scale_rewards="group"):
    """A = (R - mean of its group) / (std + 1e-4); rewards in [prompt][generation] order.  scale_rewards: "group" (the group's std,
    ddof=1), "batch" (the std of all rewards of the call, ddof=1) or "none" (no division).  Returns float64 [len(rewards)]."""
    G = int(num_generations)
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    if G < 2:
        raise ValueError(f"num_generations must be at least 2 (a group of one has no baseline), got {num_generations}")
    if r.size == 0 or r.size % G:
        raise ValueError(f"{r.size} rewards are not a whole number of groups of {G}")
    if not np.isfinite(r).all():
        raise ValueError("rewards must be finite")
    if scale_rewards not in SCALE_REWARDS:
        raise ValueError(f"scale_rewards must be one of {SCALE_REWARDS}, got {scale_rewards!r}")
    g = r.reshape(-1, G)
    a = g - g.mean(1, keepdims=True)
    if scale_rewards == "group":
        a = a / (g.std(1, ddof=1, keepdims=True) + 1e-4)
    elif scale_rewards == "batch":
        a = a / (r.std(ddof=1) + 1e-4)
    return a.reshape(-1)


def token_weights(lengths, loss_type="dapo", max_completion_length=None):
    """The weight of every scored token of each sequence of ONE optimizer step, float64 [N]: n_i = lengths[i] scored tokens.
    "grpo": 1 / (N n_i) (a mean per sequence, then over sequences); "dapo" / "bnpo": 1 / sum n_i (a mean over the step's tokens);
    "dr_grpo": 1 / (N max_completion_length).  A sequence with n_i = 0 gets weight 0 and contributes nothing."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size == 0 or (n < 0).any():
        raise ValueError("lengths must be a non-empty list of non-negative token counts")
    N = n.size
    w = np.zeros(N, dtype=np.float64)
    live = n > 0
    if loss_type == "grpo":
        w[live] = 1.0 / (N * n[live].astype(np.float64))
    elif loss_type in ("dapo", "bnpo"):
        if n.sum() > 0:
            w[live] = 1.0 / float(n.sum())
    elif loss_type == "dr_grpo":
        if max_completion_length is None or int(max_completion_length) < 1:
            raise ValueError("dr_grpo needs max_completion_length >= 1")
        w[live] = 1.0 / (N * float(max_completion_length))
    else:
        raise ValueError(f"loss_type must be one of {LOSS_TYPES}, got {loss_type!r}")
    return w


def assemble(prompts, completions, pad_id):
    """Right-padded training rows of prompt + completion: (input_ids int64 [B, T], attention_mask bool [B, T], labels int64 [B, T]).
    Labels are -100 on the prompt and the padding and the completion's ids (its EOS included) elsewhere."""
    if len(prompts) != len(completions) or not len(prompts):
        raise ValueError(f"{len(prompts)} prompts for {len(completions)} completions")
    rows = [(np.asarray(p, dtype=np.int64).reshape(-1), np.asarray(c, dtype=np.int64).reshape(-1)) for p, c in zip(prompts, completions)]
    T = max(p.size + c.size for p, c in rows)
    ids = np.full((len(rows), T), int(pad_id), dtype=np.int64)
    am = np.zeros((len(rows), T), dtype=bool)
    lab = np.full((len(rows), T), -100, dtype=np.int64)
    for b, (p, c) in enumerate(rows):
        if p.size == 0:
            raise ValueError(f"sample {b}: empty prompt")
        n = p.size + c.size
        ids[b, :p.size], ids[b, p.size:n] = p, c
        am[b, :n] = True
        lab[b, p.size:n] = c
    return ids, am, lab


def sample_seeds(base, step, n_prompts, num_generations):
    """The sampler seed of generation g of prompt p at optimizer step `step`: base + ((step P + p) G + g), in [prompt][generation]
    order; every value is checked against [0, 2^63) (the sampler's seed range)."""
    base, step, P, G = int(base), int(step), int(n_prompts), int(num_generations)
    if base < 0 or step < 0 or P < 1 or G < 1:
        raise ValueError("sample_seeds: base and step must be >= 0, n_prompts and num_generations >= 1")
    seeds = [base + ((step * P + p) * G + g) for p in range(P) for g in range(G)]
    if seeds[-1] >= 1 << 63:
        raise ValueError(f"sample_seeds: seed {seeds[-1]} is outside [0, 2^63)")
    return seeds


@dataclass
class PolicyTerms:
    """What the GRPO loss needs beside the batch.  advantages: one float per sample, or one array per sample (per scored token), or
    the concatenation of those.  weights: likewise (None: 1 / number of scored tokens of the batch).  old_logps / ref_logps: per
    scored token (one array per sample or the concatenation) or None.  epsilon_high None: epsilon.  importance_sampling_level:
    "token" (one clipped ratio per token) or "sequence" (GSPO: one per sample, which then needs one advantage per sample)."""
    advantages: object
    weights: object = None
    old_logps: object = None
    ref_logps: object = None
    epsilon: float = 0.2
    epsilon_high: object = None
    beta: float = 0.0
    importance_sampling_level: str = "token"

    def __post_init__(self):
        check_importance_sampling_level(self.importance_sampling_level)

    @property
    def eps_high(self):
        return float(self.epsilon if self.epsilon_high is None else self.epsilon_high)

    def per_token(self, counts):
        """Validate against the scored-token count of every sample and return float64 arrays of sum(counts) entries in scored order:
        (advantages, weights, old_logps or None, ref_logps or None).  ValueError on any mismatch."""
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        B, n = counts.size, int(counts.sum())
        eps, eps_hi, beta = float(self.epsilon), self.eps_high, float(self.beta)
        if not (np.isfinite(eps) and eps >= 0 and np.isfinite(eps_hi) and eps_hi >= 0):
            raise ValueError(f"epsilon / epsilon_high must be finite and >= 0, got {self.epsilon} / {self.epsilon_high}")
        if not (np.isfinite(beta) and beta >= 0):
            raise ValueError(f"beta must be finite and >= 0, got {self.beta}")
        if beta > 0 and self.ref_logps is None:
            raise ValueError("beta > 0 needs ref_logps")
        adv = _expand("advantages", self.advantages, counts, per_sample_ok=True)
        w = np.full(n, 1.0 / n if n else 0.0) if self.weights is None else _expand("weights", self.weights, counts, per_sample_ok=True)
        if (w < 0).any():
            raise ValueError("weights must be >= 0")
        old = None if self.old_logps is None else _expand("old_logps", self.old_logps, counts)
        ref = None if self.ref_logps is None else _expand("ref_logps", self.ref_logps, counts)
        for name, a in (("old_logps", old), ("ref_logps", ref)):
            if a is not None and (a > 0).any():
                raise ValueError(f"{name} must be log-probabilities (<= 0)")
        assert adv.size == n and w.size == n and B == counts.size
        return adv, w, old, ref

    def per_sequence(self, counts):
        """The sequence level's view of the advantages: (adv_seq float64 [B], seg_off int32 [B + 1]), sample b owning the scored
        tokens [seg_off[b], seg_off[b + 1]).  One ratio per sample needs one advantage per sample: ValueError when a sample's
        per-token advantages vary.  A sample without scored tokens is legal (a masked truncated completion): it contributes
        nothing and its advantage is reported as 0."""
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        adv = _expand("advantages", self.advantages, counts, per_sample_ok=True)
        seg_off = np.concatenate([[0], np.cumsum(counts)])
        if seg_off[-1] >= 1 << 31:
            raise ValueError(f"{int(seg_off[-1])} scored tokens do not fit the kernel's int32 offsets")
        adv_seq = np.zeros(counts.size, dtype=np.float64)
        for b in range(counts.size):
            a = adv[seg_off[b]:seg_off[b + 1]]
            if a.size and (a != a[0]).any():
                raise ValueError(f"importance_sampling_level='sequence' needs one advantage per sample; sample {b}'s vary over its tokens")
            if a.size:
                adv_seq[b] = a[0]
        return adv_seq, seg_off.astype(np.int32)


IMPORTANCE_SAMPLING_LEVELS = ("token", "sequence")


def check_importance_sampling_level(level):
    if level not in IMPORTANCE_SAMPLING_LEVELS:
        raise ValueError(f"importance_sampling_level must be one of {IMPORTANCE_SAMPLING_LEVELS}, got {level!r}")
    return level


def _host(a):
    if hasattr(a, "detach"):        # a torch tensor, host or device
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _expand(name, value, counts, per_sample_ok=False):
    """value -> float64 [sum(counts)] in scored order.  Accepted: a list of B 1-D arrays (sample b's must have counts[b] entries); a
    flat array of sum(counts) entries; with per_sample_ok a scalar per sample (B floats), repeated over the sample's tokens."""
    B, n = counts.size, int(counts.sum())
    if isinstance(value, (list, tuple)) and len(value) and any(np.ndim(_host(v)) >= 1 for v in value):
        if len(value) != B:
            raise ValueError(f"{name}: {len(value)} per-sample arrays for {B} samples")
        parts = []
        for b, v in enumerate(value):
            v = _host(v)
            if v.ndim == 0 and per_sample_ok:
                v = np.full(int(counts[b]), float(v))
            if v.ndim != 1 or v.size != counts[b]:
                raise ValueError(f"{name}: sample {b} has {int(counts[b])} scored tokens, got an array of shape {v.shape}")
            parts.append(v)
        out = np.concatenate(parts) if parts else np.zeros(0)
    else:
        v = _host(value).reshape(-1) if np.ndim(_host(value)) <= 1 else None
        if v is None:
            raise ValueError(f"{name}: expected per-sample arrays or one flat array, got shape {np.shape(_host(value))}")
        if per_sample_ok and v.size == B:      # B == n: one token per sample, both readings agree
            if not np.isfinite(v).all():       # also the value of a sample without scored tokens
                raise ValueError(f"{name} must be finite")
            out = np.repeat(v, counts)
        elif v.size == n:
            out = v
        else:
            b_short = _first_mismatch(v.size, counts)
            raise ValueError(f"{name}: {v.size} entries for {n} scored tokens ({B} samples; the array ends inside sample {b_short})")
    if not np.isfinite(out).all():
        raise ValueError(f"{name} must be finite")
    return out


def _first_mismatch(size, counts):
    ends = np.cumsum(counts)
    b = int(np.searchsorted(ends, size, side="right"))
    return min(b, counts.size - 1)

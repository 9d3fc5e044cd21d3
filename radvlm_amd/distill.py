"""Host planning of knowledge distillation (numpy only): the record of terms the engine hands to rv_distill_loss_bf16 and the
per-step draw that decides whether a GKD step trains on the dataset's answers or on the student's own samples.  The definitions are
TRL's GKDTrainer's: the generalised Jensen-Shannon divergence with interpolation `beta` (0: forward KL, 1: reverse KL) of the two
models' temperature-scaled distributions over the whole vocabulary, averaged over the scored tokens; `lmbda` the on-policy fraction.

Scored tokens and their order are policy.py's: the positions of a sample's spliced row whose shifted target is not -100, ascending,
sample by sample -- row j of the teacher's logits is scored token j.
"""
from dataclasses import dataclass

import numpy as np

from .policy import _expand

_M64 = (1 << 64) - 1


def check_beta(beta):
    b = float(beta)
    if not 0.0 <= b <= 1.0:                      # NaN fails both comparisons
        raise ValueError(f"beta must lie in [0, 1] (0: forward KL, 1: reverse KL), got {beta}")
    return b


def check_temperature(temperature):
    t = float(temperature)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"temperature must be finite and > 0, got {temperature}")
    return t


def check_lmbda(lmbda):
    v = float(lmbda)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"lmbda must lie in [0, 1] (the fraction of on-policy steps), got {lmbda}")
    return v


@dataclass
class DistillTerms:
    """What the distillation loss needs beside the batch.  teacher_logits: a bf16 device tensor [n_scored, >= vocab] with unit column
    stride, row j the teacher's logits at scored token j (LlavaEngine.label_logits gives it).  weights: one float per sample, one array
    per sample, or the concatenation in scored order (None: 1 / number of scored tokens of the batch -- TRL's batchmean)."""
    teacher_logits: object
    beta: float = 0.5
    temperature: float = 1.0
    weights: object = None
    teacher_scored: object = None        # the teacher's scored count per sample, when it scored the batch itself: must equal the student's

    def __post_init__(self):
        self.beta, self.temperature = check_beta(self.beta), check_temperature(self.temperature)

    def per_token(self, counts, vocab):
        """Validate against the scored-token count of every sample and the student's vocabulary; returns the weights as float64
        [sum(counts)] in scored order.  ValueError on any mismatch."""
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        n = int(counts.sum())
        if self.teacher_scored is not None:
            check_same_scored(counts, self.teacher_scored)
        t = self.teacher_logits
        shape, dtype = tuple(getattr(t, "shape", ())), str(getattr(t, "dtype", None))
        if not dtype.endswith("bfloat16"):
            raise ValueError(f"teacher_logits must be bf16, got {dtype}")
        if len(shape) != 2 or shape[0] != n or shape[1] < int(vocab):
            raise ValueError(f"teacher_logits must be [n_scored = {n}, >= vocab = {int(vocab)}], got {list(shape)}")
        w = np.full(n, 1.0 / n if n else 0.0) if self.weights is None else _expand("weights", self.weights, counts, per_sample_ok=True)
        if (w < 0).any():
            raise ValueError("weights must be >= 0")
        return w


def check_same_scored(student_counts, teacher_counts):
    """The teacher scored the same batch: both models must see the same number of scored tokens in every sample (models that splice
    another number of image tokens may truncate a row elsewhere).  ValueError names the first sample that differs."""
    s, t = np.asarray(student_counts, dtype=np.int64).reshape(-1), np.asarray(teacher_counts, dtype=np.int64).reshape(-1)
    if s.size != t.size:
        raise ValueError(f"the teacher scored {t.size} samples, the student {s.size}")
    bad = np.flatnonzero(s != t)
    if bad.size:
        b = int(bad[0])
        raise ValueError(f"sample {b}: the teacher scores {int(t[b])} tokens, the student {int(s[b])} (different image-token counts or "
                         "sequence limits); distillation pairs the scored tokens one to one")


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def step_uniform(seed, step):
    """The uniform of optimizer step `step` under `seed`, in (0, 1): a counter-based draw (two rounds of splitmix64 on Python integers),
    a function of (seed, step) alone -- no generator state, so a resumed run draws what the uninterrupted one drew, and nothing else
    that is drawn (the sampler's seeds, the data order) moves it."""
    seed, step = int(seed), int(step)
    if seed < 0 or step < 0:
        raise ValueError("step_uniform: seed and step must be >= 0")
    bits = _splitmix64(_splitmix64(seed & _M64) ^ ((step * 0xD1342543DE82EF95) & _M64) ^ 0x474B44)      # "GKD": apart from other users of the seed
    return ((bits >> 11) + 0.5) / 9007199254740992.0


def on_policy_step(seed, step, lmbda):
    """True when step `step` trains on the student's own samples: step_uniform(seed, step) < lmbda.  lmbda 0: never; 1: always."""
    return step_uniform(seed, step) < check_lmbda(lmbda)

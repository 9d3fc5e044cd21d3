"""Host planning of DPO preference training (numpy only): the pair batch, the scored-order offsets and the record of per-sequence
terms the engine hands to rv_dpo_pairs_f64, plus the text half of the reference's DPO record contract (train_dpo.py:1155-1183,
1239-1305).  `trl` is not a dependency; the objective is stated in include/radvlm_hip.h and DESIGN.md section 5e.

A batch of P pairs runs as 2 P sequences, TRL's concatenated_forward: sample p is prompt + chosen, sample P + p prompt + rejected.
Scored tokens and their order are policy.py's: the positions of a sample's spliced row whose shifted target is not -100, ascending,
sample by sample.
"""
import re
from dataclasses import dataclass

import numpy as np

LOSS_TYPES = ("sigmoid", "hinge", "ipo")          # the codes of rv_dpo_pairs_f64, in order


def pair_offsets(counts):
    """Scored counts per sequence -> seg_off int32 [len(counts) + 1] in scored order (seg_off[0] = 0)."""
    n = np.asarray(counts, dtype=np.int64).reshape(-1)
    if n.size == 0 or (n < 0).any():
        raise ValueError("counts must be a non-empty list of non-negative token counts")
    off = np.concatenate([[0], np.cumsum(n)])
    if off[-1] >= 1 << 31:
        raise ValueError(f"{int(off[-1])} scored tokens do not fit int32 offsets")
    return off.astype(np.int32)


def concatenate_pairs(chosen_input_ids, chosen_attention_mask, chosen_labels, rejected_input_ids, rejected_attention_mask, rejected_labels,
                      pad_id=0):
    """The 2 P right-padded rows of a pair batch: (input_ids int64 [2P, T], attention_mask bool [2P, T], labels int64 [2P, T]) with
    T the longer of the two halves; the shorter half is padded with pad_id / False / -100.  Rows 0 .. P-1 are the chosen ones."""
    ci, ri = np.asarray(chosen_input_ids, dtype=np.int64), np.asarray(rejected_input_ids, dtype=np.int64)
    halves = [(ci, np.asarray(chosen_attention_mask).astype(bool), np.asarray(chosen_labels, dtype=np.int64)),
              (ri, np.asarray(rejected_attention_mask).astype(bool), np.asarray(rejected_labels, dtype=np.int64))]
    if ci.ndim != 2 or ri.ndim != 2 or ci.shape[0] != ri.shape[0] or ci.shape[0] < 1:
        raise ValueError(f"chosen rows {ci.shape} and rejected rows {ri.shape} are not the two halves of a pair batch")
    for name, (i, a, l) in zip(("chosen", "rejected"), halves):
        if a.shape != i.shape or l.shape != i.shape:
            raise ValueError(f"{name}: input_ids {i.shape}, attention_mask {a.shape} and labels {l.shape} differ in shape")
    P, T = ci.shape[0], max(ci.shape[1], ri.shape[1])
    ids = np.full((2 * P, T), int(pad_id), dtype=np.int64)
    am = np.zeros((2 * P, T), dtype=bool)
    lab = np.full((2 * P, T), -100, dtype=np.int64)
    for h, (i, a, l) in enumerate(halves):
        ids[h * P:(h + 1) * P, :i.shape[1]] = i
        am[h * P:(h + 1) * P, :i.shape[1]] = a
        lab[h * P:(h + 1) * P, :i.shape[1]] = l
    return ids, am, lab


def _host(a):
    if hasattr(a, "detach"):        # a torch tensor, host or device
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64).reshape(-1)


@dataclass
class PreferenceTerms:
    """What the DPO loss needs beside the pair batch.  ref_chosen_logps / ref_rejected_logps: the reference model's SUMMED log-prob of
    every chosen / rejected answer (P floats each; sequence_logps() gives them -- sums for every loss type, "ipo" divides by the
    scored counts itself), or None with reference_free."""
    ref_chosen_logps: object = None
    ref_rejected_logps: object = None
    beta: float = 0.1
    dpo_alpha: float = 1.0
    gamma: float = 1.0
    loss_type: str = "sigmoid"
    label_smoothing: float = 0.0
    reference_free: bool = False

    def check(self):
        beta, eps = float(self.beta), float(self.label_smoothing)
        if self.loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {LOSS_TYPES}, got {self.loss_type!r}")
        if not (np.isfinite(beta) and beta > 0):
            raise ValueError(f"beta must be finite and > 0, got {self.beta}")
        if not (0 <= eps < 0.5):
            raise ValueError(f"label_smoothing must lie in [0, 0.5), got {self.label_smoothing}")
        if self.loss_type == "ipo" and eps != 0:
            raise ValueError("label_smoothing is not defined for loss_type 'ipo'")
        if not (np.isfinite(float(self.dpo_alpha)) and np.isfinite(float(self.gamma))):
            raise ValueError("dpo_alpha and gamma must be finite")
        if not self.reference_free and (self.ref_chosen_logps is None or self.ref_rejected_logps is None):
            raise ValueError("ref_chosen_logps and ref_rejected_logps are required unless reference_free=True")

    def per_pair(self, counts):
        """Validate against the scored count of each of the 2 P sequences.  Returns (P, seg_off int32 [2P + 1], rho float64 [2P] or None,
        alpha_over_P, gamma_over_Nc); rho is the quantity the pair kernel subtracts (the mean for "ipo").  ValueError on a pair
        without a scored chosen or rejected token and on reference log-probs that are missing, of the wrong length or non-finite."""
        self.check()
        counts = np.asarray(counts, dtype=np.int64).reshape(-1)
        if counts.size < 2 or counts.size % 2:
            raise ValueError(f"a pair batch has 2 P sequences, got {counts.size}")
        P = counts.size // 2
        for name, n in (("chosen", counts[:P]), ("rejected", counts[P:])):
            if (n < 1).any():
                raise ValueError(f"pair {int(np.nonzero(n < 1)[0][0])}: the {name} answer has no scored token")
        rho = None
        if not self.reference_free:
            parts = []
            for name, v in (("ref_chosen_logps", self.ref_chosen_logps), ("ref_rejected_logps", self.ref_rejected_logps)):
                v = _host(v)
                if v.size != P:
                    raise ValueError(f"{name}: {v.size} entries for {P} pairs")
                if not np.isfinite(v).all():
                    raise ValueError(f"{name} must be finite")
                parts.append(v)
            rho = np.concatenate(parts)
            if self.loss_type == "ipo":
                rho = rho / counts.astype(np.float64)
        n_c = int(counts[:P].sum())
        return P, pair_offsets(counts), rho, float(self.dpo_alpha) / P, float(self.gamma) / n_c


# ---------------------------------------------------------------------------------------------- the record contract (text half)
IMAGE_MARK = "<image>"


def rewrite_prompt(prompt):
    """train_dpo.py:1159-1163: every earlier <image> mark is removed, the rest stripped, and one mark put in front."""
    return IMAGE_MARK + "\n" + str(prompt).replace(IMAGE_MARK, "").strip()


def make_conv(prompt, answer):
    """train_dpo.py:475-485: one answer as a two-turn conversation."""
    return [{"from": "human", "value": prompt}, {"from": "gpt", "value": answer}]


def check_record(rec, i=0):
    missing = [k for k in ("prompt", "chosen", "rejected") if k not in rec]
    if missing:
        raise ValueError(f"record {i}: a DPO record needs 'prompt', 'chosen', 'rejected' (and 'image'); missing {missing}")
    if "video" in rec:
        raise NotImplementedError(f"record {i}: video records are outside the DPO path")
    return rec


def record_words(rec):
    """The text length the reference's samplers group DPO records by (train_dpo.py:982-990, without its unused "answer" column):
    whitespace-separated words of prompt + chosen + rejected."""
    return sum(len(re.findall(r"\S+", str(rec[k]))) for k in ("prompt", "chosen", "rejected"))

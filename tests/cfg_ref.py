"""Host reference of classifier-free guidance for the tests of rv_cfg_guide_rows_f32, generate(guidance_scale=) and generate_batch().
hf_guided runs the INSTALLED transformers UnbatchedClassifierFreeGuidanceLogitsProcessor on a stub model that returns the given
unconditional logits, so the pin is HF's own code (as logits_ref.py restates the other processors); combine is the numpy fp32
restatement of its last line, three separately rounded operations in HF's order with the scale rounded to fp32."""
import numpy as np
import torch


class _Out(dict):
    """What HF's processor reads of a model output: .logits [B, T, V] and .get("past_key_values")."""

    @property
    def logits(self):
        return self["logits"]


class StubModel:
    """Returns the given unconditional logits as the last position's logits; records every call's input_ids and attention_mask."""

    def __init__(self, uncond_logits):
        self.uncond = uncond_logits
        self.calls = []

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        self.calls.append(dict(input_ids=None if input_ids is None else input_ids.clone(),
                               attention_mask=None if attention_mask is None else attention_mask.clone()))
        return _Out(logits=self.uncond[:, None, :], past_key_values=None)


def _rows(x, dtype):
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().cpu().to(dtype)
    return x[None] if x.dim() == 1 else x


def hf_guided(cond_logits, uncond_logits, g, dtype=torch.float32, input_ids=None, negative_prompt_ids=None, stub=None):
    """HF's guided scores of one step: cond_logits / uncond_logits [rows, V] (or [V]) raw logits, converted to `dtype`; g the guidance
    scale as the caller passes it (a Python number).  input_ids: what HF's loop hands the processor ([rows, T]; default one token per
    row).  stub: a StubModel to inspect afterwards.  Returns a tensor [rows, V] of `dtype`."""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    c, u = _rows(cond_logits, dtype), _rows(uncond_logits, dtype)
    stub = StubModel(u) if stub is None else stub
    stub.uncond = u
    if input_ids is None:
        input_ids = torch.zeros(c.shape[0], 1, dtype=torch.long)
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(g, stub, unconditional_ids=negative_prompt_ids)
    with torch.no_grad():
        return proc(torch.as_tensor(input_ids), c.clone())


def torch_log_softmax32(x):
    """torch's fp32 log-softmax of each row, numpy fp32."""
    return torch.log_softmax(_rows(x, torch.float32), dim=-1).numpy()


def combine(lc, lu, g):
    """fl(fl(g32 * fl(lc - lu)) + lu) on numpy fp32 arrays, g32 = fl32(g): HF's `g * (scores - uncond) + uncond`."""
    lc, lu = np.asarray(lc, dtype=np.float32), np.asarray(lu, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = lc - lu
        p = np.float32(g) * d
        out = p + lu
    assert d.dtype == p.dtype == out.dtype == np.float32
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def log_softmax64(x):
    """float64 log-softmax of each row of fp32 logits (numpy)."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def error_bound(lc64, lu64, g, n):
    """The bound csrc/cfg.hip derives for |kernel - exact|, per entry, from the exact (float64) log-softmax values lc64 / lu64, the
    caller's g and the row width n:  (1 + 2^-20) (|g| E(lc) + |1 - g| E(lu) + |fl32(g) - g| |D| + u (2 |g| |D| + |exact|)),
    E(l) = u (2 |l| + 4 ln n + 3), u = 2^-24, D = lc - lu, exact = g D + lu."""
    u = 2.0 ** -24
    E = lambda l: u * (2 * np.abs(l) + 4 * np.log(n) + 3)
    g = float(g)
    D = lc64 - lu64
    exact = g * D + lu64
    return (1 + 2.0 ** -20) * (abs(g) * E(lc64) + abs(1 - g) * E(lu64) + abs(float(np.float32(g)) - g) * np.abs(D) +
                               u * (2 * abs(g) * np.abs(D) + np.abs(exact)))


G_LIST = (0, 0.5, 1.5, 2, 7.5, -1, 1 / 3)


def logits_rows(rng, rows, n, kind):
    """Test rows, fp32 [rows, n]: 'flat' (standard normal) or 'peaked' (x 8)."""
    x = rng.standard_normal((rows, n)).astype(np.float32)
    return x * np.float32(8) if kind == "peaked" else x

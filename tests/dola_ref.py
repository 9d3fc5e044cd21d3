"""DoLa ("decoding by contrasting layers") restated in torch on the CPU: the reference of the DoLa tests.

The rule is HF's _dola_decoding / _dola_select_contrast / _relative_top_filter (transformers 4.43 - 4.5x; the installed 5.x moved it
out of the package, so there is nothing to import) with the differences DESIGN.md 5b "DoLa" lists: every row chooses its own layer,
out-of-range layers raise, the scores are fp32.  Nothing here imports the code under test except where a function says so."""
import math

import numpy as np
import torch

RELATIVE_TOP = 0.1
LOG_RT = np.float32(math.log(RELATIVE_TOP))          # fl32(ln relative_top)
MAX_LAYERS = 16
U = 2.0 ** -24


def candidate_layers(spec, L, tied=False):
    """The candidate layer numbers of `dola_layers=spec` on a decoder of L layers; ValueError as the issue lists them."""
    start = (2 if L > 2 else (1 if L == 2 else 0)) if tied else 0
    if isinstance(spec, str):
        if spec == "low":
            out = list(range(start, L // 2, 2)) if L <= 40 else list(range(start, 20, 2))
        elif spec == "high":
            out = list(range(L // 2, L, 2)) if L <= 40 else list(range(L - 20, L, 2))
        else:
            raise ValueError(spec)
    elif isinstance(spec, (list, tuple)):
        if any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) for c in spec):
            raise ValueError(spec)
        out = [int(c) for c in spec]
    else:
        raise ValueError(spec)
    if not out or len(set(out)) != len(out) or min(out) < 0 or max(out) >= L or len(out) > MAX_LAYERS:
        raise ValueError(spec)
    return out


def jsd64(lf, lq):
    """J of the issue in float64 from log-softmax values lf [..., V] and lq [..., V] (any float dtype): 0.5 * (mean M (log M - lf) +
    mean M (log M - lq)), a term with M == 0 being 0."""
    lf, lq = lf.double(), lq.double()
    M = 0.5 * (lf.exp() + lq.exp())
    lm = torch.where(M > 0, M.clamp_min(1e-320).log(), torch.zeros_like(M))
    t = torch.where(M > 0, M * ((lm - lf) + (lm - lq)), torch.zeros_like(M))
    return 0.5 * t.mean(-1)


def select(J):
    """argmax over the last axis, an exact tie going to the lowest index.  J [..., n_layers] -> int64 [...]."""
    J = np.asarray(J)
    return np.argmax(J, axis=-1).astype(np.int64)          # numpy's argmax returns the first maximum


def contrast(lf, lb):
    """The relative-top filter and the contrast on given fp32 log-softmax rows lf, lb [..., V]: -inf where lf < fl32(max lf + fl32(ln
    0.1)), else fl32(lf - lb)."""
    assert lf.dtype == torch.float32 and lb.dtype == torch.float32
    thresh = lf.max(-1, keepdim=True).values + torch.tensor(LOG_RT)        # fp32 + fp32: one rounding
    assert thresh.dtype == torch.float32
    return torch.where(lf < thresh, torch.full_like(lf, float("-inf")), lf - lb)


def dola_rows(lf, lqs):
    """One step on fp32 log-softmax rows: lf [B, V], lqs [n, B, V].  Returns (contrasted fp32 [B, V], chosen int64 [B], J float64
    [B, n] or None for n == 1)."""
    n, B = lqs.shape[0], lf.shape[0]
    if n == 1:
        ch, J = np.zeros(B, dtype=np.int64), None
    else:
        J = torch.stack([jsd64(lf, lqs[k]) for k in range(n)], 1).numpy()
        ch = select(J)
    lb = lqs[torch.from_numpy(ch), torch.arange(B)]
    return contrast(lf, lb), ch, J


def jsd_error_bound(lf, lq):
    """The bound on |J^ - J| of csrc/dola.hip's header, evaluated in float64 from log-softmax values lf, lq [..., V] (the float64
    images of the rows the kernel saw): per leading index."""
    lf, lq = lf.double(), lq.double()
    V = lf.shape[-1]
    E = lambda l: U * (2 * l.abs() + 4 * math.log(V) + 3)
    X = lambda l: U * (l.abs() + 2)
    p, q = lf.exp(), lq.exp()
    M = 0.5 * (p + q)
    lm = torch.where(M > 0, M.clamp_min(1e-320).log(), torch.zeros_like(M))
    A = (lm - lf) + (lm - lq)
    Ab = (lm - lf).abs() + (lm - lq).abs()
    T = M * A
    dlf, dlq = (0.5 * p * A + 0.5 * (p - q)).abs(), (0.5 * q * A + 0.5 * (q - p)).abs()          # |dT/dlf|, |dT/dlq|
    dM = 0.5 * (p * X(lf) + q * X(lq)) + U * M
    Bv = dlf * E(lf) + dlq * E(lq) + (A.abs() + 2) * dM + 8 * U * M * lm.abs() + 2 * U * M * Ab + U * T.abs()
    Bv = torch.where(M > 0, Bv, torch.zeros_like(Bv))
    J = 0.5 * torch.where(M > 0, T, torch.zeros_like(T)).mean(-1)
    return (1 + 2.0 ** -10) * 0.5 * Bv.mean(-1) + U * J.abs() + 2.0 ** -100


def dola_generate_ref(engine_like, ids, layers, T, eos=(), pad=0, process=None, log_softmax=None, pick=None):
    """The generation loop in the plainest form, for the host tests: engine_like has prefill(ids, am, images, sizes, max_new_tokens=,
    tap_layers=) -> (cache, logits [B, V], cand [n, B, V]) and decode_step(cache, tokens, tap_layers=) -> (logits, cand).
    process(row fp32 numpy [V], tokens so far) -> the processed row (None: identity); log_softmax(rows fp32 [R, V]) -> fp32 (None:
    torch's); pick(scores [B, V], t) -> tokens (None: argmax).
    Returns dict(sequences [B, steps], scores [steps][B, V], logits [steps][B, V], layers int64 [B, steps])."""
    log_softmax = log_softmax or (lambda x: torch.log_softmax(x, -1))
    cache, f, c = engine_like.prefill(ids, None, None, None, max_new_tokens=T, tap_layers=tuple(layers))
    B = f.shape[0]
    alive = np.ones(B, dtype=bool)
    seq, scores, raw, lay = [], [], [], []
    for t in range(T):
        raw.append(f.clone())
        lf = log_softmax(f.clone())
        lqs = torch.stack([log_softmax(c[k].clone()) for k in range(c.shape[0])])
        out, ch, _ = dola_rows(lf, lqs)
        if process is not None:
            hist = np.array(seq).reshape(t, B).T if t else np.zeros((B, 0), dtype=np.int64)
            out = torch.stack([torch.from_numpy(process(out[b].numpy().copy(), hist[b])) for b in range(B)])
        scores.append(out)
        tok = (out.argmax(-1) if pick is None else pick(out, t)).numpy().astype(np.int64)
        tok = np.where(alive, tok, pad)
        lay.append(np.where(alive, np.asarray(layers, dtype=np.int64)[ch], -1))
        seq.append(tok)
        alive = alive & ~np.isin(tok, list(eos))
        if not alive.any() or t == T - 1:
            break
        f, c = engine_like.decode_step(cache, torch.from_numpy(tok), tap_layers=tuple(layers))
    return dict(sequences=np.stack(seq, 1), scores=scores, logits=raw, layers=np.stack(lay, 1))

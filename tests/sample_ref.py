"""numpy float64 restatement of seeded sampling (rv_sample_rows_f32; HF's warpers temperature -> top-k -> top-p -> min-p, then one
counter-based draw), for the tests of the kernel and of generate(do_sample=True, seed=...).  One row at a time.  The only fp32 step is
the temperature division, whose quotient the kernel reproduces bit for bit; everything after it is float64 on that quotient."""
import numpy as np

from radvlm_amd import portable_rng

DEPTH = 1                                        # include/radvlm_hip.h, rv_sample_rows_f32: fp32 additions a term of the CDF sum passes through
DELTA = (DEPTH + 4) * 2.0 ** -23                 # the band the kernel's documented order allows around a cut or a CDF boundary


def uniform(seed, t):
    """u(seed, t) in (0, 1): an odd multiple of 2^-25, exact in float64."""
    return (float(int(portable_rng._stream(int(seed), 0, int(t) + 1)[int(t)]) >> 40) + 0.5) * 2.0 ** -24


def tail_mass(s64, mask):
    """Per entry of `mask`: sum of softmax(s over mask)_j over the j with s_j <= s_i (the entry itself included); 0 outside the mask."""
    idx = np.flatnonzero(mask)
    v = s64[idx]
    e = np.exp(v - v.max())
    order = np.argsort(v, kind="stable")
    cum = np.cumsum(e[order]) / e.sum()
    pos = np.searchsorted(v[order], v, side="right") - 1          # equal scores share the tail of the last of them
    out = np.zeros(s64.shape, dtype=np.float64)
    out[idx] = cum[pos]
    return out


def warp_row(x, T=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """x: processed fp32 scores [n].  Returns (s, kept, tail, q): s = fp32 x / T; kept: the mask the warpers leave; tail: the inclusive
    tail mass of each entry that survives top-k, under the softmax over those (what top-p compares with 1 - top_p; 0 for the others);
    q: float64 softmax over the kept set."""
    s = (np.asarray(x, dtype=np.float32) / np.float32(T)).astype(np.float32)
    s64 = s.astype(np.float64)
    n = s.size
    kept = np.ones(n, dtype=bool)
    if top_k and top_k < n:
        v = np.partition(s, n - top_k)[n - top_k]                 # the k-th largest
        kept &= s >= v
    tail = tail_mass(s64, kept)
    if top_p < 1.0:
        keep_p = tail > 1.0 - float(top_p)
        keep_p[np.argmax(s)] = True                               # min_tokens_to_keep = 1
        kept &= keep_p
    if min_p > 0.0:
        e = np.where(kept, np.exp(s64 - s64[kept].max()), 0.0)    # p_i / max p
        kept &= ~(e < float(min_p))
    e = np.where(kept, np.exp(s64 - s64[kept].max()), 0.0)
    return s, kept, tail, e / e.sum()


def cdf(s, kept):
    """float64 CDF in token-id order of the softmax of s over `kept`."""
    s64 = np.asarray(s, dtype=np.float64)
    e = np.where(kept, np.exp(s64 - s64[kept].max()), 0.0)
    return np.cumsum(e) / e.sum()


def draw(q, kept, u):
    """The lowest id i with sum{q_j : j <= i, j kept} > u."""
    c = np.cumsum(np.where(kept, q, 0.0))
    i = int(np.searchsorted(c, u, side="right"))
    return min(i, int(np.flatnonzero(kept)[-1]))

"""numpy float64 restatement of speculative sampling's accept / resample step (rv_spec_accept_rows_f32; HF's _speculative_sampling),
one group at a time, built on sample_ref's cdf / draw and on portable_rng's streams: tag 0 the resample / bonus draw, tag 1 the accept
tests, tag 2 the draft model's own draws.  Rows are warped scores: finite where kept, -inf where removed."""
from fractions import Fraction

import numpy as np

import sample_ref
from radvlm_amd import portable_rng

DELTA = 2.0 ** -25                               # include/radvlm_hip.h, rv_spec_accept_rows_f32: the band, relative to the larger side
assert DELTA <= sample_ref.DELTA
TAG_DRAW, TAG_ACCEPT, TAG_DRAFT = 0, 1, 2
_M64 = (1 << 64) - 1


def uniform(seed, tag, t):
    """u(seed, tag, t) in (0, 1): an odd multiple of 2^-25 from the top 24 bits of portable_rng._stream(seed, tag, t + 1)[t]."""
    with np.errstate(over="ignore"):
        base = portable_rng._splitmix64(np.array([(int(seed) * 1000003 + int(tag)) & _M64], dtype=np.uint64))
        v = portable_rng._splitmix64(np.array([int(t)], dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + base)[0]
    return (float(int(v) >> 40) + 0.5) * 2.0 ** -24


def usable(row):
    row = np.asarray(row)
    return not (np.isnan(row).any() or np.isposinf(row).any() or not np.isfinite(row).any())


def softmax(row):
    """float64 softmax over the finite entries of a usable row (0 elsewhere)."""
    s = np.asarray(row, dtype=np.float64)
    kept = np.isfinite(s)
    e = np.where(kept, np.exp(np.where(kept, s, 0.0) - s[kept].max()), 0.0)
    return e / e.sum()


def rule_probs(p, q):
    """The rule on two distributions (sequences of numbers or Fractions): (a, r), a[x] = the probability that a draft x is accepted,
    min(1, p[x] / q[x]) and 0 where p[x] == 0 (1 where q[x] == 0 < p[x]: such an x is never drafted); r = the distribution the token
    is drawn from after a rejection, max(0, p - q) normalised, and p itself when that is identically 0."""
    one = Fraction(1) if isinstance(p[0], Fraction) else 1.0
    a = [0 * one if px == 0 else (one if qx <= px else px / qx) for px, qx in zip(p, q)]
    d = [max(px - qx, 0 * one) for px, qx in zip(p, q)]
    tot = sum(d)
    r = [v / tot for v in d] if tot > 0 else list(p)
    return a, r


def residual(P, Q):
    """rule_probs' r on float64 arrays."""
    d = np.maximum(P - Q, 0.0)
    return d / d.sum() if d.sum() > 0 else P


def accept_group(p_rows, q_rows, draft, seed, t0, tags=(TAG_DRAW, TAG_ACCEPT)):
    """One group: p_rows [R, n], q_rows [R - 1, n], draft [R - 1].  Returns dict(n_accept, token, logprob, margins, cdf, u_r): margins[i]
    = |u Q(x) - P(x)| / max(u Q(x), P(x)) of every accept test that was made (inf where it cannot flip: a draft out of range or with
    P(x) = 0), cdf = the float64 CDF in token-id order of the distribution the token was drawn from.  An unusable row on the path:
    token -1, logprob NaN."""
    p_rows, R = np.asarray(p_rows), len(p_rows)
    n = p_rows.shape[1]
    a, margins = 0, []
    dead = False
    while a < R - 1:
        if not usable(p_rows[a]) or not usable(q_rows[a]):
            dead = True
            break
        x = int(draft[a])
        if not 0 <= x < n:
            margins.append(np.inf)
            break
        P, Q = softmax(p_rows[a]), softmax(q_rows[a])
        if P[x] == 0:
            margins.append(np.inf)
            break
        lhs, rhs = uniform(seed, tags[1], t0 + a) * Q[x], P[x]
        margins.append(abs(lhs - rhs) / max(lhs, rhs))
        if not lhs <= rhs:
            break
        a += 1
    if dead or not usable(p_rows[a]) or (a < R - 1 and not usable(q_rows[a])):
        return dict(n_accept=a, token=-1, logprob=float("nan"), margins=margins, cdf=None, u_r=None)
    P = softmax(p_rows[a])
    dist = P
    if a < R - 1:
        dist = residual(P, softmax(q_rows[a]))
    u = uniform(seed, tags[0], t0 + a)
    kept = dist > 0
    tok = sample_ref.draw(dist, kept, u)
    return dict(n_accept=a, token=tok, logprob=float(np.log(P[tok])) if P[tok] > 0 else float("-inf"), margins=margins,
                cdf=np.cumsum(dist), u_r=u)


def accept_test(p_row, q_row, x, seed, t, tag=TAG_ACCEPT):
    """(accepted, margin) of one accept test on usable rows; margin as in accept_group."""
    P, Q = softmax(p_row), softmax(q_row)
    if not 0 <= x < len(P) or P[x] == 0:
        return False, np.inf
    lhs, rhs = uniform(seed, tag, t) * Q[x], P[x]
    return bool(lhs <= rhs), abs(lhs - rhs) / max(lhs, rhs)


def draw_cdf(p_rows, q_rows, a):
    """The float64 CDF in token-id order of the distribution the token after `a` accepted drafts is drawn from, and log P_a."""
    P = softmax(p_rows[a])
    dist = P if a == len(p_rows) - 1 else residual(P, softmax(q_rows[a]))
    with np.errstate(divide="ignore"):
        return np.cumsum(dist), np.log(P)


def near_boundary(res):
    """How many of a group's decisions fall within DELTA of a boundary: its accept tests, and its draw against the CDF."""
    k = sum(m <= DELTA for m in res["margins"])
    if res["cdf"] is not None:
        k += int((np.abs(res["cdf"] - res["u_r"]) <= DELTA).any())
    return k


def _keep_top(row, top):
    """-inf outside the `top` largest finite entries of the row (ties with the cut stay), in place."""
    fin = np.flatnonzero(np.isfinite(row))
    if top < fin.size:
        cut = np.partition(row[fin], fin.size - top)[fin.size - top]
        row[fin[row[fin] < cut]] = -np.inf
    return row


def warped_rows(seed, rows, n, top=None, scale=3.0):
    """`rows` score rows as the sampler leaves them: normal scores times `scale`, -inf outside each row's `top` largest (None: all
    kept).  Three rows are drawn; row r is row r % 3 rotated by a multiple of 7919 ids, so that many long rows stay cheap to make."""
    base = portable_rng.normal(seed, 7, (min(rows, 3), n), std=scale)
    if top is not None:
        for b in base:
            _keep_top(b, top)
    return np.stack([np.roll(base[r % 3], 7919 * (r // 3)) for r in range(rows)]) if rows else np.zeros((0, n), dtype=np.float32)


def kernel_case(n, R, groups, seed=0):
    """The inputs of the GPU kernel test for (n, R, groups), shared with the host test of the band's occupancy: p [groups * R, n], q
    [groups * (R - 1), n], draft int32 [groups, R - 1] drawn from the q rows with the draft stream, seeds and t0.  The q rows are the
    p rows plus a perturbation, on a narrower kept set, so that accepted and rejected drafts both occur."""
    base = 1000 * seed + 17 * n + 3 * R + groups
    top = None if n <= 8 else max(4, n // 3)
    p = warped_rows(base, groups * R, n, top)
    nq = groups * (R - 1)
    q = np.zeros((nq, n), dtype=np.float32)
    draft = np.zeros((groups, R - 1), dtype=np.int32)
    seeds = np.array([(base * 7919 + 13 * g) % (1 << 62) for g in range(groups)], dtype=np.int64)
    t0 = np.array([5 + 11 * g for g in range(groups)], dtype=np.int32)
    noise = warped_rows(base + 1, nq, n, None, scale=0.7)
    for g in range(groups):
        for i in range(R - 1):
            row = p[g * R + i] + np.roll(noise[g * (R - 1) + i], 31 * (i + 1))
            if top is not None:                                   # a draft row keeps fewer entries than the target's
                _keep_top(row, max(2, top * 3 // 4))
            q[g * (R - 1) + i] = row
            Q = softmax(row)
            draft[g, i] = sample_ref.draw(Q, Q > 0, uniform(int(seeds[g]), TAG_DRAFT, int(t0[g]) + i))
    return p, q, draft, seeds, t0

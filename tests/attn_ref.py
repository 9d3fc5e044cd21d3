"""float64 reference of ONE call of the training attention (radvlm_amd/csrc/attention.hip), forward and backward, with a per-element error
budget for every output, the input families that stress the softmax rescale, and a CPU emulation of the natural-layout kernels' rounding
points.  Plain torch on the CPU on the bf16-rounded inputs; nothing here touches a GPU, so tests/test_attn_ref_host.py pins the reference to
float64 autograd of the oracle without one, and tests/test_attention_edges_gpu.py holds the kernels to it.

Budgets.  With P = softmax(scale Q K^T + mask), dP = dO V^T, delta_i = sum_e dO_ie O_ie, D_i = sum_e |dO_ie| |O_ie| and
W_ij = P_ij (|dP_ij - delta_i| + D_i):

    A_out = P |V|        A_dV = P^T |dO|        A_dQ = scale W |K|        A_dK = scale W^T |Q|

(grouped-query heads: A_dK and A_dV are summed over the group).  A is what ONE relative rounding of the P (or dS) operand can move the
element by: the kernels round P and dS = P (dP - delta) to bf16 before the second product, and form delta from the bf16 `out`, whose
rounding moves delta by up to 2^-8 D -- that is the D term of W.  The gate of an element is

    |got - ref| <= (roundings 2^-8 + 2^-16) A + 1e-30

2^-8 bounds the relative error of one round-to-nearest to bf16; `roundings` counts the bf16 roundings on the path: 2 for out and dV (P, the
store), 2 for dQ and dK (the dS rounding and the delta error share one 2^-8 W term; the store), 3 for dK / dV when the per-query-head
partials are stored and summed by group_sum_heads_kernel.  2^-16 covers fp32 accumulation and the hardware exp / log.  lse is fp32 and is
held to the project's fp32 figure, 1e-4 max(1, |ref|).

Rotary adjoint (rope= of the backward: dq / dk come out as gradients of the UN-rotated q / k).  unrope() turns a gradient g of the rotated
q or k and its budget A into g' = R^T g and A' = |R^T| A, per pair (lo, hi) = (e, e + hd/2) with (c, s) = cs[pos[row], e]:

    g'_lo = g_lo c + g_hi s     g'_hi = g_hi c - g_lo s     A'_lo = |c| A_lo + |s| A_hi     A'_hi = |c| A_hi + |s| A_lo

The gate stays the one above with ONE more rounding: 3 for dq, 3 for dk on the register-accumulating shape, 4 for dk on the per-query-head
+ group-sum shape; dv is untouched (2 and 3).  Why one: the un-rotated path's terms (the dS rounding and the delta error) move g by at most
2^-8 A element-wise, which the rotation carries to at most 2^-8 A'.  The kernels then round the gradient to bf16 BEFORE they rotate it
(the unfused sequence stored it first): one 2^-8 rounding of a value bounded by A -- |g| <= A holds element-wise because |dS| <= W --
which the rotation again carries to 2^-8 A'.  That rounding takes the place of the un-rotated path's store.  The rotated value is rounded
once more on the store: one 2^-8 rounding of a value bounded by A'.  cos / sin are the caller's fp32 table (values rounded through bf16,
as the ABI says), read as float64: they are inputs, not errors, and the two fp32 products and their sum fall under the 2^-16 term.
"""
import math

import numpy as np
import torch

from radvlm_amd import portable_rng as prng

BF16 = torch.bfloat16
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
EPS_BF16 = 2.0 ** -8      # worst-case relative error of one round-to-nearest to bf16, as the gates count it
EPS_F32 = 2.0 ** -16      # fp32 accumulation + hardware exp / log
FLOOR = 1e-30
RESCALE_LAG = 8           # attn_fwd_nat_kernel
KEY_TILE = 64
WAVE_ROWS = 32
FAMILIES = ("rand", "stair", "stair7", "mixed", "sink", "big")
STRESS = ("stair", "stair7", "mixed", "sink")          # families that must trigger the deferred rescale after the first key tile
STEP = {"stair": 9.5, "stair7": 7.0, "mixed": 9.5}      # rise of the scaled score per 64-key tile, exp2 units
MIXED_ROWS = (5, 21)      # rows of each 32-row wave that see the rise in family `mixed`


def rbf(x):
    """Round a float64 tensor through bf16."""
    return x.to(BF16).double()


def sample_rows(B, S, cu=None):
    """[(first row, number of rows)] of every sample: b * S padded layout, cu[b] .. cu[b + 1] packed."""
    if cu is None:
        return [(b * S, S) for b in range(B)]
    return [(int(cu[b]), int(cu[b + 1] - cu[b])) for b in range(B)]


def positions(B, S, cu=None):
    """Position of every token row inside its sample."""
    return np.concatenate([np.arange(n) for _, n in sample_rows(B, S, cu)])


# ---------------------------------------------------------------------------------------------------------------- input families
def make_inputs(family, pos, H, Hkv, hd, seed=0):
    """(q [M, H hd], k, v [M, Hkv hd], dout [M, H hd]) bf16 on the CPU for token rows at positions `pos` of their samples.

    rand    std 1, as the older attention tests draw them.
    big     std 3: scaled scores of std 13 exp2 units, magnitudes up to about 60.
    stair   q = noise + 8 u, k = 0.1 noise + c(tile) u with |u| = 1 (16 entries of 0.25, no q noise on them): the scaled score of every
            key of 64-key tile t is 9.5 t exp2 units (+- 0.2 of noise), and |v| falls by 2^-round(9.5 t), so every tile contributes to
            P |V| alike and a lost or wrong rescale factor is an O(1) error against the budget.  Use at most 5 key tiles (|v| >= 2^-38).
    stair7  the same with steps of 7: the first step stays inside the lag of 8, the second leaves it.
    mixed   stair, but only rows 5 and 21 of every 32-row wave carry the 8 u term; the others see flat scores.
    sink    c = -60 exp2 units for the first key tile and 0 after it; v of std 1.
    """
    assert family in FAMILIES, family
    pos = np.asarray(pos)
    M = len(pos)
    tile = torch.from_numpy(pos // KEY_TILE).double()
    draw = lambda tag, cols: torch.from_numpy(prng.normal(5000 + seed, tag, (M, cols), 1.0)).double()
    q, k = draw(1, H * hd).view(M, H, hd), draw(2, Hkv * hd).view(M, Hkv, hd)
    v, dout = draw(3, Hkv * hd).view(M, Hkv, hd), draw(4, H * hd).view(M, H, hd)
    if family == "big":
        q, k = q * 3.0, k * 3.0
    elif family != "rand":
        sl2 = LOG2E / math.sqrt(hd)
        a = 8.0
        sup = torch.zeros(hd, dtype=torch.bool)
        sup[::hd // 16] = True                       # u = 0.25 on these 16 dimensions
        if family == "sink":
            c = torch.where(tile == 0, torch.full_like(tile, -60.0 / (sl2 * a)), torch.zeros_like(tile))
        else:
            c = STEP[family] * tile / (sl2 * a)
            v = v * torch.exp2(-torch.round(STEP[family] * tile))[:, None, None]
        rise = torch.ones(M, dtype=torch.bool)
        if family == "mixed":
            rise = torch.from_numpy(np.isin(pos % WAVE_ROWS, MIXED_ROWS))
        q[:, :, sup] = (a * 0.25 * rise.double())[:, None, None]
        k = 0.1 * k
        k[:, :, sup] += (0.25 * c)[:, None, None]
    return tuple(t.reshape(M, -1).to(BF16) for t in (q, k, v, dout))


# ---------------------------------------------------------------------------------------------------------------- reference
def _heads(t, r0, n, heads, hd):
    return t[r0:r0 + n].double().view(n, heads, hd).transpose(0, 1)        # [heads, n, hd]


def _rows(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)                        # [heads, n, hd] -> [n, heads hd]


def _mask(n, length, causal):
    """[n, n] bool: key j may be seen by query i."""
    j = torch.arange(n)
    ok = (j < length)[None, :].expand(n, n)
    if causal:
        ok = ok & (j[None, :] <= j[:, None])
    return ok


def reference(q, k, v, dout, B, S, H, Hkv, hd, causal, lens=None, cu=None, scale=None, keep_scores=False):
    """float64 attention forward and backward of one call on token-major bf16 (or any) tensors.

    Returns a dict: out, dq [M, H hd]; dk, dv [M, Hkv hd]; lse [B, H, S] (natural log; NaN where a packed sample has no such row);
    A_out, A_dq, A_dk, A_dv of the outputs' shapes; valid [M] bool (row < lens[b]: rows of a padded sample beyond its length are
    computed like the kernels compute them -- they see the keys below lens[b] -- but only `valid` rows are a contract); with keep_scores,
    scores2 = per sample the [H, n, n] scaled scores in exp2 units (-inf where masked)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    rep = H // Hkv
    M = q.shape[0]
    res = {n: torch.zeros(M, H * hd, dtype=torch.float64) for n in ("out", "dq", "A_out", "A_dq")}
    res.update({n: torch.zeros(M, Hkv * hd, dtype=torch.float64) for n in ("dk", "dv", "A_dk", "A_dv")})
    res["lse"] = torch.full((B, H, S), float("nan"), dtype=torch.float64)
    res["valid"] = torch.zeros(M, dtype=torch.bool)
    if keep_scores:
        res["scores2"] = []
    for b, (r0, n) in enumerate(sample_rows(B, S, cu)):
        length = int(lens[b]) if (lens is not None and cu is None) else n
        Q, dO = _heads(q, r0, n, H, hd), _heads(dout, r0, n, H, hd)
        K = _heads(k, r0, n, Hkv, hd).repeat_interleave(rep, 0)
        V = _heads(v, r0, n, Hkv, hd).repeat_interleave(rep, 0)
        s = (Q @ K.transpose(1, 2)) * scale
        s = s.masked_fill(~_mask(n, length, causal)[None], float("-inf"))
        lse = torch.logsumexp(s, -1)
        P = torch.exp(s - lse[..., None])
        O = P @ V
        dP = dO @ V.transpose(1, 2)
        delta = (dO * O).sum(-1, keepdim=True)
        D = (dO.abs() * O.abs()).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        W = P * ((dP - delta).abs() + D)
        fold = lambda t: t.view(Hkv, rep, n, hd).sum(1)                    # sum over the group's query heads
        sl = slice(r0, r0 + n)
        res["out"][sl], res["A_out"][sl] = _rows(O), _rows(P @ V.abs())
        res["dq"][sl], res["A_dq"][sl] = _rows(scale * (dS @ K)), _rows(scale * (W @ K.abs()))
        res["dk"][sl], res["A_dk"][sl] = _rows(fold(scale * (dS.transpose(1, 2) @ Q))), _rows(fold(scale * (W.transpose(1, 2) @ Q.abs())))
        res["dv"][sl], res["A_dv"][sl] = _rows(fold(P.transpose(1, 2) @ dO)), _rows(fold(P.transpose(1, 2) @ dO.abs()))
        res["lse"][b, :, :n] = lse
        res["valid"][r0:r0 + length] = True
        if keep_scores:
            res["scores2"].append(s * LOG2E)
    return res


# ---------------------------------------------------------------------------------------------------------------- rotary adjoint
def unrope(g, A, cs, pos, heads, hd):
    """Adjoint of the rotary embedding on a gradient g [M, heads hd] of the ROTATED q or k and on its budget A (module docstring), in
    float64.  cs: the [positions, hd/2, 2] (cos, sin) table handed to the kernel; pos [M]: the table row of every token row.
    Returns (g', A')."""
    M, half = g.shape[0], hd // 2
    t = cs.detach().cpu().double()[torch.as_tensor(np.asarray(pos), dtype=torch.long)]          # [M, hd/2, 2]
    c, s = t[:, None, :, 0], t[:, None, :, 1]
    g, A = g.double().view(M, heads, hd), A.double().view(M, heads, hd)
    lo, hi, a_lo, a_hi = g[..., :half], g[..., half:], A[..., :half], A[..., half:]
    out = torch.cat((lo * c + hi * s, hi * c - lo * s), -1)
    bound = torch.cat((c.abs() * a_lo + s.abs() * a_hi, c.abs() * a_hi + s.abs() * a_lo), -1)
    return out.reshape(M, heads * hd), bound.reshape(M, heads * hd)


# ---------------------------------------------------------------------------------------------------------------- gates
def gate(A, roundings):
    return (roundings * EPS_BF16 + EPS_F32) * A.double() + FLOOR


def assert_within_budget(got, ref, A, roundings, what=""):
    """|got - ref| <= (roundings 2^-8 + 2^-16) A + 1e-30 for EVERY element; returns the worst ratio to the gate (<= 1)."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert tuple(got.shape) == tuple(ref.shape) == tuple(A.shape), (what, got.shape, ref.shape, A.shape)
    r = (got - ref).abs() / gate(A, roundings)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    worst = float(r.max()) if r.numel() else 0.0
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        idx = tuple(int(x) for x in np.unravel_index(i, tuple(r.shape)))
        raise AssertionError(f"{what}: element {idx}: got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, "
                             f"A {float(A.reshape(-1)[i])!r}, error / gate = {worst:.4g} (roundings = {roundings}); "
                             f"{int((r > 1.0).sum())} of {r.numel()} elements over the gate")
    return worst


def assert_lse_close(got, ref, what=""):
    """fp32 gate of lse: |got - ref| <= 1e-4 max(1, |ref|) for every element; returns the worst ratio."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    r = (got - ref).abs() / (1e-4 * ref.abs().clamp_min(1.0))
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    worst = float(r.max()) if r.numel() else 0.0
    assert worst <= 1.0, f"{what}: lse error / (1e-4 max(1, |ref|)) = {worst:.4g}"
    return worst


# ---------------------------------------------------------------------------------------------------------------- rescale triggers
def rescale_events(s2, causal):
    """From the float64 scaled scores (exp2 units) of one (sample, head) [n, n]: for every 32-row wave, the key tiles it walks and, per
    tile u >= 1, whether some row of the wave has a score above ceil(maximum of its earlier tiles) + RESCALE_LAG -- the stored integer
    maximum of a row never exceeds that ceiling, so such a tile MUST take the rescale branch.  Also whether any row exceeds
    the same walk with the kernel's own bookkeeping (`fires`): a row's integer maximum m is raised to max(m, ceil(tile maximum)) only in
    a tile where some row of the wave exceeds m + RESCALE_LAG -- what family stair7 needs, whose first step must NOT fire.
    Returns [(q0, ntiles, must [bool per tile u >= 1], fires [bool per tile u >= 1])]."""
    n = s2.shape[0]
    nk = int(torch.isfinite(s2).any(0).sum())               # keys some row may see (= lens[b])
    out = []
    for q0 in range(0, n, WAVE_ROWS):
        rows = s2[q0:min(q0 + WAVE_ROWS, n)]
        kv_end = min(nk, (q0 // 128) * 128 + 128) if causal else nk
        ntiles = (kv_end + KEY_TILE - 1) // KEY_TILE
        if causal:
            ntiles = min(ntiles, (q0 + WAVE_ROWS - 1) // KEY_TILE + 1)    # later tiles are skipped by this wave
        tmax = torch.stack([rows[:, u * KEY_TILE:(u + 1) * KEY_TILE].max(-1).values for u in range(ntiles)], 1)      # [rows, tiles]
        must, fires = [], []
        m = torch.ceil(tmax[:, 0])
        for u in range(1, ntiles):
            ceil_before = torch.ceil(tmax[:, :u].max(-1).values)
            must.append(bool((tmax[:, u] > ceil_before + RESCALE_LAG).any()))
            fires.append(bool((tmax[:, u] > m + RESCALE_LAG).any()))
            if fires[-1]:
                m = torch.maximum(m, torch.ceil(tmax[:, u]))
        out.append((q0, ntiles, must, fires))
    return out


# ---------------------------------------------------------------------------------------------------------------- emulation
def emulate_natural(q, k, v, dout, B, S, H, Hkv, hd, causal, lens=None, cu=None, scale=None):
    """The natural-layout forward and backward with their rounding points, in float64 between them: 64-key tiles, an integer running
    maximum of the exp2 domain raised (wave-uniformly, per 32 query rows) only when a score outgrows it by more than 2^8, fp32 `l`, P
    rounded to bf16 before the P V product, out rounded to bf16; backward: p from the fp32 lse, delta from the bf16 out, P and dS rounded to
    bf16 before their products, bf16 stores.  Returns out, lse, dq, dk, dv like reference(), plus `rescales` = the number of times a wave
    took the rescale branch after its first tile."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    sl2 = scale * LOG2E
    rep = H // Hkv
    M = q.shape[0]
    res = {n: torch.zeros(M, H * hd, dtype=torch.float64) for n in ("out", "dq")}
    res.update({n: torch.zeros(M, Hkv * hd, dtype=torch.float64) for n in ("dk", "dv")})
    res["lse"] = torch.full((B, H, S), float("nan"), dtype=torch.float64)
    res["rescales"] = 0
    f32 = lambda t: t.float().double()
    for b, (r0, n) in enumerate(sample_rows(B, S, cu)):
        length = int(lens[b]) if (lens is not None and cu is None) else n
        Q, dO = _heads(q, r0, n, H, hd), _heads(dout, r0, n, H, hd)
        K = _heads(k, r0, n, Hkv, hd).repeat_interleave(rep, 0)
        V = _heads(v, r0, n, Hkv, hd).repeat_interleave(rep, 0)
        ok = _mask(n, length, causal)
        raw = f32(Q @ K.transpose(1, 2)).masked_fill(~ok[None], float("-inf"))           # [H, n, n] raw scores, fp32 accumulators
        O = torch.zeros(H, n, hd, dtype=torch.float64)
        lse = torch.zeros(H, n, dtype=torch.float64)
        for q0 in range(0, n, WAVE_ROWS):
            w = slice(q0, min(q0 + WAVE_ROWS, n))
            kv_end = min(length, (q0 // 128) * 128 + 128) if causal else length
            nt = (kv_end + KEY_TILE - 1) // KEY_TILE
            nr = w.stop - w.start
            m = torch.full((H, nr), float("-inf"), dtype=torch.float64)
            l = torch.zeros(H, nr, dtype=torch.float64)
            o = torch.zeros(H, nr, hd, dtype=torch.float64)
            for u in range(nt):
                if causal and u * KEY_TILE > q0 + WAVE_ROWS - 1:
                    continue
                ks = slice(u * KEY_TILE, min((u + 1) * KEY_TILE, n))
                st = raw[:, w, ks]
                mx = st.max(-1).values
                for h in range(H):                                                       # a wave serves one head
                    if bool((f32(mx[h] * sl2) > m[h] + RESCALE_LAG).any()):
                        mnew = torch.maximum(m[h], torch.ceil(f32(mx[h] * sl2)))
                        alpha = torch.where(torch.isfinite(m[h]), torch.exp2(m[h] - mnew), torch.zeros_like(mnew))
                        l[h], o[h], m[h] = l[h] * alpha, o[h] * alpha[:, None], mnew
                        res["rescales"] += int(u > 0)
                p = f32(torch.exp2(f32(st * sl2 - m[..., None])))
                l = f32(l + p.sum(-1))
                o = f32(o + rbf(p) @ V[:, ks])
            O[:, w] = rbf(f32(o / l[..., None]))
            lse[:, w] = f32((m + torch.log2(l)) * LN2)
        # backward
        p = f32(torch.exp2(f32(raw * sl2 - f32(lse * LOG2E)[..., None])))
        p = torch.where(ok[None], p, torch.zeros_like(p))
        delta = f32((dO * O).sum(-1, keepdim=True))
        dS = torch.where(ok[None], f32(p * (f32(dO @ V.transpose(1, 2)) - delta)), torch.zeros_like(p))
        pb, dsb = rbf(p), rbf(dS)
        fold = lambda t: t.view(Hkv, rep, n, hd).sum(1)
        sl = slice(r0, r0 + n)
        res["out"][sl] = _rows(O)
        res["dq"][sl] = rbf(_rows(scale * (dsb @ K)))
        res["dk"][sl] = rbf(_rows(fold(scale * (dsb.transpose(1, 2) @ Q))))
        res["dv"][sl] = rbf(_rows(fold(pb.transpose(1, 2) @ dO)))
        res["lse"][b, :, :n] = lse
    return res

"""GPU tests of rv_gspo_seqs_f64 (radvlm_amd/csrc/preference.hip) on synthetic fp32 rows, against the float64 restatement of
tests/gspo_ref.py (pinned to autograd in tests/test_gspo_host.py).  With u = 2^-52, per sequence b of n scored tokens:
  m        bit for bit against the restated order
  s        within 8 u relative of np.exp(m): one libm call on each side, the per-call allowance of the pair-loss gate
  l        within 9 u |l_ref| (floor 2^-1022): the s gate through one product, plus that product's rounding
  wkl      within G_b = 8 u sum_j lw_j |expm1(q_j)| + (ceil(n / 64) + 8) u sum_j lw_j kl_j: one libm call per token, then the
           subtraction, the product and the ceil(n / 64) + 6 additions on the longest path of the fixed order, on each side
  batch    T_b = W_l,b |l_b|, K_b = wkl_b:  |batch[1] - ref| <= beta sum_b G_b + (B + 8) u beta sum_b K_b;
           |batch[0] - ref| <= 10 u sum_b T_b (the l gate and the product's rounding) + the batch[1] gate + (B + 8) u (sum_b T_b + beta sum_b K_b)
  coef     within one fp32 ulp of fp32(ref), floor 1e-30
  kl       within two fp32 ulp of fp32(ref), floor 1e-30
  clip     exact
Rows that hold no scored token keep a sentinel in coef and kl; every per-row input outside the map is NaN, so a stray read would
show.  The worst ratio of every gate goes to conftest.record_measurement."""
import functools

import numpy as np
import pytest
import torch

import gspo_ref as G
from preference_ref import fp32_ulp

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 129, 2049)
BS = (1, 3, 5)
FIRSTS = (0, 3, 6)                     # with BS: every length occurs, alone and among others, and every (region, sign) pair below
SENTINEL = 0x7fc5a5a5
EPS_LOW, EPS_HIGH = 0.2, 0.28
U = 2.0 ** -52
# (target sequence ratio, sign of the advantage): below, inside and above the clip range, each with both signs
REGIONS = ((0.6, -1), (1.03, 1), (1.6, 1), (0.6, 1), (0.97, -1), (1.6, -1))


def _record(test, **kw):
    from conftest import record_measurement
    record_measurement(test, **kw)


def _rc(*args):
    """The entry point's return code, without lib.call's raise."""
    from radvlm_amd import lib
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
    return lib.load().rv_gspo_seqs_f64(*[ptr(a) for a in args], torch.cuda.current_stream().cuda_stream)


def _scatter(c, a):
    """A host array in scored order -> fp32 device rows, NaN where no scored token lives."""
    if a is None:
        return None
    full = np.full(c["rows"], np.nan, dtype=np.float32)
    full[c["idx"]] = a
    return torch.from_numpy(full).cuda()


@functools.lru_cache(maxsize=None)
def _case(B, mapped, first=0, const_gw=False):
    """B sequences with the lengths LENGTHS[first], LENGTHS[first + 1], ...: host arrays in scored order and the device buffers.
    mapped: the scored tokens sit at a permuted subset of 2 n + 5 rows; else at rows 0 .. n - 1 of n + 3."""
    counts = np.array([LENGTHS[(first + b) % len(LENGTHS)] for b in range(B)], dtype=np.int64)
    n = int(counts.sum())
    rng = np.random.default_rng(1000 * B + 10 * first + mapped)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    x = f32(-rng.exponential(0.5, n))
    seq = np.repeat(np.arange(B), counts)
    region = [REGIONS[(first + b) % len(REGIONS)] for b in range(B)]
    adv = f32([sg * (0.3 + 0.2 * b) for b, (_, sg) in enumerate(region)])
    target = np.log(np.array([t for t, _ in region]))
    old = f32(x - target[seq] + rng.normal(0, 0.02, n))
    ref = f32(x + rng.normal(0, 0.3, n))
    lw = f32(rng.uniform(0.5, 1.5, n) / max(n, 1))
    if const_gw:
        lw = f32(np.repeat(rng.uniform(0.5, 1.5, B) / max(n, 1), counts))
    gw = f32(lw.astype(np.float64) * 37.5)
    rows = 2 * n + 5 if mapped else n + 3
    idx = np.sort(rng.permutation(rows)[:n])[rng.permutation(n)].astype(np.int32) if mapped else np.arange(n, dtype=np.int32)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    c = dict(B=B, n=n, rows=rows, idx=idx, counts=counts, x=x, adv=adv, old=old, ref=ref, lw=lw, gw=gw, seq=seq)
    dev = lambda a: torch.from_numpy(a).cuda()
    c.update(d_logp=_scatter(c, x), d_old=_scatter(c, old), d_ref=_scatter(c, ref), d_lw=_scatter(c, lw), d_gw=_scatter(c, gw), d_adv=dev(adv),
             d_seg=dev(seg), d_idx=dev(idx) if mapped else None)
    return c


def _run(c, old, ref, beta, d_old=None, d_ref=None):
    """One launch on sentinel-filled outputs.  old / ref: host arrays in scored order for the reference (None: not given)."""
    B, rows = c["B"], c["rows"]
    planes = torch.full((5, B), float("nan"), dtype=torch.float64, device="cuda")
    batch = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    coef = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    kl = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    d_old = _scatter(c, old) if d_old is None else d_old
    d_ref = _scatter(c, ref) if d_ref is None else d_ref
    rc = _rc(c["d_logp"], c["d_seg"], c["d_idx"], c["d_adv"], c["d_lw"], c["d_gw"], d_old, d_ref, EPS_LOW, EPS_HIGH, beta, planes, batch,
             coef, kl, B, rows)
    assert rc == 0
    torch.cuda.synchronize()
    want = G.gspo(c["x"], c["counts"], c["adv"], c["lw"], c["gw"], old_logp=old, ref_logp=ref, eps_low=EPS_LOW, eps_high=EPS_HIGH, beta=beta)
    untouched = np.ones(rows, dtype=bool)
    untouched[c["idx"]] = False
    cf, k = coef.cpu(), kl.cpu()
    for name, t in (("coef", cf), ("kl", k)):
        assert (t.view(torch.int32).numpy()[untouched] == SENTINEL).all(), f"{name}: a row without a scored token was written"
    got = dict(zip(("m", "s", "l", "clip", "wkl"), planes.cpu().numpy()), coef=cf.numpy()[c["idx"]], kl=k.numpy()[c["idx"]],
               batch=batch.cpu().numpy())
    return got, want


def _ratios(c, got, want, beta):
    """Worst error / gate of every gate of the module docstring; the exact ones are asserted here."""
    B, counts = c["B"], c["counts"]
    assert got["m"].view(np.int64).tolist() == want["m"].view(np.int64).tolist(), "m: not the restated order's bits"
    assert got["clip"].tolist() == want["clip"].tolist()
    r = {}
    r["s"] = float(np.max(np.abs(got["s"] - np.exp(got["m"])) / (8 * U * np.exp(got["m"]))))
    r["l"] = float(np.max(np.abs(got["l"] - want["l"]) / np.maximum(9 * U * np.abs(want["l"]), 2.0 ** -1022)))
    off = np.concatenate([[0], np.cumsum(counts)])
    lw = c["lw"].astype(np.float64)
    Gb = np.zeros(B)
    for b in range(B):
        sl = slice(int(off[b]), int(off[b + 1]))
        kl = want["kl"][sl]
        em1 = kl + (c["ref"][sl].astype(np.float64) - c["x"][sl].astype(np.float64)) if beta > 0 else np.zeros_like(kl)
        Gb[b] = 8 * U * (lw[sl] * np.abs(em1)).sum() + (-(-int(counts[b]) // 64) + 8) * U * (lw[sl] * kl).sum()
    r["wkl"] = float(np.max(np.abs(got["wkl"] - want["wkl"]) / np.maximum(Gb, 2.0 ** -1022)))
    T, K = np.abs(want["W_l"] * want["l"]).sum(), want["wkl"].sum()
    g1 = beta * Gb.sum() + (B + 8) * U * beta * K
    g0 = 10 * U * T + g1 + (B + 8) * U * (T + beta * K)
    r["batch0"] = float(abs(got["batch"][0] - want["L"]) / max(g0, 2.0 ** -1022))
    r["batch1"] = float(abs(got["batch"][1] - want["kl_loss"]) / max(g1, 2.0 ** -1022))
    for k, ulps in (("coef", 1), ("kl", 2)):
        w32 = want[k].astype(np.float32)
        r[k] = float(np.max(np.abs(got[k].astype(np.float64) - w32.astype(np.float64)) / (ulps * fp32_ulp(w32)), initial=0.0))
    return r


@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("with_old", [True, False])
def test_sequence_terms_and_coefficients(with_old, beta):
    worst, seen = {}, set()
    for B in BS:
        for mapped in (False, True):
            for first in FIRSTS:
                c = _case(B, mapped, first)
                got, want = _run(c, c["old"] if with_old else None, c["ref"] if beta > 0 else None, beta,
                                 d_old=c["d_old"] if with_old else None, d_ref=c["d_ref"] if beta > 0 else None)
                ratios = _ratios(c, got, want, beta)
                print(f"old={with_old} beta={beta} B={B} mapped={mapped} first={first}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
                for k, v in ratios.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                empty = c["counts"] == 0
                assert (got["m"][empty].view(np.int64) == 0).all() and (got["s"][empty] == 1.0).all() and (got["l"][empty] == 0.0).all()
                assert (got["clip"][empty] == 0.0).all() and (got["wkl"][empty].view(np.int64) == 0).all()
                assert np.isfinite(got["batch"]).all()
                if not with_old:
                    assert (got["s"] == 1.0).all() and (got["m"].view(np.int64) == 0).all()
                if beta == 0:
                    assert not got["kl"].any() and got["batch"][1] == 0.0
                for b in np.flatnonzero(~empty):       # the reference's own classification: region of s, sign of A, clip code
                    s, A = want["s"][b], c["adv"][b]
                    seen.add((-1 if s < 1 - EPS_LOW else 1 if s > 1 + EPS_HIGH else 0, int(np.sign(A)), int(want["clip"][b])))
    if with_old:        # all three clip regions with both signs of A, as the reference sees them
        assert seen == {(-1, -1, 1), (-1, 1, 0), (0, -1, 0), (0, 1, 0), (1, -1, 0), (1, 1, 2)}, seen
    _record(f"gspo_kernel_terms[{'old' if with_old else 'on_policy'}-{beta}]", **{f"worst_ratio_{k}": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("mapped", [False, True])
def test_bit_promise_on_policy(mapped):
    """old_logp NULL or equal to logp, beta 0 or ref_logp equal to logp, gweight constant inside each sequence: coef is the fp32
    product gweight * adv, the token kernel's coefficient at r = 1.  Lengths 1, 63, 64, 65 and 65, 129, 2049."""
    for c in (_case(4, mapped, first=1, const_gw=True), _case(3, mapped, first=4, const_gw=True)):
        want = (c["gw"] * c["adv"][c["seq"]]).view(np.int32)
        assert want.dtype == np.int32 and c["gw"].dtype == np.float32 and c["adv"].dtype == np.float32
        for old, ref, beta in ((None, None, 0.0), (c["x"], None, 0.0), (None, c["x"], 0.04), (c["x"], c["x"], 0.04)):
            got, _ = _run(c, old, ref, beta)
            assert got["coef"].view(np.int32).tolist() == want.tolist(), (old is None, ref is None, beta)
            assert (got["s"] == 1.0).all() and not got["kl"].any()


def test_launcher_refusals():
    from radvlm_amd import lib
    c = _case(3, False, 3)
    B, rows = c["B"], c["rows"]
    planes = torch.full((5, B), 3.0, dtype=torch.float64, device="cuda")
    batch = torch.full((2,), 3.0, dtype=torch.float64, device="cuda")
    coef = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    kl = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    good = dict(logp=c["d_logp"], seg=c["d_seg"], row_idx=None, adv=c["d_adv"], lw=c["d_lw"], gw=c["d_gw"], old=c["d_old"], ref=c["d_ref"],
                eps_low=0.2, eps_high=0.2, beta=0.04, planes=planes, batch=batch, coef=coef, kl=kl, B=B, rows=rows)
    nan = float("nan")
    bad = [dict(logp=None), dict(seg=None), dict(adv=None), dict(lw=None), dict(gw=None), dict(planes=None), dict(batch=None), dict(coef=None),
           dict(kl=None), dict(B=0), dict(B=-1), dict(rows=0), dict(rows=-1), dict(eps_low=-0.1), dict(eps_low=nan), dict(eps_high=-0.1),
           dict(eps_high=nan), dict(beta=-0.04), dict(beta=nan), dict(ref=None)]
    for change in bad:
        a = dict(good, **change)
        assert _rc(*[a[k] for k in good]) == -1, change
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert (planes == 3.0).all() and (batch == 3.0).all()
    assert (coef.view(torch.int32) == SENTINEL).all() and (kl.view(torch.int32) == SENTINEL).all()
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_gspo_seqs_f64", c["d_logp"], c["d_seg"], None, c["d_adv"], c["d_lw"], c["d_gw"], None, None, 0.2, 0.2, 0.04, planes, batch,
                 coef, kl, B, rows)

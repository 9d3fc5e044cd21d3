"""GPU tests of rv_seq_logp_sums_f64 and rv_dpo_pairs_f64 (radvlm_amd/csrc/preference.hip) on synthetic fp32 logp rows, against the
float64 restatement of tests/preference_ref.py (pinned to autograd in tests/test_preference_host.py).  Gates:
  sums         bit for bit against the restated order, and within 2^-52 sum|x| of math.fsum
  h, rewards   within 4 * 2^-53 * beta * (|pi_c| + |pi_r| + |rho_c| + |rho_r|): three subtractions and one product
  pair loss    within 16 * 2^-52 * max(|l_ref|, 2^-1022): two libm calls of a few ulp each plus four roundings
  coefficient  within one fp32 ulp of fp32(ref), floor 1e-30
  batch        L, dpo_loss, sft_loss: the pair-loss gate on every summand plus (P + 8) roundings of the sums' magnitudes
Rows that hold no scored token keep a sentinel; logp rows outside the map are NaN, so a stray read would show.  The worst ratio of
every gate goes to conftest.record_measurement."""
import functools
import math

import numpy as np
import pytest
import torch

import preference_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = ((1, 1), (1, 65), (63, 64), (64, 129), (2049, 7))           # (chosen, rejected) scored tokens
PS = (1, 3, 5)
SENTINEL = 0x7fc5a5a5
BETA = 0.1


def _record(test, **kw):
    from conftest import record_measurement
    record_measurement(test, **kw)


def _call(name, *args):
    from radvlm_amd import lib
    lib.call(name, *args)


def _rc(name, *args):
    """The entry point's return code, without lib.call's raise."""
    from radvlm_amd import lib
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a
    return getattr(lib.load(), name)(*[ptr(a) for a in args], torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(P, mapped, first=0):
    """P pairs with the lengths LENGTHS[first], LENGTHS[first + 1], ...: host x (fp32, scored order), counts, and the device buffers.
    mapped: the scored tokens sit at a permuted subset of 2 n + 5 rows (the other rows are NaN); else at rows 0 .. n - 1 of n + 3."""
    pairs = [LENGTHS[(first + p) % len(LENGTHS)] for p in range(P)]
    counts = np.array([c for c, _ in pairs] + [r for _, r in pairs], dtype=np.int64)
    n = int(counts.sum())
    rng = np.random.default_rng(100 * P + first)
    x = (-rng.exponential(0.5, n)).astype(np.float32)
    x[::7] = -np.float32(2.0) ** -rng.integers(1, 20, x[::7].size).astype(np.float32)       # tiny magnitudes among ordinary ones
    rows = 2 * n + 5 if mapped else n + 3
    idx = np.sort(rng.permutation(rows)[:n])[rng.permutation(n)].astype(np.int32) if mapped else np.arange(n, dtype=np.int32)
    full = np.full(rows, np.nan, dtype=np.float32)
    full[idx] = x
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dev = lambda a: torch.from_numpy(a).cuda()
    return dict(P=P, x=x, counts=counts, n=n, rows=rows, idx=idx, logp=dev(full), seg=dev(seg), row_idx=dev(idx) if mapped else None)


@functools.lru_cache(maxsize=None)
def _rho(P, first=0):
    c = _case(P, False, first)
    rng = np.random.default_rng(7 + P)
    sums = np.array([R.ordered_sum(s) for s in np.split(c["x"], np.cumsum(c["counts"])[:-1])])
    return sums + rng.normal(0, 2.0, 2 * P)           # a reference a few nats away from the policy


def _run_pairs(c, rho, loss_type, eps, beta=BETA, dpo_alpha=0.8, gamma=1.25):
    P, rows = c["P"], c["rows"]
    planes = torch.full((7, P), float("nan"), dtype=torch.float64, device="cuda")
    batch = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    coef = torch.full((rows,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    n_c = int(c["counts"][:P].sum())
    rho_k = None if rho is None else (rho / c["counts"] if loss_type == "ipo" else rho)
    _call("rv_dpo_pairs_f64", c["logp"], c["seg"], c["row_idx"], None if rho_k is None else torch.from_numpy(rho_k).cuda(), P,
          R.LOSS_TYPES.index(loss_type), beta, eps, dpo_alpha / P, gamma / n_c, planes, batch, coef, rows)
    torch.cuda.synchronize()
    ref = R.dpo(c["x"], c["counts"], ref=rho_k, beta=beta, dpo_alpha=dpo_alpha, gamma=gamma, loss_type=loss_type, label_smoothing=eps)
    pl = planes.cpu().numpy()
    cf = coef.cpu()
    got = dict(zip(("pi_c", "pi_r", "h", "loss", "reward_c", "reward_r", "sum_c"), pl), coef=cf.numpy()[c["idx"]].astype(np.float64))
    untouched = np.ones(rows, dtype=bool)
    untouched[c["idx"]] = False
    assert (cf.view(torch.int32).numpy()[untouched] == SENTINEL).all(), "a row without a scored token was written"
    return got, ref, batch.cpu().numpy(), rho_k


def test_sums_bit_for_bit_and_against_fsum():
    worst = 0.0
    for P in PS:
        for mapped in (False, True):
            for first in (0, 3):
                c = _case(P, mapped, first)
                sums = torch.full((2 * P,), float("nan"), dtype=torch.float64, device="cuda")
                _call("rv_seq_logp_sums_f64", c["logp"], c["seg"], c["row_idx"], sums, 2 * P, c["rows"])
                got = sums.cpu().numpy()
                parts = np.split(c["x"].astype(np.float64), np.cumsum(c["counts"])[:-1])
                want = np.array([R.ordered_sum(s) for s in parts])
                assert got.view(np.int64).tolist() == want.view(np.int64).tolist(), (P, mapped, first)
                for g, s in zip(got, parts):
                    gate = 2.0 ** -52 * np.abs(s).sum()
                    err = abs(g - math.fsum(s))
                    print(f"P={P} mapped={mapped} n={s.size}: |sum - fsum| = {err:.3g}, gate {gate:.3g}")
                    assert err <= gate
                    worst = max(worst, err / gate)
    # an empty sequence sums to +0.0, wherever it sits
    logp = torch.from_numpy(np.array([-1.0, -2.0, -4.0], dtype=np.float32)).cuda()
    seg = torch.tensor([0, 0, 2, 2, 3], dtype=torch.int32, device="cuda")
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    _call("rv_seq_logp_sums_f64", logp, seg, None, sums, 4, 3)
    assert sums.cpu().numpy().view(np.int64).tolist() == np.array([0.0, -3.0, 0.0, -4.0]).view(np.int64).tolist()
    _record("preference_kernel_sums_vs_fsum", worst_ratio_of_gate=worst)


@pytest.mark.parametrize("with_rho", [True, False])
@pytest.mark.parametrize("loss_type,eps", [("sigmoid", 0.0), ("sigmoid", 0.1), ("hinge", 0.0), ("hinge", 0.1), ("ipo", 0.0)])
def test_pair_terms_and_coefficients(loss_type, eps, with_rho):
    worst = {}
    for P in PS:
        for mapped in (False, True):
            for first in (0, 3):
                c = _case(P, mapped, first)
                got, ref, batch, rho_k = _run_pairs(c, _rho(P, first) if with_rho else None, loss_type, eps)
                # the two sums are rv_seq_logp_sums_f64's, bit for bit
                assert got["sum_c"].view(np.int64).tolist() == ref["sum_c"].view(np.int64).tolist()
                if loss_type != "ipo":
                    assert got["pi_c"].view(np.int64).tolist() == ref["sums"][:P].view(np.int64).tolist()
                    assert got["pi_r"].view(np.int64).tolist() == ref["sums"][P:].view(np.int64).tolist()
                else:
                    assert np.allclose(got["pi_c"], ref["pi_c"], rtol=2.0 ** -52, atol=0) and np.allclose(got["pi_r"], ref["pi_r"], rtol=2.0 ** -52, atol=0)
                ratios = R.gate_ratios(got, ref, BETA, rho_k)
                a_P, g_N = 0.8 / P, 1.25 / int(c["counts"][:P].sum())
                mag = a_P * np.abs(ref["loss"]).sum() + g_N * np.abs(ref["sum_c"]).sum()
                bgate = 16 * 2.0 ** -52 * a_P * np.abs(ref["loss"]).sum() + (P + 8) * 2.0 ** -52 * mag
                ratios["batch"] = max(abs(batch[0] - ref["L"]), abs(batch[1] - ref["dpo_loss"]), abs(batch[2] - ref["sft_loss"]) * 1.25) / bgate
                print(f"{loss_type} eps={eps} rho={with_rho} P={P} mapped={mapped} first={first}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
                for k, v in ratios.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                assert np.isfinite(batch).all()
    _record(f"preference_kernel_pairs[{loss_type}-{eps}-{'rho' if with_rho else 'free'}]", **{f"worst_ratio_{k}": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("target", [60.0, -60.0, 800.0, -800.0])
def test_extreme_margins_stay_finite(target):
    """h ~ +-60 and +-800 (set through the reference log-probs): every output finite, the gates hold."""
    worst = {}
    for loss_type, eps in (("sigmoid", 0.0), ("sigmoid", 0.1), ("hinge", 0.0), ("ipo", 0.0)):
        c = _case(3, True)
        P = 3
        sums = np.array([R.ordered_sum(s) for s in np.split(c["x"], np.cumsum(c["counts"])[:-1])])
        pi = sums / c["counts"] if loss_type == "ipo" else sums
        rho = np.zeros(2 * P)
        rho[:P] = (pi[:P] - pi[P:]) - target / BETA * (1 + 0.01 * np.arange(P))
        rho_sums = rho * c["counts"] if loss_type == "ipo" else rho
        got, ref, batch, rho_k = _run_pairs(c, rho_sums, loss_type, eps)
        assert np.abs(ref["h"] / target - 1).max() < 0.05
        for k, v in got.items():
            assert np.isfinite(v).all(), (loss_type, k)
        assert np.isfinite(batch).all()
        for k, v in R.gate_ratios(got, ref, BETA, rho_k).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _record(f"preference_kernel_extreme[{target}]", **{f"worst_ratio_{k}": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_launcher_refusals():
    from radvlm_amd import lib
    c = _case(1, False)
    P, rows = 1, c["rows"]
    planes = torch.full((7, P), 3.0, dtype=torch.float64, device="cuda")
    batch = torch.full((3,), 3.0, dtype=torch.float64, device="cuda")
    coef = torch.full((rows,), 3.0, dtype=torch.float32, device="cuda")
    sums = torch.full((2,), 3.0, dtype=torch.float64, device="cuda")
    good = dict(logp=c["logp"], seg=c["seg"], row_idx=None, rho=None, P=P, lt=0, beta=0.1, eps=0.0, a_P=1.0, g_N=1.0, planes=planes, batch=batch,
                coef=coef, rows=rows)
    bad = [dict(logp=None), dict(seg=None), dict(planes=None), dict(batch=None), dict(coef=None), dict(P=0), dict(P=-1), dict(rows=0),
           dict(beta=0.0), dict(beta=-0.1), dict(beta=float("inf")), dict(beta=float("nan")), dict(eps=0.5), dict(eps=-0.01), dict(eps=float("nan")),
           dict(lt=3), dict(lt=-1), dict(lt=2, eps=0.1), dict(a_P=float("nan")), dict(g_N=float("nan"))]
    for change in bad:
        a = dict(good, **change)
        rc = _rc("rv_dpo_pairs_f64", a["logp"], a["seg"], a["row_idx"], a["rho"], a["P"], a["lt"], a["beta"], a["eps"], a["a_P"], a["g_N"], a["planes"],
                 a["batch"], a["coef"], a["rows"])
        assert rc == -1, change
    for args in ((None, c["seg"], None, sums, 2, rows), (c["logp"], None, None, sums, 2, rows), (c["logp"], c["seg"], None, None, 2, rows),
                 (c["logp"], c["seg"], None, sums, 0, rows), (c["logp"], c["seg"], None, sums, 2, 0)):
        assert _rc("rv_seq_logp_sums_f64", *args) == -1, args
    torch.cuda.synchronize()
    # nothing was launched: every output still holds its fill
    assert (planes == 3.0).all() and (batch == 3.0).all() and (coef == 3.0).all() and (sums == 3.0).all()
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_dpo_pairs_f64", c["logp"], c["seg"], None, None, P, 0, 0.0, 0.0, 1.0, 1.0, planes, batch, coef, rows)

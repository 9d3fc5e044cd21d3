"""GPU tests of rv_policy_loss_bf16 (radvlm_amd/csrc/policy.hip), the GRPO token loss, against the float64 reference of tests/policy_ref.py
(pinned to autograd in tests/test_policy_host.py).  The gates are the cross-entropy kernel's: the gradient per element at 2^-7 A + 1e-30
(rowops_ref.assert_close_elementwise), the fp32 rows logp / loss / kl at 1e-4 max(1, |lse| + |target|); clip codes are exact.  Two anchors
are bit for bit: logp against -loss_rows of rv_cross_entropy, and the gradient with adv = 1, no old log-probs, beta = 0 and gweight = c
against rv_cross_entropy's with inv_count = c.  The kernel gets the fp32 roundings of the per-row terms and the reference the same values;
the reference rejects inputs within 1e-3 of a clip edge, so no case here can flip between fp32 and float64."""
import functools

import pytest
import torch

import policy_ref as P
from rowops_ref import BF16, assert_close_elementwise, assert_rows_close

pytestmark = pytest.mark.gpu

VS = (8, 9, 2049, 32003)
ROWS = 9
EPS_LO, EPS_HI = 0.2, 0.28
NAN = float("nan")
ADV = (1.0, -0.7, 2.0, -1.5, -0.5, 0.8, NAN, 0.0, 1.2)
RATIO = (1.0, 0.9, 1.5, 1.5, 0.5, 0.5, NAN, 1.1, 1.1)          # row 0: r ~ 1 (old = the fp32 rounding of the reference logp)
CLIP = (0, 0, 2, 0, 1, 0, 0, 0, 0)
WEIGHT = (0.1, 0.2, 0.3, 0.1, 0.05, 0.4, NAN, 0.25, 0.15)
# ref_logp = logp - shift.  Shift 0 (ref == policy, kl = 0) sits on rows whose policy term is live: on a clipped or A = 0 row the whole
# coefficient g would be beta (exp(q) - 1) at q = fp32 rounding residue of (ref - logp), a number with no relative accuracy to hold anyone to.
REF_SHIFT = (-0.3, 0.0, 0.5, 0.0, -0.3, 0.5, NAN, -0.3, 0.5)
IGNORED, A_ZERO, DOMINANT = 6, 7, 8
GSCALE = 0.5


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _call(name, *args):
    from radvlm_amd import lib
    lib.call(name, *args)


def _record(test, worst, **kw):
    from conftest import record_measurement
    record_measurement(test, worst_ratio_of_gate=worst, **kw)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sentinel(shape, dtype=BF16):
    if dtype == BF16:
        return torch.full(shape, 0x7fc5, dtype=torch.int16, device="cuda").view(BF16)
    return torch.full(shape, 0x7fc5a5a5, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_sentinel(t):
    return _same_bits(t, _sentinel(tuple(t.shape), t.dtype))


def _ceil8(v):
    return (v + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def _inputs(V, masked):
    """(bf16 logits [9, V], labels, per-row fp32 terms): N(0, 2) rows, labels at both ends and inside, row 6 ignored with NaN floats,
    row 8 with a dominant label logit (40 above the rest).  masked: -inf logits away from the labels -- scattered, every other column,
    the first vector thread 0 sees, and the first vector of its second trip."""
    g = torch.Generator().manual_seed(1300 + V)
    z = torch.randn(ROWS, V, generator=g) * 2.0
    dom = min(5, V - 1)
    z[DOMINANT, dom] = z[DOMINANT].max() + 40
    labels = torch.tensor([0, V - 1, V // 2, V // 3, 0, V - 1, -100, V // 5, dom])
    if masked:
        keep = z[torch.arange(ROWS), labels.clamp_min(0)].clone()
        z[0, 3::5] = float("-inf")
        z[1, 1::2] = float("-inf")
        if V > 8:
            z[2, :8] = float("-inf")
        if V > 2048:
            z[3, 2048:2056] = float("-inf")
            z[4, :16] = float("-inf")
            z[4, 2048:min(V - 1, 2056)] = float("-inf")
        z[torch.arange(ROWS), labels.clamp_min(0)] = keep              # none at a label
    z = z.to(BF16)
    logp = torch.log_softmax(z.double(), -1)[torch.arange(ROWS), labels.clamp_min(0)]
    f32 = lambda t: t.to(torch.float32)
    old = f32(logp - torch.tensor(RATIO, dtype=torch.float64).log())
    ref = f32(logp - torch.tensor(REF_SHIFT, dtype=torch.float64))
    w = torch.tensor(WEIGHT, dtype=torch.float64)
    return z, labels, dict(adv=torch.tensor(ADV, dtype=torch.float32), lw=f32(w), gw=f32(w * GSCALE), old=old, ref=ref)


@functools.lru_cache(maxsize=None)
def _reference(V, masked, beta, with_old):
    z, labels, t = _inputs(V, masked)
    return P.policy_loss(z, labels, V, t["adv"], t["lw"], t["gw"], t["old"] if with_old else None, t["ref"] if beta > 0 else None,
                         EPS_LO, EPS_HI, beta)


def _packed(z, V):
    """z [rows, V] as the first rows of a [rows + 1, ceil8(V)] buffer: NaN in the pad columns (never read) and in the row past the end."""
    buf = _sentinel((z.shape[0] + 1, _ceil8(V)))
    buf[:-1, :V] = z.cuda()
    return buf


def _launch(logits, ld, lab, t, dl, ld_d, V, beta, with_old, eps=(EPS_LO, EPS_HI), rows=ROWS, adv=None, gw=None):
    stats = _sentinel((5 * rows + 1,), torch.float32)
    dev = lambda a: None if a is None else a.cuda()
    _call("rv_policy_loss_bf16", logits, ld, lab, dev(t["adv"] if adv is None else adv), dev(t["lw"]), dev(t["gw"] if gw is None else gw),
          dev(t["old"]) if with_old else None, dev(t["ref"]) if beta > 0 else None, eps[0], eps[1], beta, stats, dl, ld_d, rows, V)
    assert _is_sentinel(stats[5 * rows:])
    return stats[:5 * rows].view(5, rows)


def _check_all_forms(V, masked, beta, with_old):
    """The four buffer forms on one input; returns the worst ratios (gradient, rows)."""
    z, labels, t = _inputs(V, masked)
    ref = _reference(V, masked, beta, with_old)
    what = f"policy V={V} masked={masked} beta={beta} old={with_old}"
    ld8, lab = _ceil8(V), labels.cuda()
    # (a) in place, ld = ceil8(V)
    a = _packed(z, V)
    st = _launch(a, ld8, lab, t, a, ld8, V, beta, with_old)
    worst_r = 0.0
    for k, name in enumerate(("logp", "loss", "wloss", "kl")):
        worst_r = max(worst_r, assert_rows_close(st[k], ref[name], ref["scale"], 1e-4, f"{what} {name} rows"))
    assert st[4].cpu().tolist() == ref["clip"].float().tolist(), what + ": clip codes"
    if with_old:
        assert st[4].cpu().tolist() == [float(c) for c in CLIP]
    worst_g = assert_close_elementwise(a[:ROWS, :V], ref["grad"], ref["A"], what + " in-place gradient")
    assert float(a[:ROWS, V:].float().abs().max() if ld8 > V else 0.0) == 0.0, what + ": gradient pad columns are zero"
    assert _is_sentinel(a[ROWS:])
    zero_rows = [IGNORED] + ([r for r in range(ROWS) if CLIP[r] and with_old] + [A_ZERO] if beta == 0 else [])
    for r in zero_rows:
        assert float(a[r].float().abs().max()) == 0.0, f"{what}: row {r} has an all-zero gradient"
    assert float(st[:, IGNORED].abs().max()) == 0.0, what + ": the ignored row's statistics are zero"
    if masked:
        assert float(a[:ROWS, :V][torch.isinf(z).cuda()].float().abs().max()) == 0.0          # p = 0 at a masked logit
    # (b) in place in a column slice of a wider buffer
    wide = _sentinel((ROWS, 8 + ld8 + 24))
    wide[:, 8:8 + V] = z.cuda()
    st_b = _launch(wide[:, 8:], wide.stride(0), lab, t, wide[:, 8:], wide.stride(0), V, beta, with_old)
    assert _same_bits(st_b, st) and _same_bits(wide[:, 8:8 + ld8], a[:ROWS]), what + ": slice form"
    assert _is_sentinel(wide[:, :8]) and _is_sentinel(wide[:, 8 + ld8:]), what + ": columns outside the slice"
    # (c) out of place, ld_d != ld; the logits stay as they are
    src = _packed(z, V)
    keep = src.clone()
    dl = _sentinel((ROWS, ld8 + 16))
    st_c = _launch(src, ld8, lab, t, dl, dl.stride(0), V, beta, with_old)
    assert _same_bits(src, keep), what + ": logits unchanged"
    assert _same_bits(st_c, st) and _same_bits(dl[:, :ld8], a[:ROWS]), what + ": out-of-place gradient bit-identical to in-place"
    assert _is_sentinel(dl[:, ld8:])
    # (d) dlogits == NULL: statistics only
    st_d = _launch(src, ld8, lab, t, None, 0, V, beta, with_old)
    assert _same_bits(src, keep) and _same_bits(st_d, st), what + ": dlogits NULL"
    return worst_g, worst_r


@pytest.mark.parametrize("with_old", [True, False])
@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("V", VS)
def test_policy_loss_rows_and_buffer_forms(V, beta, with_old):
    _gpu()
    worst_g, worst_r = _check_all_forms(V, False, beta, with_old)
    _record("policy_loss_kernel", worst_g, V=V, beta=beta, old_logp=with_old, worst_row_ratio_of_1e_4=worst_r)


@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("V", VS)
def test_policy_loss_masked_logits(V, beta):
    _gpu()
    worst_g, worst_r = _check_all_forms(V, True, beta, True)
    _record("policy_loss_kernel_masked", worst_g, V=V, beta=beta, worst_row_ratio_of_1e_4=worst_r)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("V", VS)
def test_bit_anchors_against_cross_entropy(V, masked):
    """logp == -loss_rows of rv_cross_entropy on every live row, whatever the other terms are; and with adv = 1, no old log-probs, beta = 0
    and gweight = c on the live rows the gradient is rv_cross_entropy's with inv_count = c, bit for bit."""
    _gpu()
    z, labels, t = _inputs(V, masked)
    ld8, lab = _ceil8(V), labels.cuda()
    live = (labels >= 0).cuda()
    c = 1.0 / 6
    ce = _packed(z, V)
    ce_loss = _sentinel((ROWS,), torch.float32)
    _call("rv_cross_entropy", ce, ld8, lab, ce_loss, ce, ld8, ROWS, V, c)
    for beta, with_old in ((0.0, True), (0.04, True), (0.0, False)):
        st = _launch(_packed(z, V), ld8, lab, t, None, 0, V, beta, with_old)
        assert _same_bits(st[0][live], -ce_loss[live]), (V, beta, with_old)
        assert float(st[0][~live].abs().max()) == 0.0 and float(ce_loss[~live].abs().max()) == 0.0
    ones = torch.where(labels >= 0, torch.ones(ROWS), torch.full((ROWS,), NAN))
    a = _packed(z, V)
    _launch(a, ld8, lab, t, a, ld8, V, 0.0, False, adv=ones, gw=ones * c)
    assert _same_bits(a, ce), f"V={V}: the SFT anchor"
    assert float(ones[IGNORED]) != float(ones[IGNORED])                 # the ignored row's gweight was NaN and was not read


def test_entry_point_refusals():
    _gpu()
    from radvlm_amd.lib import RadvlmHipError
    V = 9
    z, labels, t = _inputs(V, False)
    buf, lab = _packed(z, V), labels.cuda()
    keep = buf.clone()
    stats = _sentinel((5 * ROWS,), torch.float32)
    dev = {k: v.cuda() for k, v in t.items()}
    good = dict(logits=buf, ld=16, labels=lab, adv=dev["adv"], lw=dev["lw"], gw=dev["gw"], old=dev["old"], ref=dev["ref"], eps_low=EPS_LO,
                eps_high=EPS_HI, beta=0.04, stats=stats, dl=buf, ld_d=16, rows=ROWS, V=V)
    bad = [dict(logits=None), dict(labels=None), dict(adv=None), dict(lw=None), dict(gw=None), dict(stats=None), dict(V=0), dict(V=-3),
           dict(rows=0), dict(V=17), dict(ld=8), dict(ld_d=8), dict(ld=20), dict(ld_d=12), dict(eps_low=-0.1), dict(eps_high=-0.1),
           dict(eps_low=NAN), dict(beta=-0.04), dict(beta=NAN), dict(ref=None), dict(logits=buf.view(-1)[4:]), dict(dl=buf.view(-1)[4:])]
    for change in bad:
        with pytest.raises(RadvlmHipError, match="rv_policy_loss_bf16"):
            _call("rv_policy_loss_bf16", *dict(good, **change).values())
    assert _same_bits(buf, keep) and _is_sentinel(stats)                # nothing was launched
    _call("rv_policy_loss_bf16", *dict(good, ref=None, beta=0.0).values())     # beta = 0 needs no ref_logp; old_logp NULL is the on-policy case
    _call("rv_policy_loss_bf16", *dict(good, old=None, dl=None, ld_d=0).values())
    torch.cuda.synchronize()
    assert not _is_sentinel(stats)

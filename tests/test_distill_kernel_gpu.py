"""GPU tests of rv_distill_loss_bf16 (radvlm_amd/csrc/distill.hip), the full-vocabulary generalised JSD of knowledge distillation, against
the float64 reference of tests/distill_ref.py (pinned to autograd on TRL's formula in tests/test_distill_host.py).  The gates are the
ones distill_ref.py derives: the gradient per element at 2^-7 A + 1e-30, the fp32 rows at 1e-4 max(1, sum |term|).  Bit for bit: the
one-hot-teacher anchor against rv_cross_entropy, teacher == student at beta 0 and 1, the teacher_row map against the identity, and the
out-of-place, slice and NULL-dlogits forms against the in-place one.  (One form of the kernel ships: a form that staged both rows in
LDS gave the same bits at twice the time and was deleted)"""
import functools

import pytest
import torch

import distill_ref as D
from rowops_ref import BF16, assert_close_elementwise, assert_rows_close

pytestmark = pytest.mark.gpu

VS = (8, 9, 2049, 32003, 152064)
BETAS = (0.0, 0.1, 0.5, 0.9, 1.0)
TAUS = (1.0, 0.5, 2.0)
ROWS = D.ROWS
PLANES = ("jsd", "wloss", "kl_teacher", "kl_student")
SCALES = ("scale", "scale", "scale_t", "scale_s")


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


_inputs = functools.lru_cache(maxsize=None)(D.make_inputs)


@functools.lru_cache(maxsize=None)
def _reference(V, beta, tau):
    z, u, labels, lw, gw = _inputs(V)
    return D.distill_loss(z, u, labels, V, lw, gw, beta, tau)


def _packed(z, V, extra_rows=1):
    """z [rows, V] as the first rows of a [rows + 1, ceil8(V)] buffer: NaN in the pad columns (never summed) and in the row past the end."""
    buf = _sentinel((z.shape[0] + extra_rows, _ceil8(V)))
    buf[:z.shape[0], :V] = z.cuda()
    return buf


@functools.lru_cache(maxsize=None)
def _teacher_dev(V):
    return _packed(_inputs(V)[1], V)


def _launch(logits, ld, teacher, ld_t, lab, lw, gw, beta, tau, dl, ld_d, V, teacher_row=None, rows=ROWS):
    stats = _sentinel((4 * rows + 1,), torch.float32)
    _call("rv_distill_loss_bf16", logits, ld, teacher, ld_t, teacher_row, lab, lw.cuda(), gw.cuda(), beta, tau, stats, dl, ld_d, rows, V)
    assert _is_sentinel(stats[4 * rows:])
    return stats[:4 * rows].view(4, rows)


def _check_all_forms(V, beta, tau):
    """The four buffer forms on one input; returns the worst ratios (gradient, rows)."""
    z, u, labels, lw, gw = _inputs(V)
    ref = _reference(V, beta, tau)
    what = f"distill V={V} beta={beta} tau={tau}"
    ld8, lab, t = _ceil8(V), labels.cuda(), _teacher_dev(V)
    t_keep = t.clone()
    # (a) in place, ld = ceil8(V)
    a = _packed(z, V)
    st = _launch(a, ld8, t, ld8, lab, lw, gw, beta, tau, a, ld8, V)
    worst_r = 0.0
    for k, (name, scale) in enumerate(zip(PLANES, SCALES)):
        ratio = assert_rows_close(st[k], ref[name], ref[scale], 1e-4, f"{what} {name} rows")
        print(f"{what}: {name} worst ratio of the rows gate {ratio:.4f}")
        worst_r = max(worst_r, ratio)
    worst_g = assert_close_elementwise(a[:ROWS, :V], ref["grad"], ref["A"], what + " in-place gradient")
    print(f"{what}: worst ratio of the gradient gate {worst_g:.4f}")
    assert float(a[:ROWS, V:].float().abs().max() if ld8 > V else 0.0) == 0.0, what + ": gradient pad columns are zero"
    assert _is_sentinel(a[ROWS:]) and _same_bits(t, t_keep)
    for r in (D.IGNORED, D.ZERO_WEIGHT) + ((D.SAME,) if beta in (0.0, 1.0) else ()):
        assert float(a[r].float().abs().max()) == 0.0, f"{what}: row {r} has an all-zero gradient"
    assert float(st[:, D.IGNORED].abs().max()) == 0.0, what + ": the ignored row's statistics are zero"
    if beta in (0.0, 1.0):
        assert float(st[0, D.SAME]) == 0.0, what + ": teacher == student gives jsd == 0"
        other, own = (3, 2) if beta == 0.0 else (2, 3)
        assert _same_bits(st[own], st[0]) and float(st[other].abs().max()) == 0.0, what + ": the end points' planes"
    assert bool(torch.isfinite(st).all())
    # (b) in place in a column slice of a wider buffer
    wide = _sentinel((ROWS, 8 + ld8 + 24))
    wide[:, 8:8 + V] = z.cuda()
    st_b = _launch(wide[:, 8:], wide.stride(0), t, ld8, lab, lw, gw, beta, tau, wide[:, 8:], wide.stride(0), V)
    assert _same_bits(st_b, st) and _same_bits(wide[:, 8:8 + ld8], a[:ROWS]), what + ": slice form"
    assert _is_sentinel(wide[:, :8]) and _is_sentinel(wide[:, 8 + ld8:]), what + ": columns outside the slice"
    # (c) out of place, ld_d != ld; the logits stay as they are
    src = _packed(z, V)
    keep = src.clone()
    dl = _sentinel((ROWS, ld8 + 16))
    st_c = _launch(src, ld8, t, ld8, lab, lw, gw, beta, tau, dl, dl.stride(0), V)
    assert _same_bits(src, keep), what + ": logits unchanged"
    assert _same_bits(st_c, st) and _same_bits(dl[:, :ld8], a[:ROWS]), what + ": out-of-place gradient bit-identical to in-place"
    assert _is_sentinel(dl[:, ld8:])
    # (d) dlogits == NULL: statistics only
    st_d = _launch(src, ld8, t, ld8, lab, lw, gw, beta, tau, None, 0, V)
    assert _same_bits(src, keep) and _same_bits(st_d, st), what + ": dlogits NULL"
    return worst_g, worst_r


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("V", VS)
def test_distill_loss_rows_and_buffer_forms(V, beta, tau):
    _gpu()
    worst_g, worst_r = _check_all_forms(V, beta, tau)
    _record("distill_loss_kernel", worst_g, V=V, beta=beta, temperature=tau, worst_row_ratio_of_1e_4=worst_r)


@pytest.mark.parametrize("V", VS)
def test_one_hot_teacher_is_the_cross_entropy(V):
    """Forward KL at temperature 1 against a teacher whose label logit is 200 above the rest (every other t underflows to exactly 0) is the
    SFT step: the jsd plane is rv_cross_entropy's loss rows and the gradient with gweight = c is its gradient with inv_count = c, bit for bit."""
    _gpu()
    z, _, labels, lw, _ = _inputs(V)
    ld8, lab = _ceil8(V), labels.cuda()
    c = 1.0 / 6
    ce = _packed(z, V)
    ce_loss = _sentinel((ROWS,), torch.float32)
    _call("rv_cross_entropy", ce, ld8, lab, ce_loss, ce, ld8, ROWS, V, c)
    hot = torch.zeros(ROWS, V)
    hot[torch.arange(ROWS), labels.clamp_min(0)] = 200.0
    hot[D.IGNORED] = D.NAN
    gw = torch.where(labels >= 0, torch.full((ROWS,), c), torch.full((ROWS,), D.NAN))
    a = _packed(z, V)
    st = _launch(a, ld8, _packed(hot.to(BF16), V), ld8, lab, lw, gw, 0.0, 1.0, a, ld8, V)
    assert _same_bits(st[0], ce_loss), f"V={V}: the jsd plane is the cross entropy's loss rows"
    assert _same_bits(a, ce), f"V={V}: the SFT anchor"


@pytest.mark.parametrize("V", VS)
def test_teacher_row_map_is_the_identity_on_a_permuted_buffer(V):
    _gpu()
    z, u, labels, lw, gw = _inputs(V)
    ld8, lab = _ceil8(V), labels.cuda()
    perm = torch.tensor([4, 7, 0, 8, 2, 6, 1, 3, 5])                # teacher row of student row r
    shuffled = torch.empty(ROWS, V, dtype=BF16)
    shuffled[perm] = u
    tmap = perm.to(torch.int32)
    tmap[D.IGNORED] = -1
    for beta, tau in ((0.0, 1.0), (0.5, 2.0), (1.0, 0.5)):
        a, b = _packed(z, V), _packed(z, V)
        st_a = _launch(a, ld8, _teacher_dev(V), ld8, lab, lw, gw, beta, tau, a, ld8, V)
        st_b = _launch(b, ld8, _packed(shuffled, V), ld8, lab, lw, gw, beta, tau, b, ld8, V, teacher_row=tmap.cuda())
        assert _same_bits(st_a, st_b) and _same_bits(a, b), (V, beta, tau)
    # -1 on a labelled row: ignored like a label of -100
    tmap[D.GENERIC] = -1
    a = _packed(z, V)
    st = _launch(a, ld8, _packed(shuffled, V), ld8, lab, lw, gw, 0.5, 1.0, a, ld8, V, teacher_row=tmap.cuda())
    assert float(st[:, D.GENERIC].abs().max()) == 0.0 and float(a[D.GENERIC].float().abs().max()) == 0.0


def test_rows_do_not_depend_on_the_grid():
    """A row's bits depend on the row pair and the scalars alone: one row launched alone equals the same row inside the nine."""
    _gpu()
    V = 2049
    z, u, labels, lw, gw = _inputs(V)
    ld8 = _ceil8(V)
    a = _packed(z, V)
    st = _launch(a, ld8, _teacher_dev(V), ld8, labels.cuda(), lw, gw, 0.5, 2.0, a, ld8, V)
    r = D.NOISY
    b = _packed(z[r:r + 1], V)
    st1 = _launch(b, ld8, _packed(u[r:r + 1], V), ld8, labels[r:r + 1].cuda(), lw[r:r + 1], gw[r:r + 1], 0.5, 2.0, b, ld8, V, rows=1)
    assert _same_bits(st1[:, 0], st[:, r]) and _same_bits(b[0], a[r])


def test_entry_point_refusals():
    _gpu()
    from radvlm_amd.lib import RadvlmHipError
    V = 9
    z, u, labels, lw, gw = _inputs(V)
    buf, t, lab = _packed(z, V), _packed(u, V), labels.cuda()
    keep = buf.clone()
    stats = _sentinel((4 * ROWS,), torch.float32)
    inf = float("inf")
    good = dict(logits=buf, ld=16, teacher=t, ld_t=16, tmap=None, labels=lab, lw=lw.cuda(), gw=gw.cuda(), beta=0.5, tau=1.0, stats=stats,
                dl=buf, ld_d=16, rows=ROWS, V=V)
    bad = [dict(logits=None), dict(teacher=None), dict(labels=None), dict(lw=None), dict(gw=None), dict(stats=None), dict(V=0), dict(V=-3),
           dict(rows=0), dict(V=17), dict(ld=8), dict(ld_t=8), dict(ld_d=8), dict(ld=20), dict(ld_t=20), dict(ld_d=12), dict(beta=-0.1),
           dict(beta=1.5), dict(beta=D.NAN), dict(tau=0.0), dict(tau=-1.0), dict(tau=D.NAN), dict(tau=inf),
           dict(logits=buf.view(-1)[4:]), dict(teacher=t.view(-1)[4:]), dict(dl=buf.view(-1)[4:])]
    for change in bad:
        with pytest.raises(RadvlmHipError, match="rv_distill_loss_bf16"):
            _call("rv_distill_loss_bf16", *dict(good, **change).values())
    assert _same_bits(buf, keep) and _is_sentinel(stats)                # nothing was launched
    _call("rv_distill_loss_bf16", *dict(good, dl=None, ld_d=0).values())
    _call("rv_distill_loss_bf16", *dict(good, beta=0.0).values())
    torch.cuda.synchronize()
    assert not _is_sentinel(stats)

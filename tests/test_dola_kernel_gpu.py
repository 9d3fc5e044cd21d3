"""GPU tests of rv_dola_contrast_rows_f32 (csrc/dola.hip) through ops.dola_contrast_rows, against tests/dola_ref.py.

Inputs as the issue sets them: f = 4 * randn(n); candidate k is f + sigma_k * randn(n), sigma_k = 0.25 * 2^(k/2) in a shuffled order;
fp32, seeded; ld = n + 5 with NaN in the padding columns.  The float64 reference (dola_ref.jsd64 / jsd_error_bound: plain torch
statements) runs on the device, where a 33 x 17 x 32000 case takes milliseconds instead of seconds; one case pins it to the CPU run."""
import functools
import math

import numpy as np
import pytest
import torch

import dola_ref

pytestmark = pytest.mark.gpu

NS = (1, 2, 255, 256, 257, 2047, 2049, 32000)
LAYERS = (1, 2, 7, 16)
ROWS = (1, 3, 33)
PAD = 5


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _inputs(n, nl, rows, seed=0):
    """(f [rows, n + PAD], c [nl, rows, n + PAD]) on the device, NaN in the padding columns."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + 31 * nl + rows)
    f = torch.full((rows, n + PAD), float("nan"))
    c = torch.full((nl, rows, n + PAD), float("nan"))
    f[:, :n] = 4 * torch.randn(rows, n, generator=g)
    order = torch.randperm(nl, generator=g).tolist()
    for k in range(nl):
        c[k, :, :n] = f[:, :n] + 0.25 * 2 ** (order[k] / 2) * torch.randn(rows, n, generator=g)
    return f.cuda(), c.cuda()


def _nan_bits(x):
    return x.view(torch.int32)


def _run_case(n, nl, rows, seed=0):
    """One launch and every per-case check; returns (rows checked for selection, rows left out, worst |J^ - J| / bound)."""
    ops = _ops()
    f0, c0 = _inputs(n, nl, rows, seed)
    f, c = f0.clone(), c0.clone()
    out, chosen, jsd = ops.dola_contrast_rows(f, c, n, want_jsd=True)
    assert out is f and chosen.dtype == torch.int32 and tuple(chosen.shape) == (rows,) and tuple(jsd.shape) == (rows, nl)
    ch = chosen.long()
    assert int(ch.min()) >= 0 and int(ch.max()) < nl
    # padding: never written, never read into a result; the candidates are only read
    assert torch.equal(_nan_bits(f[:, n:]), _nan_bits(f0[:, n:])) and torch.equal(_nan_bits(c), _nan_bits(c0))
    assert not torch.isnan(f[:, :n]).any() and torch.isfinite(jsd).all()
    # contrast bits: torch on the log-softmax kernel's rows of the mature and the chosen row
    lf = ops.log_softmax_rows(f0.clone(), n)[:, :n]
    lq = ops.log_softmax_rows(c0.clone().view(nl * rows, n + PAD), n).view(nl, rows, n + PAD)[:, :, :n]
    lb = lq[ch, torch.arange(rows, device="cuda")]
    thresh = lf.max(1, keepdim=True).values + torch.tensor(dola_ref.LOG_RT, device="cuda")
    want = torch.where(lf < thresh, torch.full_like(lf, float("-inf")), lf - lb)
    assert torch.equal(f[:, :n], want), (n, nl, rows)
    am = f0[:, :n].argmax(1)
    assert torch.isfinite(f[torch.arange(rows), am]).all()                  # the row maximum survives the filter
    if nl == 1:
        assert int(ch.max()) == 0 and not jsd.any()                         # no divergence computed: written as 0
        return 0, 0, 0.0
    # divergence: against float64 on the exact log-softmax of the fp32 logits, per row and per candidate
    lf64 = torch.log_softmax(f0[:, :n].double(), -1)
    lq64 = torch.log_softmax(c0[:, :, :n].double(), -1)
    J64 = torch.stack([dola_ref.jsd64(lf64, lq64[k]) for k in range(nl)], 1)
    bound = torch.stack([dola_ref.jsd_error_bound(lf64, lq64[k]) for k in range(nl)], 1)
    err = (jsd.double() - J64).abs()
    assert (err <= bound).all(), (n, nl, rows, float((err / bound).max()))
    if n == 1:                                                              # lf = lq = 0 exactly: J = 0, the tie rule decides
        assert not jsd.any() and not ch.any()
        return rows, 0, 0.0
    # selection: argmax J64 wherever the two largest J64 differ by more than the sum of their bounds
    top = torch.topk(J64, 2, dim=1)
    gap = top.values[:, 0] - top.values[:, 1]
    slack = bound.gather(1, top.indices).sum(1)
    sure = gap > slack
    assert torch.equal(ch[sure], top.indices[sure, 0]), (n, nl, rows)
    return rows, int((~sure).sum()), float((err / bound).max())


@functools.lru_cache(maxsize=None)
def _sweep(n, rows):
    return tuple(_run_case(n, nl, rows) for nl in LAYERS)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
def test_contrast_bits_padding_divergence_and_selection(n, rows):
    _sweep(n, rows)


def test_qwen_vocabulary_row():
    checked, left, worst = _run_case(152064, 7, 1)
    assert checked == 1 and left == 0 and worst <= 1.0


def test_at_most_five_percent_of_the_rows_are_too_close_to_call():
    from conftest import record_measurement
    res = [r for n in NS for rows in ROWS for r in _sweep(n, rows)] + [_run_case(152064, 7, 1)]
    checked, left = sum(r[0] for r in res), sum(r[1] for r in res)
    worst = max(r[2] for r in res)
    print(f"dola selection: {checked} rows, {left} left out, worst |J^ - J| / bound {worst:.3g}")
    record_measurement("dola_kernel", rows=checked, left_out=left, worst_err_over_bound=worst)
    assert checked >= 800 and left * 20 <= checked, (checked, left)


def test_device_float64_reference_is_the_cpu_one():
    _ops()
    f0, c0 = _inputs(257, 7, 3)
    lf, lq = torch.log_softmax(f0[:, :257].double(), -1), torch.log_softmax(c0[:, :, :257].double(), -1)
    for k in range(7):
        a, b = dola_ref.jsd64(lf, lq[k]).cpu(), dola_ref.jsd64(lf.cpu(), lq[k].cpu())
        assert ((a - b).abs() <= 1e-12 * b.abs()).all()
        a, b = dola_ref.jsd_error_bound(lf, lq[k]).cpu(), dola_ref.jsd_error_bound(lf.cpu(), lq[k].cpu())
        assert ((a - b).abs() <= 1e-9 * b.abs()).all()


@pytest.mark.parametrize("n,nl", [(257, 7), (2049, 16), (32000, 2), (32000, 7)])
def test_a_row_does_not_depend_on_its_neighbours(n, nl):
    """Row r's f, chosen and jsd bits among 33 rows are those of the row alone and among 3 rows (other grids, other workspaces)."""
    ops = _ops()
    f0, c0 = _inputs(n, nl, 33)
    f, c = f0.clone(), c0.clone()
    _, ch, jsd = ops.dola_contrast_rows(f, c, n, want_jsd=True)
    for r in (0, 17, 32):
        f1, c1 = f0[r:r + 1].clone(), c0[:, r:r + 1].clone()
        _, ch1, jsd1 = ops.dola_contrast_rows(f1, c1, n, want_jsd=True)
        assert torch.equal(_nan_bits(f1), _nan_bits(f[r:r + 1])) and int(ch1[0]) == int(ch[r]) and torch.equal(jsd1[0], jsd[r])
    f3, c3 = f0[15:18].clone(), c0[:, 15:18].clone()
    ws = ops.dola_workspace(64, 16, "cuda")                                 # a larger shared workspace changes nothing
    _, ch3, jsd3 = ops.dola_contrast_rows(f3, c3, n, ws=ws, want_jsd=True)
    assert torch.equal(_nan_bits(f3), _nan_bits(f[15:18])) and torch.equal(ch3, ch[15:18]) and torch.equal(jsd3, jsd[15:18])
    # a garbage neighbour (an idle slot's row) touches no other row and cannot push `chosen` out of range
    fg, cg = f0[:3].clone(), c0[:, :3].clone()
    fg[1, :n], cg[:, 1, :n] = float("nan"), float("inf")
    _, chg, jsdg = ops.dola_contrast_rows(fg, cg, n, want_jsd=True)
    assert 0 <= int(chg[1]) < nl
    for r in (0, 2):
        assert torch.equal(_nan_bits(fg[r]), _nan_bits(f[r])) and int(chg[r]) == int(ch[r]) and torch.equal(jsdg[r], jsd[r])


def test_jsd_does_not_depend_on_the_other_candidates():
    ops = _ops()
    n = 2049
    f0, c0 = _inputs(n, 7, 3)
    _, _, jsd = ops.dola_contrast_rows(f0.clone(), c0.clone(), n, want_jsd=True)
    _, _, two = ops.dola_contrast_rows(f0.clone(), c0[[5, 2]].clone(), n, want_jsd=True)
    assert torch.equal(two[:, 0], jsd[:, 5]) and torch.equal(two[:, 1], jsd[:, 2])


def test_ties():
    ops = _ops()
    n = 2047
    f0, c0 = _inputs(n, 4, 3)
    J = ops.dola_contrast_rows(f0.clone(), c0.clone(), n, want_jsd=True)[2]
    best = J.argmax(1)
    for r in range(3):                                                      # the winner twice: the lower index is chosen
        b = int(best[r])
        order = [k for k in range(4) if k != b]
        c = torch.stack([c0[order[0]], c0[b], c0[order[1]], c0[b], c0[order[2]]])
        _, ch, jsd = ops.dola_contrast_rows(f0.clone(), c, n, want_jsd=True)
        assert int(ch[r]) == 1 and jsd[r, 1] == jsd[r, 3] == J[r, b]
    f, c = f0.clone(), torch.stack([f0, f0])                                # every candidate equals the mature row
    _, ch, jsd = ops.dola_contrast_rows(f, c, n, want_jsd=True)
    assert not ch.any() and float(jsd.abs().max()) <= float(dola_ref.jsd_error_bound(torch.log_softmax(f0[:, :n].double(), -1),
                                                                                    torch.log_softmax(f0[:, :n].double(), -1)).max())
    kept = torch.isfinite(f[:, :n])
    assert kept.any(1).all() and not f[:, :n][kept].any()                   # out = 0 on the kept entries
    f1 = torch.tensor([[3.25] + [float("nan")] * PAD], device="cuda")       # n = 1, one candidate: out = 0
    c1 = torch.tensor([[[-7.5] + [float("nan")] * PAD]], device="cuda")
    _, ch, jsd = ops.dola_contrast_rows(f1, c1, 1, want_jsd=True)
    assert float(f1[0, 0]) == 0.0 and int(ch[0]) == 0 and float(jsd[0, 0]) == 0.0 and torch.isnan(f1[0, 1:]).all()


def test_argument_errors_are_refused_and_a_good_call_follows():
    ops = _ops()
    from radvlm_amd import lib
    n, nl, rows = 300, 3, 2
    f, c = _inputs(n, nl, rows)
    ld = n + PAD
    ch = torch.empty(rows, dtype=torch.int32, device="cuda")
    ws = ops.dola_workspace(rows, nl, "cuda")
    need = lib.load().rv_dola_ws_bytes(rows, nl)
    assert need == rows * (1 + nl) * 8 + rows * nl * 64 * 8 and lib.load().rv_dola_ws_bytes(0, nl) == 0
    good = dict(f=f, ld_f=ld, c=c, ld_c=ld, st=rows * ld, rows=rows, nl=nl, n=n, ch=ch, ws=ws, wsb=ws.numel() * 8)

    def call(**kw):
        a = dict(good, **kw)
        lib.call("rv_dola_contrast_rows_f32", a["f"], a["ld_f"], a["c"], a["ld_c"], a["st"], a["rows"], a["nl"], a["n"], ops.DOLA_LOG_RT,
                 a["ch"], None, a["ws"], a["wsb"])

    bad = [dict(f=None), dict(c=None), dict(ch=None), dict(ws=None), dict(rows=0), dict(rows=-1), dict(nl=0), dict(nl=17), dict(n=0),
           dict(n=262145), dict(ld_f=n - 1), dict(ld_c=n - 1), dict(wsb=need - 8), dict(ws=ws.data_ptr() + 4, wsb=need)]
    for kw in bad:
        with pytest.raises(lib.RadvlmHipError, match="code -1"):
            call(**kw)
    before = f.clone()
    call()
    torch.cuda.synchronize()
    assert not torch.equal(_nan_bits(f), _nan_bits(before)) and 0 <= int(ch.min()) and int(ch.max()) < nl
    want = ops.dola_contrast_rows(before, c, n)
    assert torch.equal(_nan_bits(f), _nan_bits(want[0])) and torch.equal(ch, want[1])

"""CPU checks of tests/rowops_ref.py: every float64 reference equals float64 torch autograd of the textbook op to 1e-12, the magnitude
tensors bound the references, and the per-element checker bites where the whole-tensor max|d| / max|ref| metric of tests/test_kernels_gpu.py
does not -- so a failure of tests/test_rowops_edges_gpu.py points at a kernel."""
import pytest
import torch
import torch.nn.functional as F

import rowops_ref as R
from rowops_ref import BF16, TOL, assert_close_elementwise, rbf

torch.manual_seed(0)


def _bf(*shape, std=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF16)


def _eq(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_rmsnorm_reference_is_autograd_of_the_textbook_op(eps):
    """oracle.llava_oracle.rmsnorm computes in fp32 whatever its input, so it pins the reference to 1e-5 only; the same formula in float64
    (and its autograd) pins it to 1e-12."""
    from oracle import llava_oracle as O
    rows, d = 5, 72
    x = (_bf(rows, d, seed=1).float() * torch.tensor([1e-3, 1.0, 30.0, 0.0, 1.0])[:, None]).to(BF16)
    w, dy, dx_in, dw_in = (1 + 0.1 * _bf(d, seed=2).float()).to(BF16), _bf(rows, d, seed=3), _bf(rows, d, seed=4), _bf(d, seed=5)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    rstd = torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps)
    y = wr * (xr * rstd)
    y.backward(dy.double())
    yref, A, alt, rs = R.rmsnorm_fwd(x, w, eps)
    _eq(rs, rstd.detach()[:, 0])
    assert float(rs[3]) == eps ** -0.5                                   # the all-zero row
    assert bool(((yref - y.detach()).abs() <= 2.0 ** -8 * y.detach().abs()).all())     # the textbook value with x * rstd rounded to bf16 once
    assert torch.equal(yref, w.double() * rbf(x.double() * rstd.detach()))
    assert torch.equal(A, yref.abs())
    differs = alt != yref
    assert bool(((alt - yref).abs() <= TOL * A + 1e-300)[differs].all())               # the other candidate is the neighbouring bf16 number
    dx, Adx, dw, Adw = R.rmsnorm_bwd(dy, x, w, eps)
    _eq(dx, xr.grad)
    _eq(dw, wr.grad)
    assert bool((dx.abs() <= Adx * (1 + 1e-12)).all()) and bool((dw.abs() <= Adw * (1 + 1e-12)).all())
    dx2, Adx2, dw2, Adw2 = R.rmsnorm_bwd(dy, x, w, eps, dx_in=dx_in, dw_in=dw_in)
    _eq(dx2, xr.grad + dx_in.double())
    _eq(dw2, wr.grad + dw_in.double())
    _eq(Adx2, Adx + dx_in.double().abs())
    # the magnitude tensor as the issue states it: |dx_in| + rstd (|g| + |xhat| mean|g xhat|)
    g, xh = dy.double() * w.double(), x.double() * rstd.detach()
    _eq(Adx2, dx_in.double().abs() + rstd.detach() * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True)))
    # the fp32 oracle on fp32 inputs agrees with the unrounded float64 formula to fp32 precision
    _eq(O.rmsnorm(x.float(), w.float(), eps).double(), y.detach(), 1e-5)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_layernorm_reference_is_autograd_of_layer_norm(eps):
    rows, d = 4, 40
    x = ((_bf(rows, d, seed=6).float() + 0.5) * torch.tensor([1e-3, 1.0, 30.0, 0.0])[:, None]).to(BF16)
    w, b, dy = (1 + 0.1 * _bf(d, seed=7).float()).to(BF16), _bf(d, std=0.1, seed=8), _bf(rows, d, seed=9)
    dx_in, dw_in, db_in = _bf(rows, d, seed=10), _bf(d, seed=11), _bf(d, seed=12)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xr, (d,), wr, br, eps)
    y.backward(dy.double())
    yref, A, mean, rstd = R.layernorm_fwd(x, w, b, eps)
    _eq(yref, y.detach())
    _eq(mean, x.double().mean(-1))
    _eq(rstd, torch.rsqrt(x.double().var(-1, unbiased=False) + eps))
    assert float(rstd[3]) == eps ** -0.5 and bool((yref.abs() <= A * (1 + 1e-12)).all())
    dx, Adx, dw, Adw, db, Adb = R.layernorm_bwd(dy, x, w, eps)
    _eq(dx, xr.grad)
    _eq(dw, wr.grad)
    _eq(db, br.grad)
    for v, a in ((dx, Adx), (dw, Adw), (db, Adb)):
        assert bool((v.abs() <= a * (1 + 1e-12)).all())
    dx2, _, dw2, _, db2, _ = R.layernorm_bwd(dy, x, w, eps, dx_in=dx_in, dw_in=dw_in, db_in=db_in)
    _eq(dx2, xr.grad + dx_in.double())
    _eq(dw2, wr.grad + dw_in.double())
    _eq(db2, br.grad + db_in.double())


@pytest.mark.parametrize("hd,nsec,heads", [(16, 1, 1), (64, 2, 3), (128, 2, 1)])
def test_rope_reference_is_apply_rope(hd, nsec, heads):
    from oracle import llava_oracle as O
    rows, S = 11, 23
    pos = torch.tensor([3, 0, 22, 3, 7, 7, 1, 19, 2, 0, 5])
    x = _bf(rows, nsec * heads * hd + 24, seed=hd)
    cos, sin = O.rope_cos_sin(S, hd)
    cos, sin = cos.to(BF16).double(), sin.to(BF16).double()
    cs = torch.stack((cos[:, :hd // 2], sin[:, :hd // 2]), dim=-1).float()
    n = nsec * heads * hd
    q = x[:, :n].double().view(rows, nsec * heads, hd).transpose(0, 1)[None]          # [1, nsec*heads, rows, hd]
    for direction in (1, -1):
        qe, _ = O.apply_rope(q, q, cos[pos], direction * sin[pos])
        y, A = R.rope(x, cs, pos, heads, hd, nsec, direction)
        _eq(y, qe[0].transpose(0, 1).reshape(rows, n))
        assert bool((y.abs() <= A * (1 + 1e-12)).all())
    # A as the issue states it: |a cos| + |b sin|
    a, b = x[:, :hd // 2].double(), x[:, hd // 2:hd].double()
    _eq(R.rope(x, cs, pos, heads, hd, nsec)[1][:, :hd // 2], (a * cos[pos][:, :hd // 2]).abs() + (b * sin[pos][:, :hd // 2]).abs())


def _act_inputs(n, seed):
    x = _bf(n, seed=seed).float()
    planted = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 10, -10, 30, -30, 100, -100, 1e4, -1e4])
    x[:planted.numel()] = planted
    return x.to(BF16)


def test_activation_references_are_autograd_of_the_textbook_ops():
    from oracle import llava_oracle as O
    n = 64
    x, dy, u = _act_inputs(n, 20), _bf(n, seed=21), _bf(n, seed=22)
    for fwd, bwd, op in ((R.quick_gelu_fwd, R.quick_gelu_bwd, O.quick_gelu), (R.gelu_fwd, R.gelu_bwd, F.gelu),
                         (R.gelu_tanh_fwd, R.gelu_tanh_bwd, lambda t: F.gelu(t, approximate="tanh"))):
        xr = x.double().requires_grad_(True)
        y = op(xr)
        y.backward(dy.double())
        yr, A = fwd(x)
        dr, Ad = bwd(dy, x)
        _eq(yr, y.detach())
        _eq(dr, xr.grad)
        assert bool((yr.abs() <= A * (1 + 1e-12)).all()) and bool((dr.abs() <= Ad * (1 + 1e-12)).all())
        assert bool(torch.isfinite(yr).all() and torch.isfinite(dr).all() and torch.isfinite(A).all() and torch.isfinite(Ad).all())
    gr, ur = x.double().requires_grad_(True), u.double().requires_grad_(True)
    act = F.silu(gr) * ur
    act.backward(dy.double())
    dg, Adg, du, Adu = R.swiglu_bwd(dy, x, u)
    _eq(dg, gr.grad)
    _eq(du, ur.grad)
    assert bool((dg.abs() <= Adg * (1 + 1e-12)).all()) and torch.equal(Adu, du.abs())
    a, A, alt = R.swiglu_fwd(x, u)
    assert bool(((a - act.detach()).abs() <= 2.0 ** -8 * act.detach().abs() + 1e-38).all())      # silu(g) rounded to bf16 once (bf16 subnormals flush)
    assert torch.equal(a, rbf(F.silu(x.double())) * u.double()) and torch.equal(A, a.abs())
    assert bool(((alt - a).abs() <= TOL * A + 1e-300).all())


@pytest.mark.parametrize("V,ld", [(8, 8), (9, 16), (1001, 1024), (2049, 2056)])
def test_cross_entropy_reference_is_autograd_of_cross_entropy(V, ld):
    rows = 8
    z = (2 * _bf(rows, ld, seed=V).float())
    z[1] += 300
    z[2] -= 200
    labels = torch.tensor([0, V - 1, V // 2, -100, 1, V - 1, 0, -100])
    z[4, 1] = z[4, :V].max() + 40                                         # a dominant label logit: p ~ 1
    if V > 8:
        z[5, :8] = float("-inf")
        z[6, 3::5] = float("-inf")
        z[6, 0] = 0.0
    z = z.to(BF16)
    z[:, V:] = float("nan")                                               # pad columns are never read
    inv = 1.0 / 6
    zr = z[:, :V].double().requires_grad_(True)
    loss = F.cross_entropy(zr, labels, ignore_index=-100, reduction="none")
    (loss.sum() * inv).backward()
    lr, scale, g, A = R.cross_entropy(z, labels, V, inv)
    _eq(lr, loss.detach())
    _eq(g, zr.grad)
    assert bool(torch.isfinite(lr).all() and torch.isfinite(g).all() and torch.isfinite(A).all())
    assert float(g[3].abs().max()) == 0.0 and float(A[3].abs().max()) == 0.0 and float(lr[3]) == 0.0
    p = torch.softmax(z[:, :V].double(), -1)
    onehot = F.one_hot(labels.clamp_min(0), V).double()
    live = (labels >= 0)[:, None].double()
    _eq(A, (p + onehot) * inv * live)
    assert bool((scale >= 1).all()) and abs(float(scale[1]) - float(torch.logsumexp(z[1, :V].double(), 0).abs() + z[1, V - 1].double().abs())) < 1e-9
    if V > 8:
        assert float(g[5, :8].abs().max()) == 0.0                         # p = 0 at a -inf logit


def test_colsum_reference():
    x, o = _bf(33, 40, seed=30), _bf(40, seed=31)
    s, A = R.colsum(x, o)
    _eq(s, x.double().sum(0) + o.double())
    _eq(A, x.double().abs().sum(0) + o.double().abs())


def _scaled_rows():
    g = torch.Generator().manual_seed(40)
    ref = torch.randn(3, 64, generator=g, dtype=torch.float64) * torch.tensor([1000.0, 1.0, 1000.0], dtype=torch.float64)[:, None]
    # The gate 2^-7 |ref| is ONE bf16 ulp at the bottom of a binade and two at its top, so a one-ulp error can only be told from rounding
    # low in a binade: the planted element is 1 + 0.7 * 2^-7, which rounds up (by 0.3 ulp) to 1 + 2^-7.
    ref[1, 17] = 1.0 + 0.7 * 2.0 ** -7
    return ref


def test_pure_bf16_rounding_of_a_reference_passes():
    ref = _scaled_rows()
    worst = assert_close_elementwise(ref.to(BF16), ref, ref.abs(), "bf16 rounding")
    assert worst <= 0.5 + 1e-9
    # and of real references, subnormal and saturated values included
    x, u, dy = _act_inputs(64, 41), _bf(64, seed=42), _bf(64, seed=43)
    for ref, A in (R.gelu_fwd(x), R.gelu_tanh_bwd(dy, x), R.quick_gelu_bwd(dy, x), R.swiglu_bwd(dy, x, u)[:2], R.swiglu_fwd(x, u)[:2]):
        assert assert_close_elementwise(ref.to(BF16), ref, A, "bf16 rounding") <= 0.5 + 1e-9


def test_checker_fails_a_one_ulp_error_in_a_small_row_that_the_whole_tensor_metric_passes():
    ref = _scaled_rows()
    got = ref.to(BF16).clone()
    assert float(got[1, 17]) == 1.0 + 2.0 ** -7
    got[1, 17] = 1.0 + 2.0 ** -6                                          # one bf16 ulp further from the reference
    with pytest.raises(AssertionError, match=r"element \(1, 17\)"):
        assert_close_elementwise(got, ref, ref.abs(), "planted ulp")
    whole = float((got.double() - ref).abs().max() / ref.abs().max())     # test_kernels_gpu.py's relerr: blind to it
    assert whole < TOL
    # an entire small row wrong by 5 % passes the old metric too, and fails here
    got = ref.to(BF16).clone()
    got[1] = (1.05 * ref[1]).to(BF16)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < TOL
    with pytest.raises(AssertionError):
        assert_close_elementwise(got, ref, ref.abs(), "small row off by 5 %")
    # NaN and inf never pass, whatever A is
    for bad in (float("nan"), float("inf")):
        got = ref.to(BF16).clone()
        got[2, 5] = bad
        with pytest.raises(AssertionError):
            assert_close_elementwise(got, ref, torch.full_like(ref, 1e30), "non-finite")
    # an exact zero where the reference is below the floor passes (A = |ref| = 1e-40)
    tiny = torch.full((4,), -1e-40, dtype=torch.float64)
    assert assert_close_elementwise(torch.zeros(4, dtype=BF16), tiny, tiny.abs(), "flushed") <= 1.0


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
def test_fp32_emulation_of_the_kernels_stays_inside_the_gate(eps):
    """The kernels' formulas in fp32 on the CPU, stored as bf16, at the GPU test's sizes and row scales: the references leave a correct
    fp32 implementation at most half of the gate (the bf16 store), intermediate-rounding ties included."""
    worst = 0.0
    for d in (8, 520, 2056, 4096, 8192):
        x = (_bf(4, d, seed=d).float() * torch.tensor([1e-3, 1.0, 30.0, 0.0])[:, None]).to(BF16)
        w, dy = (1 + 0.1 * _bf(d, seed=d + 1).float()).to(BF16), _bf(4, d, seed=d + 2)
        xf, wf, gf = x.float(), w.float(), dy.float() * w.float()
        rs = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        y = (wf * (xf * rs).to(BF16).float()).to(BF16)
        yref, A, alt, _ = R.rmsnorm_fwd(x, w, eps)
        worst = max(worst, assert_close_elementwise(y, yref, A, f"rmsnorm fwd d={d}", alt=alt))
        xh = xf * rs
        dx = (rs * (gf - xh * (gf * xh).mean(-1, keepdim=True))).to(BF16)
        dxr, Adx, _, _ = R.rmsnorm_bwd(dy, x, w, eps)
        worst = max(worst, assert_close_elementwise(dx, dxr, Adx, f"rmsnorm bwd d={d}"))
    for V in (9, 1001, 32003):
        z = 2 * _bf(4, V, seed=V).float()
        z[1] += 300
        z[2, 5] = z[2].max() + 40
        z = z.to(BF16)
        labels = torch.tensor([0, V - 1, 5, 3])
        zf = z.float()
        lse = torch.logsumexp(zf, -1, keepdim=True)
        g = ((torch.exp(zf - lse) - F.one_hot(labels, V).float()) * 0.25).to(BF16)
        _, _, gr, A = R.cross_entropy(z, labels, V, 0.25)
        worst = max(worst, assert_close_elementwise(g, gr, A, f"ce grad V={V}"))
    assert worst <= 0.5 + 1e-3, worst

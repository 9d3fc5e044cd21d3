"""float64 references of the row and elementwise training kernels (radvlm_amd/csrc/ops.hip): RMSNorm and LayerNorm forward / backward, RoPE,
SwiGLU, the three GELUs, cross entropy and the column sums.  Plain torch on the CPU on the bf16-rounded inputs; nothing here touches a GPU, so
tests/test_rowops_ref_host.py pins every reference to float64 autograd of the textbook op without one, and tests/test_rowops_edges_gpu.py
holds the kernels to them.

Every reference returns its value AND a magnitude tensor A of the same shape: the kernel's own formula with every term replaced by its
absolute value and every subtraction by an addition.  A is what the rounding of the formula's terms can add up to, so an error is judged
against A of its own element (assert_close_elementwise) and not against the largest value of the tensor: a row 1000x smaller than its
neighbours, or an element that is a small difference of large terms, is held to its own scale.

Where the kernel rounds an intermediate through bf16 by design, the reference rounds at the same place: rbf(x * rstd) in the RMSNorm forward,
rbf(silu(g)) in the SwiGLU forward.  The kernel evaluates that intermediate in fp32, the reference in float64; where the float64 value lies
within 2^-17 (relative) of the midpoint of two bf16 numbers, fp32 arithmetic may legitimately round to the other one, so these two references
also return `alt`, the result with that intermediate rounded the other way (equal to the reference elsewhere), and the checker accepts an
element that meets the gate against either.  2^-17: the fp32 intermediate is a product of two factors each good to a few ulps (2^-22), or
silu through the fast exp, whose argument rounding costs |g| 2^-24 <= 2^-19 where exp(-g) still matters (|g| < 32).
"""
import math

import torch

BF16 = torch.bfloat16
TOL = 2.0 ** -7           # the project's bf16 gate (tests/test_kernels_gpu.py), applied per element here
FLOOR = 1e-30             # values below fp32's normal range, where the fast exp flushes to zero
TIE = 2.0 ** -17          # see the module docstring


def rbf(x):
    """Round a float64 tensor through bf16 (round to nearest even, straight from float64)."""
    return x.to(BF16).double()


def _f64(*ts):
    return [t.detach().cpu().double() for t in ts]


def _rbf_alt(v):
    """(rbf(v), the other neighbour where v is within TIE of a bf16 rounding midpoint, else rbf(v))."""
    r = rbf(v)
    f = v.float()                                           # only to find the bf16 neighbours: truncate the fp32 bit pattern
    lo = (f.view(torch.int32) & -65536).view(torch.float32).double()          # towards zero
    hi = ((f.view(torch.int32) & -65536) + 65536).view(torch.float32).double()   # away from zero
    mid = 0.5 * (lo + hi)
    near = (v - mid).abs() <= TIE * v.abs()
    other = torch.where(r == lo, hi, lo)
    return r, torch.where(near & torch.isfinite(hi), other, r)


def ratios(got, ref, A, alt=None):
    """|got - ref| / (TOL * A + FLOOR) per element (float64); with `alt`, the smaller of the two candidates' ratios."""
    got, ref, A = got.detach().cpu().double(), ref.double(), A.double()
    r = (got - ref).abs() / (TOL * A + FLOOR)
    if alt is not None:
        r = torch.minimum(r, (got - alt.double()).abs() / (TOL * A + FLOOR))
    return torch.where(torch.isfinite(got) | (got == ref), r, torch.full_like(r, float("inf")))


def assert_close_elementwise(got, ref, A, what, alt=None):
    """|got - ref| <= 2^-7 A + 1e-30 for EVERY element.  A bf16 store alone costs up to 2^-8 |ref| <= 2^-8 A, so the gate carries a 2x margin.
    Returns the worst ratio err / (2^-7 A + 1e-30) (<= 1); a failure names the worst element."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(A.shape), (what, got.shape, ref.shape, A.shape)
    r = ratios(got, ref, A, alt)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    worst = float(r.max()) if r.numel() else 0.0
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        idx = tuple(int(k) for k in torch.unravel_index(torch.tensor(i), r.shape)) if r.dim() else ()
        g = float(got.detach().cpu().double().reshape(-1)[i])
        msg = (f"{what}: element {idx}: got {g!r}, ref {float(ref.reshape(-1)[i])!r}, A {float(A.reshape(-1)[i])!r}, "
               f"|got-ref| / (2^-7 A + 1e-30) = {worst:.4g}; {int((r > 1.0).sum())} of {r.numel()} elements over the gate")
        print(msg)
        raise AssertionError(msg)
    return worst


def assert_rows_close(got, ref, scale, rel, what):
    """fp32 per-row outputs: |got - ref| <= rel * scale + 1e-30 for every row.  Returns the worst err / (rel * scale + 1e-30)."""
    got, ref, scale = got.detach().cpu().double(), ref.double(), scale.double()
    assert got.shape == ref.shape == scale.shape, (what, got.shape, ref.shape)
    r = (got - ref).abs() / (rel * scale + FLOOR)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    worst = float(r.max())
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        msg = f"{what}: row {i}: got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, err / gate = {worst:.4g}"
        print(msg)
        raise AssertionError(msg)
    return worst


# ------------------------------------------------------------------------------------------------ RMSNorm
def rmsnorm_fwd(x, w, eps):
    """y = w * rbf(x * rstd), rstd = (mean(x^2) + eps)^-1/2.  Returns (y, A, alt, rstd)."""
    x, w = _f64(x, w)
    rstd = torch.rsqrt(x.pow(2).mean(-1) + eps)
    xh, xh_alt = _rbf_alt(x * rstd[:, None])
    return w * xh, w.abs() * xh.abs(), w * xh_alt, rstd


def rmsnorm_bwd(dy, x, w, eps, dx_in=None, dw_in=None):
    """dx = dx_in + rstd (g - xhat mean(g xhat)), g = dy w, xhat = x rstd (not rounded: the backward recomputes it in fp32);
    dw = dw_in + sum_rows dy xhat.  Returns (dx, A_dx, dw, A_dw)."""
    dy, x, w = _f64(dy, x, w)
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh, g = x * rstd, dy * w
    dx = rstd * (g - xh * (g * xh).mean(-1, keepdim=True))
    A = rstd * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    dw, Aw = (dy * xh).sum(0), (dy * xh).abs().sum(0)
    if dx_in is not None:
        dx, A = dx + _f64(dx_in)[0], A + _f64(dx_in)[0].abs()
    if dw_in is not None:
        dw, Aw = dw + _f64(dw_in)[0], Aw + _f64(dw_in)[0].abs()
    return dx, A, dw, Aw


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, w, b, eps):
    """y = (x - mean) rstd w + b.  Returns (y, A, mean, rstd); the saved stats are gated per row (mean against mean|x|, rstd relative)."""
    x, w, b = _f64(x, w, b)
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps)
    y = (x - mean) * rstd * w + b
    A = (x.abs() + mean.abs()) * rstd * w.abs() + b.abs()
    return y, A, mean[:, 0], rstd[:, 0]


def layernorm_bwd(dy, x, w, eps, dx_in=None, dw_in=None, db_in=None):
    """dx = dx_in + rstd (g - mean(g) - xhat mean(g xhat)), g = dy w; dw = sum dy xhat, db = sum dy.
    Returns (dx, A_dx, dw, A_dw, db, A_db)."""
    dy, x, w = _f64(dy, x, w)
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps)
    xh, xa = (x - mean) * rstd, (x.abs() + mean.abs()) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    A = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xa * (g.abs() * xa).mean(-1, keepdim=True))
    dw, Aw = (dy * xh).sum(0), (dy.abs() * xa).sum(0)
    db, Ab = dy.sum(0), dy.abs().sum(0)
    if dx_in is not None:
        dx, A = dx + _f64(dx_in)[0], A + _f64(dx_in)[0].abs()
    if dw_in is not None:
        dw, Aw = dw + _f64(dw_in)[0], Aw + _f64(dw_in)[0].abs()
    if db_in is not None:
        db, Ab = db + _f64(db_in)[0], Ab + _f64(db_in)[0].abs()
    return dx, A, dw, Aw, db, Ab


# ------------------------------------------------------------------------------------------------ RoPE
def rope(x, cos_sin, positions, heads, hd, nsec, direction=1):
    """Half-split rotation of the first nsec * heads * hd columns of x [rows, >=]: (a, b) = (first, second half of a head),
    a' = a cos - b sin dir, b' = b cos + a sin dir, cos/sin = cos_sin[positions[row], i, 0/1] (fp32 table [S, hd/2, 2]).
    Returns (y, A) of the rotated columns only, [rows, nsec * heads * hd]."""
    rows, n = x.shape[0], nsec * heads * hd
    xs = _f64(x)[0][:, :n].reshape(rows, nsec * heads, 2, hd // 2)
    cs = _f64(cos_sin)[0][torch.as_tensor(positions, dtype=torch.int64)]            # [rows, hd/2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1] * (1.0 if direction > 0 else -1.0)
    a, b = xs[:, :, 0], xs[:, :, 1]
    y = torch.stack((a * c - b * s, b * c + a * s), dim=2)
    A = torch.stack(((a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()), dim=2)
    return y.reshape(rows, n), A.reshape(rows, n)


# ------------------------------------------------------------------------------------------------ SwiGLU / GELU
def swiglu_fwd(g, u):
    """act = rbf(silu(g)) * u.  Returns (act, A, alt)."""
    g, u = _f64(g, u)
    s, s_alt = _rbf_alt(g * torch.sigmoid(g))
    return s * u, s.abs() * u.abs(), s_alt * u


def swiglu_bwd(dact, g, u):
    """du = dact silu(g) (not rounded); dg = dact u sg (1 + g (1 - sg)).  Returns (dg, A_dg, du, A_du)."""
    dact, g, u = _f64(dact, g, u)
    sg = torch.sigmoid(g)
    du = dact * g * sg
    dg = dact * u * sg * (1 + g * (1 - sg))
    return dg, (dact * u).abs() * sg * (1 + g.abs() * (1 + sg)), du, du.abs()


def quick_gelu_fwd(x):
    x = _f64(x)[0]
    y = x * torch.sigmoid(1.702 * x)
    return y, y.abs()


def quick_gelu_bwd(dy, x):
    dy, x = _f64(dy, x)
    sg = torch.sigmoid(1.702 * x)
    return dy * sg * (1 + 1.702 * x * (1 - sg)), dy.abs() * sg * (1 + 1.702 * x.abs() * (1 + sg))


def gelu_fwd(x):
    """0.5 x (1 + erf(x / sqrt 2)): for x << 0 a difference of two ones, so A ~ |x| there."""
    x = _f64(x)[0]
    e = torch.erf(x / math.sqrt(2.0))
    return 0.5 * x * (1 + e), 0.5 * x.abs() * (1 + e.abs())


def gelu_bwd(dy, x):
    dy, x = _f64(dy, x)
    e = torch.erf(x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy * (0.5 * (1 + e) + x * pdf), dy.abs() * (0.5 * (1 + e.abs()) + x.abs() * pdf)


_K = math.sqrt(2.0 / math.pi)


def gelu_tanh_fwd(x):
    x = _f64(x)[0]
    t = torch.tanh(_K * (x + 0.044715 * x ** 3))
    return 0.5 * x * (1 + t), 0.5 * x.abs() * (1 + t.abs())


def gelu_tanh_bwd(dy, x):
    dy, x = _f64(dy, x)
    t = torch.tanh(_K * (x + 0.044715 * x ** 3))
    d = 0.5 * x * (1 - t * t) * _K * (1 + 3 * 0.044715 * x * x)
    A = 0.5 * (1 + t.abs()) + 0.5 * x.abs() * (1 + t * t) * _K * (1 + 3 * 0.044715 * x * x)
    return dy * (0.5 * (1 + t) + d), dy.abs() * A


# ------------------------------------------------------------------------------------------------ cross entropy
def cross_entropy(logits, labels, V, inv_count, ignore_index=-100):
    """Rows of logits[:, :V]; a label outside [0, V) (ignore_index) gives loss 0 and a zero gradient row.
    Returns (loss_rows, loss_scale, grad, A): loss_rows = lse - target, gated at 1e-4 * loss_scale with loss_scale = max(1, |lse| + |target|);
    grad = (softmax - onehot) inv_count with A = (softmax + onehot) inv_count, both [rows, V]."""
    z = _f64(logits)[0][:, :V]
    labels = torch.as_tensor(labels, dtype=torch.int64).cpu()
    live = (labels >= 0) & (labels < V) & (labels != ignore_index)
    lab = torch.where(live, labels, torch.zeros_like(labels))
    lse = torch.logsumexp(z, -1)
    target = z.gather(1, lab[:, None])[:, 0]
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(z).scatter_(1, lab[:, None], 1.0)
    lv = live[:, None].double()
    loss = torch.where(live, lse - target, torch.zeros_like(lse))
    scale = torch.where(live, (lse.abs() + target.abs()).clamp_min(1.0), torch.ones_like(lse))
    return loss, scale, (p - onehot) * inv_count * lv, (p + onehot) * abs(inv_count) * lv


# ------------------------------------------------------------------------------------------------ column sums
def colsum(x, out_in=None):
    """sum over rows of x [rows, cols] (+ out_in).  Returns (s, A)."""
    x = _f64(x)[0]
    s, A = x.sum(0), x.abs().sum(0)
    if out_in is not None:
        s, A = s + _f64(out_in)[0], A + _f64(out_in)[0].abs()
    return s, A

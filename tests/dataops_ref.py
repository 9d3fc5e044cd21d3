"""CPU references of the data-movement and optimizer kernels of radvlm_amd/csrc/ops.hip: the dropout mask and its two elementwise consumers,
gather / segment sum / 2x2 max over rows, the CLIP embedding kernels, the image normalisation, the transposes and AdamW.  numpy and torch on
the CPU only; tests/test_dataops_ref_host.py pins every reference to the textbook op (or to the definition it restates) without a GPU, and
tests/test_dataops_edges_gpu.py holds the kernels to them.

Most of these kernels have ONE right answer, bit for bit, and their reference returns it as a bf16 (or uint8) tensor: it redoes the kernel's
own fp32 arithmetic where that is a single correctly rounded operation (a product, a sum, a quotient), in numpy float32.  The two that sum
(segment_sum, adamw_step) are float64 and return, the rowops_ref way, a magnitude tensor A per output: the formula with every term replaced by
its absolute value, against which the error of that element is judged.
"""
import numpy as np
import torch

from rowops_ref import BF16

_GOLD = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the dropout mask
def hash64(seed, b):
    """splitmix64 of (seed, b) as common.h states it: z = b + seed * G + G, two xor-shift-multiply rounds, a final xor-shift.
    `seed` a Python int (taken mod 2^64), `b` a numpy uint64 array."""
    z = b.astype(np.uint64) + np.uint64((int(seed) * _GOLD + _GOLD) & _M64)          # array arithmetic wraps mod 2^64
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def thr16(p):
    """round(p * 2^16) of the fp32 value of p (the C ABI takes p as a float)."""
    return int(float(np.float32(p)) * 65536 + 0.5)


def keep_mask(seed, n, p):
    """bool [n]: element i is kept iff bits [16 (i & 3), +16) of hash64(seed, i >> 2) are >= thr16(p)."""
    i = np.arange(n, dtype=np.uint64)
    h = hash64(seed, i >> np.uint64(2))
    bits = (h >> (np.uint64(16) * (i & np.uint64(3)))) & np.uint64(0xFFFF)
    return bits >= np.uint64(thr16(p))


def _scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def _f32(t):
    return t.detach().cpu().float().reshape(-1).numpy()


def _to_bf16(a32, shape):
    return torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(BF16).reshape(shape)


def dropout(x, p, seed):
    """bf16 tensor of x's shape: bf16(fp32(x) * fp32(1 / (1 - p))) where kept, +0 where dropped.  Bit-exact: one fp32 product, one rounding."""
    keep = keep_mask(seed, x.numel(), p)
    y = np.where(keep, _f32(x) * _scale(p), np.float32(0))
    return _to_bf16(y, x.shape)


def dropout_add(x, y, p, seed):
    """y + dropout(x).  Returns (ref, alt), both bf16: the kernel computes y + x * s in fp32 and the compiler may contract it into one fused
    multiply-add, so a kept position has two candidates -- bf16(fp32(fp32(x s) + y)) and bf16(fp32(x s + y)) (the fused form: x s is exact in
    float64, 8 x 24 bits).  A dropped position is y + 0."""
    keep = keep_mask(seed, x.numel(), p)
    x32, y32, s = _f32(x), _f32(y), _scale(p)
    two = (x32 * s).astype(np.float32) + y32
    fused = (x32.astype(np.float64) * np.float64(s) + y32.astype(np.float64)).astype(np.float32)
    drop = y32 + np.float32(0)
    return _to_bf16(np.where(keep, two, drop), x.shape), _to_bf16(np.where(keep, fused, drop), x.shape)


# ------------------------------------------------------------------------------------------------ rows: gather, segment sum, max of four
def gather_rows(idx, d, table_a, table_b=None):
    """out[r] = table_a[idx[r]] (idx >= 0), a +0 row (idx == -1), table_b[-idx - 2] (idx <= -2); the first d columns of the tables."""
    out = torch.zeros(len(idx), d, dtype=BF16)
    for r, i in enumerate(int(k) for k in idx):
        if i >= 0:
            out[r] = table_a[i, :d]
        elif i <= -2:
            out[r] = table_b[-i - 2, :d]
    return out


def segment_sum(src, seg_off, pos, w=None):
    """Row s = sum over j in [seg_off[s], seg_off[s + 1]) of w[j] * src[pos[j]] (w = 1 when None), in float64 from the bf16 rows and the fp32
    weights.  Returns (sum [nseg, d], A = sum_j |w_j| |src[pos[j]]|, J = the segment lengths [nseg])."""
    src = src.detach().cpu().double()
    seg_off = [int(k) for k in seg_off]
    pos = torch.as_tensor([int(k) for k in pos], dtype=torch.int64)
    wt = torch.ones(len(pos), dtype=torch.float64) if w is None else torch.as_tensor(w).detach().cpu().float().double().reshape(-1)
    nseg, d = len(seg_off) - 1, src.shape[1]
    out, A = torch.zeros(nseg, d, dtype=torch.float64), torch.zeros(nseg, d, dtype=torch.float64)
    for s in range(nseg):
        j0, j1 = seg_off[s], seg_off[s + 1]
        if j1 > j0:
            rows = src[pos[j0:j1]] * wt[j0:j1, None]
            out[s], A[s] = rows.sum(0), rows.abs().sum(0)
    J = torch.tensor([seg_off[s + 1] - seg_off[s] for s in range(nseg)], dtype=torch.int64)
    return out, A, J


def max4_fwd(src, idx4):
    """(out bf16 [n, d], which uint8 [n, d]): the elementwise maximum of the four rows src[idx4[s]] and the slot that holds it, by
    max_pool2d's window scan: slot 0 starts, a later slot takes over when `v > best or isnan(v)` -- the first maximum wins a tie (and
    +0 == -0 is a tie), a NaN wins and is only replaced by a later NaN."""
    idx4 = torch.as_tensor(idx4, dtype=torch.int64).reshape(-1, 4)
    rows = src.detach().cpu()[idx4]                                     # [n, 4, d] bf16
    best, which = rows[:, 0].clone(), torch.zeros(rows[:, 0].shape, dtype=torch.uint8)
    for j in range(1, 4):
        v = rows[:, j]
        take = (v.float() > best.float()) | torch.isnan(v)
        best = torch.where(take, v, best)
        which = torch.where(take, torch.full_like(which, j), which)
    return best, which


def max4_bwd(dout, idx4, dout_row, which, dsrc):
    """A copy of dsrc (bf16 [rows, d]) with row idx4[s][j] = where(which[s] == j, dout[dout_row[s]], +0) for every window s and slot j.  Rows
    in no window keep what dsrc held.  dout may be dsrc itself (the in-place form): the gradients are read before anything is written."""
    idx4 = torch.as_tensor(idx4, dtype=torch.int64).reshape(-1, 4)
    g = dout.detach().cpu()[torch.as_tensor(dout_row, dtype=torch.int64)].clone()
    out = dsrc.detach().cpu().clone()
    which = which.cpu()
    for s in range(idx4.shape[0]):
        for j in range(4):
            out[int(idx4[s, j])] = torch.where(which[s] == j, g[s], torch.zeros_like(g[s]))
    return out


# ------------------------------------------------------------------------------------------------ CLIP embeddings
def add_pos(x, pos, n, P):
    """x [n P, d] + pos [P, d] for every image: one fp32 sum, one rounding."""
    d = x.shape[1]
    return (x.float().view(n, P, d) + pos.float()[None]).to(BF16).view(n * P, d)


def clip_embed(patch_out, cls, pos, n, P):
    """[n (P + 1), d]: row 0 of an image = cls + pos[0], row t = patch_out[img P + t - 1] + pos[t]."""
    d = patch_out.shape[1]
    tok = torch.cat((cls.float().expand(n, 1, d), patch_out.float().view(n, P, d)), dim=1)
    return (tok + pos.float()[None]).to(BF16).view(n * (P + 1), d)


def im2col(pix, p, kp):
    """pix [n, 3, H, W] -> [n (H // p) (W // p), kp]: row (img, gy, gx) holds the patch at (gy p, gx p) in (channel, row, column) order --
    conv2d's weight layout -- then +0 up to kp columns.  Rows and columns of pixels beyond a whole patch are ignored."""
    n, c, H, W = pix.shape
    gh, gw = H // p, W // p
    t = pix[:, :, :gh * p, :gw * p].reshape(n, c, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(n * gh * gw, c * p * p)
    out = torch.zeros(n * gh * gw, kp, dtype=pix.dtype)
    out[:, :c * p * p] = t
    return out


def normalize_tiles(u8, tile, mean, std, mode, factor, gh, gw):
    """uint8 HWC canvases [n, gh tile, gw tile, 3] -> bf16 CHW tiles [n gh gw, 3, tile, tile] in row-major tile order, in the host processors'
    fp32 arithmetic: mode 0 float32(u8) / float32(255), mode 1 float32(float64(u8) * factor); then (v - mean) / std in float32, then bf16."""
    a = np.asarray(u8)
    n = a.shape[0]
    if mode == 0:
        v = a.astype(np.float32) / np.float32(255)
    elif mode == 1:
        v = (a.astype(np.float64) * np.float64(factor)).astype(np.float32)
    else:
        raise ValueError(mode)
    v = ((v - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)).astype(np.float32)
    v = v.reshape(n, gh, tile, gw, tile, 3).transpose(0, 1, 3, 5, 2, 4).reshape(n * gh * gw, 3, tile, tile)
    return torch.from_numpy(np.ascontiguousarray(v)).to(BF16)


# ------------------------------------------------------------------------------------------------ transpose
def perm32_source(r_pad):
    """Position pos of every aligned group of 32 holds index 32 (pos // 32) + 16 ((pos % 8) // 4) + 4 ((pos % 32) // 8) + pos % 4 (the
    MFMA contraction order the attention kernels read; stated in tests/test_kernels_gpu.py::test_transpose)."""
    assert r_pad % 32 == 0
    return torch.tensor([(q // 32) * 32 + 16 * ((q % 8) // 4) + 4 * ((q % 32) // 8) + q % 4 for q in range(r_pad)])


def transpose(x, r_pad, perm32=False, cu=None, B=1, H=1):
    """x: token-major rows [rows, H C] -> [B, H, C, r_pad]: out[b, h, c, r] = x[row of (b, r), h C + c], +0 for r beyond the sample's rows.
    Without cu sample b owns rows [b S, (b + 1) S), S = rows / B; with cu (B + 1 offsets) rows [cu[b], cu[b + 1]), and rows of x after
    cu[B] are never read.  perm32 then reorders the padded r axis by perm32_source.  B = H = 1: the plain [R, C] -> [C, r_pad] transpose."""
    rows, HC = x.shape
    C = HC // H
    out = torch.zeros(B, H, C, r_pad, dtype=x.dtype)
    for b in range(B):
        r0, r1 = (b * (rows // B), (b + 1) * (rows // B)) if cu is None else (int(cu[b]), int(cu[b + 1]))
        if r1 > r0:
            out[b, :, :, :r1 - r0] = x[r0:r1].reshape(r1 - r0, H, C).permute(1, 2, 0)
    return out[..., perm32_source(r_pad)] if perm32 else out


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_step(master, m, v, g, lr, b1, b2, eps, wd, step, gscale=None, abi_fp32=True):
    """One torch.optim.AdamW step in float64 from the fp32 state and the bf16 gradient:
        g' = g gscale;  p = p (1 - lr wd);  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
    with bc = 1 - b^step.  The C ABI takes lr, b1, b2, eps, wd, bc1, bc2 as floats and gscale as an fp32 device scalar, so with abi_fp32 (the
    default) those INPUTS are rounded to fp32 first, as ops.adamw hands them over (bc from the unrounded betas, then rounded): 1 - fp32(0.999)
    is 1.3e-5 away from 0.001, which is the kernel's input and not its error.  abi_fp32=False takes every hyperparameter as given
    (tests/test_dataops_ref_host.py holds that form to torch.optim.AdamW).
    Returns (master, m, v, A_p, A_m, A_v), the magnitudes formed the rowops_ref way (every term of the kernel's formula by its absolute
    value): A_m = b1 |m| + (1 - b1) |g'|, A_v = the new v (all its terms are positive), A_p = |p| + (lr / bc1) A_m / denom.  The step
    carries A_m and not the new |m|: where b1 m and (1 - b1) g' cancel, an fp32 m is good to 2^-24 A_m, which is many ulps of |m|, and the
    step inherits exactly that (one element in a thousand cancels to 1/265 of A_m with ordinary gradients)."""
    f = (lambda x: float(np.float32(x))) if abi_fp32 else float
    bc1, bc2 = f(1.0 - b1 ** step), f(1.0 - b2 ** step)
    lr, b1, b2, eps, wd = f(lr), f(b1), f(b2), f(eps), f(wd)
    gs = 1.0 if gscale is None else f(gscale)
    p0, m0, v0 = (t.detach().cpu().double() for t in (master, m, v))
    gg = g.detach().cpu().double() * gs
    p = p0 * (1.0 - lr * wd)
    m1 = b1 * m0 + (1.0 - b1) * gg
    v1 = b2 * v0 + (1.0 - b2) * gg * gg
    denom = v1.sqrt() / (bc2 ** 0.5) + eps
    upd = (lr / bc1) * m1 / denom
    A_m = b1 * m0.abs() + (1.0 - b1) * gg.abs()
    return p - upd, m1, v1, p0.abs() + (lr / bc1) * A_m / denom, A_m, v1


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound for every element (float64; a non-finite got fails).  Returns the worst |got - ref| / bound (0 where both are 0)."""
    got, ref, bound = got.detach().cpu().double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    worst = float(r.max()) if r.numel() else 0.0
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        msg = (f"{what}: flat element {i}: got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, bound "
               f"{float(bound.reshape(-1)[i])!r}, err / bound = {worst:.4g}; {int((r > 1.0).sum())} of {r.numel()} elements over the gate")
        print(msg)
        raise AssertionError(msg)
    return worst


def ulp_bf16(x):
    """The spacing of bf16 numbers at |x| (float64 tensor): 2^(floor(log2 |x|) - 7), and the smallest normal's spacing below it."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.full_like(e, 2.0), e - 7)

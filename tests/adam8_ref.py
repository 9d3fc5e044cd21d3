"""numpy definition of the 8-bit AdamW state (rv_adam8_quantize_f32, rv_adam8_dequantize_f32, rv_adamw8; radvlm_amd/csrc/adam8.hip).

Block-wise dynamic quantisation after Dettmers et al., "8-bit Optimizers via Block-wise Quantization", restated here and pinned by this
file: a block is 256 consecutive elements of one tensor (the last block may be shorter), one fp32 absmax per block and state, one of
two sorted 256-entry fp32 codebooks (signed for exp_avg, unsigned for exp_avg_sq).

  quantise   s = absmax, or 1 for an all-zero block;  a = fp32(x / s);  mid[i] = fp32((float64(q[i]) + float64(q[i+1])) / 2);
             code = number of midpoints strictly below a.  This midpoint rule is the definition (it is not "nearest code in float64").
  guard      exp_avg_sq only (kind 1): a value > 0 never takes code 0, it takes code 1 -- otherwise a v far below its block's
             maximum dequantises to 0 and the next step divides by eps.
  dequantise x^ = fp32(q[code] * absmax).

Non-finite values are outside the contract.  The committed tables are radvlm_amd/csrc/adam8_codebook.h; codebook() is their provenance.
"""
import numpy as np

BLOCK = 256
SIGNED, UNSIGNED = 0, 1


def codebook(kind):
    """The sorted 256-entry table, from the dynamic-map formula in float64, rounded to fp32."""
    vals = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i if kind == SIGNED else 2 ** (i + 1)
        b = np.linspace(0.1, 1.0, k + 1, dtype=np.float64)
        means = (b[:-1] + b[1:]) / 2.0 * 10.0 ** (i - 6)
        vals += means.tolist()
        if kind == SIGNED:
            vals += (-means).tolist()
    q = np.sort(np.asarray(vals, np.float64)).astype(np.float32)
    assert q.shape == (256,)
    return q


def midpoints(q):
    return ((q[:-1].astype(np.float64) + q[1:].astype(np.float64)) / 2.0).astype(np.float32)


_Q = {k: codebook(k) for k in (SIGNED, UNSIGNED)}
_MID = {k: midpoints(_Q[k]) for k in (SIGNED, UNSIGNED)}


def nblocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def quantize(x, kind, guard=True):
    """fp32 [n] -> (codes uint8 [n], absmax fp32 [nblocks(n)]), blocks counted from the first element."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    n = x.size
    codes = np.empty(n, np.uint8)
    absmax = np.empty(nblocks(n), np.float32)
    for b in range(absmax.size):
        xb = x[b * BLOCK:(b + 1) * BLOCK]
        am = np.float32(np.max(np.abs(xb)) if kind == SIGNED else np.max(xb))
        absmax[b] = am
        s = am if am != 0 else np.float32(1.0)
        a = (xb / s).astype(np.float32)                     # IEEE fp32 division
        c = np.searchsorted(_MID[kind], a, side="left")
        if kind == UNSIGNED and guard:
            c = np.where((xb > 0) & (c == 0), 1, c)
        codes[b * BLOCK:(b + 1) * BLOCK] = c
    return codes, absmax


def dequantize(codes, absmax, kind):
    codes = np.asarray(codes, np.uint8).reshape(-1)
    return (_Q[kind][codes] * np.repeat(np.asarray(absmax, np.float32), BLOCK)[:codes.size]).astype(np.float32)


def roundtrip(x, kind, guard=True):
    return dequantize(*quantize(x, kind, guard), kind)


F32 = np.float32


def _neighbours(x):
    x = np.asarray(x, F32)
    return np.concatenate([np.nextafter(x, F32(-np.inf)), x, np.nextafter(x, F32(np.inf))])


def probe_block(kind, scale):
    """Every midpoint and its two fp32 neighbours, times `scale` (a power of two keeps them exact; 3 does not and need not), cut into
    blocks of 256 that each hold the value `scale` itself so that the block's absmax is `scale`."""
    a = _neighbours(_MID[kind])
    a = a[np.abs(a) <= 1]
    x = (a * F32(scale)).astype(F32)
    blocks = []
    for i in range(0, x.size, 255):
        blocks.append(np.concatenate([[F32(scale)], x[i:i + 255]]))
    return np.concatenate(blocks).astype(F32)


def host_inputs(kind):
    """name -> fp32 vector: the inputs shared by tests/test_adam8_host.py and tests/test_adam8_kernels_gpu.py (insertion-ordered)."""
    r = np.random.RandomState(7 + kind)
    out = {}
    for s, tag in ((1.0, "1"), (3.0, "3"), (2.0 ** -40, "2^-40")):
        out["midpoints_scale_" + tag] = probe_block(kind, s)
    out["all_zero"] = np.zeros(300, F32)
    x = r.randn(257).astype(F32)
    out["n257"] = x if kind == SIGNED else x * x
    if kind == SIGNED:
        y = (0.5 * r.rand(256)).astype(F32)
        y[17] = -2.0                                         # the block's largest |m| is negative
        out["negative_max"] = y
    else:
        z = (r.rand(256) * 3).astype(F32)
        z[5] = 7.0
        z[9] = F32(7.0 * 1e-9)                               # far below the maximum: the guard's case
        z[11] = 0.0
        out["guard"] = z
    return out


def adam_step(p, m, v, g, lr, b1, b2, eps, step):
    """Plain fp32 Adam (no weight decay) on numpy arrays; returns new (p, m, v).  The convergence study's arithmetic, not the kernel's."""
    f = np.float32
    m = (f(b1) * m + f(1 - b1) * g).astype(f)
    v = (f(b2) * v + f(1 - b2) * g * g).astype(f)
    mh = m / f(1 - b1 ** step)
    vh = v / f(1 - b2 ** step)
    return (p - f(lr) * mh / (np.sqrt(vh) + f(eps))).astype(f), m, v


def noisy_quadratic(sigma, bits, guard=True, n=8192, steps=300, lr=1e-2, seed=0):
    """Loss curve of Adam on L(p) = mean(c (p - t)^2 / 2), c = exp(sigma N(0,1)), gradient c (p - t) + 0.1 c xi, with fp32 (bits 32)
    or block-quantised (bits 8) moments.  The draws depend on (sigma, seed) only, so both widths see the same problem and noise."""
    r = np.random.RandomState(seed)
    c = np.exp(sigma * r.randn(n)).astype(np.float32)
    t = r.randn(n).astype(np.float32)
    p = np.zeros(n, np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    losses = []
    for step in range(1, steps + 1):
        g = (c * (p - t) + np.float32(0.1) * c * r.randn(n).astype(np.float32)).astype(np.float32)
        p, m, v = adam_step(p, m, v, g, lr, 0.9, 0.999, 1e-8, step)
        if bits == 8:
            m, v = roundtrip(m, SIGNED), roundtrip(v, UNSIGNED, guard)
        losses.append(float(np.mean(c.astype(np.float64) * (p.astype(np.float64) - t) ** 2) / 2))
    return np.asarray(losses)

"""CPU references and input builders for the decode kernels (radvlm_amd/csrc/gemv.hip, decode.hip, extend.hip).  Plain torch on the CPU, float64
unless a dtype is asked for; nothing here touches a GPU, so tests/test_decode_ref_host.py can show without one that the constructions
meet the exact conditions tests/test_decode_edges_gpu.py asserts of the kernels."""
import math

import torch

BF16 = torch.bfloat16


def bf16_ulp(x):
    """The bf16 ulp of each element's binade (as _bf16_ulp of tests/test_decode_kernels_gpu.py)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


def gemv_ref(x, w, bias=None, residual=None):
    """float64 x[M,K] @ w[N,K]^T (+ bias[N]) (+ residual[M,N])."""
    y = x.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if residual is not None:
        y = y + residual.double()
    return y


def attn_decode_ref(q, K, V, lens, H, Hkv, hd, scale=None, dtype=torch.float64):
    """softmax(scale * q[b,h] K[b]^T) V[b] over the keys [0, lens[b]) of kv head h // (H // Hkv): q [B, H*hd], K and V [B, L, Hkv*hd]
    (the caller decides how they sit in a cache).  Returns [B, H*hd] in `dtype`; a sequence of length 0 gives zeros."""
    B, L = K.shape[0], K.shape[1]
    G = H // Hkv
    scale = 1.0 / math.sqrt(hd) if scale is None else scale
    Q = q.to(dtype).view(B, Hkv, G, hd)
    Kh = K.to(dtype).view(B, L, Hkv, hd)
    Vh = V.to(dtype).view(B, L, Hkv, hd)
    s = torch.einsum("bkgd,bjkd->bkgj", Q, Kh) * scale
    lens = torch.as_tensor(lens, dtype=torch.int64)
    live = torch.arange(L)[None, :] < lens[:, None]                                 # [B, L]
    s = s.masked_fill(~live[:, None, None, :], float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)                         # an empty sequence: exp(-inf - 0) = 0 everywhere
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    # masked V rows are dropped, not multiplied by a zero weight: a stale NaN or inf past lens[b] must not reach the reference either
    Vl = torch.where(live[:, :, None, None], Vh, torch.zeros_like(Vh))
    o = torch.einsum("bkgj,bjkd->bkgd", p, Vl)
    o = torch.where(l > 0, o / l.clamp_min(torch.finfo(dtype).tiny), torch.zeros_like(o))
    return o.reshape(B, H * hd)


def attn_extend_ref(q, K, V, rs, ns, H, Hkv, hd, scale=None, dtype=torch.float64):
    """Causal extend attention: sequence b's ns[b] new query rows (consecutive rows of q [sum(ns), H*hd]) sit at positions rs[b] + i and
    attend to the keys [0, rs[b] + i] of K[b] / V[b] ([B, L, Hkv*hd]).  Returns [sum(ns), H*hd] in `dtype`."""
    out, row = [], 0
    for b, (r, n) in enumerate(zip(rs, ns)):
        for i in range(n):
            out.append(attn_decode_ref(q[row + i:row + i + 1], K[b:b + 1], V[b:b + 1], [r + i + 1], H, Hkv, hd, scale, dtype))
        row += n
    return torch.cat(out)


def integer_operands(M, N, K, seed):
    """bf16 (x [M,K], w [N,K], bias [N], residual [M,N]) with integer entries: x in [-2, 2], w in [-3, 3], bias and residual in [-4, 4].
    Every fp32 partial sum of x @ w^T (+ bias + residual) is an integer of magnitude <= 6 K + 8 <= 12344 for K <= 2056, so it is exact
    in any summation order: an fp32 output must equal the float64 product bit for bit, a bf16 output its one round-to-nearest-even."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (M, K), generator=g).to(BF16)
    w = torch.randint(-3, 4, (N, K), generator=g).to(BF16)
    bias = torch.randint(-4, 5, (N,), generator=g).to(BF16)
    residual = torch.randint(-4, 5, (M, N), generator=g).to(BF16)
    return x, w, bias, residual


def needle_cache(n, hd, Hkv, targets, seed):
    """One sequence whose attention output is known exactly: (q [hd] all 4, K [n, Hkv*hd], V [n, Hkv*hd]), bf16.
    A K row of a kv head holds +-2, exactly hd/2 of each sign in a seeded permutation, so its score against q is exactly 0; a target's K
    row is all 2, score 8 hd * hd^-1/2 (64 at hd 64, 90.5 at hd 128).  The other keys together weigh n e^-64 < 1e-23 against a target's 1,
    far below half an fp32 ulp of the result.  V is random bf16; a target's V row holds integers in [1, 8] (positive only: two targets
    never sum to a zero that would let the e^-64 tail show)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.cat([torch.full((hd // 2,), 2.0), torch.full((hd // 2,), -2.0)])
    perm = torch.rand(n, Hkv, hd, generator=g).argsort(dim=-1)
    K = base[perm]
    V = torch.randn(n, Hkv, hd, generator=g)
    for t in targets:
        K[t] = 2.0
        V[t] = torch.randint(1, 9, (Hkv, hd), generator=g).float()
    q = torch.full((hd,), 4.0)
    return q.to(BF16), K.reshape(n, Hkv * hd).to(BF16), V.reshape(n, Hkv * hd).to(BF16)

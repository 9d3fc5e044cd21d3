"""CPU references and input builders for the decode kernels (radvlm_amd/csrc/gemv.hip, decode.hip, extend.hip).  Plain torch on the CPU, float64
unless a dtype is asked for; nothing here touches a GPU, so tests/test_decode_ref_host.py can show without one that the constructions
meet the exact conditions tests/test_decode_edges_gpu.py and tests/test_attn_extend_edges_gpu.py assert of the kernels."""
import math

import numpy as np
import torch

import attn_ref

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


# ------------------------------------------------------------------------------------------------ extend attention
# One "document" of EXTEND_L positions (no multiple of 64) and the windows (r, n) of new rows the extend tests cut from it: n rows at
# positions r .. r + n - 1 against the keys [0, r + n).  They are the smallest set at which every 64-key stage, chunk (64 / 128 / 256) and
# query-tile (64 / 32 / 16 rows for G = 1 / 2 / >= 3) edge occurs; tests/test_decode_ref_host.py asserts that coverage.
EXTEND_L = 330
EXTEND_CHUNKS = (64, 128, 256)
EXTEND_WINDOWS = ((0, 1), (0, 70), (1, 16), (15, 2), (48, 17), (63, 1), (64, 1), (63, 66), (127, 3), (250, 70), (329, 1),
                  (256, 3), (241, 15))          # the last two: a start on and an end at an edge of every chunk size


def extend_query_tile(G):
    """Query rows per workgroup of the extend kernels (16 * xt_qs(G) of csrc/attn_split.h)."""
    return 16 * (1 if G >= 4 else 4 // G)


def extend_rows_exposed(r, n, G, chunk):
    """Rows of a window that a non-finite K|V row at its LAST suffix key reaches (include/radvlm_hip.h, rv_attn_extend_bf16): the key is
    staged by the workgroups of the last query tile only (tiles of extend_query_tile(G) rows counted from the first new row), and of that
    tile's rows those whose own position lies in the key's chunk merge what the key's workgroup accumulated."""
    QT = extend_query_tile(G)
    last = r + n - 1
    return [i for i in range((n - 1) // QT * QT, n) if (r + i) // chunk == last // chunk]


def stair_windows(windows=EXTEND_WINDOWS):
    """The windows cut to at most 64 rows (staircase_cache's limit): (r, n > 64) becomes (r, 64) and the remainder (r + 64, n - 64)."""
    out = []
    for r, n in windows:
        while n > 64:
            out.append((r, 64))
            r, n = r + 64, n - 64
        out.append((r, n))
    return tuple(out)


def staircase_cache(r, n, L_max, hd, Hkv, seed, stale="decoy"):
    """One extend sequence whose every output row is known exactly: bf16 (q [n, hd] all 4, K, V [L_max, Hkv*hd], want [n, Hkv*hd]).
    Background keys as needle_cache's (+-2, hd/2 of each sign: score exactly 0, random V).  Suffix key r + i is all 4 + 2 i with integers in
    [1, 8] as its V row: its score 4 (4 + 2 i) hd^1/2 lies 8 hd^1/2 >= 64 nats above the previous suffix key's and >= 128 above the
    background, so row i (which sees the keys [0, r + i]) is one-hot on key r + i up to weights < e^-64, far below half an fp32 ulp of an
    entry >= 1: want[i] = V[r + i] to the bit.  n <= 64 keeps every K entry (<= 132) an exact bf16 integer and every dot product
    (<= 4 * 132 * 128) below 2^24.  Positions >= r + n hold what a reused slot may: stale = "decoy": the next step of the staircase (K all
    4 + 2 n, 64 nats above every suffix key) with V all 1000; "nan": NaN; None: background."""
    assert 1 <= n <= 64 and r >= 0 and r + n <= L_max and stale in ("decoy", "nan", None)
    g = torch.Generator().manual_seed(seed)
    base = torch.cat([torch.full((hd // 2,), 2.0), torch.full((hd // 2,), -2.0)])
    K = base[torch.rand(L_max, Hkv, hd, generator=g).argsort(dim=-1)]
    V = torch.randn(L_max, Hkv, hd, generator=g)
    for i in range(n):
        K[r + i] = 4.0 + 2 * i
    V[r:r + n] = torch.randint(1, 9, (n, Hkv, hd), generator=g).float()
    if stale == "decoy":
        K[r + n:], V[r + n:] = 4.0 + 2 * n, 1000.0
    elif stale == "nan":
        K[r + n:], V[r + n:] = float("nan"), float("nan")
    K, V = K.reshape(L_max, Hkv * hd).to(BF16), V.reshape(L_max, Hkv * hd).to(BF16)
    return torch.full((n, hd), 4.0).to(BF16), K, V, V[r:r + n].clone()


def extend_windows(family, L, H, Hkv, hd, windows, seed=0, keep_scores=False):
    """Random-data extend cases cut from one document: q / k / v of L positions from attn_ref.make_inputs(family, ...), ONE float64
    causal reference over the document, and per window (r, n) the query rows [r, r + n), a cache row that holds the document's keys
    [0, r + n) and NaN beyond, and the reference rows.  Extend row i of a window IS row r + i of causal attention over the document, so
    no second reference is needed.  Returns a dict: q [sum n, H hd] bf16; K, V [len(windows), L, Hkv hd] bf16; rs, ns; out, A_out
    [sum n, H hd] float64 (A_out = P |V|, attn_ref's budget of `out`); doc = the document's (q, k, v); with keep_scores, scores2 =
    the document's [H, L, L] scaled scores in exp2 units."""
    q, k, v, dout = attn_ref.make_inputs(family, np.arange(L), H, Hkv, hd, seed)
    ref = attn_ref.reference(q, k, v, dout, 1, L, H, Hkv, hd, causal=True, keep_scores=keep_scores)
    K = torch.full((len(windows), L, Hkv * hd), float("nan"), dtype=BF16)
    V = K.clone()
    rows = []
    for b, (r, n) in enumerate(windows):
        assert n >= 1 and r + n <= L
        K[b, :r + n], V[b, :r + n] = k[:r + n], v[:r + n]
        rows.append(torch.arange(r, r + n))
    rows = torch.cat(rows)
    res = dict(q=q[rows].contiguous(), K=K, V=V, rs=[r for r, _ in windows], ns=[n for _, n in windows], out=ref["out"][rows],
               A_out=ref["A_out"][rows], doc=(q, k, v))
    if keep_scores:
        res["scores2"] = ref["scores2"][0]
    return res

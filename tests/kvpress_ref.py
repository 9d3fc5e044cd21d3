"""numpy restatement of the SnapKV prompt-cache compression rule (include/radvlm_hip.h, rv_kv_votes_f32 / rv_kv_select_i32 /
rv_kv_gather_bf16; radvlm_amd/csrc/kvpress.hip), written from the rule with fp64 sums and plain loops so that it and the kernels check
each other.  One sequence at a time: P prompt rows, the last w the observation window, n = P - w prefix rows before it."""
import numpy as np


def votes(q, k, w, scale):
    """q [P, H, hd], k [P, Hkv, hd] (the post-RoPE rows, any float dtype; read as fp64) -> fp64 [Hkv, n]: vote[g, j] is the sum over
    the H / Hkv query heads h of kv head g and the w window rows t of softmax_j'(scale * q[n + t, h] . k[j', g])[j], row t's softmax
    over its causal keys [0, n + t]."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    P, H, _ = q.shape
    Hkv = k.shape[1]
    G, n = H // Hkv, P - w
    out = np.zeros((Hkv, n), dtype=np.float64)
    for g in range(Hkv):
        for h in range(g * G, (g + 1) * G):
            for t in range(w):
                s = (k[:n + t + 1, g] @ q[n + t, h]) * scale
                p = np.exp(s - s.max())
                out[g] += (p / p.sum())[:n]
    return out


def pool(v, k):
    """pooled[j] = max(v[max(0, j - k // 2) .. min(n - 1, j + k // 2)]): a max, so pooling adds no rounding and no summation order."""
    v = np.asarray(v)
    n, half = v.shape[0], k // 2
    return np.array([v[max(0, j - half):min(n, j + half + 1)].max() for j in range(n)], dtype=v.dtype)


def select(v, N, w, k):
    """The N positions kept of a prompt of P = len(v) + w > N positions with prefix votes v: the N - w prefix positions with the
    largest pooled vote, ties to the lower position (a total order), ascending, then the w window positions."""
    v = np.asarray(v)
    n, m = v.shape[0], N - w
    assert 1 <= m < n and k % 2 == 1
    pooled = pool(v, k)
    order = sorted(range(n), key=lambda j: (-pooled[j], j))
    return np.array(sorted(order[:m]) + list(range(n, n + w)), dtype=np.int64)


def needle(P, w, hd, j_star, seed=0, sigma=0.1, amp=4.0):
    """The needle input for one (q head, kv head): keys N(0, sigma^2), every window query amp * u for a unit vector u, and prefix key
    j_star equal to amp * u.  Returns (q [P, 1, hd], k [P, 1, hd]) in fp32; the prefix rows of q are zeros (they are not window rows)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(hd)
    u /= np.linalg.norm(u)
    k = rng.standard_normal((P, 1, hd)) * sigma
    k[j_star, 0] = amp * u
    q = np.zeros((P, 1, hd))
    q[P - w:, 0] = amp * u
    return q.astype(np.float32), k.astype(np.float32)

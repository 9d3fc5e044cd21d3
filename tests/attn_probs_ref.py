"""float64 reference of rv_attn_decode_probs_f32 (radvlm_amd/csrc/attn_probs.hip) on the bf16 inputs, with its per-element budget.
Plain torch on the CPU; tests/test_attn_probs_kernel_gpu.py and tests/test_output_attentions_gpu.py hold the kernel to it.

    s[b,h,j] = scale * sum_i q[b,h,i] k[b,j,g,i]          p = softmax over j < n,  n = min(kv_len[b], L_max, L_out)

Budget, derived and not tuned, per element:

    |p - p64| <= p64 * (2 E + (n + 16) 2^-24) + 1e-37

E = max_j hd 2^-24 scale sum_i |q_i| |k_ji| is the worst-case fp32 error of an hd-term dot product in any order; it enters once through
the element's own score and once through the normaliser.  (n + 16) 2^-24 covers the n-term fp32 sum in any fixed order plus expf, the
division and the * scale rounding; the floor is what fp32 cannot represent.  Head mean: the same relative budget applied to mean64
(with the largest E of the heads), plus H 2^-24 mean64 for the H-term sum and the division.
"""
import math

import torch

EPS = 2.0 ** -24
FLOOR = 1e-37


def reference(q, cache, kv_len, H, Hkv, hd, L_out, scale=None):
    """q bf16 [B, H*hd]; cache bf16 [B, L_max, >= Hkv*hd] (K of kv head g at columns g*hd); kv_len ints [B].  Returns float64
    (p [B, H, L_out], gate_p, mean [B, L_out], gate_mean); columns at or past a row's key count are 0 with gate 0 (exact)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    q, cache = q.detach().cpu().double(), cache.detach().cpu()
    B, L_max = cache.shape[0], cache.shape[1]
    G = H // Hkv
    p = torch.zeros(B, H, L_out, dtype=torch.float64)
    gp = torch.zeros_like(p)
    mean = torch.zeros(B, L_out, dtype=torch.float64)
    gm = torch.zeros_like(mean)
    for b in range(B):
        n = min(int(kv_len[b]), L_max, L_out)
        if n <= 0:
            continue
        Q = q[b].view(H, hd)
        K = cache[b, :n, :Hkv * hd].double().view(n, Hkv, hd).transpose(0, 1).repeat_interleave(G, 0)       # [H, n, hd]
        s = scale * torch.einsum("hi,hji->hj", Q, K)
        E = hd * EPS * scale * torch.einsum("hi,hji->hj", Q.abs(), K.abs()).max(-1).values                  # [H]
        ph = torch.softmax(s, -1)
        rel = 2 * E + (n + 16) * EPS
        p[b, :, :n] = ph
        gp[b, :, :n] = ph * rel[:, None] + FLOOR
        mean[b, :n] = ph.mean(0)
        gm[b, :n] = mean[b, :n] * (float(rel.max()) + H * EPS) + FLOOR
    return p, gp, mean, gm


def assert_within_budget(got, ref, gate, what=""):
    """|got - ref| <= gate for EVERY element (gate 0: exact); prints and returns the worst ratio to the gate (<= 1)."""
    got, ref, gate = got.detach().cpu().double(), ref.double(), gate.double()
    assert tuple(got.shape) == tuple(ref.shape) == tuple(gate.shape), (what, got.shape, ref.shape, gate.shape)
    err = (got - ref).abs()
    r = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    worst = float(r.max()) if r.numel() else 0.0
    print(f"{what}: worst error / gate = {worst:.4g}")
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        raise AssertionError(f"{what}: flat element {i}: got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, gate "
                             f"{float(gate.reshape(-1)[i])!r}, error / gate = {worst:.4g}; {int((r > 1.0).sum())} of {r.numel()} over")
    return worst

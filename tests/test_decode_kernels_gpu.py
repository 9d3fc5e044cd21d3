"""GPU tests of the decode kernels (radvlm_amd/csrc/gemv.hip, decode.hip): the skinny GEMM, decode attention, the cache append and the row argmax,
each against a CPU fp32 reference or the kernel the prefill path uses."""
import math

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _decode_shapes(name):
    """(label, N, K, has_bias) of the decode products of a geometry: qkv (Qwen2 bias), o_proj, gate|up, down, lm_head."""
    l = GEOMETRIES[name]["lm"]
    d, F, H = l["d"], l["ffn"], l["heads"]
    kvd = l.get("kv_heads", H) * (d // H)
    return [("qkv", d + 2 * kvd, d, bool(l.get("qkv_bias"))), ("o", d, d, False), ("gu", 2 * F, d, False), ("down", d, F, False),
            ("lm_head", l["vocab"], d, False)]


def _bf16_ulp(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


SHAPES = [(g, *s) for g in ("toy", "toy_qwen", "llava15_7b", "llava_ov_qwen2_7b") for s in _decode_shapes(g)]


@pytest.mark.parametrize("geo,label,N,K,has_bias", SHAPES, ids=[f"{s[0]}-{s[1]}" for s in SHAPES])
def test_gemv_matches_fp32_matmul(geo, label, N, K, has_bias):
    _need_gpu()
    from radvlm_amd import ops
    g = torch.Generator().manual_seed(N * 7 + K)
    x = torch.randn(32, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    bias = (torch.randn(N, generator=g) * 0.02).to(BF16) if has_bias else None
    res = torch.randn(32, N, generator=g).to(BF16)
    xd, wd = x.cuda(), w.cuda()
    bd = bias.cuda() if bias is not None else None
    ref0 = x.float() @ w.float().t()
    scale = x.float().abs() @ w.float().abs().t()           # sum |x||w| per output
    out_f32 = label == "lm_head"
    worst = 0.0
    for with_res in ((False,) if out_f32 else (False, True)):
        ref = ref0 + (bias.float() if bias is not None else 0.0) + (res.float() if with_res else 0.0)
        for M in (1, 3, 16, 32):
            y = ops.gemv(xd[:M], wd, bias=bd, residual=res.cuda()[:M] if with_res else None,
                         out_dtype=torch.float32 if out_f32 else BF16).float().cpu()
            r = ref[:M]
            if out_f32:
                err = (y - r).abs() / scale[:M].clamp_min(1e-30)
                assert float(err.max()) <= 1e-5, (M, float(err.max()))
            else:
                # within one bf16 ulp of the fp32 result (plus the fp32 accumulation error of a K-long sum where the result cancels)
                bound = _bf16_ulp(r) + 1e-5 * scale[:M]
                over = (y - r).abs() - bound
                worst = max(worst, float(((y - r).abs() / _bf16_ulp(r)).max()))
                assert float(over.max()) <= 0, (M, with_res, float(over.max()))
    from conftest import record_measurement
    record_measurement("gemv_bf16", geo=geo, shape=label, N=N, K=K, split=ops.gemv_split(N, K), max_err_in_ulps=worst)


@pytest.mark.parametrize("geo", ["toy_qwen", "llava15_7b", "llava_ov_qwen2_7b"])
def test_gemv_row_bit_identical_for_every_m(geo):
    _need_gpu()
    from radvlm_amd import ops
    for label, N, K, has_bias in _decode_shapes(geo):
        g = torch.Generator().manual_seed(N + K)
        x = torch.randn(32, K, generator=g).to(BF16).cuda()
        w = (torch.randn(N, K, generator=g) * 0.02).to(BF16).cuda()
        b = (torch.randn(N, generator=g) * 0.02).to(BF16).cuda() if has_bias else None
        dt = torch.float32 if label == "lm_head" else BF16
        y32 = ops.gemv(x, w, bias=b, out_dtype=dt)
        for r in (0, 5, 16, 31):
            y1 = ops.gemv(x[r:r + 1].contiguous(), w, bias=b, out_dtype=dt)
            assert torch.equal(y1[0], y32[r]), (label, r)


def _attn_ref(q, cache, lens, H, Hkv, hd):
    """fp32 softmax(q K^T / sqrt(hd)) V per (sequence, head) on the CPU."""
    B = q.shape[0]
    G = H // Hkv
    kvd = Hkv * hd
    out = torch.zeros(B, H * hd)
    for b in range(B):
        n = int(lens[b])
        K = cache[b, :n, :kvd].float().view(n, Hkv, hd)
        V = cache[b, :n, kvd:].float().view(n, Hkv, hd)
        for h in range(H):
            s = (K[:, h // G] @ q[b, h * hd:(h + 1) * hd].float()) / math.sqrt(hd)
            p = torch.softmax(s, 0)
            out[b, h * hd:(h + 1) * hd] = p @ V[:, h // G]
    return out


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 7])
def test_attn_decode_matches_fp32_softmax(hd, G):
    _need_gpu()
    from radvlm_amd import ops
    Hkv = 2
    H = G * Hkv
    lens = [1, 63, 64, 65, 1000, 8192]
    B, L_max = len(lens), 8192
    g = torch.Generator().manual_seed(hd * 10 + G)
    cache = torch.randn(B, L_max, 2 * Hkv * hd, generator=g).to(BF16)
    q = torch.randn(B, H * hd, generator=g).to(BF16)
    kv_len = torch.tensor(lens, dtype=torch.int32)
    got = ops.attn_decode(q.cuda(), cache.cuda(), kv_len.cuda(), H, Hkv, hd, Hkv * hd).float().cpu()
    ref = _attn_ref(q, cache, lens, H, Hkv, hd)
    for b in range(B):
        err = float((got[b] - ref[b]).abs().max() / ref[b].abs().max())
        assert err <= 4e-3, (lens[b], err)
    from conftest import record_measurement
    record_measurement("attn_decode", hd=hd, G=G, rel_inf=float((got - ref).abs().max() / ref.abs().max()))


@pytest.mark.parametrize("G", [1, 7])
def test_attn_decode_matches_prefill_kernel_last_row(G):
    """The decode kernel on a sequence's cache = the last query row of rv_attn_fwd_nat (the prefill's causal attention) on the same K/V."""
    _need_gpu()
    from radvlm_amd import ops
    hd, Hkv = 128, 2
    H = G * Hkv
    kvd = Hkv * hd
    for S in (65, 1000):
        g = torch.Generator().manual_seed(S + G)
        qkv = torch.randn(S, H * hd + 2 * kvd, generator=g).to(BF16).cuda()
        q, k, v = qkv[:, :H * hd], qkv[:, H * hd:H * hd + kvd], qkv[:, H * hd + kvd:]
        full, _ = ops.attn_fwd(q, k, None, 1, S, H, hd, ((S + 63) // 64) * 64, causal=True, kv_heads=Hkv, v=v)
        cache = qkv[:, H * hd:].contiguous().view(1, S, 2 * kvd)
        got = ops.attn_decode(q[S - 1:].contiguous(), cache, torch.tensor([S], dtype=torch.int32, device="cuda"), H, Hkv, hd, kvd)
        nat = full[S - 1:].float().cpu()
        ref = _attn_ref(q[S - 1:].cpu(), cache.cpu(), [S], H, Hkv, hd)        # fp32
        # the prefill kernel rounds P to bf16 for its P.V MFMAs: it sits its own distance away from fp32, which the bound adds
        nat_err = float((nat - ref).abs().max() / ref.abs().max())
        err = float((got.float().cpu() - nat).abs().max() / ref.abs().max())
        from conftest import record_measurement
        record_measurement("attn_decode_vs_fwd_nat", S=S, G=G, rel_inf=err, fwd_nat_vs_fp32=nat_err)
        assert err <= 4e-3 + nat_err, (S, err, nat_err)


@pytest.mark.parametrize("name", ["toy", "toy_qwen"])
def test_append_rope_equals_prefill_row(name):
    """RoPE at position p (rv_rope_inplace_pos) + the cache append of one q|k|v row = row p of the prefill's fused q|k|v + RoPE GEMM."""
    _need_gpu()
    from radvlm_amd import ops
    l = GEOMETRIES[name]["lm"]
    d, H = l["d"], l["heads"]
    Hkv = l.get("kv_heads", H)
    hd = d // H
    kvd = Hkv * hd
    S = 300
    g = torch.Generator().manual_seed(3)
    h = torch.randn(S, d, generator=g).to(BF16).cuda()
    w = (torch.randn(d + 2 * kvd, d, generator=g) * 0.05).to(BF16).cuda()
    cs = ops.rope_table(S, hd, l.get("rope_theta", 10000.0), "cuda")
    pos = torch.arange(S, dtype=torch.int32, device="cuda")
    fused = ops.gemm_rope(h, w, cs, S, H + Hkv, hd, positions=pos)
    plain = ops.gemm_nt(h, w)
    cache = torch.zeros(1, S, 2 * kvd, dtype=BF16, device="cuda")
    for p in (0, 1, 77, S - 1):
        row = plain[p:p + 1].clone()
        pp = torch.tensor([p], dtype=torch.int32, device="cuda")
        ops.rope_inplace(row, cs, 1, H + Hkv, hd, 1, 1, positions=pp)
        ops.kv_append(row[:, d:], cache, pp)
        assert torch.equal(cache[0, p], fused[p, d:]), p
        assert torch.equal(row[0, :d], fused[p, :d]), p


def test_argmax_rows_matches_torch():
    _need_gpu()
    from radvlm_amd import ops
    g = torch.Generator().manual_seed(0)
    n, phys = 1000, 1008
    x = torch.randn(9, phys, generator=g)
    x[0, 5] = x[0, 900] = 50.0                   # tie: the lower index wins
    x[1, :n] = 1.0                               # all equal: index 0
    x[2, 1003] = 1e9                             # the maximum sits in a pad column: ignored
    x[3, n - 1] = 60.0                           # the last logical column
    x[4, :] = -float("inf")
    x[4, 17] = -1e30
    x[5, 300] = x[5, 200] = x[5, 999] = 70.0
    got = ops.argmax_rows(x.cuda(), n).cpu()
    ref = torch.argmax(x[:, :n], dim=1)
    assert torch.equal(got, ref), (got, ref)
    assert int(got[0]) == 5 and int(got[2]) != 1003 and int(got[5]) == 200
    big = torch.randn(32, 152064, generator=g)
    big[7, 151000] = big[7, 3] = big[7].max() + 1
    assert torch.equal(ops.argmax_rows(big.cuda(), 152064).cpu(), torch.argmax(big, dim=1))

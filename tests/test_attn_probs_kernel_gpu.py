"""GPU tests of rv_attn_decode_probs_f32 (radvlm_amd/csrc/attn_probs.hip) through ops.attn_decode_probs: every element of the per-head
probabilities and of their head mean against the float64 reference within its derived budget (tests/attn_probs_ref.py), the exact
properties (zeros past a row's keys, untouched columns past L_out, NaN-filled cache tails and guards that never leak, a row alone = the
row in a batch, two L_out values, strided operands, rows that sum to 1), consistency with the attention the model really runs
(ops.attn_decode), and the argument refusals."""
import functools
import math

import numpy as np
import pytest
import torch

import attn_probs_ref as R
import attn_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
HEADS = ((4, 4), (8, 2), (7, 1))
B = 3
CASES = [(hd, H, Hkv, L_max) for hd in (64, 128) for H, Hkv in HEADS for L_max in (130, 515)]
IDS = [f"hd{hd}-H{H}kv{Hkv}-L{L}" for hd, H, Hkv, L in CASES]


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _nan(shape, dtype):
    """A buffer of one NaN bit pattern: a kernel cannot produce it by accident, and a read of it poisons the result."""
    if dtype == BF16:
        return torch.full(shape, 0x7fc5, dtype=torch.int16, device="cuda").view(BF16)
    return torch.full(shape, 0x7fc5a5a5, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _kv_len(L_max):
    return (1, 129, L_max)


@functools.lru_cache(maxsize=None)
def _case(hd, H, Hkv, L_max, family):
    """CPU operands and the float64 reference of one case, computed once: q [B, H hd], cache [B, L_max, 2 Hkv hd] (K | V) with every
    position filled (the device copy gets NaN past kv_len), kv_len, and reference() at L_out = L_max."""
    pos = np.tile(np.arange(L_max), B)
    q, k, v, _ = attn_ref.make_inputs(family, pos, H, Hkv, hd, seed=hd + H)
    q = q.view(B, L_max, -1)[:, 7].contiguous()
    cache = torch.cat([k.view(B, L_max, -1), v.view(B, L_max, -1)], -1).contiguous()
    kv_len = _kv_len(L_max)
    return dict(q=q, cache=cache, kv_len=kv_len, ref=R.reference(q, cache, kv_len, H, Hkv, hd, L_max))


def _device(c, guard=2):
    """The case on the device inside NaN guards: q and cache are the middle rows of larger NaN buffers, and the cache rows at or past
    kv_len[b] are NaN too.  Returns (q, cache, kv_len int32)."""
    q, cache = c["q"], c["cache"]
    qb = _nan((B + 2 * guard, q.shape[1]), BF16)
    qb[guard:guard + B] = q.cuda()
    cb = _nan((B + 2 * guard,) + tuple(cache.shape[1:]), BF16)
    for b, n in enumerate(c["kv_len"]):
        cb[guard + b, :n] = cache[b, :n].cuda()
    return qb[guard:guard + B], cb[guard:guard + B], torch.tensor(c["kv_len"], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("family", ["rand", "big"])
@pytest.mark.parametrize("hd,H,Hkv,L_max", CASES, ids=IDS)
def test_every_element_within_budget(hd, H, Hkv, L_max, family):
    ops = _ops()
    c = _case(hd, H, Hkv, L_max, family)
    p64, gp, m64, gm = c["ref"]
    q, cache, kv_len = _device(c)
    probs, mean = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max, per_head=True, mean=True)
    assert probs.dtype == mean.dtype == torch.float32 and tuple(probs.shape) == (B, H, L_max) and tuple(mean.shape) == (B, L_max)
    what = f"hd {hd} H {H} Hkv {Hkv} L_max {L_max} {family}"
    R.assert_within_budget(probs, p64, gp, what + " probs")
    R.assert_within_budget(mean, m64, gm, what + " mean")
    # the two outputs asked for alone are the bits of the joint call
    assert torch.equal(_bits(ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max)[0]), _bits(probs))
    only = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max, per_head=False, mean=True)
    assert only[0] is None and torch.equal(_bits(only[1]), _bits(mean))
    pc = probs.cpu()
    for b, n in enumerate(c["kv_len"]):
        assert not bool(pc[b, :, n:].any()) and not bool(mean[b, n:].any())                      # exactly +0.0 or -0.0 ...
        assert torch.equal(_bits(probs[b, :, n:]), torch.zeros(H, L_max - n, dtype=torch.int32))  # ... and +0.0f at that
        assert torch.equal(_bits(mean[b, n:]), torch.zeros(L_max - n, dtype=torch.int32))
        assert float((pc[b, :, :n].double().sum(-1) - 1).abs().max()) <= (n + 16) * 2.0 ** -24


@pytest.mark.parametrize("hd,H,Hkv,L_max", CASES, ids=IDS)
def test_exact_properties(hd, H, Hkv, L_max):
    ops = _ops()
    c = _case(hd, H, Hkv, L_max, "big")
    q, cache, kv_len = _device(c)
    probs, mean = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max, per_head=True, mean=True)
    # row b alone (its own B = 1 cache) equals row b of the batch
    for b in range(B):
        p1, m1 = ops.attn_decode_probs(q[b:b + 1], cache[b:b + 1], kv_len[b:b + 1], H, Hkv, hd, L_max, per_head=True, mean=True)
        assert torch.equal(_bits(p1[0]), _bits(probs[b])) and torch.equal(_bits(m1[0]), _bits(mean[b])), b
    # a smaller L_out: the rows whose keys all lie below it keep their bits in the common columns; wider outputs keep their sentinel
    # past L_out, and the guard rows around them stay as they were
    L2, pad, guard = 129, 5, 1
    ob = _nan((B + 2 * guard, H, L2 + pad), torch.float32)
    mb = _nan((B + 2 * guard, L2 + pad), torch.float32)
    ob0, mb0 = _bits(ob), _bits(mb)
    p2, m2 = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L2, out=ob[guard:guard + B], mean_out=mb[guard:guard + B])
    assert tuple(p2.shape) == (B, H, L2) and tuple(m2.shape) == (B, L2)
    for b, n in enumerate(c["kv_len"]):
        if n <= L2:
            assert torch.equal(_bits(p2[b]), _bits(probs[b, :, :L2])) and torch.equal(_bits(m2[b]), _bits(mean[b, :L2])), b
    ob1, mb1 = _bits(ob), _bits(mb)
    assert torch.equal(ob1[guard:guard + B, :, L2:], ob0[guard:guard + B, :, L2:]) and torch.equal(mb1[guard:guard + B, L2:], mb0[guard:guard + B, L2:])
    for g in (slice(0, guard), slice(guard + B, None)):
        assert torch.equal(ob1[g], ob0[g]) and torch.equal(mb1[g], mb0[g])
    assert not bool(torch.isnan(p2).any()) and not bool(torch.isnan(m2).any())
    # strided q, cache and outputs give the bits of the contiguous call
    qs = _nan((B, q.shape[1] + 24), BF16)
    qs[:, 8:8 + q.shape[1]] = q
    width = cache.shape[2]
    cs = _nan((B, L_max + 2, width + 16), BF16)
    cs[:, :L_max, 8:8 + width] = cache
    os_ = _nan((B, H, L_max + 3), torch.float32)
    ms = _nan((B, L_max + 9), torch.float32)
    p3, m3 = ops.attn_decode_probs(qs[:, 8:8 + q.shape[1]], cs[:, :L_max, 8:8 + width], kv_len, H, Hkv, hd, L_max, out=os_, mean_out=ms)
    assert torch.equal(_bits(p3), _bits(probs)) and torch.equal(_bits(m3), _bits(mean))
    assert bool(torch.isnan(os_[:, :, L_max:]).all()) and bool(torch.isnan(ms[:, L_max:]).all())
    # kv_len <= 0: an all-zero row; kv_len above L_max is clamped to it
    kv = torch.tensor([0, -3, L_max + 1000], dtype=torch.int32, device="cuda")
    full = cache.clone()
    full[2] = c["cache"][2].cuda()
    p4, m4 = ops.attn_decode_probs(q, full, kv, H, Hkv, hd, L_max, per_head=True, mean=True)
    assert not bool(_bits(p4[:2]).any()) and not bool(_bits(m4[:2]).any())
    assert torch.equal(_bits(p4[2]), _bits(probs[2])) and torch.equal(_bits(m4[2]), _bits(mean[2]))


@pytest.mark.parametrize("family", ["rand", "big"])
@pytest.mark.parametrize("hd,H,Hkv,L_max", CASES, ids=IDS)
def test_consistent_with_the_decode_attention(hd, H, Hkv, L_max, family):
    """sum_j p[b,h,j] V[j] in float64 against ops.attn_decode's bf16 output: one bf16 rounding of A_out = sum_j p |V| (attn_ref.gate) plus
    what the p budget can move the sum by."""
    ops = _ops()
    c = _case(hd, H, Hkv, L_max, family)
    p64, gp, _, _ = c["ref"]
    q, cache, kv_len = _device(c)
    kvd, G = Hkv * hd, H // Hkv
    probs = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max)[0].cpu().double()
    out = ops.attn_decode(q.contiguous(), cache.contiguous(), kv_len, H, Hkv, hd, kvd).cpu().double().view(B, H, hd)
    worst = 0.0
    for b, n in enumerate(c["kv_len"]):
        V = c["cache"][b, :n, kvd:].double().view(n, Hkv, hd).transpose(0, 1).repeat_interleave(G, 0)          # [H, n, hd]
        pv = torch.einsum("hj,hjd->hd", probs[b, :, :n], V)
        A = torch.einsum("hj,hjd->hd", p64[b, :, :n], V.abs())
        gate = attn_ref.gate(A, roundings=1) + torch.einsum("hj,hjd->hd", gp[b, :, :n], V.abs())
        r = ((pv - out[b]).abs() / gate).max()
        worst = max(worst, float(r))
    print(f"hd {hd} H {H} Hkv {Hkv} L_max {L_max} {family}: worst |sum p V - attn_decode| / gate = {worst:.4g}")
    assert worst <= 1.0


def test_refusals_and_a_good_call_after_them():
    ops = _ops()
    from radvlm_amd import lib
    hd, H, Hkv, L_max = 64, 4, 4, 130
    c = _case(hd, H, Hkv, L_max, "rand")
    q, cache, kv_len = _device(c)
    q, cache = q.contiguous(), cache.contiguous()
    width = cache.shape[2]
    qw = torch.zeros(B, 9 * hd, dtype=BF16, device="cuda")                 # wide enough for the head counts refused below, as are probs and ws
    probs = torch.empty(B * 9 * L_max, dtype=torch.float32, device="cuda")[:B * H * L_max].view(B, H, L_max)
    mean = torch.empty(B, L_max, dtype=torch.float32, device="cuda")
    ws_bytes = lib.load().rv_attn_decode_probs_ws_bytes(B, H, L_max)
    assert ws_bytes == (B * H * L_max + 2 * B * H) * 4 and lib.load().rv_attn_decode_probs_ws_bytes(B, 9, L_max) > ws_bytes
    ws = torch.empty(lib.load().rv_attn_decode_probs_ws_bytes(B, 9, L_max) // 4, dtype=torch.float32, device="cuda")
    good = dict(q=q, ld_q=q.stride(0), cache=cache, ld_c=width, bs_c=L_max * width, kv_len=kv_len, L_max=L_max, L_out=L_max, probs=probs,
                ld_p=L_max, mean=mean, ld_m=L_max, ws=ws, ws_bytes=ws.numel() * 4, B=B, H=H, Hkv=Hkv, hd=hd, scale=0.125)

    def call(**kw):
        lib.call("rv_attn_decode_probs_f32", *{**good, **kw}.values())

    wide = dict(q=qw, ld_q=qw.stride(0))
    bad = [dict(hd=96), dict(hd=32), dict(H=6, Hkv=4, **wide), dict(H=9, Hkv=1, **wide), dict(Hkv=0), dict(B=0), dict(q=None), dict(cache=None), dict(kv_len=None),
           dict(ws=None), dict(probs=None, mean=None), dict(ws_bytes=ws_bytes - 4), dict(ld_q=q.stride(0) + 4), dict(ld_q=H * hd - 8),
           dict(ld_c=width + 4), dict(bs_c=L_max * width + 4), dict(bs_c=L_max * width - 8), dict(ld_c=hd * Hkv - 8), dict(L_out=L_max + 1),
           dict(L_out=0), dict(ld_p=L_max - 1), dict(ld_m=L_max - 1), dict(L_max=0)]
    for kw in bad:
        with pytest.raises(lib.RadvlmHipError, match="code -1"):
            call(**kw)
    probs.fill_(float("nan")), mean.fill_(float("nan"))
    call()
    want_p, want_m = ops.attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_max, per_head=True, mean=True, scale=0.125)
    assert torch.equal(_bits(probs), _bits(want_p)) and torch.equal(_bits(mean), _bits(want_m))
    call(mean=None)
    call(probs=None)
    torch.cuda.synchronize()

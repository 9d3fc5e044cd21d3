"""GPU tests of the int8 KV cache kernels (radvlm_amd/csrc/kvq.hip): the quantising cache writes bit-exact against the numpy
restatement (tests/kv8_ref.py), and rv_attn_decode_kv8_bf16 bit-identical to rv_attn_decode_bf16 on the dequantised cache.  Every
comparison is exact."""
import math

import numpy as np
import pytest
import torch

import kv8_ref
import w8_ref
from radvlm_amd import portable_rng

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SHAPES = [(2, 2, 128), (7, 1, 128), (4, 2, 64), (8, 1, 64)]               # (H, Hkv, hd): G = 1, 7, 2, 8 at both head sizes
IDS = [f"H{h}_Hkv{k}_hd{d}" for h, k, d in SHAPES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32_bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _kv_source(M, Hkv, hd, seed):
    """M K|V rows as fp32 (exactly bf16-representable after the cast): every (row, head, K / V) group is scaled by its own power of two
    in 2^-3 .. 2^3, so a scale read from the wrong group shows; group (0, 0) is zeros and group (M - 1, last)'s maximum sits in its last
    element."""
    G2 = 2 * Hkv
    x = portable_rng.normal(seed, portable_rng.name_tag(f"kv8_{M}_{Hkv}_{hd}"), (M, G2, hd), 1.0)
    e = portable_rng.integers(seed + 1, M * 1000 + G2, (M, G2), -3, 4).astype(np.float32)
    x = x * np.exp2(e)[:, :, None]
    x[0, 0] = 0.0
    x[M - 1, G2 - 1, hd - 1] = 100.0
    return x.reshape(M, G2 * hd).astype(np.float32)


# ------------------------------------------------------------------------------------------------ quantise / append
@pytest.mark.parametrize("H,Hkv,hd", SHAPES, ids=IDS)
@pytest.mark.parametrize("M", [1, 5, 37])
def test_quantize_rows_bit_exact(H, Hkv, hd, M):
    _need_gpu()
    from radvlm_amd import ops
    width, d = 2 * Hkv * hd, H * hd
    B, L_max = 3, 20                                                        # 60 flat rows, guard rows around each cache
    wide = torch.zeros(M, d + width + 8, dtype=BF16, device="cuda")
    wide[:, :d] = 9.0
    wide[:, d:d + width] = torch.from_numpy(_kv_source(M, Hkv, hd, 21)).to(BF16)
    src = wide[:, d:d + width]                                              # the k|v columns of a wider product
    assert src.stride(0) == d + width + 8 and src.storage_offset() == d    # a strided column view (a single row is trivially contiguous)
    perm = portable_rng.integers(5, M, (B * L_max,), 0, 1 << 30).argsort()[:M].astype(np.int64)      # distinct rows, out of order
    rows = perm.copy()
    skipped = None
    if M > 1:
        skipped = M // 2
        rows[skipped] = B * L_max + 3 if M == 5 else -1                    # one row index outside the cache
    q8g = torch.full((B + 2, L_max, width), 77, dtype=torch.int8, device="cuda")
    sg = torch.full((B + 2, L_max, 2 * Hkv), -3.0, dtype=torch.float32, device="cuda")
    xg = torch.full((B + 2, L_max, width), -5.0, dtype=BF16, device="cuda")
    q8, s, xh = q8g[1:B + 1], sg[1:B + 1], xg[1:B + 1]
    ops.kv_quantize_rows(src, torch.from_numpy(rows).cuda(), Hkv, hd, cache=(q8, s), xhat=xh)
    torch.cuda.synchronize()
    rq, rs, rx = kv8_ref.quantize_kv_rows(_bits(src), Hkv, hd)
    want_q = np.full((B * L_max, width), 77, np.int8)
    want_s = np.full((B * L_max, 2 * Hkv), -3.0, np.float32)
    want_x = np.full((B * L_max, width), _bits(torch.tensor([-5.0], dtype=BF16))[0], np.uint16)
    for m in range(M):
        if m != skipped:
            want_q[rows[m]], want_s[rows[m]], want_x[rows[m]] = rq[m], rs[m], rx[m]
    assert np.array_equal(q8.cpu().numpy().reshape(-1, width), want_q)
    assert np.array_equal(_f32_bits(s).reshape(-1, 2 * Hkv), want_s.view(np.uint32))
    assert np.array_equal(_bits(xh).reshape(-1, width), want_x)
    for t, v in ((q8g, 77), (sg, -3.0), (xg, -5.0)):                        # the guard rows keep the sentinel
        assert bool((t[0] == v).all()) and bool((t[B + 1] == v).all())
    assert bool((wide[:, :d] == 9.0).all()) and bool((wide[:, d + width:] == 0.0).all())
    assert rs[0, 0] == np.float32(1.0) and not rq[0, :hd].any()            # the zero group
    assert rq[M - 1, width - 1] == 127                                      # the group whose maximum is its last element
    # either output alone gives the same bits
    q2, s2, x2 = torch.zeros_like(q8), torch.zeros_like(s), torch.zeros_like(xh)
    ok = torch.from_numpy(np.delete(rows, skipped) if skipped is not None else rows).cuda()
    src_ok = src[torch.from_numpy(np.delete(np.arange(M), skipped) if skipped is not None else np.arange(M)).cuda()]
    ops.kv_quantize_rows(src_ok, ok, Hkv, hd, cache=(q2, s2))
    ops.kv_quantize_rows(src_ok, ok, Hkv, hd, xhat=x2)
    sel = ok.cpu().numpy()
    assert np.array_equal(q2.cpu().numpy().reshape(-1, width)[sel], want_q[sel])
    assert np.array_equal(_f32_bits(s2).reshape(-1, 2 * Hkv)[sel], want_s.view(np.uint32)[sel])
    assert np.array_equal(_bits(x2).reshape(-1, width)[sel], want_x[sel])


@pytest.mark.parametrize("H,Hkv,hd", SHAPES, ids=IDS)
def test_append_q8_bit_exact(H, Hkv, hd):
    _need_gpu()
    from radvlm_amd import ops
    width, d = 2 * Hkv * hd, H * hd
    B, L_max = 5, 9
    wide = torch.zeros(B, d + width, dtype=BF16, device="cuda")
    wide[:, d:] = torch.from_numpy(_kv_source(B, Hkv, hd, 33)).to(BF16)
    src = wide[:, d:]
    pos = np.array([0, 8, 3, 9, -1], dtype=np.int32)                        # rows 3 and 4 lie outside the cache: skipped
    q8g = torch.full((B + 2, L_max, width), 77, dtype=torch.int8, device="cuda")
    sg = torch.full((B + 2, L_max, 2 * Hkv), -3.0, dtype=torch.float32, device="cuda")
    xg = torch.full((B + 2, L_max, width), -5.0, dtype=BF16, device="cuda")
    q8, s, xh = q8g[1:B + 1], sg[1:B + 1], xg[1:B + 1]
    ops.kv_append_q8(src, torch.from_numpy(pos).cuda(), Hkv, hd, cache=(q8, s), xhat=xh)
    torch.cuda.synchronize()
    rq, rs, rx = kv8_ref.quantize_kv_rows(_bits(src), Hkv, hd)
    want_q = np.full((B, L_max, width), 77, np.int8)
    want_s = np.full((B, L_max, 2 * Hkv), -3.0, np.float32)
    want_x = np.full((B, L_max, width), _bits(torch.tensor([-5.0], dtype=BF16))[0], np.uint16)
    for b in range(3):
        want_q[b, pos[b]], want_s[b, pos[b]], want_x[b, pos[b]] = rq[b], rs[b], rx[b]
    assert np.array_equal(q8.cpu().numpy(), want_q)
    assert np.array_equal(_f32_bits(s), want_s.view(np.uint32))
    assert np.array_equal(_bits(xh), want_x)
    for t, v in ((q8g, 77), (sg, -3.0), (xg, -5.0)):
        assert bool((t[0] == v).all()) and bool((t[B + 1] == v).all())


# ------------------------------------------------------------------------------------------------ attention
def _attn_case(H, Hkv, hd, B, L_max, seed):
    """A quantised cache made by the kernel from per-group scaled rows, its dequantised bf16 twin built with plain torch from the public
    layout, and one query row per sequence."""
    from radvlm_amd import ops
    width = 2 * Hkv * hd
    src = torch.from_numpy(_kv_source(B * L_max, Hkv, hd, seed)).to(BF16).cuda()
    q8 = torch.zeros(B, L_max, width, dtype=torch.int8, device="cuda")
    s = torch.ones(B, L_max, 2 * Hkv, dtype=torch.float32, device="cuda")
    ops.kv_quantize_rows(src, torch.arange(B * L_max, dtype=torch.int64, device="cuda"), Hkv, hd, cache=(q8, s))
    deq = (q8.float() * s.repeat_interleave(hd, -1)).to(BF16)
    q = torch.from_numpy(portable_rng.normal(seed + 7, 3, (B, H * hd), 1.0)).to(BF16).cuda()
    return q, q8, s, deq


@pytest.mark.parametrize("H,Hkv,hd", SHAPES, ids=IDS)
@pytest.mark.parametrize("L_max,chunk,lens", [(260, 128, [1, 128, 129, 260]), (300, 512, [0, 300])], ids=["chunk128", "chunk512"])
def test_attn_decode_kv8_bit_identical_to_bf16_on_dequantised(H, Hkv, hd, L_max, chunk, lens):
    _need_gpu()
    from radvlm_amd import ops
    B, kvd = len(lens), Hkv * hd
    q, q8, s, deq = _attn_case(H, Hkv, hd, B, L_max, 41)
    kv_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    want = ops.attn_decode(q, deq, kv_len, H, Hkv, hd, kvd, chunk=chunk)
    got = ops.attn_decode_kv8(q, (q8, s), kv_len, H, Hkv, hd, kvd, chunk=chunk)
    assert got.dtype == BF16 and torch.equal(got, want)
    assert bool(torch.isfinite(got.float()).all()) and bool((got[kv_len > 0].float().abs().sum(1) > 0).all())
    if 0 in lens:
        assert not bool(got[lens.index(0)].any())                          # the zero-length row gives zeros
    # garbage at and past kv_len changes nothing: byte -128 and a NaN scale
    q8g, sg = q8.clone(), s.clone()
    for b, n in enumerate(lens):
        q8g[b, n:] = -128
        sg[b, n:] = float("nan")
    assert torch.equal(ops.attn_decode_kv8(q, (q8g, sg), kv_len, H, Hkv, hd, kvd, chunk=chunk), want)
    # row b alone, with its own cache slice, gives row b's bits
    for b in range(B):
        one = ops.attn_decode_kv8(q[b:b + 1].contiguous(), (q8[b:b + 1].contiguous(), s[b:b + 1].contiguous()), kv_len[b:b + 1].contiguous(),
                                  H, Hkv, hd, kvd, chunk=chunk)
        assert torch.equal(one[0], want[b]), b


def test_attn_decode_kv8_refuses_bad_arguments():
    _need_gpu()
    from radvlm_amd import lib
    B, H, Hkv, hd, L_max, chunk = 2, 2, 2, 128, 64, 128
    width = 2 * Hkv * hd
    q = torch.zeros(B, H * hd, dtype=BF16, device="cuda")
    q8 = torch.zeros(B, L_max, width, dtype=torch.int8, device="cuda")
    s = torch.ones(B, L_max, 2 * Hkv, dtype=torch.float32, device="cuda")
    kv_len = torch.ones(B, dtype=torch.int32, device="cuda")
    out = torch.zeros(B, H * hd, dtype=BF16, device="cuda")
    part = torch.zeros(B * H * (hd + 2), dtype=torch.float32, device="cuda")

    def call(hd_=hd, chunk_=chunk, part_bytes=part.numel() * 4):
        lib.call("rv_attn_decode_kv8_bf16", q, H * hd, q8, width, L_max * width, Hkv * hd, s, 2 * Hkv, L_max * 2 * Hkv, Hkv, kv_len, L_max,
                 out, H * hd, part, part_bytes, B, H, Hkv, hd_, chunk_, 1.0 / math.sqrt(hd))

    call()
    for kw in (dict(hd_=96), dict(chunk_=520), dict(part_bytes=part.numel() * 4 - 4)):
        with pytest.raises(lib.RadvlmHipError) as e:
            call(**kw)
        assert str(e.value).endswith("code -1"), str(e.value)              # RV_ERR_ARG
    torch.cuda.synchronize()

"""GPU tests of rv_attn_decode_verify_bf16 (radvlm_amd/csrc/lookup.hip): every query row of the R-row staircase bit for bit against
rv_attn_decode_bf16 run on that row alone (a B = 1 cache, its own kv_len), over both head sizes, group sizes 1 .. 8, row counts 1 .. 32,
three chunk sizes and key counts that put the staircase across the kernel's row-step and chunk boundaries; strides and refused
arguments.

Masking is made visible: the keys at positions kv_len0 - 1 .. kv_len0 + R - 2 (the last key each row may see) are needles -- K rows
along the queries' common direction, stronger with the position, so that the last needle a row sees takes nearly all of its softmax
weight, with a V of their own -- and every position from kv_len0 + R - 1 on (past the last row's range) is NaN.  A row that reads one
key too many or too few lands on another needle's V, or on NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L_MAX = 300                       # no multiple of any chunk size used
RS = (1, 2, 5, 8, 32)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(B, R, H, Hkv, hd, seed):
    """(q [B * R, H * hd], base cache [B, L_MAX, 2 * kvd], u [hd]): every q head is u + noise, u a +-1 vector."""
    g = torch.Generator().manual_seed(seed)
    u = (torch.randint(0, 2, (hd,), generator=g) * 2 - 1).float()
    q = (u.repeat(H)[None, :] + 0.3 * torch.randn(B * R, H * hd, generator=g)).to(torch.bfloat16).cuda()
    cache = torch.randn(B, L_MAX, 2 * Hkv * hd, generator=g).to(torch.bfloat16).cuda()
    return q, cache, u.cuda()


def _plant(base, kv0, R, u, Hkv, hd):
    """The case's cache: needles at kv_len0 - 1 .. kv_len0 + R - 2, NaN from kv_len0 + R - 1 on."""
    cache = base.clone()
    kvd = Hkv * hd
    for b, n0 in enumerate(kv0):
        for p in range(max(n0 - 1, 0), min(n0 + R - 1, L_MAX)):
            r = p - n0 + 1
            cache[b, p, :kvd] = (u * (2.0 + 0.5 * r)).repeat(Hkv).to(torch.bfloat16)
            cache[b, p, kvd:] = 10.0 + 3.0 * r
        cache[b, max(min(n0 + R - 1, L_MAX), 0):] = float("nan")
    return cache


def _reference(q, cache, kv0, R, H, Hkv, hd, chunk):
    from radvlm_amd import ops
    rows = []
    for b, n0 in enumerate(kv0):
        one = cache[b:b + 1].contiguous()
        for i in range(R):
            n = torch.tensor([n0 + i], dtype=torch.int32, device="cuda")
            rows.append(ops.attn_decode(q[b * R + i:b * R + i + 1], one, n, H, Hkv, hd, Hkv * hd, chunk=chunk))
    return torch.cat(rows)


@pytest.mark.parametrize("hd,G", [(64, 1), (64, 2), (64, 8), (128, 1), (128, 4), (128, 7)])
def test_bit_identical_to_one_row_decode_attention(hd, G):
    _need_gpu()
    from radvlm_amd import ops
    Hkv = 2
    H = Hkv * G
    rpb = 16 if hd == 128 else 32
    lens0 = [0, 1, rpb - 1, rpb] + list(range(120, 131)) + [255, 256]
    seen_needle = seen_clamp = 0
    for B in (1, 3):
        for R in RS:
            q, base, u = _inputs(B, R, H, Hkv, hd, seed=hd * 100 + G * 10 + B + R)
            for n0 in lens0 + [L_MAX - 3]:
                kv0 = [n0, n0 + 3, max(n0 - 5, 0)][:B]
                cache = _plant(base, kv0, R, u, Hkv, hd)
                kv_d = torch.tensor(kv0, dtype=torch.int32, device="cuda")
                for chunk in (rpb, 128, 512):
                    if n0 == L_MAX - 3 and chunk != 128:
                        continue
                    got = ops.attn_decode_verify(q, cache, kv_d, R, H, Hkv, hd, Hkv * hd, chunk=chunk)
                    want = _reference(q, cache, kv0, R, H, Hkv, hd, chunk)
                    assert torch.equal(got, want), (B, R, n0, chunk, (got.float() - want.float()).abs().max(1).values.tolist())
                    assert not torch.isnan(got.float()).any()
                    if n0 == 0:
                        assert not got[0].any()                              # a row without keys: zeros
                    # the needles decide the rows: row i sits on the V of needle i (the key at kv_len0 - 1 + i)
                    if R > 1 and 1 <= n0 and n0 + R - 1 <= L_MAX:
                        v = got[:R, :hd].float().mean(1).cpu().numpy()
                        assert np.all(np.abs(v - (10.0 + 3.0 * np.arange(R))) < 1.5), (n0, R, v)
                        seen_needle += 1
                seen_clamp += n0 + R - 1 > L_MAX
    assert seen_needle > 0 and seen_clamp > 0                                # kv_len0 + R - 1 > L_max was among the cases


def test_strided_q_and_out_keep_the_guard_columns():
    _need_gpu()
    from radvlm_amd import lib, ops
    H, Hkv, hd, B, R, chunk = 4, 2, 64, 2, 5, 128
    kvd = Hkv * hd
    q, base, u = _inputs(B, R, H, Hkv, hd, seed=7)
    kv0 = [126, 40]
    cache = _plant(base, kv0, R, u, Hkv, hd)
    kv_d = torch.tensor(kv0, dtype=torch.int32, device="cuda")
    want = ops.attn_decode_verify(q, cache, kv_d, R, H, Hkv, hd, kvd, chunk=chunk)
    qkv = torch.randn(B * R, H * hd + 2 * kvd, device="cuda").to(torch.bfloat16)          # q as a slice of a wider q|k|v row
    qkv[:, :H * hd] = q
    wide = torch.full((B * R, H * hd + 16), 77.0, dtype=torch.bfloat16, device="cuda")    # out inside wider rows
    got = ops.attn_decode_verify(qkv[:, :H * hd], cache, kv_d, R, H, Hkv, hd, kvd, out=wide[:, 8:8 + H * hd], chunk=chunk)
    torch.cuda.synchronize()
    assert got.data_ptr() == wide[:, 8:].data_ptr()
    assert torch.equal(wide[:, 8:8 + H * hd], want)
    assert (wide[:, :8] == 77.0).all() and (wide[:, 8 + H * hd:] == 77.0).all()

    out = torch.zeros(B * R, H * hd, dtype=torch.bfloat16, device="cuda")
    nch = (L_MAX + chunk - 1) // chunk
    part = torch.zeros(B * 32 * H * nch * (hd + 2), dtype=torch.float32, device="cuda")

    def call(rows, part_bytes, ld_q=H * hd, ld_o=H * hd):
        lib.call("rv_attn_decode_verify_bf16", q, ld_q, cache, 2 * kvd, L_MAX * 2 * kvd, kvd, kv_d, L_MAX, out, ld_o, part, part_bytes, B,
                 rows, H, Hkv, hd, chunk, 0.125)

    need = B * R * H * nch * (hd + 2) * 4
    call(R, need)
    for rows, nbytes in ((0, need), (33, part.numel() * 4), (R, need - 4)):
        with pytest.raises(lib.RadvlmHipError):
            call(rows, nbytes)
    with pytest.raises(lib.RadvlmHipError):
        call(R, need, ld_q=H * hd - 8)
    with pytest.raises(lib.RadvlmHipError):
        call(R, need, ld_o=H * hd - 8)
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_attn_decode_verify_bf16", q, H * hd, cache, 2 * kvd, L_MAX * 2 * kvd, kvd, kv_d, L_MAX, out, H * hd, part, need, B, R,
                 H, Hkv, hd, 48, 0.125)                                               # a chunk rv_attn_decode_bf16 refuses too

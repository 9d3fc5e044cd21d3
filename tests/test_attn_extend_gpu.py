"""GPU tests of the extend attention kernel (rv_attn_extend_bf16): new query rows of each sequence against its KV cache, checked against
an fp32 torch reference over the model shapes, at key-chunk boundaries, for partial and many query tiles and mixed batches; a row's
result bit for bit alone and in a batch and whatever the cache holds past its position; one new row against the decode attention."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EXTEND_TOL = 1e-2           # max |out - ref| / max |ref|; the measured figures are recorded by record_measurement (attn_extend_vs_fp32): 0.36-0.50 %

# (hd, H, Hkv): toy_qwen, toy, Qwen2-7B, Llama-7B (heads cut to 4: the kernel's work split is per kv head), G = 8
SHAPES = [(64, 4, 2), (128, 2, 2), (128, 28, 4), (128, 4, 4), (128, 8, 1)]
R_VALUES = (0, 1, 255, 256, 257, 1100)     # chunk = 256: 0, 1, chunk - 1, chunk, chunk + 1, > 1000
N_VALUES = (1, 2, 15, 16, 17, 64, 200)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    assert ops.EXTEND_CHUNK == 256
    return ops


def _case(rs, ns, H, Hkv, hd, seed=0, slack=37):
    g = torch.Generator().manual_seed(seed)
    B, kvd = len(rs), Hkv * hd
    L_max = max(r + n for r, n in zip(rs, ns)) + slack
    cache = (torch.randn(B, L_max, 2 * kvd, generator=g) * torch.linspace(0.5, 1.5, 2 * kvd)).to(torch.bfloat16).cuda()
    q = (torch.randn(sum(ns), H * hd, generator=g) * 1.3).to(torch.bfloat16).cuda()
    cu = torch.tensor(np.concatenate([[0], np.cumsum(ns)]), dtype=torch.int32).cuda()
    r = torch.tensor(rs, dtype=torch.int32).cuda()
    return q, cache, cu, r


def _ref(q, cache, rs, ns, H, Hkv, hd):
    G, kvd = H // Hkv, Hkv * hd
    out, row = [], 0
    for b, (r, n) in enumerate(zip(rs, ns)):
        Lk = r + n
        K = cache[b, :Lk, :kvd].float().view(Lk, Hkv, hd).repeat_interleave(G, dim=1)
        V = cache[b, :Lk, kvd:].float().view(Lk, Hkv, hd).repeat_interleave(G, dim=1)
        Q = q[row:row + n].float().view(n, H, hd)
        s = torch.einsum("nhd,khd->hnk", Q, K) / hd ** 0.5
        mask = torch.arange(Lk, device=q.device)[None, :] <= (r + torch.arange(n, device=q.device))[:, None]
        p = torch.softmax(s.masked_fill(~mask, float("-inf")), dim=-1)
        out.append(torch.einsum("hnk,khd->nhd", p, V).reshape(n, H * hd))
        row += n
    return torch.cat(out)


def _run(ops, q, cache, cu, r, ns, H, Hkv, hd):
    return ops.attn_extend(q, cache, cu, r, H, Hkv, hd, Hkv * hd, max(ns))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"hd{s[0]}_H{s[1]}_Hkv{s[2]}" for s in SHAPES])
def test_extend_matches_fp32_reference(shape):
    ops = _ops()
    hd, H, Hkv = shape
    worst = 0.0
    # every (r, n) pair, packed into mixed batches of 7 sequences (row b of batch k: R_VALUES[(b + k) % 6], N_VALUES[b])
    for k in range(len(R_VALUES)):
        rs = [R_VALUES[(b + k) % len(R_VALUES)] for b in range(len(N_VALUES))]
        ns = list(N_VALUES)
        q, cache, cu, r = _case(rs, ns, H, Hkv, hd, seed=k)
        got = _run(ops, q, cache, cu, r, ns, H, Hkv, hd).float()
        ref = _ref(q, cache, rs, ns, H, Hkv, hd)
        assert torch.isfinite(got).all()
        row = 0
        for b, n in enumerate(ns):      # per sequence: the error relative to that sequence's own output scale
            e = float((got[row:row + n] - ref[row:row + n]).abs().max() / ref[row:row + n].abs().max())
            worst = max(worst, e)
            assert e <= EXTEND_TOL, (shape, rs[b], n, e)
            row += n
    from conftest import record_measurement
    record_measurement("attn_extend_vs_fp32", shape=list(shape), max_rel=worst)


@pytest.mark.parametrize("shape", [(64, 4, 2), (128, 28, 4)], ids=["hd64_G2", "hd128_G7"])
def test_row_bit_identical_alone_and_in_batch(shape):
    ops = _ops()
    hd, H, Hkv = shape
    rs, ns = [300, 0, 257, 1100], [17, 40, 1, 64]
    q, cache, cu, r = _case(rs, ns, H, Hkv, hd, seed=3)
    full = _run(ops, q, cache, cu, r, ns, H, Hkv, hd)
    row = 0
    for b, n in enumerate(ns):
        L1 = rs[b] + n
        c1 = cache[b:b + 1, :L1 + 5].contiguous()                     # another L_max too: only the sequence's own keys count
        one = ops.attn_extend(q[row:row + n].contiguous(), c1, torch.tensor([0, n], dtype=torch.int32).cuda(),
                              r[b:b + 1].contiguous(), H, Hkv, hd, Hkv * hd, n)
        assert torch.equal(one, full[row:row + n]), b
        row += n


def test_cache_rows_past_a_query_do_not_matter():
    ops = _ops()
    hd, H, Hkv = 128, 28, 4
    rs, ns = [300, 5], [40, 3]
    q, cache, cu, r = _case(rs, ns, H, Hkv, hd, seed=4)
    a = _run(ops, q, cache, cu, r, ns, H, Hkv, hd)
    i = 10                                                            # query 10 of sequence 0 sits at position 310
    c2 = cache.clone()
    c2[0, 311:] = (torch.randn(c2.shape[1] - 311, c2.shape[2]) * 3).to(torch.bfloat16).cuda()
    b = _run(ops, q, c2, cu, r, ns, H, Hkv, hd)
    assert torch.equal(a[i], b[i]) and torch.equal(a[:i], b[:i])
    assert torch.equal(a[40:], b[40:])                                # the other sequence is not touched either
    assert not torch.equal(a[i + 1:40], b[i + 1:40])                  # later queries do see the changed rows


@pytest.mark.parametrize("shape", [(64, 4, 2), (128, 28, 4), (128, 4, 4)], ids=["hd64_G2", "hd128_G7", "hd128_G1"])
def test_single_new_row_agrees_with_decode_attention(shape):
    ops = _ops()
    hd, H, Hkv = shape
    rs, ns = [0, 1, 255, 256, 1100], [1] * 5
    q, cache, cu, r = _case(rs, ns, H, Hkv, hd, seed=5)
    ext = _run(ops, q, cache, cu, r, ns, H, Hkv, hd).float()
    dec = ops.attn_decode(q, cache, (r + 1).contiguous(), H, Hkv, hd, Hkv * hd).float()
    e = float((ext - dec).abs().max() / dec.abs().max())
    from conftest import record_measurement
    record_measurement("attn_extend_vs_decode", shape=list(shape), max_rel=e)
    assert e <= EXTEND_TOL, e


def test_extend_rejects_bad_arguments():
    ops = _ops()
    from radvlm_amd.lib import RadvlmHipError
    q, cache, cu, r = _case([4], [3], 4, 2, 64)
    with pytest.raises(RadvlmHipError):
        ops.attn_extend(q, cache, cu, r, 4, 2, 64, 128, 3, chunk=100)       # the chunk must be a multiple of 64
    q2, cache2, cu2, r2 = _case([4], [3], 18, 2, 64)
    with pytest.raises(RadvlmHipError):
        ops.attn_extend(q2, cache2, cu2, r2, 18, 2, 64, 128, 3)              # 9 q heads per kv head

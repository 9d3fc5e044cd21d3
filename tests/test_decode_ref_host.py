"""CPU checks of tests/decode_ref.py: the references alone meet the exact conditions tests/test_decode_edges_gpu.py asserts of the HIP
kernels (exact integer products, needle attention rows that equal a V row bit for bit), so a failure there points at a kernel."""
import math

import pytest
import torch

from decode_ref import BF16, attn_decode_ref, attn_extend_ref, gemv_ref, integer_operands, needle_cache


@pytest.mark.parametrize("K", [8, 40, 520, 2056])
def test_integer_operands_are_exact_in_fp32(K):
    M, N = 32, 65
    x, w, bias, res = integer_operands(M, N, K, seed=K)
    for t, lim in ((x, 2), (w, 3), (bias, 4), (res, 4)):
        assert torch.equal(t.float(), t.float().round()) and float(t.float().abs().max()) == lim       # integers, the full range drawn
    ref = gemv_ref(x, w)
    assert float(ref.abs().max()) <= 6 * K
    assert torch.equal((x.float() @ w.float().t()).double(), ref)
    # and in another summation order: the K range in 32-deep steps dealt to four partial sums, as the kernel's waves take them
    parts = [sum((x[:, k:k + 32].float() @ w[:, k:k + 32].float().t() for k in range(32 * u, K, 128)), torch.zeros(M, N)) for u in range(4)]
    assert torch.equal((((parts[0] + parts[1]) + parts[2]) + parts[3]).double(), ref)
    full = gemv_ref(x, w, bias, res)
    assert torch.equal(((x.float() @ w.float().t()) + bias.float() + res.float()).double(), full)
    assert torch.equal(full.float().double(), full)                    # the fp32 output the GPU test expects loses nothing


N_NEEDLE = 8192


@pytest.mark.parametrize("hd", [64, 128])
def test_needle_cache_gives_the_target_row_bit_for_bit(hd):
    Hkv, G = 2, 2
    H = Hkv * G
    for t in (0, 127, 128, N_NEEDLE - 1):
        q1, K, V = needle_cache(N_NEEDLE, hd, Hkv, [t], seed=hd + t)
        Kf = K.float().view(N_NEEDLE, Hkv, hd)
        assert torch.equal(Kf.abs(), torch.full_like(Kf, 2.0))
        rows = torch.ones(N_NEEDLE, dtype=torch.bool)
        rows[t] = False
        assert torch.equal(Kf[rows].sum(-1), torch.zeros(N_NEEDLE - 1, Hkv))        # hd/2 of each sign
        assert torch.equal(Kf[t], torch.full((Hkv, hd), 2.0))
        q = q1.repeat(H)[None]
        scores = (Kf[:, 0] @ q1.float()) / math.sqrt(hd)
        assert float(scores[t]) == pytest.approx(8 * math.sqrt(hd)) and torch.equal(scores[rows], torch.zeros(N_NEEDLE - 1))
        want = V[t].view(Hkv, hd).repeat_interleave(G, dim=0).reshape(1, H * hd)
        for dtype in (torch.float32, torch.float64):
            got = attn_decode_ref(q, K[None], V[None], [N_NEEDLE], H, Hkv, hd, dtype=dtype)
            assert torch.equal(got.to(BF16), want), (t, dtype)


@pytest.mark.parametrize("hd", [64, 128])
def test_needle_cache_two_targets_give_their_mean(hd):
    Hkv, G = 2, 2
    H = Hkv * G
    for a, b in ((127, 128), (0, N_NEEDLE - 1)):
        q1, K, V = needle_cache(N_NEEDLE, hd, Hkv, [a, b], seed=hd + a + b)
        want = ((V[a].float() + V[b].float()) / 2).to(BF16).view(Hkv, hd).repeat_interleave(G, dim=0).reshape(1, H * hd)
        assert float(V[a].float().min()) >= 1 and float(V[b].float().max()) <= 8
        for dtype in (torch.float32, torch.float64):
            got = attn_decode_ref(q1.repeat(H)[None], K[None], V[None], [N_NEEDLE], H, Hkv, hd, dtype=dtype)
            assert torch.equal(got.to(BF16), want), (a, b, dtype)


def test_attn_decode_ref_agrees_with_the_kernel_tests_fp32_reference():
    from test_decode_kernels_gpu import _attn_ref
    hd, Hkv, G = 64, 2, 3
    H, kvd = Hkv * G, Hkv * hd
    lens = [1, 17, 40]
    g = torch.Generator().manual_seed(0)
    cache = torch.randn(3, 40, 2 * kvd, generator=g).to(BF16)
    q = torch.randn(3, H * hd, generator=g).to(BF16)
    ref = attn_decode_ref(q, cache[:, :, :kvd], cache[:, :, kvd:], lens, H, Hkv, hd)
    old = _attn_ref(q, cache, lens, H, Hkv, hd)
    assert float((ref - old.double()).abs().max()) <= 1e-5 * float(ref.abs().max())
    # keys at and past a sequence's length do not reach the reference, whatever they hold; an empty sequence gives zeros
    c2 = cache.clone()
    c2[1, 17:] = float("nan")
    ref2 = attn_decode_ref(q, c2[:, :, :kvd], c2[:, :, kvd:], [1, 17, 0], H, Hkv, hd)
    assert torch.equal(ref2[:2], ref[:2]) and torch.equal(ref2[2], torch.zeros(H * hd, dtype=torch.float64))


def test_attn_extend_ref_agrees_with_the_extend_tests_fp32_reference():
    from test_attn_extend_gpu import _ref
    hd, H, Hkv = 64, 4, 2
    kvd = Hkv * hd
    rs, ns = [5, 0], [3, 4]
    g = torch.Generator().manual_seed(1)
    cache = torch.randn(2, 12, 2 * kvd, generator=g).to(BF16)
    q = torch.randn(sum(ns), H * hd, generator=g).to(BF16)
    ref = attn_extend_ref(q, cache[:, :, :kvd], cache[:, :, kvd:], rs, ns, H, Hkv, hd)
    old = _ref(q, cache, rs, ns, H, Hkv, hd)
    assert float((ref - old.double()).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_torch_argmax_conventions_the_argmax_kernel_is_held_to():
    """The indices tests/test_decode_edges_gpu.py writes out by hand are what torch.argmax gives on the CPU."""
    nan, inf = float("nan"), float("inf")
    x = torch.full((4, 256), -1.0)
    x[0, 50], x[0, 20] = nan, inf
    x[1, 200] = x[1, 100] = nan
    x[2, :] = -inf
    x[3, 3], x[3, 9] = -0.0, 0.0
    assert torch.argmax(x, dim=1).tolist() == [50, 100, 0, 3]

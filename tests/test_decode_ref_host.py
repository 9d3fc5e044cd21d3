"""CPU checks of tests/decode_ref.py: the references alone meet the exact conditions tests/test_decode_edges_gpu.py and
tests/test_attn_extend_edges_gpu.py assert of the HIP kernels (exact integer products, needle and staircase attention rows that equal a V
row bit for bit, extend windows that cover every tile and chunk edge and force the rescale), so a failure there points at a kernel."""
import math

import pytest
import torch

from decode_ref import (BF16, EXTEND_CHUNKS, EXTEND_L, EXTEND_WINDOWS, attn_decode_ref, attn_extend_ref, extend_query_tile, extend_rows_exposed, extend_windows,
                        gemv_ref, integer_operands, needle_cache, stair_windows, staircase_cache)


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


# ------------------------------------------------------------------------------------------------ extend attention
@pytest.mark.parametrize("hd", [64, 128])
def test_staircase_cache_gives_each_rows_own_v_row_under_float64(hd):
    """Every (r, n) tests/test_attn_extend_edges_gpu.py sends: the float64 reference is want to 2^-20, every weight off a row's own key is
    below 1e-20, and the decoy past the sequence would move any row that saw it by more than 100."""
    Hkv, L = 2, EXTEND_L
    scale = 1.0 / math.sqrt(hd)
    for k, (r, n) in enumerate(stair_windows()):
        q1, K, V, want = staircase_cache(r, n, L, hd, Hkv, seed=hd + k, stale="decoy")
        Kf = K.float().view(L, Hkv, hd)
        assert torch.equal(Kf[:r].abs(), torch.full_like(Kf[:r], 2.0)) and torch.equal(Kf[:r].sum(-1), torch.zeros(r, Hkv))
        assert torch.equal(Kf[r:r + n], (4.0 + 2 * torch.arange(n))[:, None, None].expand(n, Hkv, hd))
        assert torch.equal(K.float(), K.float().round()) and float(K.float().abs().max()) * 4 * hd < 2 ** 24
        assert torch.equal(want, V[r:r + n]) and float(want.float().min()) >= 1 and float(want.float().max()) <= 8
        q = q1.repeat(1, Hkv)                                      # G = 1
        ref = attn_extend_ref(q, K[None], V[None], [r], [n], Hkv, Hkv, hd)
        assert float((ref - want.double()).abs().max()) < 2.0 ** -20, (r, n)
        s = torch.einsum("id,jkd->kij", q1.double(), K.double().view(L, Hkv, hd)) * scale                 # [Hkv, n, L]
        seen = torch.arange(L)[None, :] <= (r + torch.arange(n))[:, None]
        p = torch.softmax(s.masked_fill(~seen[None], float("-inf")), dim=-1)
        own = torch.zeros(n, L, dtype=torch.bool)
        own[torch.arange(n), r + torch.arange(n)] = True
        assert float(p.masked_fill(own[None], 0.0).max()) < 1e-20, (r, n)
        if r + n < L:                                              # every row, were the key at r + n visible to it
            see = seen.clone()
            see[:, r + n] = True
            p2 = torch.softmax(s.masked_fill(~see[None], float("-inf")), dim=-1)
            moved = torch.einsum("kij,jkd->ikd", p2, V.double().view(L, Hkv, hd)).reshape(n, Hkv * hd)
            assert float((moved - want.double()).abs().min()) > 100, (r, n)
        # the NaN variant differs in the stale rows only
        _, Kn, Vn, wantn = staircase_cache(r, n, L, hd, Hkv, seed=hd + k, stale="nan")
        assert torch.equal(Kn[:r + n], K[:r + n]) and torch.equal(Vn[:r + n], V[:r + n]) and torch.equal(wantn, want)
        assert torch.isnan(Kn[r + n:].float()).all() and torch.isnan(Vn[r + n:].float()).all()


def test_stair_windows_keep_every_row_of_the_windows():
    cut = stair_windows()
    assert all(1 <= n <= 64 for _, n in cut)
    pos = lambda ws: sorted(r + i for r, n in ws for i in range(n))
    assert pos(cut) == pos(EXTEND_WINDOWS) and (0, 64) in cut and (64, 6) in cut and (314, 6) in cut


def test_extend_windows_cover_every_query_tile_edge():
    """For every group size: a window with rows QT - 1 and QT (two query tiles) whose row count is no multiple of 16 (a partial MFMA tile)."""
    assert [extend_query_tile(G) for G in range(1, 9)] == [64, 32, 16, 16, 16, 16, 16, 16]
    for G in range(1, 9):
        QT = extend_query_tile(G)
        assert any(n > QT and n % 16 for _, n in EXTEND_WINDOWS), G


def test_extend_windows_cover_every_chunk_edge():
    """For every chunk size: rows on both sides of a chunk edge, a first row exactly on one, a last row exactly below one."""
    for chunk in EXTEND_CHUNKS:
        assert any(r // chunk != (r + n - 1) // chunk for r, n in EXTEND_WINDOWS), chunk
        assert any(r > 0 and r % chunk == 0 for r, n in EXTEND_WINDOWS), chunk
        assert any((r + n) % chunk == 0 for r, n in EXTEND_WINDOWS), chunk


def test_extend_windows_reach_the_end_of_the_cache():
    assert EXTEND_L % 64 and all(r + n <= EXTEND_L for r, n in EXTEND_WINDOWS)
    assert any(r + n == EXTEND_L for r, n in EXTEND_WINDOWS)
    assert any(r + n == EXTEND_L for r, n in stair_windows())


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("family", ["stair", "sink"])
def test_extend_families_raise_the_running_maximum_inside_a_chunk(family, hd):
    """The extend body walks a chunk in 64-key stages and rescales o and l by alpha = exp(m_old - m_new).  For every window at r >= 64
    and the chunk sizes with more than one stage, the float64 scores of some row raise the running maximum by more than 5 exp2 units
    (alpha < 2^-5) in a stage after the chunk's first: a lost or wrong alpha is an O(1) error there."""
    Hkv = 2
    case = extend_windows(family, EXTEND_L, Hkv, Hkv, hd, EXTEND_WINDOWS, keep_scores=True)
    s2 = case["scores2"]                                           # [H, L, L], -inf where masked
    for r, n in EXTEND_WINDOWS:
        if r < 64:
            continue
        for chunk in (128, 256):
            rise = 0.0
            for pos in range(r, r + n):
                for c0 in range(0, pos + 1, chunk):
                    m = s2[:, pos, c0:c0 + 64].max(-1).values      # the first stage of a chunk the row owns always holds a visible key
                    for k0 in range(c0 + 64, min(c0 + chunk, pos + 1), 64):
                        mx = s2[:, pos, k0:k0 + 64].max(-1).values
                        rise = max(rise, float((mx - m).max()))
                        m = torch.maximum(m, mx)
            assert rise > 5.0, (family, hd, r, n, chunk, rise)


def test_extend_rows_exposed_written_out_by_hand():
    ex = extend_rows_exposed
    assert ex(48, 17, 1, 64) == [16] and ex(48, 17, 1, 256) == list(range(17)) and ex(48, 17, 8, 256) == [16]
    assert ex(63, 66, 1, 64) == [65] and ex(63, 66, 1, 256) == [64, 65] and ex(63, 66, 3, 256) == [64, 65]
    assert ex(250, 70, 1, 64) == list(range(64, 70)) and ex(250, 70, 8, 256) == list(range(64, 70))
    assert ex(250, 70, 2, 256) == list(range(64, 70))


def test_extend_windows_rows_are_the_documents_rows():
    """A window's reference rows are attn_extend_ref of its own cache row (NaN past r + n included), to float64 rounding."""
    hd, Hkv, G = 64, 2, 2
    case = extend_windows("rand", 80, G * Hkv, Hkv, hd, ((0, 3), (15, 2), (63, 17)))
    assert torch.isnan(case["K"][1, 17:].float()).all() and not torch.isnan(case["K"][1, :17].float()).any()
    ref = attn_extend_ref(case["q"], case["K"], case["V"], case["rs"], case["ns"], G * Hkv, Hkv, hd)
    assert float((ref - case["out"]).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((case["A_out"] - case["out"].abs()).min()) >= -1e-12


def test_torch_argmax_conventions_the_argmax_kernel_is_held_to():
    """The indices tests/test_decode_edges_gpu.py writes out by hand are what torch.argmax gives on the CPU."""
    nan, inf = float("nan"), float("inf")
    x = torch.full((4, 256), -1.0)
    x[0, 50], x[0, 20] = nan, inf
    x[1, 200] = x[1, 100] = nan
    x[2, :] = -inf
    x[3, 3], x[3, 9] = -0.0, 0.0
    assert torch.argmax(x, dim=1).tolist() == [50, 100, 0, 3]

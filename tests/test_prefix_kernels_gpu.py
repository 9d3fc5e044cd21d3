"""GPU tests of rv_attn_decode_shared_bf16 (radvlm_amd/csrc/prefix.hip): ops.attn_decode_shared bit for bit against ops.attn_decode on
the same cache, with tile tables built by generation.shared_tiles.  Chunk 32 and L_max 160 give five chunks; every position at or past
a row's kv_len holds NaN bit patterns, so a key read one position too far shows.

Reading of the 19 rows: a lineage of 17 (P = 96, one row P = 70), one ungrouped active row and one idle row (ungrouped, kv_len = 1);
the second case has two lineages, two ungrouped active rows and an idle row.  That equal outputs come from the SHARED path is shown
separately: the followers' own copies of the shared chunks are overwritten with NaN and the result does not change."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, L_MAX, B = 32, 160, 19
SHAPES = [(4, 4, 128), (4, 4, 64), (8, 2, 128), (7, 1, 128), (8, 1, 64)]
BF16 = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _case(H, Hkv, hd, lineage, P, kv_len, seed, active):
    """(q, cache, kv_len device, plan, c0, tile): rows of one lineage hold one common content at their first P positions, their own
    after it, NaN from kv_len on."""
    from radvlm_amd import ops
    from radvlm_amd.generation import shared_tiles
    g = torch.Generator().manual_seed(seed)
    kvd = Hkv * hd
    q = torch.randn(B, H * hd, generator=g).to(BF16).cuda()
    cache = torch.randn(B, L_MAX, 2 * kvd, generator=g).to(BF16)
    for lin in set(int(v) for v in lineage if v >= 0):
        common = torch.randn(L_MAX, 2 * kvd, generator=g).to(BF16)
        for s in np.flatnonzero(lineage == lin):
            cache[s, :P[s]] = common[:P[s]]
    for s in range(B):
        cache[s, kv_len[s]:] = float("nan")
    c0, tile = shared_tiles(active, lineage, P, 16 // (H // Hkv), CHUNK, B)
    plan = ops.shared_tiles_upload(c0, tile, 16 // (H // Hkv), "cuda")
    return q, cache.cuda(), torch.tensor(kv_len, dtype=torch.int32, device="cuda"), plan, c0, tile


def _both(q, cache, kv_d, plan, H, Hkv, hd):
    from radvlm_amd import ops
    got = ops.attn_decode_shared(q, cache, kv_d, plan.c0, plan.tile, H, Hkv, hd, Hkv * hd, chunk=CHUNK)
    want = ops.attn_decode(q, cache, kv_d, H, Hkv, hd, Hkv * hd, chunk=CHUNK)
    torch.cuda.synchronize()
    return got, want


def _kv_lens(P, c0):
    """Per row, cycling: P + 1, exactly c0 * chunk + 1, one mid-chunk (at or past the row's shared chunks), L_max."""
    out = []
    for s in range(B):
        c = max(int(c0[s]), 1) * CHUNK
        out.append([int(P[s]) + 1, c + 1, max(113, c + 17), L_MAX][(s + 1) % 4])
    return out


def _one_lineage(H, Hkv):
    from radvlm_amd.generation import shared_tiles
    lineage = np.full(B, -1, dtype=np.int64)
    members = [s for s in range(B) if s not in (5, 11)]                            # 17 rows; 5: ungrouped, 11: idle
    lineage[members] = 0
    P = np.where(lineage == 0, 96, 0)
    P[7] = 70                                                                      # pulls its tile to c0 = 2
    c0, _ = shared_tiles(members, lineage, P, 16 // (H // Hkv), CHUNK, B)          # the tiles do not depend on kv_len
    kv_len = _kv_lens(np.where(lineage == 0, P, 40), c0)
    kv_len[11] = 1
    return lineage, P, kv_len, [s for s in range(B) if s != 11]


@pytest.mark.parametrize("H,Hkv,hd", SHAPES)
def test_one_lineage_bit_identical_to_plain(H, Hkv, hd):
    _need_gpu()
    lineage, P, kv_len, active = _one_lineage(H, Hkv)
    q, cache, kv_d, plan, c0, tile = _case(H, Hkv, hd, lineage, P, kv_len, seed=H * 1000 + hd, active=active)
    rpt = 16 // (H // Hkv)
    members = np.flatnonzero(lineage == 0)
    assert len(members) == 17 and c0[5] == 0 and c0[11] == 0
    assert c0[members[-1]] == 0 and tile[members[-1], 0] == -1                     # 17 = k * rpt + 1: the last tile is one row, plain
    seven = members[(list(members).index(7) // rpt) * rpt:][:rpt]
    assert (c0[seven] == 2).all() and (c0[np.setdiff1d(members[:16], seven)] == 3).all()
    if rpt == 16:
        assert tile[0].tolist() == list(members[:16])                              # MHA: one full tile of 16
    if rpt == 16:
        assert {97, 71, 65, 113, L_MAX} <= set(kv_len[s] for s in members)         # P + 1 (both P), c0 * chunk + 1, mid-chunk, L_max
    got, want = _both(q, cache, kv_d, plan, H, Hkv, hd)
    assert torch.equal(got, want), (got.float() - want.float()).abs().max(1).values.tolist()
    assert not torch.isnan(got.float()).any()


@pytest.mark.parametrize("H,Hkv,hd", SHAPES)
def test_two_lineages_in_one_launch(H, Hkv, hd):
    _need_gpu()
    from radvlm_amd.generation import shared_tiles
    lineage = np.full(B, -1, dtype=np.int64)
    lineage[[0, 2, 4, 6, 8, 10, 12]] = 3                                           # interleaved with the other lineage's rows
    lineage[[1, 3, 7, 9, 13, 15, 16, 17, 18]] = 9
    P = np.where(lineage == 3, 64, np.where(lineage == 9, 130, 0))
    P[13] = 100
    active = [s for s in range(B) if s != 14]                                      # 5, 11: ungrouped and active; 14: idle
    c0, _ = shared_tiles(active, lineage, P, 16 // (H // Hkv), CHUNK, B)
    kv_len = _kv_lens(np.where(lineage >= 0, P, 50), c0)
    kv_len[14] = 1
    q, cache, kv_d, plan, c0, tile = _case(H, Hkv, hd, lineage, P, kv_len, seed=H * 1000 + hd + 1, active=active)
    assert set(c0[lineage == 3].tolist()) <= {0, 2} and set(c0[lineage == 9].tolist()) <= {0, 3, 4} and (c0 > 0).sum() >= 14
    assert (tile[:, 0] >= 0).sum() >= 2
    got, want = _both(q, cache, kv_d, plan, H, Hkv, hd)
    assert torch.equal(got, want), (got.float() - want.float()).abs().max(1).values.tolist()
    assert not torch.isnan(got.float()).any()


@pytest.mark.parametrize("H,Hkv,hd", [(4, 4, 128), (7, 1, 128), (8, 1, 64)])
def test_shared_chunks_are_read_from_the_leading_row_only(H, Hkv, hd):
    """The followers' own shared chunks replaced by NaN: the shared kernel still gives the plain kernel's bits on the intact cache."""
    _need_gpu()
    lineage, P, kv_len, active = _one_lineage(H, Hkv)
    q, cache, kv_d, plan, c0, tile = _case(H, Hkv, hd, lineage, P, kv_len, seed=H * 1000 + hd + 2, active=active)
    _, want = _both(q, cache, kv_d, plan, H, Hkv, hd)
    broken = cache.clone()
    followers = [s for s in range(B) if c0[s] > 0 and tile[s, 0] != s]
    assert len(followers) >= 8
    for s in followers:
        broken[s, :int(c0[s]) * CHUNK] = float("nan")
    got, plain = _both(q, broken, kv_d, plan, H, Hkv, hd)
    assert torch.equal(got, want)
    assert torch.isnan(plain[followers].float()).any(1).all()                      # the plain kernel does read them


def test_no_tiles_is_the_plain_kernel_and_bad_tables_stay_in_bounds():
    _need_gpu()
    from radvlm_amd import ops
    H, Hkv, hd = 8, 2, 128
    lineage, P, kv_len, active = _one_lineage(H, Hkv)
    q, cache, kv_d, plan, c0, tile = _case(H, Hkv, hd, lineage, P, kv_len, seed=5, active=active)
    zero = ops.shared_tiles_upload(np.zeros(B, np.int32), np.full((B, 16), -1, np.int32), 4, "cuda")
    got, want = _both(q, cache, kv_d, zero, H, Hkv, hd)
    assert torch.equal(got, want)
    # entries outside [0, B) end a tile's list in the kernel; the wrapper refuses such a table before it is uploaded
    bad = tile.copy()
    bad[0, 1] = B
    with pytest.raises(ValueError, match="outside"):
        ops.shared_tiles_upload(c0, bad, 4, "cuda")
    raw = torch.from_numpy(bad).cuda()
    out = ops.attn_decode_shared(q, cache, kv_d, plan.c0, raw, H, Hkv, hd, Hkv * hd, chunk=CHUNK)
    torch.cuda.synchronize()
    listed = [int(s) for s in tile[0] if s >= 0]
    others = [s for s in range(B) if s not in listed[1:]]
    assert torch.equal(out[others], want[others])                                  # the rows the broken list no longer reaches aside


def test_refused_arguments():
    _need_gpu()
    from radvlm_amd import lib
    H, Hkv, hd = 4, 2, 64
    kvd = Hkv * hd
    q = torch.zeros(2, H * hd, dtype=BF16, device="cuda")
    cache = torch.zeros(2, L_MAX, 2 * kvd, dtype=BF16, device="cuda")
    kv = torch.ones(2, dtype=torch.int32, device="cuda")
    c0 = torch.zeros(2, dtype=torch.int32, device="cuda")
    tile = torch.full((2, 16), -1, dtype=torch.int32, device="cuda")
    out = torch.empty_like(q)
    nch = (L_MAX + CHUNK - 1) // CHUNK
    part = torch.empty(2 * H * nch * (hd + 2), dtype=torch.float32, device="cuda")

    def call(c0=c0, tile=tile, chunk=CHUNK, part_bytes=part.numel() * 4, Hq=H):
        lib.call("rv_attn_decode_shared_bf16", q, H * hd, cache, 2 * kvd, L_MAX * 2 * kvd, kvd, kv, c0, tile, L_MAX, out, H * hd, part,
                 part_bytes, 2, Hq, Hkv, hd, chunk, 0.125)

    call()
    for kw in (dict(c0=None), dict(tile=None), dict(chunk=48), dict(chunk=1024), dict(part_bytes=part.numel() * 4 - 4), dict(Hq=18)):
        with pytest.raises(lib.RadvlmHipError):
            call(**kw)


def test_engine_routes_give_the_same_logits():
    """decode_step(shared=plan) with shared_route "shared" and "plain", and the plain call, on clones of one cache (toy: MHA, hd 128)."""
    _need_gpu()
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.engine import LlavaEngine
    from radvlm_amd.generation import shared_tiles
    eng = LlavaEngine(GEOMETRIES["toy"], device="cuda:0", init="portable", seed=0)
    S, L = 5, 300
    lens = np.array([140, 131, 260, 0, 129])
    base = eng.new_kv_cache(S, L)
    for t in base.layers:
        t.copy_(torch.randn(t.shape, device=t.device).to(t.dtype))
        t[[1, 2, 4], :128] = t[0, :128]                                            # slots 0, 1, 2, 4: one lineage, one whole chunk
        for s in range(S):
            t[s, int(lens[s]):] = float("nan")
    lineage = np.array([0, 0, 0, -1, 0])
    c0, tile = shared_tiles([0, 1, 2, 4], lineage, np.array([128, 128, 128, 0, 128]), eng.shared_rows_per_tile, 128, S)
    assert c0.tolist() == [1, 1, 1, 0, 1]
    plan = eng.shared_plan(c0, tile)
    toks = [3, 5, 7, 0, 11]
    outs = []
    for route, kw in (("plain", {}), ("plain", dict(shared=plan)), ("shared", dict(shared=plan)), (None, dict(shared=plan))):
        cache = eng.new_kv_cache(S, L)
        for a, b in zip(cache.layers, base.layers):
            a.copy_(b)
        cache.lens[:] = lens
        eng.shared_route = route
        try:
            outs.append((eng.decode_step(cache, toks).clone() if not kw else eng.decode_step(cache, toks, **kw).clone(),
                         [t.clone() for t in cache.layers]))
        finally:
            eng.shared_route = None
        assert cache.lens.tolist() == (lens + 1).tolist()
    for lg, layers in outs[1:]:
        assert torch.equal(lg, outs[0][0]) and bool(torch.isfinite(lg).all())
        for a, b in zip(layers, outs[0][1]):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    with pytest.raises(NotImplementedError):
        eng.decode_step(base, toks, shared=plan, beams=object())
    eng.shared_route = "both"
    try:
        with pytest.raises(ValueError):
            eng.decode_step(base, toks, shared=plan)
    finally:
        eng.shared_route = None

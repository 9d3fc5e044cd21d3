"""CPU checks of tests/dataops_ref.py: the dropout mask against its stated definition and its statistics, AdamW against torch.optim.AdamW and
the fp32 oracle, the 2x2 max against max_pool2d and its autograd, the weighted segment sum against bilinear interpolation, im2col against
conv2d, the transpose against the stated index rule and the image normalisation against the two host processors -- so a failure of
tests/test_dataops_edges_gpu.py points at a kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dataops_ref as D
from dataops_ref import BF16

SEEDS = (0, (1 << 32) + 5, (1 << 63) - 1)


def _bf(*shape, std=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF16)


# ------------------------------------------------------------------------------------------------ the mask
def test_keep_mask_threshold_edges():
    assert D.thr16(0.0) == 0 and D.thr16(2.0 ** -18) == 0 and D.thr16(2.0 ** -17) == 1 and D.thr16(0.99999) == 65535
    assert D.thr16(0.25) == 16384 and D.thr16(0.5) == 32768
    for seed in SEEDS:
        assert bool(D.keep_mask(seed, 4099, 0.0).all()) and bool(D.keep_mask(seed, 4099, 2.0 ** -18).all())


def test_keep_mask_restates_the_definition_one_element_at_a_time():
    """Python integers, no numpy: splitmix64 of (seed, i >> 2), half-word i & 3, kept when >= the threshold."""
    G, M = 0x9E3779B97F4A7C15, (1 << 64) - 1
    for seed in SEEDS:
        got = D.keep_mask(seed, 67, 0.5)
        for i in range(67):
            z = ((i >> 2) + seed * G + G) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            assert bool(got[i]) == (((z >> (16 * (i & 3))) & 0xFFFF) >= 32768), (seed, i)
    # splitmix64's published first output for state 0 (seed 0, counter 0 here: z = G)
    assert int(D.hash64(0, np.zeros(1, dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_keep_mask_depends_on_seed_and_index_only():
    for seed in SEEDS:
        long, short = D.keep_mask(seed, 10007, 0.25), D.keep_mask(seed, 1001, 0.25)
        assert np.array_equal(long[:1001], short)
    masks = [D.keep_mask(seed, 4096, 0.5) for seed in SEEDS + (1, 2)]
    for a in range(len(masks)):
        for b in range(a + 1, len(masks)):
            # independent fair bits agree on 2048 +- 32 of 4096 positions: 8 sigma is 256
            assert abs(int((masks[a] == masks[b]).sum()) - 2048) < 256, (a, b)


@pytest.mark.parametrize("p", [0.05, 0.25, 0.5, 0.9])
def test_keep_fraction_of_the_reference_mask(p):
    n = 1 << 20
    for seed in SEEDS:
        frac = float(D.keep_mask(seed, n, p).mean())
        assert abs(frac - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n), (seed, p, frac)


def test_dropout_references_scale_and_candidates():
    x, y = _bf(4096, seed=1) + 3.0, _bf(4096, seed=2)
    p, seed = 0.3, 77
    keep = torch.from_numpy(D.keep_mask(seed, 4096, p))
    d = D.dropout(x, p, seed)
    assert d.dtype == BF16 and bool((d[~keep] == 0).all()) and not bool(torch.signbit(d[~keep]).any())
    want = x.double() / (1 - float(np.float32(p)))
    assert bool(((d.double() - want).abs()[keep] <= 2.0 ** -8 * want.abs()[keep]).all())
    ref, alt = D.dropout_add(x, y, p, seed)
    assert torch.equal(ref[~keep], y[~keep]) and torch.equal(alt[~keep], y[~keep])
    both = want + y.double()
    for c in (ref, alt):
        assert bool(((c.double() - both).abs()[keep] <= 2.0 ** -8 * (want.abs() + y.double().abs())[keep]).all())
    assert bool(((ref.double() - alt.double()).abs() <= D.ulp_bf16(ref.double())).all())          # neighbours at most
    assert torch.equal(D.dropout(x, 0.0, seed), x)


# ------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("gscale", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adamw_reference_is_torch_adamw(wd, gscale):
    from oracle import llava_oracle as O
    n, lr, b1, b2, eps = 257, 1e-3, 0.9, 0.999, 1e-8
    p0 = (_bf(n, std=0.02, seed=3).float() * 1.0001)
    par = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    master, m, v = p0.double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    op, om, ov = p0.double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 4):
        g = _bf(n, std=0.01, seed=10 + step)
        gs = 1.0 if gscale is None else gscale
        par.grad = g.double() * gs
        opt.step()
        master, m, v, A_p, A_m, A_v = D.adamw_step(master, m, v, g, lr, b1, b2, eps, wd, step, gscale=gscale, abi_fp32=False)
        O.adamw_step(op, g.double() * gs, om, ov, step, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd)
        assert float((master - par.detach()).abs().max()) <= 1e-14 and float((master - op).abs().max()) <= 1e-14
        assert float((m - om).abs().max()) <= 1e-16 and float((v - ov).abs().max()) <= 1e-18
        st = opt.state[par]
        assert float((m - st["exp_avg"]).abs().max()) <= 1e-16 and float((v - st["exp_avg_sq"]).abs().max()) <= 1e-18
        assert bool((m.abs() <= A_m * (1 + 1e-12)).all()) and torch.equal(A_v, v) and bool((master.abs() <= A_p * (1 + 1e-12)).all())
    # with the hyperparameters rounded to fp32 as the C ABI takes them, the same step moves by the rounding of its inputs and no more:
    # 1 - fp32(0.999) is 1.3e-5 (relative) away from 0.001, and v carries that
    g = _bf(n, std=0.01, seed=20)
    a = D.adamw_step(master, m, v, g, lr, b1, b2, eps, wd, 4, gscale=gscale, abi_fp32=False)
    b = D.adamw_step(master, m, v, g, lr, b1, b2, eps, wd, 4, gscale=gscale)
    for x, y, A, rel in ((a[0], b[0], a[3], 2e-5), (a[1], b[1], a[4], 1e-6), (a[2], b[2], a[5], 2e-5)):
        assert float(((x - y).abs() / A.clamp_min(1e-300)).max()) <= rel
    assert float(((a[2] - b[2]).abs() / a[5]).max()) > 1e-7            # and it is not a no-op


def test_adamw_reference_extremes():
    """Zero gradient: only the weight decay moves the parameter.  A gradient far below eps: the step is (lr / bc1) m / eps."""
    z = torch.zeros(4, dtype=torch.float64)
    p0 = torch.tensor([1.0, -2.0, 0.5, 0.0], dtype=torch.float64)
    p, m, v, *_ = D.adamw_step(p0, z, z, torch.zeros(4, dtype=BF16), 0.25, 0.5, 0.75, 2.0 ** -20, 0.5, 1)
    assert torch.equal(p, p0 * (1 - 0.125)) and torch.equal(m, z) and torch.equal(v, z)
    g = torch.full((4,), 2.0 ** -70, dtype=BF16)
    p, m, v, *_ = D.adamw_step(z, z, z, g, 0.25, 0.5, 0.75, 2.0 ** -20, 0.0, 1)
    want = -(0.25 / 0.5) * (0.5 * 2.0 ** -70) / (2.0 ** -70 + 2.0 ** -20)           # sqrt(v / bc2) = |g| at step 1
    assert float((p - want).abs().max()) <= 1e-12 * abs(want)
    assert float((p + 0.25 * 2.0 ** -70 / 2.0 ** -20).abs().max()) <= 2.0 ** -49 * 2.0 ** -52      # m / eps-sized, to 2^-50 relative


# ------------------------------------------------------------------------------------------------ max over four rows
def test_max4_reference_is_max_pool2d_with_ties_and_a_nan():
    h, w, d = 4, 6, 5
    grid = torch.randint(-3, 4, (d, h, w), generator=torch.Generator().manual_seed(4)).double()          # small integers: many ties
    grid[0, 0, 1] = float("nan")
    grid[1, 2:4, 2:4] = 2.0                                                                              # a four-way tie
    src = grid.permute(1, 2, 0).reshape(h * w, d).to(BF16)                                                # row y * w + x
    idx4 = torch.tensor([[(2 * py) * w + 2 * px, (2 * py) * w + 2 * px + 1, (2 * py + 1) * w + 2 * px, (2 * py + 1) * w + 2 * px + 1]
                         for py in range(h // 2) for px in range(w // 2)])
    gr = grid.clone().requires_grad_(True)
    want, flat = F.max_pool2d(gr[None], 2, return_indices=True)
    out, which = D.max4_fwd(src, idx4)
    want_rows = want[0].detach().permute(1, 2, 0).reshape(-1, d)
    assert torch.equal(torch.nan_to_num(out.double(), nan=1e9), torch.nan_to_num(want_rows, nan=1e9))
    flat_rows = flat[0].permute(1, 2, 0).reshape(-1, d)                                                  # index y * w + x into the plane
    assert torch.equal(torch.stack([idx4[s][which[s].long()] for s in range(idx4.shape[0])]), flat_rows)
    assert int(which[0, 0]) == 1 and bool(torch.isnan(out[0, 0]))                                        # the NaN wins its window
    gout = _bf(idx4.shape[0], d, seed=5)
    want[0].backward(gout.double().reshape(h // 2, w // 2, d).permute(2, 0, 1))
    dsrc = D.max4_bwd(gout, idx4, range(idx4.shape[0]), which, torch.full((h * w, d), 7.0, dtype=BF16))
    assert torch.equal(dsrc.double(), gr.grad.permute(1, 2, 0).reshape(h * w, d))


def test_max4_reference_scan_rule_on_planted_columns():
    nan, inf = float("nan"), float("inf")
    cols = [(1, 1, 0, 0), (0, 1, 1, 1), (2, 2, 2, 2), (0.0, -0.0, -1, -1), (-0.0, 0.0, -1, -1), (-inf, -inf, -inf, -inf),
            (nan, 5, 6, 7), (5, nan, 6, 7), (5, 6, nan, 7), (5, 6, 7, nan), (nan, 5, nan, 9), (3, nan, 9, nan)]
    src = torch.tensor(cols).t().contiguous().to(BF16)                                                   # [4 rows, 12 columns]
    out, which = D.max4_fwd(src, [[0, 1, 2, 3]])
    assert which[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 2, 3, 2, 3]
    assert out[0, :3].tolist() == [1, 1, 2] and float(out[0, 5]) == -inf and bool(torch.isnan(out[0, 6:]).all())
    assert not bool(torch.signbit(out[0, 3])) and bool(torch.signbit(out[0, 4]))                         # +0 == -0: the first one stays


# ------------------------------------------------------------------------------------------------ segment sum, im2col, transpose
def test_weighted_segment_sum_reference_is_bilinear_interpolation():
    from radvlm_amd.splice import bilinear_taps
    h, w, oh, ow, d = 9, 7, 6, 5, 8
    src = _bf(h * w, d, seed=6)
    idx, wt = bilinear_taps(h, w, oh, ow)
    n = oh * ow
    out, A, J = D.segment_sum(src, np.arange(0, 4 * n + 1, 4), idx.reshape(-1), wt.reshape(-1))
    want = F.interpolate(src.double().view(h, w, d).permute(2, 0, 1)[None], [oh, ow], mode="bilinear")[0].permute(1, 2, 0).reshape(n, d)
    # the taps are fp32 (source coordinates and weights): 2^-20 of the magnitude, against float64 interpolation
    assert bool(((out - want).abs() <= 2.0 ** -20 * A + 1e-300).all()) and bool((J == 4).all())
    assert bool((out.abs() <= A * (1 + 1e-12)).all())
    o2, A2, J2 = D.segment_sum(src, [0, 0, 1, 3], [5, 2, 2])                                             # empty, one row, a repeated row
    assert J2.tolist() == [0, 1, 2] and float(o2[0].abs().max()) == 0.0 and torch.equal(o2[1], src[5].double())
    assert torch.equal(o2[2], 2 * src[2].double()) and torch.equal(A2[2], 2 * src[2].double().abs())


def test_im2col_reference_is_conv2d_on_a_non_square_image():
    n, H, W, p, d = 2, 10, 16, 4, 6
    pix, wgt = _bf(n, 3, H + 1, W + 2, seed=7), _bf(d, 3, p, p, seed=8)                                  # trailing pixels past a whole patch
    kp = 3 * p * p + 8
    cols = D.im2col(pix, p, kp)
    assert cols.shape == (n * (H // p) * (W // p), kp) and float(cols[:, 3 * p * p:].float().abs().max()) == 0.0
    got = cols[:, :3 * p * p].double() @ wgt.double().view(d, -1).t()
    want = F.conv2d(pix.double(), wgt.double(), stride=p).flatten(2).transpose(1, 2).reshape(-1, d)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_transpose_reference_follows_the_stated_index_rule():
    B, S, H, hd, s_pad = 2, 50, 3, 8, 64
    x = _bf(B * S, H * hd, seed=9)
    ref = x.view(B, S, H, hd).permute(0, 2, 3, 1)
    t = D.transpose(x, s_pad, B=B, H=H)
    assert torch.equal(t[..., :S], ref) and float(t[..., S:].float().abs().max()) == 0.0
    full = torch.zeros(B, H, hd, s_pad, dtype=BF16)
    full[..., :S] = ref
    src = torch.tensor([(pos // 32) * 32 + 16 * ((pos % 8) // 4) + 4 * ((pos % 32) // 8) + pos % 4 for pos in range(s_pad)])
    assert torch.equal(D.transpose(x, s_pad, perm32=True, B=B, H=H), full[..., src])
    assert sorted(D.perm32_source(128).tolist()) == list(range(128))                                     # a permutation, group by group
    assert all(a // 32 == i // 32 for i, a in enumerate(D.perm32_source(128).tolist()))
    # plain form and the packed form
    y = _bf(5, 3, seed=10)
    assert torch.equal(D.transpose(y, 8)[0, 0, :, :5], y.t()) and D.transpose(y, 8).shape == (1, 1, 3, 8)
    cu = [0, 0, 2, 5]
    v = D.transpose(y, 8, cu=cu, B=3)
    assert float(v[0].float().abs().max()) == 0.0 and torch.equal(v[1, 0, :, :2], y[0:2].t()) and torch.equal(v[2, 0, :, :3], y[2:5].t())
    assert float(v[1, 0, :, 2:].float().abs().max()) == 0.0


@pytest.mark.parametrize("kind", ["clip", "siglip"])
def test_normalize_reference_is_the_host_processor(kind):
    from PIL import Image
    from radvlm_amd.llava.mm_utils import ClipImageProcessor, SigLipImageProcessor
    tile = 16
    proc = ClipImageProcessor(tile) if kind == "clip" else SigLipImageProcessor(size=(tile, tile), crop_size={"height": tile, "width": tile})
    vals = np.arange(256, dtype=np.uint8).reshape(tile, tile)
    canvas = np.stack([vals, vals[::-1], vals.T], axis=-1)                                               # all 256 byte values in every channel
    want = proc.preprocess(Image.fromarray(canvas))["pixel_values"][0].to(BF16)
    factor = getattr(proc, "rescale_factor", 1.0 / 255)
    got = D.normalize_tiles(canvas[None], tile, proc.image_mean, proc.image_std, proc.normalize_mode, factor, 1, 1)
    assert got.shape == (1, 3, tile, tile) and torch.equal(got[0], want)
    # the tile grid is row-major and each tile keeps its own rows and columns
    big = np.random.default_rng(0).integers(0, 256, size=(2, 2 * tile, 3 * tile, 3), dtype=np.uint8)
    tiles = D.normalize_tiles(big, tile, proc.image_mean, proc.image_std, proc.normalize_mode, factor, 2, 3)
    for im in range(2):
        for ty in range(2):
            for tx in range(3):
                one = D.normalize_tiles(big[im:im + 1, ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile], tile, proc.image_mean,
                                        proc.image_std, proc.normalize_mode, factor, 1, 1)
                assert torch.equal(tiles[(im * 2 + ty) * 3 + tx], one[0])


def test_gather_and_embedding_references():
    ta, tb = _bf(5, 16, seed=11), _bf(3, 16, seed=12)
    out = D.gather_rows([4, -1, -2, 0, -4, 4], 8, ta, tb)
    assert torch.equal(out, torch.stack([ta[4, :8], torch.zeros(8, dtype=BF16), tb[0, :8], ta[0, :8], tb[2, :8], ta[4, :8]]))
    n, P, d = 2, 3, 8
    po, cls, pos = _bf(n * P, d, seed=13), _bf(d, seed=14), _bf(P + 1, d, seed=15)
    e = D.clip_embed(po, cls, pos, n, P).view(n, P + 1, d)
    assert torch.equal(e[1, 0], (cls.float() + pos[0].float()).to(BF16)) and torch.equal(e[1, 2], (po[P + 1].float() + pos[2].float()).to(BF16))
    a = D.add_pos(po, pos[:P], n, P)
    assert torch.equal(a[P + 2], (po[P + 2].float() + pos[2].float()).to(BF16))

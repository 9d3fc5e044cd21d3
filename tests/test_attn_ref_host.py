"""CPU checks of tests/attn_ref.py: the float64 reference equals float64 autograd of oracle.llava_oracle.attention to 1e-12, a CPU
emulation of the natural-layout kernels' rounding points stays inside the per-element gates on every input family, and the stress
families do trigger the forward's deferred softmax rescale after the first key tile -- so a failure of
tests/test_attention_edges_gpu.py points at a kernel, not at the reference, the gates or the inputs."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_ref as R


def _eq(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


def _oracle_f64(q, k, v, dout, lens, causal):
    """float64 autograd of oracle.llava_oracle.attention on [b, h, n, hd] tensors.  The oracle asks F.softmax for fp32 whatever its input
    (the model's softmax_fp32), which would pin the reference to 1e-7 only: the dtype request is dropped here, nothing else changes."""
    from oracle import llava_oracle as O
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    soft = F.softmax
    with mock.patch.object(O.F, "softmax", lambda s, dim, dtype=None: soft(s, dim=dim)):
        out = O.attention(q, k, v, lens=lens, causal=causal)
    assert out.dtype == torch.float64
    out.backward(dout)
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,S,H,Hkv,hd,causal,lens,packed", [
    (2, 70, 2, 2, 64, True, None, False),
    (2, 70, 2, 2, 128, False, None, False),
    (2, 75, 3, 3, 64, True, [75, 33], False),
    (2, 75, 2, 2, 128, False, [1, 64], False),
    (3, 70, 2, 2, 64, True, [70, 1, 33], True),
    (2, 66, 4, 2, 128, True, [66, 20], False),
    (2, 66, 6, 1, 64, False, [66, 40], True),
])
def test_reference_is_float64_autograd_of_the_oracle(B, S, H, Hkv, hd, causal, lens, packed):
    cu = np.concatenate([[0], np.cumsum(lens)]) if packed else None
    pos = R.positions(B, S, cu)
    q, k, v, dout = R.make_inputs("rand", pos, H, Hkv, hd, seed=B + S)
    if lens is not None and not packed:
        for b, L in enumerate(lens):
            dout.view(B, S, -1)[b, L:] = 0
    ref = R.reference(q, k, v, dout, B, S, H, Hkv, hd, causal, lens=None if packed else lens, cu=cu)
    rep = H // Hkv
    for b, (r0, n) in enumerate(R.sample_rows(B, S, cu)):
        hq = lambda t: t[r0:r0 + n].double().view(1, n, H, hd).transpose(1, 2)
        hk = lambda t: t[r0:r0 + n].double().view(1, n, Hkv, hd).transpose(1, 2)
        L = None if (packed or lens is None) else [lens[b]]
        o, gq, gk, gv = _oracle_f64(hq(q), hk(k).repeat_interleave(rep, 1), hk(v).repeat_interleave(rep, 1), hq(dout), L, causal)
        back = lambda t, heads: t[r0:r0 + n].view(1, n, heads, hd).transpose(1, 2)
        fold = lambda g: g.view(1, Hkv, rep, n, hd).sum(2)
        _eq(back(ref["out"], H), o)
        _eq(back(ref["dq"], H), gq)
        _eq(back(ref["dk"], Hkv), fold(gk))
        _eq(back(ref["dv"], Hkv), fold(gv))
        nv = n if L is None else L[0]
        assert bool(ref["valid"][r0:r0 + nv].all()) and not bool(ref["valid"][r0 + nv:r0 + n].any())
        if L is not None:                      # rows of a padded sample beyond its length: zero dout there gives exactly zero gradients
            for name, heads in (("dq", H), ("dk", Hkv), ("dv", Hkv)):
                assert float(back(ref[name], heads)[:, :, nv:].abs().max()) == 0.0 if nv < n else True
    # lse against logsumexp of the masked scores of one (sample, head)
    r0, n = R.sample_rows(B, S, cu)[-1]
    L = n if (packed or lens is None) else lens[-1]
    s = (q[r0:r0 + n, -hd:].double() @ k[r0:r0 + n, -hd:].double().T) / hd ** 0.5
    s = s.masked_fill(~R._mask(n, L, causal), float("-inf"))
    _eq(ref["lse"][-1, -1, :n], torch.logsumexp(s, -1))
    # the budgets bound the references (every term replaced by its absolute value)
    for name in ("out", "dq", "dk", "dv"):
        assert bool((ref[name].abs() <= ref["A_" + name] * (1 + 1e-12) + 1e-300).all()), name


def test_the_gate_bites_where_the_whole_tensor_metric_does_not():
    """One query row wrong by 10 % of its own magnitude, small next to the tensor's maximum: max|d| / max|ref| passes, the budget does not."""
    B, S, H, hd = 1, 70, 2, 64
    q, k, v, dout = R.make_inputs("rand", R.positions(B, S), H, H, hd)
    v = (v.double() * torch.where(torch.arange(S) < 8, 1.0, 2.0 ** -8)[:, None]).to(R.BF16)       # causal rows near the top are large
    ref = R.reference(q, k, v, dout, B, S, H, H, hd, True)
    got = R.rbf(ref["out"])
    assert R.assert_within_budget(got, ref["out"], ref["A_out"], 2) <= 0.5
    got[60] *= 1.1
    assert float((got - ref["out"]).abs().max() / ref["out"].abs().max()) < 2.0 ** -7
    with pytest.raises(AssertionError):
        R.assert_within_budget(got, ref["out"], ref["A_out"], 2)
    with pytest.raises(AssertionError):
        R.assert_within_budget(torch.full_like(got, float("nan")), ref["out"], ref["A_out"], 2)
    with pytest.raises(AssertionError):
        R.assert_lse_close(ref["lse"] + 2e-4 * ref["lse"].abs().clamp_min(1.0), ref["lse"])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_of_the_natural_kernels_stays_inside_the_gates(family, hd, causal):
    B, S, H = 1, 320, 2
    q, k, v, dout = R.make_inputs(family, R.positions(B, S), H, H, hd)
    ref = R.reference(q, k, v, dout, B, S, H, H, hd, causal)
    emu = R.emulate_natural(q, k, v, dout, B, S, H, H, hd, causal)
    worst = {n: R.assert_within_budget(emu[n], ref[n], ref["A_" + n], 2, f"{family} {n}") for n in ("out", "dq", "dk", "dv")}
    worst["lse"] = R.assert_lse_close(emu["lse"], ref["lse"], family)
    print(family, hd, causal, {n: round(w, 3) for n, w in worst.items()}, "rescales", emu["rescales"])
    if family in R.STRESS:
        assert emu["rescales"] > 0


def test_emulation_with_key_padding_and_grouped_heads():
    B, S, H, Hkv, hd, lens = 2, 200, 4, 2, 128, [65, 199]
    for family in ("rand", "stair"):
        for causal in (True, False):
            q, k, v, dout = R.make_inputs(family, R.positions(B, S), H, Hkv, hd)
            for b, L in enumerate(lens):
                dout.view(B, S, -1)[b, L:] = 0
            ref = R.reference(q, k, v, dout, B, S, H, Hkv, hd, causal, lens=lens)
            emu = R.emulate_natural(q, k, v, dout, B, S, H, Hkv, hd, causal, lens=lens)
            ok = ref["valid"]
            for n in ("out", "dq", "dk", "dv"):
                R.assert_within_budget(emu[n][ok], ref[n][ok], ref["A_" + n][ok], 2, f"{family} {n}")
                if n != "out":
                    assert float(emu[n][~ok].abs().max()) == 0.0


# (S, B) of the stress cases tests/test_attention_edges_gpu.py runs: the rescale cases, the paired-form case and the grouped-query cases
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("S", [320, 300, 257, 129])
@pytest.mark.parametrize("family", R.STRESS)
def test_stress_families_trigger_the_deferred_rescale(family, S, hd, causal):
    """From the float64 scores: in every 32-row wave that walks at least two key tiles, some later tile exceeds
    ceil(maximum of the earlier tiles) + 8, so the kernel's rescale branch must run there with alpha != 0.  stair7 is built so that its
    FIRST step stays inside the lag: there the statement holds for waves with at least three key tiles, and no row may leave the lag in
    tile 1 (both read off the same walk with the kernel's bookkeeping of the stored maximum)."""
    B, H = 2, 2
    q, k, v, dout = R.make_inputs(family, R.positions(B, S), H, H, hd)
    ref = R.reference(q, k, v, dout, B, S, H, H, hd, causal, keep_scores=True)
    seen = 0
    for b in range(B):
        for h in range(H):
            for q0, ntiles, must, fires in R.rescale_events(ref["scores2"][b][h], causal):
                if family == "mixed" and min(q0 + 32, S) - q0 <= min(R.MIXED_ROWS):
                    continue                                        # a last wave too short to hold one of the rising rows
                if family == "stair7":
                    assert not any(fires[:1]), (b, h, q0, fires)
                    if ntiles >= 3:
                        assert fires[1], (b, h, q0, fires)
                        seen += 1
                elif ntiles >= 2:
                    assert any(must) and any(fires), (b, h, q0, must)
                    seen += 1
                    if family in ("stair", "mixed") and not causal and S % 64 == 0:
                        assert all(must), (b, h, q0, must)          # every step of the stair leaves the lag (whole tiles)
    assert seen > 0


def test_input_families_are_what_they_claim():
    hd, S = 128, 320
    for family in R.FAMILIES:
        q, k, v, dout = R.make_inputs(family, R.positions(1, S), 2, 2, hd)
        assert all(t.dtype == R.BF16 and bool(torch.isfinite(t.float()).all()) for t in (q, k, v, dout))
        assert float(v.float().abs().max()) <= 2.0 ** 40
        s2 = (q[:, :hd].double() @ k[:, :hd].double().T) * R.LOG2E / hd ** 0.5
        if family == "big":
            assert 40 <= float(s2.abs().max()) <= 70
        if family == "sink":
            assert float((s2[:, :64] + 60).abs().max()) < 2 and float(s2[:, 64:].abs().max()) < 2
        if family in ("stair", "stair7"):
            for t in range(5):
                assert float((s2[:, 64 * t:64 * t + 64] - R.STEP[family] * t).abs().max()) < 1.0, (family, t)
        if family == "mixed":
            rise = np.isin(np.arange(S) % 32, R.MIXED_ROWS)
            assert float((s2[rise][:, 256:] - 38).abs().max()) < 1.0 and float(s2[~rise].abs().max()) < 1.0

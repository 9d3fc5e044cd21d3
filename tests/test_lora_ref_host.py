"""CPU checks of tests/lora_ref.py: both references equal float64 autograd of alpha (mask o x / (1 - p)) A^T with the mask held constant,
the mask is the one of the dropout kernels over x as M K contiguous elements, the case tables cover what they claim, and the integer
constructions of tests/test_lora_kernels_edges_gpu.py are exact in fp32 -- so a failure there points at a kernel."""
import numpy as np
import pytest
import torch

import dataops_ref as D
import gemm_ref as G
import lora_ref as L


def _eq(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize("M,R,K,p,alpha,seed", [(7, 4, 64, 0.0, 2.0, 0), (33, 12, 128, 0.25, 0.5, 5), (65, 8, 72, 0.5, 1.0, (1 << 63) - 1)])
def test_references_are_float64_autograd_with_the_mask_held_constant(M, R, K, p, alpha, seed):
    gen = torch.Generator().manual_seed(M)
    x, a, dy, g0 = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((M, K), (R, K), (M, R), (R, K)))
    keep = torch.from_numpy(D.keep_mask(seed, M * K, p)).view(M, K) if p > 0 else torch.ones(M, K, dtype=torch.bool)
    p32 = float(np.float32(p))
    A = a.clone().requires_grad_(True)
    t = alpha * ((x * keep / (1.0 - p32)) @ A.t())
    t.backward(dy)
    ref_t, bound_t = L.lora_down(x, a, alpha, p, seed)
    _eq(ref_t, t.detach())
    # the kernel takes dt = alpha dy (the engine folds alpha into the upstream gradient): d/dA of sum(dy o t)
    for accumulate in (False, True):
        ref_g, bound_g = L.lora_a_grad(alpha * dy, x, g0, p, seed, accumulate)
        _eq(ref_g, A.grad + (g0 if accumulate else 0))
        assert bool((ref_g.abs() <= bound_g * (1 + 1e-12) + 1e-300).all())
    assert bool((ref_t.abs() <= bound_t * (1 + 1e-12) + 1e-300).all())
    # the mask is dataops_ref.dropout's: the same elements are zero
    if p > 0:
        xb = (x.abs() + 1).to(L.BF16)
        assert torch.equal(D.dropout(xb, p, seed) != 0, L.masked(xb, p, seed)[0] != 0)
        assert 0.5 * p < 1.0 - float(keep.double().mean()) < 1.5 * p


def test_case_tables_cover_every_listed_size():
    d = L.DOWN_CASES
    assert {c.K for c in d} == set(L.DOWN_K) and {c.M for c in d} == set(L.DOWN_M) and {c.R for c in d} == set(L.DOWN_R)
    assert any((c.M, c.R, c.K) == (1, 4, 256) for c in d) and any((c.M, c.R, c.K) == (130, 60, 256) for c in d)
    assert {c.ldt_pad for c in d} == {0, 4, 8} and {c.t_off for c in d} == {0, 4} and {c.p for c in d} == {0.0, 0.5}
    assert any(c.lda_pad for c in d) and any(c.ldx_pad for c in d)
    for c in d:
        assert c.K % 64 == 0 and c.R % 4 == 0 and c.R <= 64 and c.ldx_pad % 8 == 0 and c.lda_pad % 8 == 0 and not (c.p > 0 and c.ldx_pad)
        assert np.log2(c.alpha) == int(np.log2(c.alpha))
    g = L.AGRAD_CASES
    assert {c.R for c in g} == set(L.AGRAD_R) and {c.K for c in g} == set(L.AGRAD_K) and set(L.AGRAD_M) <= {c.M for c in g}
    assert {c.accumulate for c in g} == {0, 1} and {c.p for c in g} == {0.0, 0.5} and any(c.ldx_pad for c in g) and any(c.tight for c in g)
    for c in g:
        assert c.R % 8 == 0 and c.K % 8 == 0 and c.R <= 64 and not (c.p > 0 and c.ldx_pad)
    # slice counts the configurations reach at a budget of 8 units (and 256 for the device's own): 1, uneven, = steps, the cap of 32
    five = next(c for c in g if (c.M, c.K) == (300, 264))
    assert [L.agrad_slices(five, 8, planes) for _, planes in L.agrad_configs(five)] == [1, 2, 5]
    big = next(c for c in g if c.M == 2113)
    assert [L.agrad_slices(big, 256 if b == 0 else 8, planes) for b, planes in L.agrad_configs(big)] == [1, 2, 24, 32]
    assert -(-big.M // L.AG_BM) == 34


def test_integer_constructions_are_exact_in_fp32():
    """Every partial sum is an integer below 2^24; 1 / (1 - p) is 1 or 2 and alpha a power of two, so the scaled sum and the accumulate
    add are exact too: the only rounding left is the bf16 store."""
    assert (L.AB_MAX, L.EPI_MAX) == (G.AB_MAX, G.EPI_MAX)
    for c in L.DOWN_CASES:
        assert L.AB_MAX ** 2 * c.K * 2 * max(c.alpha, 1.0) < 2 ** 24
    for c in L.AGRAD_CASES:
        assert L.AB_MAX ** 2 * c.M * 2 + L.EPI_MAX < 2 ** 24
    for p in (0.0, 0.5):
        assert L.masked(torch.ones(2, 8), p, 0)[1] in (1.0, 2.0)

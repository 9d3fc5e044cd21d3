"""float64 reference of the LoRA one-pass kernels of radvlm_amd/csrc/gemm_bf16.hip (lora_down_kernel behind rv_lora_down_bf16,
lora_agrad_kernel + the split-K reduce behind rv_lora_a_grad_bf16), with a per-element budget for each.  numpy / torch on the CPU only;
tests/test_lora_ref_host.py pins both to float64 autograd without a GPU, tests/test_lora_kernels_edges_gpu.py holds the kernels to them.

Both kernels apply the adapter's input dropout to x [M, K] with the mask of rv_dropout_bf16 over x viewed as M K contiguous elements
(dataops_ref.keep_mask, element m K + k) and the scale 1 / (1 - p); p is taken as the fp32 number the C ABI receives.

    lora_down    t [M, R]  = alpha / (1 - p) (mask o x) a^T                      A = alpha / (1 - p) |mask o x| |a|^T
    lora_a_grad  gA [R, K] = [g0 +] 1 / (1 - p) dt^T (mask o x)                  A = 1 / (1 - p) |dt|^T |mask o x| [+ |g0|]

The products are accumulated in fp32 and an element meets ONE bf16 rounding, its store (the partial sums of lora_a_grad's token slices
stay fp32 in the workspace; the scale and the accumulate add are fp32): the gate of an element is (2^-8 + 2^-16) A + 1e-30, 2^-8 for the
store, 2^-16 for the fp32 sums and the fp32 quotient alpha / (1 - p).  With integer operands, p in {0, 0.5} and alpha a power of two
every fp32 value on the path is exact, and the stored bf16 must equal the float64 result rounded once, bit for bit."""
import collections

import numpy as np
import torch

from dataops_ref import keep_mask

BF16 = torch.bfloat16
EPS_BF16, EPS_F32, FLOOR = 2.0 ** -8, 2.0 ** -16, 1e-30


AB_MAX, EPI_MAX = 3, 8          # gemm_ref's bounds: |x|, |a|, |dt| entries <= 3, |g0| entries <= 8

# rv_lora_down_bf16, exact cases.  K / 64 = 1..4 K-tiles walk the 3-stage ring up to its first wrap; M either side of the 16 rows of a wave
# and the 64 of a block; R either side of the 16 columns of an accumulator group and at 4 and 64.  A covering set: every value of
# DOWN_K, DOWN_M, DOWN_R appears, the corners (1, 4, 256) and (130, 60, 256) included.  pads: ldx - K, lda - K (multiples of 8; ldx
# only with p = 0), ldt - R in {0, 4, 8}; t_off: elements between a 16-byte boundary and T (4: T is 8-byte but not 16-byte aligned).
DOWN_K, DOWN_M, DOWN_R = (64, 128, 192, 256), (1, 15, 17, 63, 64, 65, 130), (4, 12, 16, 20, 60, 64)
DownCase = collections.namedtuple("DownCase", "M R K p alpha ldx_pad lda_pad ldt_pad t_off")
DOWN_CASES = [
    DownCase(1, 4, 256, 0.5, 2.0, 0, 0, 0, 4),
    DownCase(130, 60, 256, 0.5, 0.5, 0, 8, 4, 0),
    DownCase(15, 12, 64, 0.0, 1.0, 8, 0, 8, 0),
    DownCase(17, 16, 128, 0.5, 4.0, 0, 16, 0, 0),
    DownCase(63, 20, 192, 0.0, 0.25, 24, 8, 4, 4),
    DownCase(64, 64, 64, 0.5, 1.0, 0, 0, 8, 4),
    DownCase(65, 64, 192, 0.0, 2.0, 0, 0, 0, 0),
    DownCase(130, 4, 128, 0.5, 0.5, 0, 0, 4, 4),
    DownCase(65, 60, 256, 0.0, 1.0, 16, 0, 4, 0),
]

# rv_lora_a_grad_bf16, exact cases.  K = 8: one partial column block; 136: a last column block of 8 columns; 264: three blocks; M: 1, either
# side of the 64 tokens of a step, 130 (3 steps), 300 (5 steps), 2113 (34 steps: uneven over the cap of 32 slices).  tight: ldt = R,
# ldg = K (otherwise both are larger, with sentinel columns); ldx_pad only with p = 0.  Every case runs at each (CU budget, workspace
# planes of R K fp32) of agrad_configs.
AGRAD_R, AGRAD_K, AGRAD_M = (8, 24, 64), (8, 128, 136, 264), (1, 63, 65, 130, 300)
AgradCase = collections.namedtuple("AgradCase", "M R K p accumulate ldx_pad tight")
AGRAD_CASES = [
    AgradCase(1, 8, 8, 0.0, 0, 8, False),
    AgradCase(63, 24, 128, 0.5, 1, 0, False),
    AgradCase(65, 64, 136, 0.5, 0, 0, True),
    AgradCase(130, 8, 264, 0.0, 1, 24, False),
    AgradCase(300, 24, 264, 0.5, 1, 0, False),
    AgradCase(300, 64, 136, 0.0, 0, 0, False),
    AgradCase(130, 64, 8, 0.5, 1, 0, False),
    AgradCase(2113, 8, 8, 0.5, 1, 0, False),
]
AG_BM, AG_BN, AG_MAX_SLICES = 64, 128, 32


def agrad_slices(case, cus, planes):
    """The token slices rv_lora_a_grad_bf16 takes (its own comment): min(ceil(3 cus / ncb), nst, 32, floor(workspace / (R K 4)))."""
    ncb, nst = -(-case.K // AG_BN), -(-case.M // AG_BM)
    return min(-(-3 * cus // ncb), nst, AG_MAX_SLICES, planes)


def agrad_configs(case):
    """[(CU budget (8, or 0 = the device's own), workspace planes)]: one slice in an exactly sized workspace; two slices (uneven when the
    steps are odd: 5 steps in 2 slices); as many slices as the budget and the steps allow in a workspace with room to spare; the big case
    also at the device's budget, where the cap of 32 binds (34 steps, uneven over 32)."""
    nst = -(-case.M // AG_BM)
    cfgs = [(8, 1)] + ([(8, 2)] if nst >= 2 else []) + [(8, 40)]
    return cfgs + ([(0, 40)] if nst > AG_MAX_SLICES else [])


def _p32(p):
    return float(np.float32(p))


def masked(x, p, seed):
    """(mask o x in float64, 1 / (1 - p)): x [M, K] with element m K + k dropped by the mask; everything kept and scale 1 for p = 0."""
    x = x.detach().cpu().double()
    if p <= 0:
        return x, 1.0
    M, K = x.shape
    keep = torch.from_numpy(keep_mask(seed, M * K, p)).view(M, K)
    return x * keep, 1.0 / (1.0 - _p32(p))


def lora_down(x, a, alpha, p, seed):
    """(t, A) float64 [M, R]."""
    xm, s = masked(x, p, seed)
    a = a.detach().cpu().double()
    return alpha * s * (xm @ a.t()), abs(alpha) * s * (xm.abs() @ a.abs().t())


def lora_a_grad(dt, x, g0, p, seed, accumulate):
    """(gA, A) float64 [R, K]; g0 is only read when `accumulate`."""
    xm, s = masked(x, p, seed)
    dt = dt.detach().cpu().double()
    g, A = s * (dt.t() @ xm), s * (dt.abs().t() @ xm.abs())
    if accumulate:
        g0 = g0.detach().cpu().double()
        g, A = g + g0, A + g0.abs()
    return g, A


def gate(A):
    return (EPS_BF16 + EPS_F32) * A.double() + FLOOR


def assert_within_gate(got, ref, A, what=""):
    """|got - ref| <= (2^-8 + 2^-16) A + 1e-30 for EVERY element; returns the worst ratio to the gate (<= 1)."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert tuple(got.shape) == tuple(ref.shape) == tuple(A.shape), (what, got.shape, ref.shape, A.shape)
    r = (got - ref).abs() / gate(A)
    r = torch.where(torch.isfinite(got) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    worst = float(r.max()) if r.numel() else 0.0
    if not worst <= 1.0:
        i = int(r.reshape(-1).argmax())
        raise AssertionError(f"{what}: flat element {i}: got {float(got.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, "
                             f"A {float(A.reshape(-1)[i])!r}, error / gate = {worst:.4g}; {int((r > 1.0).sum())} of {r.numel()} over the gate")
    return worst

"""CPU reference, input builders and the case table for the launch shapes of rv_gemm_bf16_ex (radvlm_amd/csrc/gemm_bf16.hip).  Plain
torch / numpy on the CPU; nothing here touches a GPU, so tests/test_gemm_ref_host.py can show without one that the constructions meet the
exact conditions tests/test_gemm_launch_shapes_gpu.py asserts of the kernels.

Integer-valued bf16 operands make every fp32 partial sum exact in any order, so EVERY launch shape -- whole tiles, second operand pair,
split-K + reduce, tail split + reduce, one tile per block or the persistent walk, buffer- or flat-addressed staging -- must give the
float64 result bit for bit over the whole output.  Which shape a call takes follows from the tile count and the CU budget
(rv_gemm_set_cu_budget, at least 8): with a budget of 8 the persistent walk starts at 9 tiles of 256x256, the tail split at 9 tiles and
32 K-tiles, the persistent tail split at 17 tiles.  Each row of CASES carries the plan (rv_gemm_plan) it must take under each budget it
runs at; a heuristic that moves makes the plan assertion fail instead of silently un-covering a path."""
import collections
import functools

import numpy as np
import torch

from radvlm_amd import portable_rng as prng

BF16 = torch.bfloat16
AB_MAX, EPI_MAX = 3, 8          # |A|, |B| entries <= 3; |bias|, |residual| entries <= 8
BK, TILE = 64, 256              # the K-tile and the output tile of the 256x256 kernel

# Operands and outputs are views inside larger sentinel-filled buffers: ROW_OFF rows before and ROW_PAD rows after the view, COL_OFF
# columns before and COL_PAD columns after it.  Column offsets and leading dimensions stay multiples of 8 elements (16 bytes of bf16).
ROW_OFF, ROW_PAD, COL_OFF, COL_PAD = 3, 5, 8, 16


def embed_geometry(rows, cols):
    """(buffer shape, leading dimension) of the buffer a [rows, cols] view sits in at [ROW_OFF:, COL_OFF:]."""
    ld = COL_OFF + cols + COL_PAD
    return (ROW_OFF + rows + ROW_PAD, ld), ld


def integers(seed, tag, shape, bound):
    """Seeded integers in [-bound, bound] as float64 (radvlm_amd.portable_rng.integers: random, not periodic)."""
    return torch.from_numpy(prng.integers(seed, tag, shape, -bound, bound + 1)).double()


Plan = collections.namedtuple("Plan", "kernel mode splits n_full grid buf")      # the six numbers of rv_gemm_plan

# One call of rv_gemm_bf16_ex.  budgets: {CU budget (0 = the device's own): Plan}.  epi: "plain" (alpha 1), "res" (residual, alpha 0.5)
# or "full" (bias + residual, alpha 0.5).  ws: the call has a workspace (sized exactly for its plan by the GPU test).  switches:
# rv_gemm_select_kernel codes set for the call (30 flat staging, 40 persistent off).
Case = collections.namedtuple("Case", "name M N K ta tb K2 epi ws switches budgets")


def _tiles(M, N, t=TILE):
    return -(-M // t) * -(-N // t)


def _lay(ta, tb):
    return "nt"[ta] + "nt"[tb]


def _case(kind, M, N, K, ta, tb, budgets, K2=0, epi="plain", ws=False, switches=()):
    name = f"{kind}-{M}x{N}x{K}" + (f"+{K2}" if K2 else "") + f"-{_lay(ta, tb)}-{epi}" + "".join(f"-s{s}" for s in switches)
    return Case(name, M, N, K, bool(ta), bool(tb), K2, epi, ws, tuple(switches), {b: Plan(*p) for b, p in budgets.items()})


LAYOUTS4 = [(0, 0), (0, 1), (1, 0), (1, 1)]
LAYOUTS3 = [(0, 0), (0, 1), (1, 1)]


def _build_cases():
    C = []
    # ---- MODE 0, buffer-addressed: persistent at budget 8 (9, 12, 16 tiles), at budget 13 only for 16 tiles, never at the device's budget
    for ta, tb in LAYOUTS4:                                  # 3 x 3 tiles: tiles_m not a multiple of RV_GROUP_M, 9 % 8 != 0 (xcd_remap remainder)
        for K in (64, 128, 192, 1024):                       # nt = 1 (the vmcnt(0) prologue), 2, 3 (odd), 16
            C.append(_case("whole", 744, 712, K, ta, tb, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 9, 1), 0: (2, 0, 1, 0, 9, 1)},
                           epi="full" if K in (128, 1024) else "plain"))
    for (ta, tb), epi in (((0, 0), "plain"), ((1, 1), "full")):     # 4 x 3 tiles
        C.append(_case("whole", 776, 712, 192, ta, tb, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 12, 1), 0: (2, 0, 1, 0, 12, 1)}, epi=epi))
    for (ta, tb), epi in (((0, 1), "plain"), ((1, 0), "full")):     # 6 x 2 tiles: a group of RV_GROUP_M = 4 tile rows and one of 2
        C.append(_case("whole", 1288, 504, 128, ta, tb, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 12, 1), 0: (2, 0, 1, 0, 12, 1)}, epi=epi))
    for (ta, tb), K, epi in (((0, 0), 192, "plain"), ((1, 0), 64, "full")):     # 2 x 8 tiles: every block walks two tiles at budget 8
        C.append(_case("whole", 392, 1800, K, ta, tb, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 13, 1), 0: (2, 0, 1, 0, 16, 1)}, epi=epi))
    for epi in ("plain", "full"):                            # odd M, N % 8 == 4: the element-wise epilogue
        C.append(_case("whole", 741, 716, 128, 0, 0, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 9, 1), 0: (2, 0, 1, 0, 9, 1)}, epi=epi))
    # persistent off (what the engine selects beside collectives): one tile per block at any budget, still buffer-addressed
    C.append(_case("whole", 744, 712, 128, 0, 0, {8: (2, 0, 1, 0, 9, 1)}, switches=(40,)))
    # ---- MODE 0, flat-addressed (never persistent): a K tail inside the rows of a row-major operand; staging switched to flat
    for (ta, tb), K in (((0, 0), 72), ((0, 1), 200), ((1, 0), 72)):
        C.append(_case("whole", 744, 712, K, ta, tb, {8: (2, 0, 1, 0, 9, 0), 0: (2, 0, 1, 0, 9, 0)}, epi="full" if K == 200 else "plain"))
    C.append(_case("whole", 744, 712, 128, 0, 0, {8: (2, 0, 1, 0, 9, 0)}, switches=(30,)))
    for M, N, K in ((16, 16, 32), (100, 200, 72)):
        C.append(_case("whole", M, N, K, 0, 0, {8: (2, 0, 1, 0, 1, 0), 0: (2, 0, 1, 0, 1, 0)}, epi="full"))
    # ---- MODE 0, buffer-addressed with a K tail: both operands contraction-major, the resource's extent ends the last K-tile
    for K, epi in ((72, "plain"), (2056, "full")):
        C.append(_case("whole", 744, 712, K, 1, 1, {8: (2, 0, 1, 0, 8, 1), 13: (2, 0, 1, 0, 9, 1), 0: (2, 0, 1, 0, 9, 1)}, epi=epi))
    # ---- MODE 1 (second operand pair): buffer-addressed only when BOTH pairs qualify; K2 = 8 / 72 put a tail into pair 2's only / last tile
    for ta, tb in LAYOUTS3:
        for K in (64, 192):                                  # nt1 = 1, 3: the `t + 2 < nt1` and `t + 2 < nt` loop seams
            for K2 in (8, 64, 72):
                buf = int(K2 % BK == 0 or (ta and tb))
                g8 = 8 if buf else 9
                C.append(_case("pair", 744, 712, K, ta, tb, {8: (2, 1, 1, 0, g8, buf), 13: (2, 1, 1, 0, 9, buf), 0: (2, 1, 1, 0, 9, buf)},
                               K2=K2, epi="full" if K2 == 64 else "res"))
    # ---- MODE 2 (split-K): the slice count comes from the budget (K = 4096: nt / 4 = 16 does not bind before the budget does)
    C.append(_case("splitk", 64, 200, 4096, 0, 0, {8: (2, 2, 8, 0, 8, 1), 13: (2, 2, 13, 0, 13, 1), 0: (2, 2, 16, 0, 16, 1)}, epi="full", ws=True))
    C.append(_case("splitk", 64, 264, 4096, 1, 1, {8: (2, 2, 4, 0, 8, 1), 13: (2, 2, 6, 0, 12, 1), 0: (2, 2, 16, 0, 32, 1)}, epi="full", ws=True))
    # nt = 17, 18, 19 over 4 slices (uneven); 3 tiles are too many for split-K at budget 8 (tiles <= budget / 4): whole tiles there
    for (ta, tb), K in (((0, 0), 1088), ((0, 1), 1152), ((1, 1), 1216)):
        C.append(_case("splitk", 64, 520, K, ta, tb, {8: (2, 0, 1, 0, 3, 1), 13: (2, 2, 4, 0, 12, 1), 0: (2, 2, 4, 0, 12, 1)}, epi="full", ws=True))
    C.append(_case("splitk", 64, 264, 1088, 0, 1, {8: (2, 2, 4, 0, 8, 1)}, epi="full", ws=True))
    for ta, tb in ((1, 1), (0, 0)):                          # a K tail (nt = 18, the last tile holds 8): buffer-addressed and flat
        C.append(_case("splitk", 64, 520, 1096, ta, tb, {13: (2, 2, 4, 0, 12, ta), 0: (2, 2, 4, 0, 12, ta)}, epi="full", ws=True))
    # ---- MODE 3 (tail split), one tile per block: budget 8, 9 to 12 tiles = 8 whole + rem 1..4 tail tiles in 4, 4, 2, 2 K-slices
    for ta, tb in LAYOUTS3:
        for K in (2048, 2112, 2056):                         # nt = 32, 33 (uneven slices), 33 with a tail of 8
            buf = int(K % BK == 0 or (ta and tb))
            C.append(_case("tail", 744, 712, K, ta, tb, {8: (2, 3, 4, 8, 12, buf)}, epi="full", ws=True))
    C.append(_case("tail", 392, 1160, 2112, 0, 1, {8: (2, 3, 4, 8, 16, 1)}, epi="full", ws=True))
    C.append(_case("tail", 200, 2720, 2048, 1, 1, {8: (2, 3, 2, 8, 14, 1)}, epi="full", ws=True))
    C.append(_case("tail", 776, 712, 2048, 0, 0, {8: (2, 3, 2, 8, 16, 1)}, epi="plain", ws=True))
    C.append(_case("tail", 776, 712, 2056, 0, 0, {8: (2, 3, 2, 8, 16, 0)}, epi="full", ws=True))
    # ---- MODE 3 with more whole tiles than the budget: 8 persistent blocks walk the 16 whole tiles, the K-slice blocks follow them
    C.append(_case("tail", 200, 4104, 2048, 0, 0, {8: (2, 3, 4, 16, 12, 1)}, epi="full", ws=True))
    C.append(_case("tail", 200, 4104, 2048, 0, 0, {8: (2, 3, 4, 16, 20, 1)}, epi="full", ws=True, switches=(40,)))
    C.append(_case("tail", 200, 4104, 2056, 0, 0, {8: (2, 3, 4, 16, 20, 0)}, epi="full", ws=True))
    C.append(_case("tail", 1000, 1160, 2048, 0, 1, {8: (2, 3, 2, 16, 16, 1)}, epi="full", ws=True))
    C.append(_case("tail", 1000, 1160, 2048, 0, 1, {8: (2, 3, 2, 16, 24, 1)}, epi="plain", ws=True, switches=(40,)))
    C.append(_case("tail", 1000, 1160, 2112, 1, 1, {8: (2, 3, 2, 16, 16, 1)}, epi="full", ws=True))
    # ---- the 128x128 kernel (plain row-major form only)
    for M, N, K, epi in ((744, 712, 64, "plain"), (744, 712, 72, "full"), (744, 712, 192, "plain"), (741, 716, 128, "full"), (16, 16, 32, "full"),
                         (100, 200, 72, "plain")):
        g = _tiles(M, N, 128)
        C.append(_case("k128", M, N, K, 0, 0, {8: (1, 0, 1, 0, g, 0), 0: (1, 0, 1, 0, g, 0)}, epi=epi))
    return C


CASES = _build_cases()


def persistent(case, plan):
    """A launch is persistent when it has fewer blocks than whole tiles + K-slice blocks."""
    tiles = _tiles(case.M, case.N)
    if plan.mode == 3:
        return plan.grid < plan.n_full + (tiles - plan.n_full) * plan.splits
    return plan.mode in (0, 1) and plan.kernel == 2 and plan.grid < tiles


def workspace_bytes(case, plan):
    """The smallest workspace with which the call takes `plan` (0: none)."""
    if plan.mode == 2:
        return plan.splits * case.M * case.N * 4
    if plan.mode == 3:
        return (_tiles(case.M, case.N) - plan.n_full) * plan.splits * TILE * TILE * 4
    return 0


BUDGETS = {8: (8, 0), 13: (16, 3)}          # rv_gemm_set_cu_budget(total, reserved) for a row's budget; 0 is the device's own
PLAIN, DROPOUT, FUSED = 0, 1, 2             # the call kinds of rv_gemm_plan


def plan_args(case, ws_bytes=0, kind=PLAIN):
    """The arguments of rv_gemm_plan before `out` for a case whose operands are embedded by embed_geometry (what the GPU test runs)."""
    c = case
    ld = lambda k, rows, tr: embed_geometry(k, rows)[1] if tr else embed_geometry(rows, k)[1]
    return (c.M, c.N, c.K, int(c.ta), int(c.tb), ld(c.K, c.M, c.ta), ld(c.K, c.N, c.tb), c.K2, ld(c.K2, c.M, c.ta) if c.K2 else 0,
            ld(c.K2, c.N, c.tb) if c.K2 else 0, ws_bytes, kind)


def alpha_of(case):
    return 1.0 if case.epi == "plain" else 0.5


@functools.lru_cache(maxsize=None)
def operands(name):
    """The case's operands as float64 tensors holding integers, in their STORED layouts: a [K, M] if ta else [M, K], b [K, N] if tb else
    [N, K], a2 / b2 likewise over K2 (None without a second pair), bias [N] / residual [M, N] (None unless the epilogue has them)."""
    c = BY_NAME[name]
    seed = prng.name_tag(name)
    a = integers(seed, 1, (c.K, c.M) if c.ta else (c.M, c.K), AB_MAX)
    b = integers(seed, 2, (c.K, c.N) if c.tb else (c.N, c.K), AB_MAX)
    a2 = integers(seed, 3, (c.K2, c.M) if c.ta else (c.M, c.K2), AB_MAX) if c.K2 else None
    b2 = integers(seed, 4, (c.K2, c.N) if c.tb else (c.N, c.K2), AB_MAX) if c.K2 else None
    bias = integers(seed, 5, (c.N,), EPI_MAX) if c.epi == "full" else None
    res = integers(seed, 6, (c.M, c.N), EPI_MAX) if c.epi in ("full", "res") else None
    return a, b, a2, b2, bias, res


def gemm_ref64(a, b, ta, tb, a2=None, b2=None, bias=None, residual=None, alpha=1.0):
    """float64 alpha * (op(a) op(b)^T + op(a2) op(b2)^T) + bias + residual on the stored layouts of `operands`."""
    op = lambda t, tr: t.double().t() if tr else t.double()
    y = op(a, ta) @ op(b, tb).t()
    if a2 is not None:
        y = y + op(a2, ta) @ op(b2, tb).t()
    y = alpha * y
    if bias is not None:
        y = y + bias.double()
    if residual is not None:
        y = y + residual.double()
    return y


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's exact result in float64 (computed once, shared by every budget and output type; do not modify)."""
    c = BY_NAME[name]
    a, b, a2, b2, bias, res = operands(name)
    return gemm_ref64(a, b, c.ta, c.tb, a2, b2, bias, res, alpha_of(c))


BY_NAME = {c.name: c for c in CASES}

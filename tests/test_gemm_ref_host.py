"""CPU checks of tests/gemm_ref.py: the operands, the float64 reference and the case table alone meet the conditions under which
tests/test_gemm_launch_shapes_gpu.py may demand bit-exact results of every launch shape of rv_gemm_bf16_ex, so a failure there points at
a kernel or at the planner -- and the planner itself, through the real library: rv_gemm_plan is integer arithmetic over sizes and
switches, so with an explicit budget (rv_gemm_set_cu_budget(total > 0, ...)) the whole case table is checked here, without a device."""
import ctypes
import os
import subprocess
import sys
import textwrap

import numpy as np
import torch

import gemm_ref as G
from gemm_ref import AB_MAX, BF16, BK, CASES, EPI_MAX, TILE


def test_every_partial_sum_of_every_case_is_exact_in_fp32():
    """|a b| <= 9 per product, so any partial sum over any subset of the K + K2 products is an integer of magnitude <= 9 (K + K2); alpha
    (1 or 0.5) keeps it a multiple of 0.5, bias and residual add at most 16.  Below 2^24 / 2 every such value is an fp32 number, so the
    order of the sums (K-tile order, slices, the reduce kernels) cannot show."""
    assert len(set(c.name for c in CASES)) == len(CASES)
    for c in CASES:
        assert AB_MAX * AB_MAX * (c.K + c.K2) + 2 * EPI_MAX < 2 ** 24, c.name
        assert 2 * (AB_MAX * AB_MAX * (c.K + c.K2) + 2 * EPI_MAX) < 2 ** 24, c.name       # in units of 0.5
        assert G.alpha_of(c) in (1.0, 0.5)


def test_operands_are_random_integers_in_range_and_bf16_holds_them():
    c = G.BY_NAME["pair-744x712x192+72-nt-res"]
    a, b, a2, b2, bias, res = G.operands(c.name)
    assert a.shape == (c.M, c.K) and b.shape == (c.K, c.N) and a2.shape == (c.M, c.K2) and b2.shape == (c.K2, c.N) and bias is None
    for t, lim in ((a, AB_MAX), (b, AB_MAX), (a2, AB_MAX), (b2, AB_MAX), (res, EPI_MAX)):
        assert torch.equal(t, t.round()) and float(t.min()) == -lim and float(t.max()) == lim
        assert torch.equal(t.to(BF16).double(), t)
        assert abs(float(t.mean())) < 0.05 * lim                                   # both signs, no bias
    # not periodic along K: no shift of a row by a K-tile or less reproduces it
    row = a[0]
    assert all(not torch.equal(row[s:], row[:-s]) for s in (1, 8, 16, 32, 64))
    full = G.BY_NAME["whole-744x712x128-nn-full"]
    assert G.operands(full.name)[4].shape == (full.N,) and float(G.operands(full.name)[4].abs().max()) == EPI_MAX


def test_float64_reference_equals_the_int64_product():
    for name in ("pair-744x712x192+72-nt-res", "whole-100x200x72-nn-full", "splitk-64x264x4096-tt-full"):
        c = G.BY_NAME[name]
        a, b, a2, b2, bias, res = G.operands(name)
        i = lambda t, tr: (t.t() if tr else t).to(torch.int64)
        y = i(a, c.ta) @ i(b, c.tb).t()
        if a2 is not None:
            y = y + i(a2, c.ta) @ i(b2, c.tb).t()
        y2 = y * (2 if c.epi == "plain" else 1)                                      # twice the result, in integers
        if bias is not None:
            y2 = y2 + 2 * bias.to(torch.int64)
        if res is not None:
            y2 = y2 + 2 * res.to(torch.int64)
        ref = G.reference(name)
        assert torch.equal(ref * 2, y2.double()), name
        assert torch.equal(ref.float().double(), ref)                               # the fp32 output loses nothing
        # one round-to-nearest-even into bf16, as the kernels' f2bf (checked against numpy's integer arithmetic on the fp32 bits)
        bits = ref.float().numpy().view(np.uint32).astype(np.uint64)
        rne = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
        assert np.array_equal(ref.to(BF16).view(torch.int16).numpy().view(np.uint16), rne), name


def test_every_case_meets_the_abi_preconditions():
    for c in CASES:
        assert c.K % 8 == 0 or (c.ta and c.tb), c.name                      # a row-major operand has K % 8 == 0
        assert not c.ta or c.M % 8 == 0, c.name
        assert not c.tb or c.N % 8 == 0, c.name
        assert c.K2 == 0 or c.K2 % 8 == 0 or (c.ta and c.tb), c.name
        assert c.K2 == 0 or not any(p.mode != 1 for p in c.budgets.values()), c.name
        for rows, cols in ((c.K, c.M) if c.ta else (c.M, c.K), (c.K, c.N) if c.tb else (c.N, c.K)):
            (R, W), ld = G.embed_geometry(rows, cols)
            assert ld % 8 == 0 and ld > cols and R > G.ROW_OFF + rows and W == ld
            assert (G.ROW_OFF * ld + G.COL_OFF) % 8 == 0                    # the view starts 16-byte aligned
        _, ldc = G.embed_geometry(c.M, c.N)
        assert ldc > c.N and (c.N % 8 != 0 or ldc % 8 == 0)                 # N % 8 == 0 keeps the vector epilogue reachable


def test_plans_are_consistent_and_cover_every_launch_shape():
    seen = set()
    for c in CASES:
        tiles = G._tiles(c.M, c.N)
        for budget, p in c.budgets.items():
            cus = budget or 256
            if p.kernel == 1:
                assert (p.mode, p.splits, p.n_full, p.buf) == (0, 1, 0, 0) and p.grid == G._tiles(c.M, c.N, 128) and not (c.ta or c.tb)
                seen.add("k128")
                continue
            assert (p.mode in (2, 3)) == bool(G.workspace_bytes(c, p)) and (p.mode in (2, 3)) <= c.ws, c.name
            if not (c.K % BK == 0 or (c.ta and c.tb)):
                assert p.buf == 0, c.name
            pers = G.persistent(c, p)
            if p.mode in (0, 1):
                assert (p.splits, p.n_full) == (1, 0) and p.grid == (min(tiles, cus) if p.buf and 40 not in c.switches else tiles), c.name
            elif p.mode == 2:
                assert p.n_full == 0 and p.grid == tiles * p.splits and tiles <= cus // 4 and 2 <= p.splits <= (c.K + BK - 1) // BK // 4, c.name
            else:
                rem = tiles - p.n_full
                assert p.n_full % cus == 0 and 0 < rem <= cus // 2 and p.splits == min(cus // rem, 4) and c.K >= 32 * BK - BK + 1, c.name
                assert p.grid == (cus if pers else p.n_full) + rem * p.splits, c.name
            assert not pers or p.buf, c.name
            seen.add((p.mode, p.buf, pers))
    # every (MODE, BUF, persistent) the 256x256 launcher can produce, and the 128x128 kernel
    want = {(0, 0, False), (0, 1, False), (0, 1, True), (1, 0, False), (1, 1, False), (1, 1, True), (2, 0, False), (2, 1, False),
            (3, 0, False), (3, 1, False), (3, 1, True), "k128"}
    assert seen == want, seen ^ want
    # both exits of the persistent walk: a launch where some blocks walk one tile more than others, and one where all walk the same number
    walks = [(G._tiles(c.M, c.N), p.grid) for c in CASES for p in c.budgets.values() if p.mode == 0 and G.persistent(c, p)]
    assert any(t % g for t, g in walks) and any(t % g == 0 for t, g in walks)
    # K-slices that do not divide the K-tiles, in both sliced modes
    for mode in (2, 3):
        assert any(((c.K + BK - 1) // BK) % p.splits for c in CASES for p in c.budgets.values() if p.mode == mode)
    assert TILE == 256


DEVICE_BUDGETS = (64, 96, 256, 304)         # a row's budget 0 is "the device's own": its plan holds from 64 compute units on


def _plan(L, case, ws_bytes, kind=G.PLAIN):
    out = (ctypes.c_int32 * 6)()
    rc = L.rv_gemm_plan(*G.plan_args(case, ws_bytes, kind), out)
    assert rc == 0, (case.name, rc)
    return G.Plan(*out)


def test_the_library_plans_every_row_of_the_table_without_a_device():
    """Every row at every budget of the row (0: at 64, 96, 256 and 304 units), under the row's forced kernel and switches: rv_gemm_plan
    gives the row's plan with the workspace gemm_ref.workspace_bytes names; one byte less, or the dropout kind, and a K-split row plans
    MODE 0."""
    from radvlm_amd import lib
    L = lib.load()
    checked = 0
    try:
        for c in CASES:
            for budget, plan in c.budgets.items():
                for total, reserved in ([G.BUDGETS[budget]] if budget else [(n, 0) for n in DEVICE_BUDGETS]):
                    assert L.rv_gemm_set_cu_budget(total, reserved) == total - reserved
                    for code in (21, 31, 41, plan.kernel) + c.switches:
                        L.rv_gemm_select_kernel(code)
                    need = G.workspace_bytes(c, plan)
                    assert _plan(L, c, need) == plan, (c.name, budget, total)
                    if need:
                        assert _plan(L, c, need - 1).mode == 0, (c.name, budget, total)
                        assert _plan(L, c, need, G.DROPOUT).mode == 0, (c.name, budget, total)
                    checked += 1
    finally:
        for code in (0, 21, 31, 41):
            L.rv_gemm_select_kernel(code)
        L.rv_gemm_set_cu_budget(0, int(os.environ.get("RV_GEMM_RESERVED_CUS", "0")))      # the device's own again, where there is a device
    assert checked == sum(1 if b else len(DEVICE_BUDGETS) for c in CASES for b in c.budgets)


def test_planning_without_a_budget_or_a_device_is_an_error_not_a_crash():
    """A fresh process whose first GEMM call is rv_gemm_plan, no budget set: where there is no device the call returns the error code
    of the failed device query and the process goes on (it used to divide by the missing budget); with a device it plans."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import ctypes, sys
        sys.path.insert(0, {root!r})
        from radvlm_amd import lib
        L = lib.load()
        out = (ctypes.c_int32 * 6)()
        rc = L.rv_gemm_plan(744, 712, 128, 0, 0, 128, 128, 0, 0, 0, 0, 0, out)
        print("RESULT", rc, L.rv_gemm_set_cu_budget(0, 0), L.rv_gemm_set_cu_budget(8, 0),
              L.rv_gemm_plan(744, 712, 128, 0, 0, 128, 128, 0, 0, 0, 0, 0, out), *out)
    """)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-800:])
    rc, device_budget, budget, rc2, *plan = (int(v) for v in p.stdout.split("RESULT")[1].split())
    assert rc == (0 if device_budget > 0 else device_budget) and (device_budget > 0 or device_budget == -2), (rc, device_budget)
    # an explicit total needs no device; 9 tiles on 8 units: 4 * 2 > 2.3 * ceil(36 / 16), the 128x128 kernel's 6 x 6 tiles
    assert budget == 8 and rc2 == 0 and G.Plan(*plan) == G.Plan(1, 0, 1, 0, 36, 0), (budget, rc2, plan)

"""GPU tests that pin EVERY launch shape of rv_gemm_bf16_ex (radvlm_amd/csrc/gemm_bf16.hip) at the smallest sizes that reach it: the
128x128 and the 256x256 kernel, MODE 0 - 3, buffer- and flat-addressed staging, one tile per block and the persistent walk, all operand
layouts, the dropout epilogue and the fused epilogues.  rv_gemm_set_cu_budget(8, 0) brings the persistent walk down to 9 tiles, the
tail split to 9 tiles x 32 K-tiles and the persistent tail split to 17 tiles; rv_gemm_plan proves which shape each call took.  Operands
are random integers (tests/gemm_ref.py; its own CPU checks: tests/test_gemm_ref_host.py), so every fp32 partial sum is exact and each
shape must equal the float64 reference bit for bit over the whole output: a tile skipped or computed twice, a K-tile mis-sliced, a
prefetch racing an epilogue or a wrong buffer extent all show.  Operands and outputs are views inside NaN-filled buffers."""
import ctypes
import os
import subprocess
import sys
import textwrap

import pytest
import torch

import gemm_ref as G
from gemm_ref import BF16, BUDGETS, CASES, COL_OFF, ROW_OFF, Plan

pytestmark = pytest.mark.gpu

WS_GUARD = 4096                             # fp32 sentinels behind an exactly sized workspace


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _lib():
    from radvlm_amd import lib
    return lib


class _Config:
    """Process-wide GEMM launch configuration for one test; reset() restores every default."""

    def __init__(self):
        self.L = _lib().load()

    def reset(self):
        budget = self.L.rv_gemm_set_cu_budget(0, int(os.environ.get("RV_GEMM_RESERVED_CUS", "0")))
        for code in (0, 21, 31, 41):
            self.L.rv_gemm_select_kernel(code)
        return budget

    def set(self, budget, kernel=0, switches=()):
        got = self.reset()
        if budget in BUDGETS:
            got = self.L.rv_gemm_set_cu_budget(*BUDGETS[budget])
            assert got == budget
        else:
            assert got >= 64, got            # the table's device-budget plans hold from 64 compute units on
        self.L.rv_gemm_select_kernel(kernel)
        for code in switches:
            self.L.rv_gemm_select_kernel(code)
        return got

    def plan(self, M, N, K, ta, tb, lda, ldb, K2=0, lda2=0, ldb2=0, ws_bytes=0, kind=G.PLAIN):
        out = (ctypes.c_int32 * 6)()
        rc = self.L.rv_gemm_plan(M, N, K, int(ta), int(tb), lda, ldb, K2, lda2, ldb2, ws_bytes, kind, out)
        assert rc == 0, rc
        return Plan(*out)


@pytest.fixture
def cfg():
    _ops()
    c = _Config()
    try:
        yield c
    finally:
        c.reset()


def _int(dtype):
    return torch.int16 if dtype == BF16 else torch.int32


def _sentinel(shape, dtype):
    """A buffer of one NaN bit pattern (bf16 0x7fc5 / fp32 0x7fc5a5a5): no kernel produces it, and a read of it as data poisons the result."""
    if dtype == BF16:
        return torch.full(shape, 0x7fc5, dtype=torch.int16, device="cuda").view(BF16)
    return torch.full(shape, 0x7fc5a5a5, dtype=torch.int32, device="cuda").view(torch.float32)


def _embed(rows, cols, dtype, data=None):
    """(buffer, view): a [rows, cols] view at [ROW_OFF:, COL_OFF:] of a sentinel buffer (row slice, column slice, ld > cols, sentinel rows
    behind the last row and sentinel columns behind the last column), holding `data` if given."""
    shape, _ = G.embed_geometry(rows, cols)
    buf = _sentinel(shape, dtype)
    view = buf[ROW_OFF:ROW_OFF + rows, COL_OFF:COL_OFF + cols]
    if data is not None:
        view.copy_(data.to(dtype))
    return buf, view


def _embed_vec(data):
    buf = _sentinel((COL_OFF + data.numel() + COL_OFF,), BF16)
    view = buf[COL_OFF:COL_OFF + data.numel()]
    view.copy_(data.to(BF16))
    return buf, view


def _untouched_outside(buf, rows, cols):
    """Every element of `buf` outside its embedded [rows, cols] view still holds the sentinel."""
    bits = buf.view(_int(buf.dtype))
    want = 0x7fc5 if buf.dtype == BF16 else 0x7fc5a5a5
    ok = bits == want
    ok[ROW_OFF:ROW_OFF + rows, COL_OFF:COL_OFF + cols] = True
    return bool(ok.all())


def _assert_exact(got, want, what):
    """torch.equal with a useful report: how many elements differ, in which 256x256 tiles, and the first of them."""
    if torch.equal(got, want):
        return
    bad = (got != want) | got.isnan()
    idx = bad.nonzero()
    tiles = sorted({(int(m) // 256, int(n) // 256) for m, n in idx[:: max(1, len(idx) // 4096)].tolist()})
    m, n = (int(v) for v in idx[0])
    raise AssertionError(f"{what}: {len(idx)} of {got.numel()} elements differ ({int(got.isnan().sum())} NaN), tiles (m, n) {tiles[:24]}, "
                         f"first [{m}, {n}] got {float(got[m, n])} want {float(want[m, n])}")


class _Operands:
    """A case's operands on the device, each a view inside a sentinel buffer, and the reference in both output types."""

    def __init__(self, case, tensors=None, ref=None):
        a, b, a2, b2, bias, res = G.operands(case.name) if tensors is None else tensors
        self.case = case
        self.keep = []                          # (buffer, view) of every embedded 2-D operand
        put = lambda t: self._put(t) if t is not None else None
        self.a, self.b, self.a2, self.b2, self.res = put(a), put(b), put(a2), put(b2), put(res)
        self.bias_buf, self.bias = _embed_vec(bias) if bias is not None else (None, None)
        ref = G.reference(case.name) if ref is None else ref
        self.ref = {torch.float32: ref.float().cuda(), BF16: ref.to(BF16).cuda()}

    def _put(self, t):
        buf, view = _embed(t.shape[0], t.shape[1], BF16, t)
        self.keep.append((buf, view))
        return view

    def operands_untouched(self):
        return all(_untouched_outside(buf, v.shape[0], v.shape[1]) for buf, v in self.keep)

    def plan(self, cfg, ws_bytes, kind=G.PLAIN):
        args = G.plan_args(self.case, ws_bytes, kind)          # the arguments the CPU test of the table plans with ...
        assert args[5:7] == (self.a.stride(0), self.b.stride(0)) and (not self.case.K2 or args[8:10] == (self.a2.stride(0), self.b2.stride(0)))
        return cfg.plan(*args)                                  # ... are those of the call run() makes

    def run(self, out_dtype, ws, alpha=None, act=0):
        """One rv_gemm_bf16_ex call into a fresh sentinel buffer; returns (buffer, view of C)."""
        c = self.case
        lib = _lib()
        cbuf, cv = _embed(c.M, c.N, out_dtype)
        ws_bytes = ws.numel() * 4 if ws is not None else 0
        lib.call("rv_gemm_bf16_ex", self.a, self.a.stride(0), self.b, self.b.stride(0), cv, cv.stride(0), self.bias, self.res,
                 self.res.stride(0) if self.res is not None else 0, c.M, c.N, c.K, int(c.ta), int(c.tb), float(G.alpha_of(c) if alpha is None else alpha),
                 act, int(out_dtype == torch.float32), 0, self.a2, self.a2.stride(0) if c.K2 else 0, self.b2, self.b2.stride(0) if c.K2 else 0, c.K2,
                 ws, ws_bytes, lib.zeros16(cv.device))
        return cbuf, cv


def _workspace(nbytes):
    """(buffer, view): an fp32 workspace of exactly nbytes (a view), NaN-filled, with WS_GUARD sentinels behind it; (None, None) for 0."""
    if not nbytes:
        return None, None
    assert nbytes % 4 == 0
    buf = _sentinel((nbytes // 4 + WS_GUARD,), torch.float32)
    return buf, buf[:nbytes // 4]


def _guard_intact(wsbuf):
    return wsbuf is None or bool((wsbuf[-WS_GUARD:].view(torch.int32) == 0x7fc5a5a5).all())


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_launch_shape_is_taken_and_exact(cfg, name):
    """For every budget of the row: rv_gemm_plan gives the row's plan (one workspace byte less: no K-split), and the fp32 and the bf16
    output equal the float64 reference bit for bit, with every sentinel around C and behind the workspace untouched.  All budgets equal
    one reference, so MODE 0 / 1 are bit-identical between the persistent walk and one tile per block."""
    c = G.BY_NAME[name]
    dev = _Operands(c)
    first = {}
    for budget, plan in c.budgets.items():
        cfg.set(budget, kernel=plan.kernel, switches=c.switches)
        need = G.workspace_bytes(c, plan)
        assert dev.plan(cfg, need) == plan, (name, budget)
        if need:
            assert dev.plan(cfg, need - 1).mode == 0, (name, budget)
            assert dev.plan(cfg, need, G.DROPOUT).mode == 0, (name, budget)     # the reduce kernels do not carry the dropout mask
        for dtype in (torch.float32, BF16):
            wsbuf, ws = _workspace(need)
            cbuf, cv = dev.run(dtype, ws)
            what = f"{name} budget {budget} {plan} {dtype}"
            _assert_exact(cv, dev.ref[dtype], what)
            assert _untouched_outside(cbuf, c.M, c.N), what
            assert _guard_intact(wsbuf), what
            assert torch.equal(first.setdefault(dtype, cv.clone()), cv), what
    assert dev.operands_untouched(), name


# rows of the table whose plan at budget 8 the random-normal and epilogue tests below reuse
_NORMAL_ROWS = ["whole-744x712x192-nn-plain", "pair-744x712x192+64-nt-full", "splitk-64x264x4096-tt-full", "tail-744x712x2112-nn-full"]


def _rnd(tag, shape, std=1.0):
    from radvlm_amd import portable_rng as prng
    return torch.from_numpy(prng.normal(23, tag, shape, std)).to(BF16)


def _relerr(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("name", _NORMAL_ROWS)
def test_random_normal_operands_per_mode(cfg, name):
    """One case per MODE with random-normal operands against the float64 product under the suite's gates (tests/test_kernels_gpu.py):
    fp32 output max|d| / max|ref| < 1e-5, bf16 output < 2^-7."""
    c = G.BY_NAME[name]
    plan = c.budgets[8]
    shapes = [t.shape if t is not None else None for t in G.operands(name)]
    a, b, a2, b2, bias, res = (_rnd(10 + i, tuple(s), (1.0, 1.0, 1.0, 1.0, 0.5, 1.0)[i]) if s is not None else None for i, s in enumerate(shapes))
    ref = G.gemm_ref64(a, b, c.ta, c.tb, a2, b2, bias, res, G.alpha_of(c))
    dev = _Operands(c, (a, b, a2, b2, bias, res), ref)
    cfg.set(8, kernel=plan.kernel)
    need = G.workspace_bytes(c, plan)
    assert dev.plan(cfg, need) == plan
    for dtype, gate in ((torch.float32, 1e-5), (BF16, 2.0 ** -7)):
        wsbuf, ws = _workspace(need)
        cbuf, cv = dev.run(dtype, ws)
        err = _relerr(cv, ref)
        print(f"{name} {dtype}: relerr {err:.3e} (gate {gate:.3e})")
        assert err < gate, (name, dtype, err)
        assert _untouched_outside(cbuf, c.M, c.N) and _guard_intact(wsbuf)


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("accumulate", [True, False])
def test_dropout_epilogue_under_the_persistent_walk(cfg, K, accumulate):
    """rv_gemm_dropout_add_bf16 with p = 0.5 (the scale 2 is exact) on integer operands: kept positions hold residual + 2 alpha A B rounded
    once, dropped positions keep C (accumulate) or become 0, the keep-mask is rv_dropout_bf16's for the same (p, seed) over M * N
    elements -- at budget 8 (9 tiles on 8 persistent blocks) and at the device's budget (one tile per block), bit-identical."""
    ops, lib = _ops(), _lib()
    M, N, p, seed, alpha = 744, 712, 0.5, 991, 0.5
    a = G.integers(41, 1, (M, K), G.AB_MAX)
    b = G.integers(41, 2, (K, N), G.AB_MAX)
    y0 = G.integers(41, 3, (M, N), G.EPI_MAX)
    prod = 2.0 * alpha * (a @ b)
    keep = ops.dropout(torch.ones(M, N, dtype=BF16, device="cuda"), p, seed) != 0
    frac = float(keep.float().mean())
    assert 0.49 < frac < 0.51, frac
    want = torch.where(keep, ((y0 if accumulate else 0) + prod).to(BF16).cuda(), (y0 if accumulate else torch.zeros_like(y0)).to(BF16).cuda())
    abuf, av = _embed(M, K, BF16, a)
    bbuf, bv = _embed(K, N, BF16, b)
    outs = []
    for budget, grid in ((8, 8), (0, 9)):
        cfg.set(budget)
        assert cfg.plan(M, N, K, 0, 1, av.stride(0), bv.stride(0), kind=G.DROPOUT) == Plan(2, 0, 1, 0, grid, 1)
        ybuf, yv = _embed(M, N, BF16, y0)
        lib.call("rv_gemm_dropout_add_bf16", av, av.stride(0), bv, bv.stride(0), yv, yv.stride(0), M, N, K, 1, alpha, p, seed, int(accumulate),
                 lib.zeros16(yv.device))
        _assert_exact(yv, want, f"dropout K {K} accumulate {accumulate} budget {budget}")
        assert _untouched_outside(ybuf, M, N)
        outs.append(yv.clone())
    assert torch.equal(outs[0], outs[1])


def _fused_plan(cfg, M, N, K, tb, lda, ldb):
    """The plan a fused entry point launches by (kernel 1: it runs the unfused sequence): gemm_kernel_256 MODE 0, buffer-addressed when the
    operands qualify, persistent when that holds and there are more tiles than the budget."""
    return cfg.plan(M, N, K, 0, tb, lda, ldb, kind=G.FUSED)


@pytest.mark.parametrize("K,hd,H,Hkv,explicit_pos", [(192, 128, 4, 1, False), (200, 128, 4, 1, True), (192, 64, 6, 3, True)])
def test_rope_epilogue_under_the_persistent_walk(cfg, K, hd, H, Hkv, explicit_pos):
    """rv_gemm_rope_bf16, 9 tiles at budget 8 (K % 64 == 0: 8 persistent buffer-addressed blocks; K = 200: flat, one tile per block):
    bit-identical to the unfused sequence on the 128x128 kernel (tied to the oracle in tests/test_kernels_gpu.py)."""
    ops = _ops()
    M, S = 744, 211
    N = (H + 2 * Hkv) * hd
    x, w, bias = _rnd(31, (M, K)).cuda(), _rnd(32, (N, K), 0.2).cuda(), _rnd(33, (N,), 0.5).cuda()
    cs = ops.rope_table(S, hd, 10000.0, "cuda")
    pos = (torch.arange(M, dtype=torch.int32) * 7 % S).cuda() if explicit_pos else None
    cfg.set(0, kernel=1)
    ref = ops.gemm_rope(x, w, cs, S, H + Hkv, hd, bias=bias, positions=pos)
    cfg.set(8, kernel=2)
    buf = int(K % 64 == 0)
    assert _fused_plan(cfg, M, N, K, 0, K, K) == Plan(2, 0, 1, 0, 8 if buf else 9, buf)
    got = ops.gemm_rope(x, w, cs, S, H + Hkv, hd, bias=bias, positions=pos)
    _assert_exact(got, ref, f"rope K {K} hd {hd}")
    cfg.set(0, kernel=2)
    _assert_exact(ops.gemm_rope(x, w, cs, S, H + Hkv, hd, bias=bias, positions=pos), ref, f"rope K {K} hd {hd}, one tile per block")


@pytest.mark.parametrize("K,d", [(256, 192), (200, 136)])
def test_swiglu_epilogues_under_the_persistent_walk(cfg, K, d):
    """rv_gemm_swiglu_fwd_bf16 (3 x 4 = 12 tiles, the last tile column half full) and rv_gemm_swiglu_bwd_bf16 (3 x 3 = 9 tiles) at budget 8,
    with a contraction that is a multiple of 64 (persistent, buffer-addressed) and one that is not (flat): bit-identical to the unfused
    sequences (tied to the oracle in tests/test_kernels_gpu.py)."""
    ops = _ops()
    M, F, Fb = 744, 448, 712
    x, wgu = _rnd(34, (M, K)).cuda(), _rnd(35, (2 * F, K), 0.1).cuda()
    dy, wd, gub = _rnd(36, (M, d)).cuda(), _rnd(37, (d, Fb), 0.1).cuda(), _rnd(38, (M, 2 * Fb)).cuda()
    cfg.set(0, kernel=1)
    gu_ref, act_ref = ops.gemm_swiglu_fwd(x, wgu, F)
    dgu_ref = ops.gemm_swiglu_bwd(dy, wd, gub, Fb)
    for budget in (8, 0):
        cfg.set(budget, kernel=2)
        buf = int(K % 64 == 0)
        assert _fused_plan(cfg, M, 2 * F, K, 0, K, K) == Plan(2, 0, 1, 0, 8 if buf and budget else 12, buf)
        gu, act = ops.gemm_swiglu_fwd(x, wgu, F)
        _assert_exact(gu, gu_ref, f"swiglu fwd gate|up K {K} budget {budget}")
        _assert_exact(act, act_ref, f"swiglu fwd act K {K} budget {budget}")
        buf = int(d % 64 == 0)
        assert _fused_plan(cfg, M, Fb, d, 1, d, Fb) == Plan(2, 0, 1, 0, 8 if buf and budget else 9, buf)
        _assert_exact(ops.gemm_swiglu_bwd(dy, wd, gub, Fb), dgu_ref, f"swiglu bwd d {d} budget {budget}")


def _swiglu_bwd_without_scratch(dy, wd, gu, dgu, F):
    """rv_gemm_swiglu_bwd_bf16 with dact_scratch = NULL: 0 exactly when the fused form runs, RV_ERR_ARG (-1) before any launch otherwise."""
    lib = _lib()
    return lib.load().rv_gemm_swiglu_bwd_bf16(dy.data_ptr(), dy.stride(0), wd.data_ptr(), wd.stride(0), gu.data_ptr(), gu.stride(0), dgu.data_ptr(),
                                              dgu.stride(0), None, 0, dy.shape[0], F, dy.shape[1], None, 0, lib.zeros16(dy.device).data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)


# (budget, M, F) -> the fused plan, or None where the round-cost rule 4 ceil(tiles256 / cus) <= 2.3 ceil(tiles128 / 2 cus) picks the 128x128 kernel
_FUSED_CELLS = {(8, 1000, 1000): Plan(2, 0, 1, 0, 8, 1),        # 16 tiles: 4 * 2 <= 2.3 * 4, 8 persistent blocks
                (13, 1000, 1000): None,                         # 4 * 2 > 2.3 * 3
                (8, 744, 712): None,                            # 9 tiles: 4 * 2 > 2.3 * 3
                (13, 744, 712): Plan(2, 0, 1, 0, 9, 1)}         # 4 * 1 <= 2.3 * 2, one tile per block


@pytest.mark.parametrize("M,F", [(1000, 1000), (744, 712)])
def test_fused_entry_points_fall_back_by_the_round_cost_rule_whatever_the_layout(cfg, M, F):
    """Under automatic kernel choice a plain call with a contraction-major operand always takes the 256x256 kernel; the fused entry points
    do not: rv_gemm_swiglu_bwd_bf16 (B contraction-major) runs fused exactly where the round-cost rule picks that kernel, and refuses a
    NULL scratch, launching nothing, where it would run the unfused sequence.  rv_gemm_plan(kind 2) says which, for nt and nn alike."""
    ops = _ops()
    d = 64
    dy, wd, gu = _rnd(51, (M, d)).cuda(), _rnd(52, (d, F), 0.1).cuda(), _rnd(53, (M, 2 * F)).cuda()
    cfg.set(0, kernel=1)
    ref = ops.gemm_swiglu_bwd(dy, wd, gu, F)
    for budget in (8, 13):
        want = _FUSED_CELLS[budget, M, F]
        cfg.set(budget)
        unfused = Plan(1, 0, 1, 0, G._tiles(M, F, 128), 0)
        assert _fused_plan(cfg, M, F, d, 1, d, F) == (want or unfused), (budget, M, F)
        assert _fused_plan(cfg, M, F, d, 0, d, d) == (want or unfused), (budget, M, F)          # the nn forms: RoPE, SwiGLU forward
        assert cfg.plan(M, F, d, 0, 1, d, F).kernel == 2                                        # the plain nt call: always the 256x256 kernel
        dgu = _sentinel((M, 2 * F), BF16)
        rc = _swiglu_bwd_without_scratch(dy, wd, gu, dgu, F)
        if want:
            assert rc == 0, (budget, M, F, rc)
            _assert_exact(dgu, ref, f"swiglu bwd fused {M}x{F} budget {budget}")
        else:
            assert rc == -1, (budget, M, F, rc)
            assert bool((dgu.view(torch.int16) == 0x7fc5).all()), (budget, M, F)


def test_kernel_choice_from_the_environment_holds_from_the_first_call():
    """RV_GEMM_KERNEL=2 in a fresh process whose FIRST GEMM call is a fused entry point: 744 x 712 at budget 8, which the round-cost rule
    would send to the unfused sequence, runs fused (a NULL scratch is accepted)."""
    _ops()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r})
        import torch
        from radvlm_amd import lib
        L = lib.load()
        assert L.rv_gemm_set_cu_budget(8, 0) == 8
        M, F, d = 744, 712, 64
        dy, wd = torch.ones(M, d, dtype=torch.bfloat16, device="cuda"), torch.ones(d, F, dtype=torch.bfloat16, device="cuda")
        gu, dgu = torch.ones(M, 2 * F, dtype=torch.bfloat16, device="cuda"), torch.empty(M, 2 * F, dtype=torch.bfloat16, device="cuda")
        rc = L.rv_gemm_swiglu_bwd_bf16(dy.data_ptr(), d, wd.data_ptr(), F, gu.data_ptr(), 2 * F, dgu.data_ptr(), 2 * F, None, 0, M, F, d, None, 0,
                                       lib.zeros16(dy.device).data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print("RESULT", rc)
    """)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, RV_GEMM_KERNEL="2"))
    assert p.returncode == 0, (p.returncode, p.stderr[-800:])
    assert p.stdout.split("RESULT")[1].split() == ["0"], p.stdout


def test_plan_refuses_what_the_gemm_refuses(cfg):
    cfg.set(8)
    out = (ctypes.c_int32 * 6)()
    L = cfg.L
    assert L.rv_gemm_plan(64, 64, 64, 0, 0, 64, 64, 0, 0, 0, 0, 0, None) != 0
    assert L.rv_gemm_plan(64, 64, 60, 0, 0, 64, 64, 0, 0, 0, 0, 0, out) != 0        # K % 8 of a row-major operand
    assert L.rv_gemm_plan(60, 64, 64, 1, 0, 64, 64, 0, 0, 0, 0, 0, out) != 0        # M % 8 of a contraction-major A
    assert L.rv_gemm_plan(64, 64, 64, 0, 0, 68, 64, 0, 0, 0, 0, 0, out) != 0        # lda % 8
    assert L.rv_gemm_plan(64, 64, 64, 0, 0, 64, 64, 0, 0, 0, 0, 0, out) == 0

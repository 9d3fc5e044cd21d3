"""Edge tests of the LoRA one-pass kernels (radvlm_amd/csrc/gemm_bf16.hip: lora_down_kernel behind rv_lora_down_bf16, lora_agrad_kernel
and the split-K reduce behind rv_lora_a_grad_bf16) against the float64 reference of tests/lora_ref.py.  Calls go through lib.call, so
leading dimensions and alignments the ops wrappers never produce are reached; operands and outputs are strided views inside NaN-sentinel
buffers (a read of a sentinel as data poisons the result, a write outside the view shows).

Exact tests: integer operands (gemm_ref.integers), p in {0, 0.5}, alpha a power of two -- every fp32 sum, the 1 / (1 - p) scale and the
accumulate add are exact (tests/test_lora_ref_host.py), so the single bf16 store must equal the float64 reference bit for bit: a K-tile
of the 3-stage ring skipped, read twice or read before it landed, a token step dropped or counted twice at a slice seam, a mask word
taken from the wrong element index, a slice plane missed by the reduce all change an integer.  Random-normal tests: every element within
(2^-8 + 2^-16) A of its own budget -- one bf16 store is the only rounding on either path."""
import pytest
import torch

import gemm_ref as G
import lora_ref as L
from lora_ref import BF16
from test_gemm_launch_shapes_gpu import WS_GUARD, _Config, _assert_exact, _sentinel

pytestmark = pytest.mark.gpu

F32 = torch.float32
SEEDS = (0, (1 << 32) + 5, (1 << 63) - 1)
HEAD, TAIL = 8, 72              # sentinel elements before a view (16 bytes: the view stays 16-byte aligned) and behind its last element


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import lib
    return lib


@pytest.fixture
def cfg():
    _lib()
    c = _Config()
    try:
        yield c
    finally:
        c.reset()


def _record(test, **kw):
    from conftest import record_measurement
    record_measurement(test, **kw)


def _view(rows, cols, ld, dtype=BF16, data=None, off=HEAD):
    """(buffer, view): a [rows, cols] view with leading dimension ld, `off` elements into a flat sentinel buffer that ends TAIL elements
    behind the view's last element."""
    assert ld >= cols
    buf = _sentinel((off + (rows - 1) * ld + cols + TAIL,), dtype)
    view = buf.as_strided((rows, cols), (ld, 1), off)
    if data is not None:
        view.copy_(data.to(dtype))
    return buf, view


def _untouched_outside(buf, view):
    """Every element of the flat buffer outside the view still holds the sentinel bits."""
    ok = buf.view(torch.int16 if buf.dtype == BF16 else torch.int32) == (0x7fc5 if buf.dtype == BF16 else 0x7fc5a5a5)
    ok.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset() - buf.storage_offset()).fill_(True)
    return bool(ok.all())


def _all_sentinel(t):
    return bool((t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32) == (0x7fc5 if t.dtype == BF16 else 0x7fc5a5a5)).all())


def _ints(seed, tag, shape, bound=L.AB_MAX):
    return G.integers(seed, tag, shape, bound)


# ------------------------------------------------------------------------------------------------------------------ rv_lora_down_bf16
def _down(lib, x, a, t, M, R, K, alpha, p, seed, zeros="default", ldx=None, lda=None, ldt=None):
    lib.call("rv_lora_down_bf16", x, x.stride(0) if ldx is None else ldx, a, a.stride(0) if lda is None else lda, t,
             t.stride(0) if ldt is None else ldt, M, R, K, float(alpha), float(p), int(seed), lib.zeros16(x.device) if zeros == "default" else zeros)


@pytest.mark.parametrize("case", L.DOWN_CASES, ids=lambda c: f"M{c.M}-R{c.R}-K{c.K}-p{c.p}")
def test_lora_down_is_exact_and_writes_only_its_view(case):
    """K / 64 = 1..4 K-tiles through the 3-stage ring (it wraps at the fourth), rows either side of a wave's 16 and a block's 64, adapter
    rows either side of an accumulator group's 16.  lda > K, ldx > K (p = 0), ldt in {R, R + 4, R + 8}, T 8-byte but not 16-byte
    aligned.  Rows at or beyond M and columns at or beyond R of the T buffer keep their sentinel; the NaN behind x and a is never read."""
    lib = _lib()
    c = case
    seed = SEEDS[(c.M + c.R) % 3]
    x, a = _ints(c.M * 1000 + c.K, 1, (c.M, c.K)), _ints(c.M * 1000 + c.K, 2, (c.R, c.K))
    want = L.lora_down(x, a, c.alpha, c.p, seed)[0].to(BF16)
    xbuf, xv = _view(c.M, c.K, c.K + c.ldx_pad, data=x)
    abuf, av = _view(c.R, c.K, c.K + c.lda_pad, data=a)
    tbuf, tv = _view(c.M, c.R, c.R + c.ldt_pad, off=HEAD + c.t_off)
    assert xv.data_ptr() % 16 == 0 and av.data_ptr() % 16 == 0 and tv.data_ptr() % 16 == (8 if c.t_off else 0)
    _down(lib, xv, av, tv, c.M, c.R, c.K, c.alpha, c.p, seed)
    _assert_exact(tv.cpu(), want, f"lora_down {c}")
    assert _untouched_outside(tbuf, tv), "rv_lora_down_bf16 wrote outside T[:M, :R]"
    assert _untouched_outside(xbuf, xv) and _untouched_outside(abuf, av)
    assert torch.equal(xv.cpu().double(), x) and torch.equal(av.cpu().double(), a)
    _record("lora_down_exact", M=c.M, R=c.R, K=c.K, p=c.p)


def test_lora_down_refuses_what_its_vector_accesses_cannot_serve():
    """RV_ERR_ARG, T untouched: R = 2 (no multiple of 4) and 68 (> 64), K = 72 (no whole K-tile), p > 0 with ldx != K (the mask indexes a
    contiguous x), ldt % 4 != 0 and T offset by 2 elements (8-byte stores), p outside [0, 1), a null zeros16."""
    lib = _lib()
    M, R, K = 17, 16, 128
    xbuf, xv = _view(M, K, K + 8, data=_ints(1, 1, (M, K)))
    abuf, av = _view(68, K, K, data=_ints(1, 2, (68, K)))
    tbuf = _sentinel((HEAD + M * 80 + TAIL,), BF16)
    t0, t2 = tbuf[HEAD:], tbuf[HEAD + 2:]
    bad = [dict(R=2), dict(R=68), dict(K=72), dict(p=0.5), dict(ldt=R + 2), dict(t=t2), dict(p=-0.1, ldx=K), dict(p=1.0, ldx=K), dict(zeros=None)]
    for kw in bad:
        args = dict(t=t0, M=M, R=R, K=K, alpha=1.0, p=0.0, seed=3, ldx=K + 8, lda=K, ldt=80)
        args.update(kw)
        with pytest.raises(lib.RadvlmHipError):
            _down(lib, xv, av, args.pop("t"), **args)
    torch.cuda.synchronize()
    assert _all_sentinel(tbuf), "a refused rv_lora_down_bf16 wrote T"
    _down(lib, xv, av, t0, M, R, K, 1.0, 0.0, 3, ldx=K + 8, lda=K, ldt=80)          # the base call itself is served
    torch.cuda.synchronize()
    assert not _all_sentinel(tbuf)


@pytest.mark.parametrize("p", [0.05, 0.25])
def test_lora_down_random_normal_within_one_bf16_rounding(p):
    """fp32 accumulation, alpha / (1 - p) in fp32, one bf16 store: that store is the only rounding on the path, so every element is held
    to (2^-8 + 2^-16) A + 1e-30 with A = alpha / (1 - p) sum_k |x o mask| |a|."""
    lib = _lib()
    M, R, K, alpha, seed = 130, 60, 256, 1.75, (1 << 32) + 5
    gen = torch.Generator().manual_seed(11)
    x, a = torch.randn(M, K, generator=gen).to(BF16), (0.1 * torch.randn(R, K, generator=gen)).to(BF16)
    ref, A = L.lora_down(x, a, alpha, p, seed)
    tbuf, tv = _view(M, R, R + 4)
    _down(lib, x.cuda(), a.cuda(), tv, M, R, K, alpha, p, seed)
    worst = L.assert_within_gate(tv.cpu(), ref, A, f"lora_down p={p}")
    assert _untouched_outside(tbuf, tv)
    _record("lora_down_random", worst_ratio_of_gate=worst, p=p)


# ------------------------------------------------------------------------------------------------------------------ rv_lora_a_grad_bf16
def _agrad(lib, dt, x, ga, M, R, K, p, seed, accumulate, ws, ws_bytes=None, ldt=None, ldx=None):
    lib.call("rv_lora_a_grad_bf16", dt, dt.stride(0) if ldt is None else ldt, x, x.stride(0) if ldx is None else ldx, ga, ga.stride(0), M, R, K,
             float(p), int(seed), int(accumulate), ws, (ws.numel() * 4 if ws is not None else 0) if ws_bytes is None else ws_bytes)


@pytest.mark.parametrize("case", L.AGRAD_CASES, ids=lambda c: f"M{c.M}-R{c.R}-K{c.K}-p{c.p}-acc{c.accumulate}")
def test_lora_a_grad_is_exact_at_every_slice_count_and_writes_what_it_may(cfg, case):
    """Token slices s0 / s1 of every block from the slice count min(ceil(3 cus / ncb), steps, 32, workspace planes): one slice in an
    exactly sized workspace, two (uneven for 5 steps), as many as the steps or the CU budget allow, and 32 of 34 steps at the device's
    budget.  Exactly that many R K fp32 planes of the workspace are written in full, everything behind them and the guard keep the
    sentinel; gA equals the reference bit for bit at every slice count (so all slice counts agree), with its sentinel columns intact."""
    lib = _lib()
    c = case
    seed = SEEDS[(c.M + c.K) % 3]
    dt, x = _ints(c.M * 1000 + c.K, 3, (c.M, c.R)), _ints(c.M * 1000 + c.K, 4, (c.M, c.K))
    g0 = _ints(c.M * 1000 + c.K, 5, (c.R, c.K), L.EPI_MAX)
    want = L.lora_a_grad(dt, x, g0, c.p, seed, c.accumulate)[0].to(BF16)
    dbuf, dv = _view(c.M, c.R, c.R if c.tight else c.R + 16, data=dt)
    xbuf, xv = _view(c.M, c.K, c.K + c.ldx_pad, data=x)
    plane = c.R * c.K
    taken = []
    for budget, planes in L.agrad_configs(c):
        cus = cfg.set(budget)
        slices = L.agrad_slices(c, cus, planes)
        wsbuf = _sentinel((planes * plane + WS_GUARD,), F32)
        gbuf, gv = _view(c.R, c.K, c.K if c.tight else c.K + 24, data=g0 if c.accumulate else None)
        _agrad(lib, dv, xv, gv, c.M, c.R, c.K, c.p, seed, c.accumulate, wsbuf[:planes * plane])
        what = f"lora_a_grad {c} budget={budget} planes={planes} slices={slices}"
        _assert_exact(gv.cpu(), want, what)
        assert _untouched_outside(gbuf, gv), what + ": wrote outside gA[:R, :K]"
        written = ~torch.isnan(wsbuf[:planes * plane].view(planes, plane))
        assert bool(written[:slices].all()), what + ": a slice plane was not written in full"
        assert _all_sentinel(wsbuf[slices * plane:]), what + ": the workspace behind the slice planes, or its guard, was written"
        taken.append(slices)
    assert _untouched_outside(dbuf, dv) and _untouched_outside(xbuf, xv)
    _record("lora_a_grad_exact", M=c.M, R=c.R, K=c.K, p=c.p, accumulate=c.accumulate, slices=taken)


def test_lora_a_grad_refuses_what_it_cannot_serve(cfg):
    """RV_ERR_ARG, gA untouched: R = 4 (no multiple of 8) and 72 (> 64), K = 12, ldx % 8, ldt % 8, p > 0 with ldx != K, X or dT off a
    16-byte boundary, a NULL workspace and one that is a byte short of one R K fp32 plane."""
    lib = _lib()
    M, R, K = 65, 24, 128
    dbuf = torch.zeros(HEAD + M * 80 + TAIL, dtype=BF16, device="cuda")
    xbuf = torch.zeros(HEAD + M * (K + 8) + TAIL, dtype=BF16, device="cuda")
    gbuf = _sentinel((72 * K,), BF16)
    ws = torch.zeros(72 * K, dtype=F32, device="cuda")
    bad = [dict(R=4), dict(R=72), dict(K=12), dict(ldx=K + 4), dict(ldt=76), dict(p=0.5), dict(x=xbuf[HEAD + 4:]), dict(dt=dbuf[HEAD + 4:]),
           dict(ws=None), dict(ws_bytes=R * K * 4 - 1)]
    for kw in bad:
        args = dict(dt=dbuf[HEAD:], x=xbuf[HEAD:], M=M, R=R, K=K, p=0.0, seed=3, accumulate=0, ws=ws, ldt=80, ldx=K + 8)
        args.update(kw)
        with pytest.raises(lib.RadvlmHipError):
            _agrad(lib, args.pop("dt"), args.pop("x"), gbuf.view(72, K), **args)
    torch.cuda.synchronize()
    assert _all_sentinel(gbuf), "a refused rv_lora_a_grad_bf16 wrote gA"
    _agrad(lib, dbuf[HEAD:], xbuf[HEAD:], gbuf.view(72, K), M, R, K, 0.0, 3, 0, ws, ws_bytes=R * K * 4, ldt=80, ldx=K + 8)     # one plane: served
    torch.cuda.synchronize()
    assert not _all_sentinel(gbuf[:R * K]) and _all_sentinel(gbuf[R * K:])


@pytest.mark.parametrize("p", [0.05, 0.25])
def test_lora_a_grad_random_normal_within_one_bf16_rounding(p):
    """The token slices' partial sums stay fp32 in the workspace, the reduce scales by 1 / (1 - p) and adds g0 in fp32: the bf16 store is
    the only rounding on the path, so every element is held to (2^-8 + 2^-16) A + 1e-30 with A = 1 / (1 - p) sum_m |dt| |x o mask| + |g0|."""
    lib = _lib()
    M, R, K, seed = 300, 24, 264, (1 << 63) - 1
    gen = torch.Generator().manual_seed(13)
    dt, x, g0 = (torch.randn(s, generator=gen).to(BF16) for s in ((M, R), (M, K), (R, K)))
    ref, A = L.lora_a_grad(dt, x, g0, p, seed, True)
    gbuf, gv = _view(R, K, K + 24, data=g0)
    ws = torch.empty(8 * R * K, dtype=F32, device="cuda")
    _agrad(lib, dt.cuda(), x.cuda(), gv, M, R, K, p, seed, 1, ws)
    worst = L.assert_within_gate(gv.cpu(), ref, A, f"lora_a_grad p={p}")
    assert _untouched_outside(gbuf, gv)
    _record("lora_a_grad_random", worst_ratio_of_gate=worst, p=p)

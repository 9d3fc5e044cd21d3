"""Edge tests of the training attention (radvlm_amd/csrc/attention.hip), forward and backward, against the float64 reference of
tests/attn_ref.py: every sequence length one either side of a block boundary, key padding with and without the causal mask, packed
batches, inputs that force the forward's deferred softmax rescale after the first key tile, grouped-query heads on both dK/dV launch
shapes, what the kernels must not read or write, and the argument checks.

Gates (attn_ref.assert_within_budget): every ELEMENT of out, dq, dk, dv is held to (roundings 2^-8 + 2^-16) A of its own budget A, lse to
1e-4 max(1, |ref|); gradients of padded rows are exactly zero.  "All forwards" = the transposed-V kernel at head_dim 64 and 128 and the
natural-layout kernel at 128; "both backwards" = natural and transposed at 128, transposed at 64.  Buffers a kernel must not touch carry
the NaN sentinel of tests/test_rowops_edges_gpu.py.  Every test that gates values appends its worst ratio through conftest.record_measurement.
"""
import functools
import math

import numpy as np
import pytest
import torch

import attn_ref as R
from attn_ref import BF16, assert_lse_close, assert_within_budget

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 320)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _record(test, worst, **kw):
    from conftest import record_measurement
    record_measurement(test, worst_ratio_of_gate=worst, **kw)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sentinel(shape, dtype=BF16):
    """A buffer of one NaN bit pattern (bf16 0x7fc5 / fp32 0x7fc5a5a5): a kernel cannot produce it by accident, and a read of it poisons the result."""
    if dtype == BF16:
        return torch.full(shape, 0x7fc5, dtype=torch.int16, device="cuda").view(BF16)
    return torch.full(shape, 0x7fc5a5a5, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_sentinel(t):
    return _same_bits(t, _sentinel(tuple(t.shape), t.dtype))


def _pad64(S):
    return (S + 63) // 64 * 64


class Case:
    """The bf16 inputs of one call on the CPU, their float64 reference, and the geometry.  Built once per parameter set (cached) and never
    modified."""

    def __init__(self, family, B, S, H, Hkv, hd, causal, lens=None, cu_lens=None, seed=0):
        self.family, self.H, self.Hkv, self.hd, self.causal = family, H, Hkv, hd, causal
        self.lens = list(lens) if lens is not None else None
        self.cu = np.concatenate([[0], np.cumsum(cu_lens)]).astype(np.int32) if cu_lens is not None else None
        self.B, self.S = (len(cu_lens), max(cu_lens)) if cu_lens is not None else (B, S)
        self.s_pad = _pad64(self.S)
        self.spans = R.sample_rows(self.B, self.S, self.cu)
        q, k, v, dout = R.make_inputs(family, R.positions(self.B, self.S, self.cu), H, Hkv, hd, seed=seed)
        if self.lens is not None:                     # padded rows carry zero dout (the loss ignores them): their gradients are exactly 0
            for b, L in enumerate(self.lens):
                dout.view(self.B, self.S, -1)[b, L:] = 0
        self.q, self.k, self.v, self.dout = q, k, v, dout
        self.M = q.shape[0]
        self.ref = R.reference(q, k, v, dout, self.B, self.S, H, Hkv, hd, causal, lens=self.lens, cu=self.cu)
        self.valid = self.ref["valid"]
        # lse [B, H, S]: entries that belong to a valid row
        self.lse_valid = torch.zeros(self.B, self.S, dtype=torch.bool)
        for b, (r0, n) in enumerate(self.spans):
            self.lse_valid[b, :n] = self.valid[r0:r0 + n]

    def device_inputs(self):
        """(q, k, v) as column slices of one fused [M, (H + 2 Hkv) hd] buffer (how the engine lays them out), dout, lens, cu on the GPU."""
        d, kvd = self.H * self.hd, self.Hkv * self.hd
        g = torch.cat([self.q, self.k, self.v], 1).cuda()
        lens_t = torch.tensor(self.lens, dtype=torch.int32, device="cuda") if self.lens is not None else None
        cu_t = torch.from_numpy(self.cu).cuda() if self.cu is not None else None
        return g[:, :d], g[:, d:d + kvd], g[:, d + kvd:], self.dout.cuda(), lens_t, cu_t


@functools.lru_cache(maxsize=None)
def _case(family, B, S, H, Hkv, hd, causal, lens=None, cu_lens=None):
    return Case(family, B, S, H, Hkv, hd, causal, lens, cu_lens)


def _forward(ops, c, kind, gq, gk, gv, lens_t, cu_t, out=None):
    """kind "T": transposed-V kernel, "N": natural-layout kernel.  lse starts as sentinels: what lies beyond a sample's rows must stay one."""
    lse = _sentinel((c.B, c.H, c.s_pad), torch.float32)
    if kind == "N":
        out, lse = ops.attn_fwd(gq, gk, None, c.B, c.S, c.H, c.hd, c.s_pad, c.causal, lens=lens_t, kv_heads=c.Hkv, cu=cu_t, v=gv, lse=lse, out=out)
    else:
        vT = ops.transpose_heads(gv, c.B, c.S, c.Hkv, c.hd, c.s_pad, cu=cu_t)
        out, lse = ops.attn_fwd(gq, gk, vT, c.B, c.S, c.H, c.hd, c.s_pad, c.causal, lens=lens_t, kv_heads=c.Hkv, cu=cu_t, lse=lse, out=out)
    for b, (_, n) in enumerate(c.spans):
        assert _is_sentinel(lse[b, :, n:]), f"lse beyond the {n} rows of sample {b} was written ({kind})"
    return out, lse


def _check_forward(c, out, lse, what):
    ok = c.valid
    w_out = assert_within_budget(out.cpu()[ok], c.ref["out"][ok], c.ref["A_out"][ok], 2, what + " out")
    got = lse[..., :c.S].cpu().transpose(1, 2)[c.lse_valid]                    # [valid (b, s), H]
    w_lse = assert_lse_close(got, c.ref["lse"].transpose(1, 2)[c.lse_valid], what)
    if not bool(ok.all()):         # padded query rows: not a value contract, but finite
        assert bool(torch.isfinite(out.cpu()[~ok].float()).all()), what + ": out of padded rows"
        pad = ~c.lse_valid & ~torch.isnan(c.ref["lse"][:, 0])
        assert bool(torch.isfinite(lse[..., :c.S].cpu().transpose(1, 2)[pad]).all()), what + ": lse of padded rows"
    return w_out, w_lse


def _check_backward(c, grads, roundings_kv, what):
    ok = c.valid
    worst = {}
    for name, g, rnd in zip(("dq", "dk", "dv"), grads, (2, roundings_kv, roundings_kv)):
        worst[name] = assert_within_budget(g.cpu()[ok], c.ref[name][ok], c.ref["A_" + name][ok], rnd, f"{what} {name}")
        if not bool(ok.all()):
            assert float(g.cpu()[~ok].float().abs().max()) == 0.0 and not bool(torch.isnan(g.cpu()[~ok].float()).any()), f"{what}: {name} of padded rows"
    return worst


def _run(ops, c, use_ws=True, roundings_kv=2):
    """All forwards and both backwards that exist for the case's head_dim; every output element gated.  Returns {output: worst ratio}."""
    gq, gk, gv, dout, lens_t, cu_t = c.device_inputs()
    worst = {}

    def upd(name, w):
        worst[name] = max(worst.get(name, 0.0), w)
    kinds = ("T", "N") if c.hd == 128 else ("T",)
    for kind in kinds:
        what = f"{c.family} S={c.S} hd={c.hd} causal={c.causal} fwd={kind}"
        out, lse = _forward(ops, c, kind, gq, gk, gv, lens_t, cu_t)
        w_out, w_lse = _check_forward(c, out, lse, what)
        upd("out", w_out), upd("lse", w_lse)
        lse_b = torch.nan_to_num(lse, nan=0.0)            # (the sentinels beyond the samples' rows are the subject of the stale-statistics test)
        grads = ops.attn_bwd(gq, gk, gv, out, dout, lse_b, c.B, c.S, c.H, c.hd, c.s_pad, c.causal, lens=lens_t, kv_heads=c.Hkv, cu=cu_t,
                             use_workspace=use_ws, natural=(kind == "N"))
        for name, w in _check_backward(c, grads, roundings_kv, what + " bwd").items():
            upd(name, w)
    return worst


def _merge(total, worst):
    for k, w in worst.items():
        total[k] = max(total.get(k, 0.0), w)


# ------------------------------------------------------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", SIZES)
def test_every_block_boundary_size(S, causal):
    """S = 1 and one either side of 32 (a wave's rows), 64 (the key tile), 128 (forward / natural dQ query block) and 256 (transposed dQ block)."""
    ops = _ops()
    total = {}
    for hd in (64, 128):
        _merge(total, _run(ops, _case("rand", 2, S, 2, 2, hd, causal)))
    _record("attention_edges_sizes", max(total.values()), S=S, causal=causal, **total)


# ------------------------------------------------------------------------------------------------------------------ 2. key padding
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("lens", [(1, 200), (63, 64), (65, 128), (199, 64)])
def test_key_padding_with_and_without_the_causal_mask(lens, causal):
    ops = _ops()
    total = {}
    for hd in (64, 128):
        _merge(total, _run(ops, _case("rand", 2, 200, 2, 2, hd, causal, lens=lens)))
    _record("attention_edges_key_padding", max(total.values()), lens=list(lens), causal=causal, **total)


# ------------------------------------------------------------------------------------------------------------------ 3. packed
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)])
@pytest.mark.parametrize("cu_lens", [(130, 1, 64, 65), (300, 129)])
def test_packed_batches_sample_by_sample(cu_lens, H, Hkv, causal):
    """Every sample of a packed batch against the reference of that sample alone (attn_ref.reference walks the samples one by one),
    through the natural forward as well as the transposed one."""
    ops = _ops()
    total = {}
    for hd in (64, 128):
        for use_ws in ((False, True) if H != Hkv else (False,)):          # grouped heads: both dK / dV launch shapes (2 and 3 roundings)
            _merge(total, _run(ops, _case("rand", None, None, H, Hkv, hd, causal, cu_lens=cu_lens), use_ws=use_ws, roundings_kv=3 if use_ws else 2))
    _record("attention_edges_packed", max(total.values()), lens=list(cu_lens), H=H, Hkv=Hkv, causal=causal, **total)


# ------------------------------------------------------------------------------------------------------------------ 4. rescale stress
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("family", ["stair", "stair7", "mixed", "sink", "big"])
def test_softmax_rescale_after_the_first_key_tile(family, causal):
    """S = 320: 5 key tiles, 3 query blocks.  tests/test_attn_ref_host.py shows from the float64 scores that these inputs make every wave
    take the rescale branch with alpha != 0; |v| falls as the scores rise, so a wrong alpha, a lost l *= alpha or a stale threshold is an
    O(1) error against the budgets."""
    ops = _ops()
    total = {}
    for hd in (64, 128):
        _merge(total, _run(ops, _case(family, 2, 320, 2, 2, hd, causal)))
    _record("attention_edges_rescale", max(total.values()), family=family, causal=causal, **total)


def test_rescale_in_the_paired_form_of_the_natural_forward():
    """The causal natural forward runs query blocks in pairs when that fills the CUs (B = 8, H = 32, S = 300 does): m, l and the threshold
    are reset at the seam between a pair's blocks.  Rows of even and odd query blocks of several heads against the reference, and the whole
    batch bit-identical to the same samples sent two at a time (one query block per block)."""
    ops = _ops()
    from radvlm_amd import lib as L_
    B, H, Hkv, S, hd = 8, 32, 8, 300, 128
    plan = L_.load().rv_attn_fwd_nat_pairs
    assert plan(B, H, S, 1) == 1 and plan(2, H, S, 1) == 0
    d, kvd, s_pad = H * hd, Hkv * hd, _pad64(S)
    q, k, v, _ = R.make_inputs("stair", R.positions(B, S), H, Hkv, hd, seed=3)
    g = torch.cat([q, k, v], 1).cuda()
    gq, gk, gv = g[:, :d], g[:, d:d + kvd], g[:, d + kvd:]
    out, lse = ops.attn_fwd(gq, gk, None, B, S, H, hd, s_pad, True, kv_heads=Hkv, v=gv)
    for b0 in range(0, B, 2):
        rows = slice(b0 * S, (b0 + 2) * S)
        o2, l2 = ops.attn_fwd(gq[rows], gk[rows], None, 2, S, H, hd, s_pad, True, kv_heads=Hkv, v=gv[rows])
        assert torch.equal(_bits(out[rows]), _bits(o2)) and torch.equal(_bits(lse[b0:b0 + 2, :, :S]), _bits(l2[:, :, :S])), b0
    worst = 0.0
    zero = torch.zeros(S, hd, dtype=BF16)
    for b, h in ((0, 0), (3, 13), (7, 31)):               # all three query blocks (even, odd, even) of each
        r, hk = slice(b * S, (b + 1) * S), h // (H // Hkv)
        ref = R.reference(q[r, h * hd:(h + 1) * hd], k[r, hk * hd:(hk + 1) * hd], v[r, hk * hd:(hk + 1) * hd], zero, 1, S, 1, 1, hd, True)
        worst = max(worst, assert_within_budget(out[r, h * hd:(h + 1) * hd].cpu(), ref["out"], ref["A_out"], 2, f"paired out b={b} h={h}"))
        assert_lse_close(lse[b, h, :S].cpu(), ref["lse"][0, 0], f"paired lse b={b} h={h}")
    _record("attention_edges_rescale_paired", worst)


# ------------------------------------------------------------------------------------------------------------------ 5. grouped-query
@pytest.mark.parametrize("family", ["rand", "stair"])
@pytest.mark.parametrize("S", [129, 257])
@pytest.mark.parametrize("use_ws", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (6, 1)])
def test_grouped_query_heads_on_both_dkv_launch_shapes(H, Hkv, use_ws, S, family):
    """use_ws False: one block per key/value head accumulates the group's dK / dV in registers (2 roundings); True: per-query-head partials
    are stored in bf16 and summed by group_sum_heads_kernel (3 roundings)."""
    ops = _ops()
    total = {}
    for hd in (64, 128):
        _merge(total, _run(ops, _case(family, 2, S, H, Hkv, hd, True), use_ws=use_ws, roundings_kv=3 if use_ws else 2))
    _record("attention_edges_gqa", max(total.values()), H=H, Hkv=Hkv, use_ws=use_ws, S=S, family=family, **total)


# ------------------------------------------------------------------------------------------------------------------ 6. memory discipline
def _wide(rows, cols, left=8, right=24, guard=1):
    """(buffer, view): a [rows, cols] column slice of a wider sentinel buffer with `guard` more rows."""
    buf = _sentinel((rows + guard, left + cols + right))
    return buf, buf[:rows, left:left + cols]


def _untouched(buf, rows, cols, left=8):
    """Sentinel columns beside the slice and the guard row(s) after it are bit-unchanged."""
    return _is_sentinel(buf[:, :left]) and _is_sentinel(buf[:, left + cols:]) and _is_sentinel(buf[rows:])


@pytest.mark.parametrize("hd,natural", [(128, True), (128, False), (64, False)])
@pytest.mark.parametrize("H,Hkv,use_ws", [(2, 2, False), (4, 2, False), (4, 2, True)])
def test_outputs_as_column_slices_and_nan_guard_rows_behind_the_inputs(H, Hkv, use_ws, hd, natural):
    """S = 200 (no multiple of 64: the last key / query tile is partial, so staging that over-reads would pick the guard rows up).  Outputs
    are column slices of wider sentinel buffers with a guard row; q, k, v, o and dout are followed by a NaN guard row.  Nothing outside the
    outputs may change, and no output bit may differ from the run on plain buffers."""
    ops = _ops()
    c = _case("rand", 2, 200, H, Hkv, hd, True)
    d, kvd, M = H * hd, Hkv * hd, c.M
    gq0, gk0, gv0, dout0, _, _ = c.device_inputs()
    kind = "N" if natural else "T"
    out0, lse0 = _forward(ops, c, kind, gq0, gk0, gv0, None, None)
    g0 = ops.attn_bwd(gq0, gk0, gv0, out0, dout0, torch.nan_to_num(lse0, nan=0.0), c.B, c.S, H, hd, c.s_pad, True, kv_heads=Hkv,
                      use_workspace=use_ws, natural=natural)
    # the same call with guarded inputs and sliced outputs
    fused = _sentinel((M + 1, d + 2 * kvd))
    fused[:M] = torch.cat([c.q, c.k, c.v], 1).cuda()
    gq, gk, gv = fused[:M, :d], fused[:M, d:d + kvd], fused[:M, d + kvd:]
    dbuf = _sentinel((M + 1, d))
    dbuf[:M] = c.dout.cuda()
    obuf, out = _wide(M, d)
    out1, lse1 = _forward(ops, c, kind, gq, gk, gv, None, None, out=out)
    assert _untouched(obuf, M, d), "forward wrote outside its output slice"
    assert _same_bits(out1, out0) and _same_bits(lse1, lse0), "forward read the guard row behind q / k / v"
    (qb, dq), (kb, dk), (vb, dv) = _wide(M, d), _wide(M, kvd), _wide(M, kvd)
    ops.attn_bwd(gq, gk, gv, out, dbuf[:M], torch.nan_to_num(lse1, nan=0.0), c.B, c.S, H, hd, c.s_pad, True, kv_heads=Hkv,
                 use_workspace=use_ws, natural=natural, dq=dq, dk=dk, dv=dv)
    assert _untouched(qb, M, d) and _untouched(kb, M, kvd) and _untouched(vb, M, kvd), "backward wrote outside its output slices"
    assert _untouched(obuf, M, d) and _is_sentinel(fused[M:]) and _is_sentinel(dbuf[M:])
    for name, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), g0):
        assert _same_bits(a.contiguous(), b), f"{name} differs with guard rows behind the inputs"


@pytest.mark.parametrize("hd,natural", [(128, True), (128, False), (64, False)])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 2)])
@pytest.mark.parametrize("layout,causal", [("padded", True), ("padded", False), ("packed", True)])
def test_stale_softmax_statistics_never_reach_a_gradient(layout, causal, H, Hkv, hd, natural):
    """lse and delta are cached by padded shape and only the entries of valid rows are rewritten (engine._stat_buffer): NaN at rows at or beyond
    a sample's length and in [S, S_pad) must give, bit for bit, the gradients of a run with zeros there, and padded rows stay exactly 0."""
    ops = _ops()
    c = _case("rand", 2, 200, H, Hkv, hd, causal, lens=(65, 199)) if layout == "padded" else _case("rand", None, None, H, Hkv, hd, causal, cu_lens=(130, 1, 64, 65))
    gq, gk, gv, dout, lens_t, cu_t = c.device_inputs()
    out, lse = _forward(ops, c, "N" if natural else "T", gq, gk, gv, lens_t, cu_t)
    live = torch.zeros(c.B, 1, c.s_pad, dtype=torch.bool, device="cuda")
    live[:, 0, :c.S] = c.lse_valid.cuda()
    assert bool(torch.isfinite(lse[live.expand_as(lse)]).all())
    res = {}
    for fill in ("zero", "nan"):
        stale = torch.zeros_like(lse) if fill == "zero" else _sentinel(tuple(lse.shape), torch.float32)
        lse_f = torch.where(live, lse, stale)
        delta = stale.clone()
        res[fill] = ops.attn_bwd(gq, gk, gv, out, dout, lse_f, c.B, c.S, H, hd, c.s_pad, causal, lens=lens_t, kv_heads=Hkv, cu=cu_t,
                                 natural=natural, delta=delta)
        assert _same_bits(lse_f, torch.where(live, lse, stale)), "the backward wrote lse"
    for name, a, b in zip(("dq", "dk", "dv"), res["zero"], res["nan"]):
        assert bool(torch.isfinite(b.float()).all()), f"{name}: stale NaN statistics reached the gradient"
        assert _same_bits(a, b), name
        if not bool(c.valid.all()):
            assert float(b.cpu()[~c.valid].float().abs().max()) == 0.0, name
    worst = _check_backward(c, res["nan"], 3 if H != Hkv else 2, f"stale {layout}")
    _record("attention_edges_stale_statistics", max(worst.values()), layout=layout, causal=causal, H=H, Hkv=Hkv, hd=hd, natural=natural, **worst)


# ------------------------------------------------------------------------------------------------------------------ 7. argument checks
def test_argument_checks_reject_before_any_launch():
    """RV_ERR_ARG (raised by lib.call) for S_pad < S or no multiple of 64, H % H_kv != 0, HD != 128 on the natural entry points, a leading
    dimension that is no multiple of 8 (inputs) / 4 (outputs), and a packed backward with total_rows <= 0.  Outputs stay sentinels."""
    _ops()
    from radvlm_amd import lib
    B, S, H, Hkv, hd = 2, 70, 2, 2, 128
    s_pad, d, M = 128, H * hd, B * S
    c = _case("rand", B, S, H, Hkv, hd, True)
    gq, gk, gv, dout, _, _ = c.device_inputs()
    ld = gq.stride(0)
    z = lib.zeros16(gq.device)
    cu = torch.tensor([0, S, 2 * S], dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(hd)
    out, dq, dk, dv = (_sentinel((M, d)) for _ in range(4))
    lse, delta = _sentinel((B, H, s_pad), torch.float32), _sentinel((B, H, s_pad), torch.float32)
    vT = torch.zeros(B, Hkv, hd, s_pad, dtype=BF16, device="cuda")
    o_in = torch.zeros(M, d, dtype=BF16, device="cuda")
    lse_in = torch.zeros(B, H, s_pad, dtype=torch.float32, device="cuda")

    def fwd_t(S_pad=s_pad, H_=H, Hkv_=Hkv, HD=hd, ld_q=ld, ld_k=ld, ld_o=d):
        lib.call("rv_attn_fwd_gqa", gq, ld_q, gk, ld_k, vT, out, ld_o, lse, None, None, B, H_, Hkv_, S, S_pad, HD, 1, scale, z)

    def fwd_n(S_pad=s_pad, H_=H, Hkv_=Hkv, HD=hd, ld_q=ld, ld_k=ld, ld_v=ld, ld_o=d):
        lib.call("rv_attn_fwd_nat", gq, ld_q, gk, ld_k, gv, ld_v, out, ld_o, lse, None, None, B, H_, Hkv_, S, S_pad, HD, 1, scale, z)

    def bwd_t(S_pad=s_pad, H_=H, Hkv_=Hkv, HD=hd, ld_q=ld, ld_do=d, ld_dq=d, ld_dk=d, ld_dv=d, cu_=None, total=0):
        lib.call("rv_attn_bwd_gqa_rope", gq, ld_q, gk, ld, gv, ld, o_in, d, dout, ld_do, vT, vT, vT, lse_in, delta, dq, ld_dq, dk, ld_dk, dv, ld_dv,
                 None, cu_, total, B, H_, Hkv_, S, S_pad, HD, 1, scale, None, 0, None, None, z)

    def bwd_n(S_pad=s_pad, H_=H, Hkv_=Hkv, HD=hd, ld_q=ld, ld_do=d, ld_dq=d, ld_dk=d, ld_dv=d, cu_=None, total=0):
        lib.call("rv_attn_bwd_nat", gq, ld_q, gk, ld, gv, ld, o_in, d, dout, ld_do, lse_in, delta, dq, ld_dq, dk, ld_dk, dv, ld_dv,
                 None, cu_, total, B, H_, Hkv_, S, S_pad, HD, 1, scale, None, 0, None, None, z)

    bad = [dict(S_pad=64), dict(S_pad=72), dict(H_=3, Hkv_=2), dict(ld_q=ld + 4)]
    cases = [(f, kw) for f in (fwd_t, fwd_n, bwd_t, bwd_n) for kw in bad]
    cases += [(fwd_n, dict(HD=64)), (bwd_n, dict(HD=64)), (fwd_t, dict(HD=96)), (bwd_t, dict(HD=96))]
    cases += [(fwd_t, dict(ld_o=d + 2)), (fwd_n, dict(ld_o=d + 2)), (fwd_n, dict(ld_v=ld + 4)), (fwd_t, dict(ld_k=ld + 4))]
    cases += [(f, kw) for f in (bwd_t, bwd_n) for kw in (dict(ld_do=d + 4), dict(ld_dq=d + 2), dict(ld_dk=d + 2), dict(ld_dv=d + 2),
                                                        dict(cu_=cu, total=0), dict(cu_=cu, total=-1))]
    for f, kw in cases:
        with pytest.raises(lib.RadvlmHipError):
            f(**kw)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv), ("lse", lse), ("delta", delta)):
        assert _is_sentinel(t), name + " was written by a rejected call"

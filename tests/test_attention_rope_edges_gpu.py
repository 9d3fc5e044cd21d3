"""Edge tests of the rotary adjoint in the attention backward's epilogues (radvlm_amd/csrc/attention.hip: unrope<DB>() in the dQ and dK
epilogues of both backward families, and the rotation inside group_sum_heads_kernel on the per-query-head launch shape) against the
float64 reference attn_ref.reference + attn_ref.unrope: sequence lengths either side of every block boundary, key padding, packed
batches, grouped-query heads on both dK/dV launch shapes, NULL and explicit positions, what the kernels must not read or write, and the
bit promise to the unfused sequence.

Gates (attn_ref.assert_within_budget, derivation in attn_ref's docstring): EVERY element of dq is held to (3 2^-8 + 2^-16) A', of dk to
3 roundings on the register-accumulating shape and 4 on the per-query-head + group-sum shape, of dv to 2 and 3 as without rope.
tests/test_attn_rope_ref_host.py shows on the CPU that every geometry used here fails for a sin sign error on one half, swapped
partners, the forward rotation, a position off by one, the row index taken for rope_positions, `row % S` on a packed batch and a dk left
rotated.  "All backwards" = natural-layout kernels at head_dim 128, transposed kernels at 128 and at 64.

Layout of every call: dq / dk / dv are the column slices of ONE fused [M, (H + 2 Hkv) hd] sentinel buffer with a sentinel guard row (the
engine's dqkv layout); the cos / sin table lies between NaN guard rows, and the positions array between guard entries that point at the
NaN row behind the table, so a read past the rows in use poisons the result without leaving the allocation.  Inputs, the un-rotated
reference and the forward machinery are those of tests/test_attention_edges_gpu.py."""
import math

import pytest
import torch

import attn_rope_cases as C
import test_attention_edges_gpu as E
from attn_ref import BF16, assert_within_budget

pytestmark = pytest.mark.gpu

BACKWARDS = ((128, True), (128, False), (64, False))          # (head_dim, natural layout)


def _record(test, worst, **kw):
    from conftest import record_measurement
    record_measurement(test, worst_ratio_of_gate=max(worst.values()), **worst, **kw)


def _merge(total, worst):
    for k, w in worst.items():
        total[k] = max(total.get(k, 0.0), w)


class _Rope:
    """The table and the positions of one (geometry, head_dim) on the device, inside their guards."""

    def __init__(self, g, hd):
        ref = C.rope_reference(g, hd)
        rows = ref["cs"].shape[0]
        self.tbuf = E._sentinel((1 + rows + 2, hd // 2, 2), torch.float32)
        self.tbuf[1:1 + rows] = ref["cs"].cuda()
        self.cs = self.tbuf[1:1 + rows]
        self.pos = None
        if g.mode != "null":
            n = len(ref["pos"])
            self.pbuf = torch.full((8 + n + 8,), rows, dtype=torch.int32, device="cuda")
            self.pbuf[8:8 + n] = torch.from_numpy(ref["pos"]).int().cuda()
            self.pos = self.pbuf[8:8 + n]

    def arg(self):
        return (self.cs, self.pos)


class _Dev:
    """One geometry at one head_dim on the device: the inputs, and the forward of each kind (run once, its outputs only read)."""

    def __init__(self, ops, g, hd):
        self.ops, self.g, self.c, self.ref = ops, g, C.case_of(g, hd), C.rope_reference(g, hd)
        self.inputs = self.c.device_inputs()
        self.rope = _Rope(g, hd)
        self.fwd = {}

    def forward(self, natural):
        kind = "N" if natural else "T"
        if kind not in self.fwd:
            gq, gk, gv, _, lens_t, cu_t = self.inputs
            out, lse = E._forward(self.ops, self.c, kind, gq, gk, gv, lens_t, cu_t)
            self.fwd[kind] = (out, torch.nan_to_num(lse, nan=0.0))
        return self.fwd[kind]

    def backward(self, natural, rope=True, use_ws=False, outs=None):
        """One backward call into a fresh fused dqkv sentinel buffer (or into `outs`); returns (dq, dk, dv) views."""
        c = self.c
        gq, gk, gv, dout, lens_t, cu_t = self.inputs
        out, lse = self.forward(natural)
        buf = None
        if outs is None:
            d, kvd = c.H * c.hd, c.Hkv * c.hd
            buf = E._sentinel((c.M + 1, d + 2 * kvd))
            outs = buf[:c.M, :d], buf[:c.M, d:d + kvd], buf[:c.M, d + kvd:]
        self.ops.attn_bwd(gq, gk, gv, out, dout, lse, c.B, c.S, c.H, c.hd, c.s_pad, c.causal, lens=lens_t, kv_heads=c.Hkv, cu=cu_t,
                          use_workspace=use_ws, natural=natural, rope=self.rope.arg() if rope else None, dq=outs[0], dk=outs[1], dv=outs[2])
        assert buf is None or E._is_sentinel(buf[c.M:]), "the backward wrote the guard row behind dq | dk | dv"
        return outs

    def check(self, grads, group_sum, what):
        """Every element of valid rows inside its gate, rows beyond lens[b] exactly zero.  Returns {output: worst ratio}."""
        ok = self.ref["valid"]
        worst = {}
        for name, g, rnd in zip(("dq", "dk", "dv"), grads, (3, 4 if group_sum else 3, 3 if group_sum else 2)):
            got = g.cpu()
            key = name if name == "dq" else name + ("_group_sum" if group_sum else "_register")
            worst[key] = assert_within_budget(got[ok], self.ref[name][ok], self.ref["A_" + name][ok], rnd, f"{what} {name}")
            if not bool(ok.all()):
                pad = got[~ok].float()
                assert float(pad.abs().max()) == 0.0 and not bool(torch.isnan(pad).any()), f"{what}: {name} of padded rows"
        return worst


def _devs(ops, g):
    """(device state, natural) of every backward that exists: one state per head_dim, shared by the two families at 128."""
    devs = {hd: _Dev(ops, g, hd) for hd in {hd for hd, _ in BACKWARDS}}
    return [(devs[hd], natural) for hd, natural in BACKWARDS]


def _gate_all(ops, g, use_ws=False):
    total = {}
    for dev, natural in _devs(ops, g):
        grads = dev.backward(natural, use_ws=use_ws)
        _merge(total, dev.check(grads, use_ws, f"{C.geo_id(g)} hd={dev.c.hd} natural={natural} ws={use_ws}"))
    return total


# ------------------------------------------------------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S", C.SIZES)
def test_block_edge_sizes_with_null_and_explicit_positions(S, causal):
    """S = 1 and either side of 64 (key tile, natural dK/dV block), 128 (natural dQ block) and 256 (transposed dQ block): a mistake
    confined to the rows next to a block boundary lands on gated elements.  rope_positions NULL (row in sample) and an explicit array
    (7 row + 3) % 401 that is not the row index: a kernel that ignores the array fails against it."""
    ops = E._ops()
    total = {}
    for mode in ("null", "explicit"):
        _merge(total, _gate_all(ops, C.size_geo(S, causal, mode)))
    _record("attention_rope_edges_sizes", total, S=S, causal=causal)


# ------------------------------------------------------------------------------------------------------------------ 2. key padding
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("lens", C.PAD_LENS)
def test_key_padding_keeps_padded_rows_exactly_zero(lens, causal):
    """Valid rows gated; dq, dk, dv of rows at or beyond lens[b] exactly zero (-0 allowed) and never NaN: the rotation of a zero
    gradient by whatever table row its position names is zero."""
    ops = E._ops()
    total = {}
    for mode in ("null", "explicit"):
        _merge(total, _gate_all(ops, C.padding_geo(lens, causal, mode)))
    _record("attention_rope_edges_key_padding", total, lens=list(lens), causal=causal)


# ------------------------------------------------------------------------------------------------------------------ 3. packed
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("cu_lens", C.PACKED)
def test_packed_batches_with_sample_relative_positions(cu_lens, causal):
    """Row r of sample b at position 7 b + r, every sample against the reference of that sample alone."""
    ops = E._ops()
    _record("attention_rope_edges_packed", _gate_all(ops, C.packed_geo(cu_lens, causal)), lens=list(cu_lens), causal=causal)


def test_packed_batch_without_positions_is_refused_by_both_entry_points():
    """cu_rows with rope_cos_sin but rope_positions = NULL: RV_ERR_ARG before any launch, dq / dk / dv stay sentinels."""
    E._ops()
    from radvlm_amd import lib
    hd = 128
    g = C.packed_geo((130, 1, 64, 65), True)
    c, rope = C.case_of(g, hd), _Rope(g, hd)
    gq, gk, gv, dout, _, cu_t = c.device_inputs()
    d, ld, z = c.H * hd, gq.stride(0), lib.zeros16(gq.device)
    dq, dk, dv = (E._sentinel((c.M, d)) for _ in range(3))
    o_in = torch.zeros(c.M, d, dtype=BF16, device="cuda")
    xT = torch.zeros(c.B, c.H, hd, c.s_pad, dtype=BF16, device="cuda")
    lse, delta = (torch.zeros(c.B, c.H, c.s_pad, dtype=torch.float32, device="cuda") for _ in range(2))
    tail = (None, cu_t, c.M, c.B, c.H, c.Hkv, c.S, c.s_pad, hd, 1, 1.0 / math.sqrt(hd), None, 0, rope.cs, None, z)
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_attn_bwd_gqa_rope", gq, ld, gk, ld, gv, ld, o_in, d, dout, d, xT, xT, xT, lse, delta, dq, d, dk, d, dv, d, *tail)
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_attn_bwd_nat", gq, ld, gk, ld, gv, ld, o_in, d, dout, d, lse, delta, dq, d, dk, d, dv, d, *tail)
    torch.cuda.synchronize()
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert E._is_sentinel(t), name + " was written by a refused call"


# ------------------------------------------------------------------------------------------------------------------ 4. grouped-query
@pytest.mark.parametrize("layout", C.GQA_LAYOUTS)
@pytest.mark.parametrize("S", C.GQA_SIZES)
@pytest.mark.parametrize("H,Hkv", C.GQA_HEADS)
def test_grouped_query_heads_on_both_dkv_launch_shapes(H, Hkv, S, layout):
    """Register shape: one block per key/value head un-rotates the group's dK in its epilogue (3 roundings).  Workspace shape: the
    per-query-head partials are stored ROTATED in bf16, group_sum_heads_kernel sums them and un-rotates the sum (4 roundings) -- with
    NULL positions through its own `m % S`, with explicit positions and packed through rope_positions[m].  The workspace shape changes
    neither dq (bit-identical to the register shape) nor dv (bit-identical to the workspace shape without rope)."""
    ops = E._ops()
    g = C.gqa_geo(H, Hkv, S, layout)
    total = {}
    for dev, natural in _devs(ops, g):
        what = f"{C.geo_id(g)} hd={dev.c.hd} natural={natural}"
        reg = dev.backward(natural, use_ws=False)
        _merge(total, dev.check(reg, False, what + " register"))
        ws = dev.backward(natural, use_ws=True)
        _merge(total, dev.check(ws, True, what + " group sum"))
        plain = dev.backward(natural, rope=False, use_ws=True)
        assert E._same_bits(ws[0].contiguous(), reg[0].contiguous()), what + ": dq differs between the dK/dV launch shapes"
        assert E._same_bits(ws[2].contiguous(), plain[2].contiguous()), what + ": dv of the group-sum shape depends on rope"
    _record("attention_rope_edges_gqa", total, H=H, Hkv=Hkv, S=S, layout=layout)


# ------------------------------------------------------------------------------------------------------------------ 5. the bit promise
def _unfused(dev, natural, use_ws):
    """attn_bwd without rope into plain tensors, then the rope kernel with direction -1 on dq and dk."""
    c, ops = dev.c, dev.ops
    d, kvd = c.H * c.hd, c.Hkv * c.hd
    outs = tuple(torch.empty(c.M, w, dtype=BF16, device="cuda") for w in (d, kvd, kvd))
    dq, dk, dv = dev.backward(natural, rope=False, use_ws=use_ws, outs=outs)
    ops.rope_inplace(dq, dev.rope.cs, c.S, c.H, c.hd, 1, -1, positions=dev.rope.pos)
    ops.rope_inplace(dk, dev.rope.cs, c.S, c.Hkv, c.hd, 1, -1, positions=dev.rope.pos)
    return dq, dk, dv


@pytest.mark.parametrize("mode", ["null", "explicit"])
@pytest.mark.parametrize("S", C.BITS_SIZES)
def test_fused_adjoint_equals_the_unfused_sequence_bit_for_bit(S, mode):
    """Register-accumulating shape, all backwards: dq, dk and dv with the adjoint in the epilogue equal attn_bwd without rope followed by
    rope_inplace(dir=-1), bit for bit (the epilogue rounds to bf16 where the unfused sequence stored)."""
    ops = E._ops()
    g = C.size_geo(S, True, mode)
    for dev, natural in _devs(ops, g):
        fused, unfused = dev.backward(natural), _unfused(dev, natural, False)
        for name, a, b in zip(("dq", "dk", "dv"), fused, unfused):
            assert E._same_bits(a.contiguous(), b), f"{C.geo_id(g)} hd={dev.c.hd} natural={natural}: {name}"


@pytest.mark.parametrize("layout", C.GQA_LAYOUTS)
def test_grouped_heads_against_the_unfused_sequence(layout):
    """Grouped heads, S = 257.  Register shape: the bit promise holds as above.  Group-sum shape: dq and dv are those of the unfused
    sequence; for dk only the number of elements that differ is RECORDED, never asserted -- from the unfused sequence on the same launch
    shape, and from the register shape, which rotates the summands where the group sum rotates the sum.  The float64 gate of
    test_grouped_query_heads_on_both_dkv_launch_shapes is the contract there."""
    ops = E._ops()
    g = C.gqa_geo(4, 2, 257, layout)
    differing = {}
    for dev, natural in _devs(ops, g):
        what = f"hd{dev.c.hd}_{'natural' if natural else 'transposed'}"
        reg, unfused = dev.backward(natural), _unfused(dev, natural, False)
        for name, a, b in zip(("dq", "dk", "dv"), reg, unfused):
            assert E._same_bits(a.contiguous(), b), f"{C.geo_id(g)} {what}: {name}"
        ws, unfused_ws = dev.backward(natural, use_ws=True), _unfused(dev, natural, True)
        assert E._same_bits(ws[0].contiguous(), unfused_ws[0]) and E._same_bits(ws[2].contiguous(), unfused_ws[2]), what
        differing[what] = dict(of=ws[1].numel(), from_unfused_same_shape=int((E._bits(ws[1]) != E._bits(unfused_ws[1])).sum()),
                               from_register_shape=int((E._bits(ws[1]) != E._bits(reg[1])).sum()))
    from conftest import record_measurement
    record_measurement("attention_rope_edges_group_sum_dk_bits", layout=layout, dk_differing=differing)


# ------------------------------------------------------------------------------------------------------------------ 6. dk / dv strides
@pytest.mark.parametrize("placement", ["stride_4_mod_8", "base_8_byte_aligned"])
def test_dk_dv_the_group_sum_cannot_store_to_take_the_register_shape(placement):
    """group_sum_heads_kernel stores 16-byte vectors into dk / dv.  A leading dimension that is a multiple of 4 but not of 8, or a base
    that is only 8-byte aligned, is legal for the entry points (the epilogues store 8 bytes): with a workspace supplied such a call takes
    the register-accumulating shape -- its bits, and nothing written outside the slices."""
    ops = E._ops()
    g = C.gqa_geo(4, 2, 129, "null")
    for dev, natural in _devs(ops, g):
        c = dev.c
        d, kvd = c.H * c.hd, c.Hkv * c.hd
        want = dev.backward(natural, use_ws=False)
        left, width = (0, kvd + 4) if placement == "stride_4_mod_8" else (4, kvd + 8)
        bufs = [E._sentinel((c.M + 1, width)) for _ in range(2)]
        dk, dv = (b[:c.M, left:left + kvd] for b in bufs)
        assert dk.stride(0) % 4 == 0 and (dk.stride(0) % 8 != 0 or dk.data_ptr() % 16 == 8) and dk.data_ptr() % 8 == 0
        dq = torch.empty(c.M, d, dtype=BF16, device="cuda")
        got = dev.backward(natural, use_ws=True, outs=(dq, dk, dv))
        for name, a, b in zip(("dq", "dk", "dv"), got, want):
            assert E._same_bits(a.contiguous(), b.contiguous()), f"hd={c.hd} natural={natural}: {name} is not the register shape's"
        for b in bufs:
            assert E._is_sentinel(b[c.M:]) and E._is_sentinel(b[:, :left]) and E._is_sentinel(b[:, left + kvd:])

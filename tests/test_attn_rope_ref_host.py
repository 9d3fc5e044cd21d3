"""CPU checks of the rotary-adjoint reference (attn_ref.unrope) and of the inputs tests/test_attention_rope_edges_gpu.py gates the kernels
with: unrope(reference dq / dk) equals float64 autograd of the oracle's attention composed with its apply_rope, taken through to the
un-rotated q / k; and for EVERY geometry of tests/attn_rope_cases.py the kernels' rounding points (reference gradient -> bf16 -> rotate ->
bf16) stay inside the gate while each wrong rotary adjoint a kernel could compute leaves it on at least one element -- so a pass of the
GPU tests means the adjoint is right, and a failure points at a kernel, not at the reference, the gate or the inputs."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_ref as R
import attn_rope_cases as C


def _eq(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("B,S,H,Hkv,hd,causal,lens,packed", [
    (2, 75, 2, 2, 64, True, [75, 33], False),
    (2, 70, 4, 2, 128, False, [1, 64], False),
    (3, 70, 2, 2, 128, True, [70, 1, 33], True),
    (2, 66, 6, 1, 64, False, [66, 40], True),
])
def test_unrope_of_the_reference_is_float64_autograd_through_the_oracles_rope(B, S, H, Hkv, hd, causal, lens, packed):
    """q = apply_rope(q0), k = apply_rope(k0) at explicit positions that are not the row index; attention on the rotated tensors; the
    gradients of q0 / k0 by autograd against unrope(reference(q, k, ...)) -- the reference sees only the rotated tensors, like the kernels."""
    from oracle import llava_oracle as O
    cu = np.concatenate([[0], np.cumsum(lens)]) if packed else None
    rows = R.positions(B, S, cu)
    M, half, T = len(rows), hd // 2, 101
    pos = (5 * np.arange(M) + 2) % T
    cos, sin = O.rope_cos_sin(T, hd, dtype=torch.float64)                          # [T, hd], both halves alike
    cs = torch.stack((cos[:, :half], sin[:, :half]), -1)                            # the kernel's [T, hd/2, 2] layout
    q0, k0, v, dout = (t.double() for t in R.make_inputs("rand", rows, H, Hkv, hd, seed=B + S))
    if not packed:
        for b, L in enumerate(lens):
            dout.view(B, S, -1)[b, L:] = 0
    heads = lambda t, n_heads: t.view(M, n_heads, hd).transpose(0, 1)[None]            # [1, heads, M, hd]
    back = lambda t: t[0].transpose(0, 1).reshape(M, -1)
    cp, sp = cos[torch.from_numpy(pos)], sin[torch.from_numpy(pos)]
    q, k = O.apply_rope(heads(q0, H), heads(k0, Hkv), cp, sp)
    ref = R.reference(back(q), back(k), v, dout, B, S, H, Hkv, hd, causal, lens=None if packed else lens, cu=cu)
    dq, A_dq = R.unrope(ref["dq"], ref["A_dq"], cs, pos, H, hd)
    dk, A_dk = R.unrope(ref["dk"], ref["A_dk"], cs, pos, Hkv, hd)
    rep = H // Hkv
    soft = F.softmax
    for b, (r0, n) in enumerate(R.sample_rows(B, S, cu)):
        sl = slice(r0, r0 + n)
        qs, ks = q0[sl].clone().requires_grad_(True), k0[sl].clone().requires_grad_(True)
        hq = lambda t, n_heads: t.view(1, n, n_heads, hd).transpose(1, 2)
        qr, kr = O.apply_rope(hq(qs, H), hq(ks, Hkv), cp[sl], sp[sl])
        with mock.patch.object(O.F, "softmax", lambda s, dim, dtype=None: soft(s, dim=dim)):        # (the oracle asks for an fp32 softmax)
            out = O.attention(qr, kr.repeat_interleave(rep, 1), hq(v[sl], Hkv).repeat_interleave(rep, 1),
                              lens=None if packed else [lens[b]], causal=causal)
        assert out.dtype == torch.float64
        out.backward(hq(dout[sl], H))
        _eq(dq[sl], qs.grad)
        _eq(dk[sl], ks.grad)
    for g, A in ((dq, A_dq), (dk, A_dk)):                      # the budgets bound the un-rotated gradients
        assert bool((g.abs() <= A * (1 + 1e-12) + 1e-300).all())
    # rotate_half states the pairing: unrope is its transpose
    x, y = torch.randn(M, H * hd, dtype=torch.float64), torch.randn(M, H * hd, dtype=torch.float64)
    fwd = lambda t: back(heads(t, H) * cp + O.rotate_half(heads(t, H)) * sp)
    _eq((fwd(x) * y).sum(), (x * R.unrope(y, y.abs(), cs, pos, H, hd)[0]).sum())


# ------------------------------------------------------------------------------------------------------------------ discrimination
def _rotate(g, cs, pos, heads, hd, form="adjoint"):
    """The rotary adjoint, or one of the wrong forms a kernel could compute, on g [M, heads hd] in float64."""
    M, half = g.shape[0], hd // 2
    t = cs.double()[torch.as_tensor(np.asarray(pos), dtype=torch.long)]
    c, s = t[:, None, :, 0], t[:, None, :, 1]
    g = g.double().view(M, heads, hd)
    lo, hi = g[..., :half], g[..., half:]
    if form == "adjoint":
        out = (lo * c + hi * s, hi * c - lo * s)
    elif form == "sin_sign_of_one_half":
        out = (lo * c + hi * s, hi * c + lo * s)
    elif form == "lo_hi_swapped":                       # the partner lane taken for the lane itself
        out = (hi * c + lo * s, lo * c - hi * s)
    elif form == "forward_rotation":
        out = (lo * c - hi * s, hi * c + lo * s)
    else:
        raise ValueError(form)
    return torch.cat(out, -1).reshape(M, heads * hd)


def _over_gate(got, ref, A, roundings, ok):
    return bool(((got - ref).abs()[ok] > R.gate(A, roundings)[ok]).any())


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("geo", C.all_geometries(), ids=C.geo_id)
def test_every_gpu_geometry_tells_a_wrong_rotary_adjoint_from_a_right_one(geo, hd):
    """Gates as the GPU tests apply them: 3 roundings for dq; for dk the WIDER of its two (4, the group-sum shape), so a mutant that
    leaves it leaves both.  S = 1 is the one exemption: with a single key dS = P (dP - delta) = 0, so dq = dk = 0 whatever the rotation
    does (asserted); there the GPU test pins the zero and the memory discipline only."""
    c, ref = C.case_of(geo, hd), C.rope_reference(geo, hd)
    ok, cs, pos = ref["valid"], ref["cs"], ref["pos"]
    # 1. the kernels' own rounding points stay inside the gate
    worst = {}
    for name, heads, rnd in (("dq", c.H, 3), ("dk", c.Hkv, 3)):
        emu = R.rbf(_rotate(R.rbf(c.ref[name]), cs, pos, heads, hd))
        worst[name] = R.assert_within_budget(emu[ok], ref[name][ok], ref["A_" + name][ok], rnd, f"emulation {name}")
        assert worst[name] <= 2.0 / 3.0 + 1e-3          # two of the three roundings are all the emulation spends
    print(C.geo_id(geo), hd, {n: round(w, 3) for n, w in worst.items()})
    if c.S == 1 and c.cu is None:
        assert float(c.ref["dq"].abs().max()) <= 1e-12 and float(c.ref["dk"].abs().max()) <= 1e-12
        return
    # 2. every wrong form leaves it
    big = C.table(C.table_rows(c, geo.mode) + 1, hd)
    assert torch.equal(big[:-1], cs)
    mutants = {form: (cs, pos) for form in ("sin_sign_of_one_half", "lo_hi_swapped", "forward_rotation")}
    wrong_pos = {"position_off_by_one": pos + 1}
    if geo.mode != "null":
        wrong_pos["row_in_sample_instead_of_the_positions"] = R.positions(c.B, c.S, c.cu)
    if geo.mode == "packed":
        wrong_pos["row_modulo_S"] = np.arange(c.M) % c.S
    for name, heads, rnd in (("dq", c.H, 3), ("dk", c.Hkv, 4)):
        g, want, A = c.ref[name], ref[name], ref["A_" + name]
        for form in mutants:
            assert _over_gate(_rotate(g, cs, pos, heads, hd, form), want, A, rnd, ok), (name, form)
        for what, p in wrong_pos.items():
            assert int(np.max(p)) < big.shape[0]
            assert _over_gate(_rotate(g, big, p, heads, hd), want, A, rnd, ok), (name, what)
    assert _over_gate(c.ref["dk"], ref["dk"], ref["A_dk"], 4, ok), "dk left rotated"
    assert _over_gate(c.ref["dq"], ref["dq"], ref["A_dq"], 3, ok), "dq left rotated"


def test_positions_of_the_gpu_cases_are_what_they_claim():
    """explicit: not the row index, not the same for equal rows of two samples; packed: sample-relative with a start per sample; the table's
    rows are exactly those the positions reach, its values are bf16 numbers, and position 0 is the identity."""
    c = C.case_of(C.size_geo(129, True, "explicit"), 128)
    p = C.row_positions(c, "explicit")
    same = lambda other: int((p == other).sum())             # 7 r + 3 = r (mod 401) has one solution per 401 rows
    assert p.max() < C.T_EXPLICIT and same(np.arange(c.M)) <= 1 and same(R.positions(c.B, c.S)) <= 2 and same(np.roll(p, c.S)) == 0
    c = C.case_of(C.packed_geo((300, 129), True), 64)
    p = C.row_positions(c, "packed")
    assert (p[:300] == np.arange(300)).all() and (p[300:] == 7 + np.arange(129)).all() and C.table_rows(c, "packed") == 300
    assert (p[300:] != (np.arange(300, 429) % c.S)).all()
    cs = C.table(40, 64)
    assert cs.shape == (40, 32, 2) and cs.dtype == torch.float32 and torch.equal(cs, cs.to(R.BF16).float())
    assert torch.equal(cs[0, :, 0], torch.ones(32)) and torch.equal(cs[0, :, 1], torch.zeros(32))
    assert abs(float(cs[1, 0, 0]) - np.cos(1.0)) < 2.0 ** -8 and abs(float(cs[1, 0, 1]) - np.sin(1.0)) < 2.0 ** -8

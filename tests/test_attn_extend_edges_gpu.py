"""GPU tests that root the extend attention family (csrc/attn_split.h's attn_extend_body behind rv_attn_extend_bf16 and
rv_attn_extend_prefix_bf16) the way tests/test_decode_edges_gpu.py roots the decode family:
  (a) staircase needles: every row's softmax is one-hot on its own key, so the output must be that key's V row to the bit -- a row that sees
      one key too many or too few, a chunk owner off by one or a stale key read gives another row;
  (b) random and rescale-stress data against ONE float64 causal reference per document, every element inside attn_ref's two-rounding
      budget (P rounded to bf16 before P V, the bf16 store; softmax, l and the chunk combine are fp32, the 2^-16 term);
  (c) a row's bits do not depend on the rows that share its query tile;
  (d) what the launch may not read or write: unwritten partial slots, the partial buffer past its size, the guards of a strided layout;
  (e) a non-finite V row INSIDE the suffix reaches exactly the rows include/radvlm_hip.h says it may.
Every group size G = 1 .. 8, chunks 64 / 128 / 256, hd 64 / 128, Hkv = 2, one document of 330 positions.  Builders and the windows:
tests/decode_ref.py (its CPU checks, the coverage of the windows among them: tests/test_decode_ref_host.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import attn_ref
from decode_ref import BF16, EXTEND_CHUNKS, EXTEND_L, EXTEND_WINDOWS, extend_rows_exposed, extend_windows, stair_windows, staircase_cache
from test_decode_edges_gpu import _bits, _call, _packed, _same_bits, _sentinel, _Strided

pytestmark = pytest.mark.gpu
HKV = 2                     # kv head 1's column offset is live
L = EXTEND_L


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32).cuda()


def _cu(ns):
    return _i32(np.concatenate([[0], np.cumsum(ns)]))


def _starts(ns):
    return np.concatenate([[0], np.cumsum(ns)])


def _per_head(t, G, hd):
    """[M, Hkv*hd] -> [M, Hkv*G*hd]: kv head k's row for each of its G query heads."""
    return t.view(t.shape[0], HKV, hd).repeat_interleave(G, dim=1).reshape(t.shape[0], HKV * G * hd)


def _extend(ops, q, K, V, rs, ns, G, hd, chunk):
    return ops.attn_extend(q, _packed(K, V).cuda(), _cu(ns), _i32(rs), G * HKV, HKV, hd, HKV * hd, max(ns), chunk=chunk)


# ------------------------------------------------------------------------------------------------ (a) staircase needles
@functools.lru_cache(maxsize=None)
def _stairs(hd, stale):
    """Two sequences per cut window, built once and never written to.  The second has the first's keys and, at the suffix positions, V' =
    9 - V (integers in [1, 8] again): the two may share one prefix row and still must give different rows."""
    wins = stair_windows()
    Ks, Vs, wants = [], [], []
    for k, (r, n) in enumerate(wins):
        _, K, V, want = staircase_cache(r, n, L, hd, HKV, seed=hd + k, stale=stale)
        Ks.append(K), Vs.append(V), wants.append(want)
    for k, (r, n) in enumerate(wins):
        V2 = Vs[k].clone()
        V2[r:r + n] = (9.0 - V2[r:r + n].float()).to(BF16)
        Ks.append(Ks[k]), Vs.append(V2), wants.append(V2[r:r + n].clone())
    rs, ns = [r for r, _ in wins] * 2, [n for _, n in wins] * 2
    return dict(rs=rs, ns=ns, K=torch.stack(Ks), V=torch.stack(Vs), want=torch.cat(wants))


def _split_at_prefix(st, stale):
    """The same keys as a prefix cache (one row per window: the keys [0, r), shared by the window's two sequences) and a tail cache (each
    sequence's own n rows); prefix positions >= r and tail positions >= n hold the stale fill."""
    B0 = len(st["rs"]) // 2
    kvd = st["K"].shape[2]
    T_max = max(st["ns"])
    prefix = torch.empty(B0, L, 2 * kvd, dtype=BF16)
    tail = torch.empty(2 * B0, T_max, 2 * kvd, dtype=BF16)
    packed = torch.cat([st["K"], st["V"]], dim=-1)
    for b, (r, n) in enumerate(zip(st["rs"], st["ns"])):
        fill = torch.full((2 * kvd,), float("nan"))
        if stale == "decoy":
            fill[:kvd], fill[kvd:] = 4.0 + 2 * n, 1000.0
        tail[b, :n], tail[b, n:] = packed[b, r:r + n], fill.to(BF16)
        if b < B0:
            prefix[b, :r], prefix[b, r:] = packed[b, :r], fill.to(BF16)
    return prefix.cuda(), tail.cuda(), list(range(B0)) * 2


@pytest.mark.parametrize("entry", ["extend", "extend_prefix"])
@pytest.mark.parametrize("stale", ["decoy", "nan"])
@pytest.mark.parametrize("hd", [64, 128])
def test_staircase_rows_equal_their_own_v_row_bit_for_bit(hd, stale, entry):
    """Row i sees the keys [0, r + i] and its softmax is one-hot on key r + i: out[i] = V[r + i] to the bit, for every group size and chunk,
    with a decoy (the staircase's next step, V = 1000) or NaN in every position at and past r + n.  extend_prefix: the same keys split at
    prefix_len = r, two sequences per prefix row, the stale fill in prefix positions >= r and tail positions >= n."""
    ops = _ops()
    st = _stairs(hd, stale)
    rs, ns, kvd = st["rs"], st["ns"], HKV * hd
    M, starts = sum(ns), _starts(ns)
    cu, r_dev = _cu(ns), _i32(rs)
    if entry == "extend":
        cache = _packed(st["K"], st["V"]).cuda()
    else:
        prefix, tail, prow = _split_at_prefix(st, stale)
        prow = _i32(prow)
    for G in range(1, 9):
        H = G * HKV
        q = torch.full((M, H * hd), 4.0, dtype=BF16).cuda()
        want = _per_head(st["want"], G, hd)
        for chunk in EXTEND_CHUNKS:
            if entry == "extend":
                got = ops.attn_extend(q, cache, cu, r_dev, H, HKV, hd, kvd, max(ns), chunk=chunk).cpu()
            else:
                got = ops.attn_extend_prefix(q, prefix, tail, cu, prow, r_dev, H, HKV, hd, kvd, max(ns), chunk=chunk).cpu()
            if not torch.equal(_bits(got), _bits(want)):
                row = int((_bits(got) != _bits(want)).any(dim=1).nonzero()[0])
                b = int(np.searchsorted(starts, row, side="right")) - 1
                raise AssertionError(f"G {G} chunk {chunk}: sequence {b} (r {rs[b]}, n {ns[b]}) row {row - starts[b]}: got "
                                     f"{got[row, :4].tolist()} ..., want {want[row, :4].tolist()} ...")


# ------------------------------------------------------------------------------------------------ (b) per-element float64 budget
ALL_G = tuple(range(1, 9))
FAMILY_GS = {"rand": ALL_G, "stair": ALL_G, "big": (1, 2, 7), "stair7": (1, 2, 7), "mixed": (1, 2, 7), "sink": (1, 2, 7)}


@functools.lru_cache(maxsize=8)
def _doc(family, hd, G):
    """One document and its float64 reference per (family, hd, G), shared by the tests below and never written to."""
    return extend_windows(family, L, G * HKV, HKV, hd, EXTEND_WINDOWS, seed=hd + G)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("family", list(FAMILY_GS))
def test_every_element_within_the_two_rounding_budget(family, hd):
    """All windows as one packed batch against the rows of float64 causal attention over the document: |out - ref| <= (2 * 2^-8 + 2^-16)
    P|V| for EVERY element.  Two roundings: P to bf16 before P V, and the bf16 store; the online softmax, l and the chunk combine are
    fp32.  The same count the training forward is held to (tests/attn_ref.py); a derived gate, not a measured one.  Measured on one
    MI355X (record_measurement "attn_extend_edges"): worst 0.795 of the gate (rand, hd 128), 0.67 - 0.70 on the stair families and sink."""
    ops = _ops()
    from conftest import record_measurement
    for G in FAMILY_GS[family]:
        case = _doc(family, hd, G)
        q, K, V = case["q"].cuda(), case["K"], case["V"]
        for chunk in EXTEND_CHUNKS:
            got = _extend(ops, q, K, V, case["rs"], case["ns"], G, hd, chunk)
            d = (got.double().cpu() - case["out"]).abs() / attn_ref.gate(case["A_out"], 2)
            print(f"attn_extend_edges {family} hd {hd} G {G} chunk {chunk}: worst error / gate = {float(d.max()):.4f}")
            worst = attn_ref.assert_within_budget(got, case["out"], case["A_out"], roundings=2, what=f"{family} hd {hd} G {G} chunk {chunk}")
            record_measurement("attn_extend_edges", family=family, hd=hd, G=G, chunk=chunk, worst_ratio=worst)


# ------------------------------------------------------------------------------------------------ (c) a row alone
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("family", ["rand", "stair"])
def test_row_same_bits_with_and_without_its_tile_neighbours(family, hd):
    """Row i of an n-row window against the same query sent alone as a one-row window at r + i (the same keys, NaN past r + i): the chunk
    grid is absolute, stages start at chunk starts, a masked p is exactly 0, 0 * finite adds nothing and MFMA rows are independent, so not
    a bit may differ."""
    ops = _ops()
    wins = [(b, r, n) for b, (r, n) in enumerate(EXTEND_WINDOWS) if n > 1]
    starts = _starts([n for _, n in EXTEND_WINDOWS])
    rows = torch.cat([torch.arange(starts[b], starts[b] + n) for b, _, n in wins])
    pos = torch.cat([torch.arange(r, r + n) for _, r, n in wins])
    for G in (1, 3, 8):
        case = _doc(family, hd, G)
        qd, kd, vd = case["doc"]
        past = torch.arange(L)[None, :] > pos[:, None]
        K1, V1 = kd[None].repeat(len(pos), 1, 1), vd[None].repeat(len(pos), 1, 1)
        K1[past], V1[past] = float("nan"), float("nan")
        cache1 = _packed(K1, V1).cuda()
        q, q1 = case["q"].cuda(), qd[pos].contiguous().cuda()
        assert torch.equal(q1.cpu(), case["q"][rows])
        for chunk in (64, 256):
            full = _extend(ops, q, case["K"], case["V"], case["rs"], case["ns"], G, hd, chunk)
            one = ops.attn_extend(q1, cache1, _cu([1] * len(pos)), _i32(pos.tolist()), G * HKV, HKV, hd, HKV * hd, 1, chunk=chunk)
            assert torch.isfinite(full.float()).all()
            same = (_bits(full)[rows] == _bits(one)).all(dim=1)
            assert bool(same.all()), (family, hd, G, chunk, [(int(pos[i]), int(rows[i])) for i in (~same).nonzero().flatten()[:8]])


# ------------------------------------------------------------------------------------------------ (d) reads and writes
def _raw_extend(q, ld_q, cache, ld_c, bs_c, v_off, cu, r, out, ld_o, part, part_floats, B, M, max_q, H, hd, chunk):
    _call("rv_attn_extend_bf16", q, ld_q, cache, ld_c, bs_c, v_off, cu, r, L, out, ld_o, part, part_floats * 4, B, M, max_q, H, HKV, hd, chunk,
          1.0 / math.sqrt(hd))


@pytest.mark.parametrize("hd", [64, 128])
def test_partial_buffer_max_q_and_strides(hd):
    """Through the C ABI: a partial buffer full of NaN sentinels gives the bits of a zeroed one (the combine reads only slots some
    workgroup wrote) and keeps its tail past the required size; max_q above every row count gives the same bits; the strided layout of
    tests/test_decode_edges_gpu.py, with a window that ends at r + n == L_max, gives the same bits and leaves its guards alone."""
    ops = _ops()
    G = 3
    H, kvd = G * HKV, HKV * hd
    case = _doc("rand", hd, G)
    rs, ns = case["rs"], case["ns"]
    B, M = len(rs), sum(ns)
    assert any(r + n == L for r, n in zip(rs, ns)) and max(ns) < 200 <= M
    q, Kd, Vd = case["q"].cuda(), case["K"].cuda(), case["V"].cuda()
    cache, cu, r_dev = _packed(Kd, Vd), _cu(ns), _i32(rs)
    for chunk in (64, 256):
        want = ops.attn_extend(q, cache, cu, r_dev, H, HKV, hd, kvd, max(ns), chunk=chunk)
        assert torch.isfinite(want.float()).all()
        need = M * H * ((L + chunk - 1) // chunk) * (hd + 2)
        packed = lambda out, part, max_q: _raw_extend(q, H * hd, cache, 2 * kvd, L * 2 * kvd, kvd, cu, r_dev, out, H * hd, part, need, B, M, max_q,
                                                      H, hd, chunk)
        p_nan = _sentinel((need + 256,), torch.float32)
        p_zero = _sentinel((need + 256,), torch.float32)
        p_zero[:need] = 0.0
        tail = _bits(p_nan[need:])
        for part in (p_nan, p_zero):
            out = _sentinel((M, H * hd), BF16)
            packed(out, part, max(ns))
            assert _same_bits(out, want), (hd, chunk)
            assert torch.equal(_bits(part[need:]), tail), (hd, chunk, "the partial buffer past part_bytes")
        out = _sentinel((M, H * hd), BF16)
        packed(out, _sentinel((need,), torch.float32), 200)
        assert _same_bits(out, want), (hd, chunk, "max_q = 200")
        s = _Strided(q, Kd, Vd)
        _raw_extend(s.q(), s.ld_q, s.flat, s.ld_c, s.bs_c, s.v_off, cu, r_dev, s.out(), s.ld_o, _sentinel((need,), torch.float32), need, B, M,
                    max(ns), H, hd, chunk)
        assert _same_bits(s.out(), want), (hd, chunk, "strided")
        assert s.guards_untouched(), (hd, chunk)


# ------------------------------------------------------------------------------------------------ (e) the suffix's own rows
POISONED = ((48, 17), (63, 66), (250, 70))


@pytest.mark.parametrize("poison", ["inf", "nan"])
@pytest.mark.parametrize("hd", [64, 128])
def test_a_non_finite_suffix_v_row_reaches_its_own_tile_only(hd, poison):
    """V of the last suffix key of three windows set to +inf or NaN.  The last row, which sees the key, is non-finite.  The header's contract
    for the others: a suffix key a row may not see gets an exact-zero weight (it is not skipped), so the rows that share the key's query tile
    and chunk are non-finite too (0 * inf); every other row of the batch -- other sequences, other tiles, rows of the tile that own no
    partial of that chunk -- keeps its bits."""
    ops = _ops()
    bad = float("inf") if poison == "inf" else float("nan")
    starts = _starts([n for _, n in EXTEND_WINDOWS])
    for G in (1, 3, 8):
        case = _doc("rand", hd, G)
        V2 = case["V"].clone()
        for r, n in POISONED:
            V2[EXTEND_WINDOWS.index((r, n)), r + n - 1] = bad
        q = case["q"].cuda()
        for chunk in (64, 256):
            clean = _extend(ops, q, case["K"], case["V"], case["rs"], case["ns"], G, hd, chunk)
            dirty = _extend(ops, q, case["K"], V2, case["rs"], case["ns"], G, hd, chunk)
            hit = torch.zeros(clean.shape[0], dtype=torch.bool)
            for r, n in POISONED:
                b = EXTEND_WINDOWS.index((r, n))
                exposed = extend_rows_exposed(r, n, G, chunk)
                assert n - 1 in exposed
                hit[[starts[b] + i for i in exposed]] = True
            same = (_bits(clean) == _bits(dirty)).all(dim=1)
            finite = torch.isfinite(dirty.float()).all(dim=1).cpu()
            nonfinite = (~torch.isfinite(dirty.float())).all(dim=1).cpu()
            assert bool(same[~hit].all()), (hd, poison, G, chunk, "rows outside the key's tile and chunk", (~same & ~hit).nonzero().flatten().tolist())
            assert bool(finite[~hit].all())
            assert bool(nonfinite[hit].all()), (hd, poison, G, chunk, "rows of the key's tile and chunk", (~nonfinite & hit).nonzero().flatten().tolist())

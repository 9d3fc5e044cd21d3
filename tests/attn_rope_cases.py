"""What tests/test_attention_rope_edges_gpu.py runs, stated once: the geometries, the rotary table and the position of every token row, and
the float64 reference of the attention backward with the rotary adjoint in its epilogues (attn_ref.reference + attn_ref.unrope).  Plain
torch / numpy on the CPU, so tests/test_attn_rope_ref_host.py can show without a GPU that EVERY geometry listed here tells a wrong rotary
adjoint from a right one.  The inputs and the un-rotated reference are the cached Case objects of tests/test_attention_edges_gpu.py.

Position modes:
    null      padded batch, rope_positions = NULL: the kernels take the row's index inside its sample; the table has S rows.
    explicit  padded batch, rope_positions[row] = (7 row + 3) % 401 over the B S rows of the batch, a table of 401 rows: not the row index,
              not monotonic, different for the same row of two samples.
    packed    packed batch (positions are required): row r of sample b sits at 7 b + r, a sample that continues 7 b tokens of context --
              `row % S` and the bare index inside the sample both differ from it in every sample but the first.
The table is built from float64 cos / sin and rounded through bf16, as the ABI asks of the caller; ops.rope_table is not used."""
import collections
import functools

import numpy as np
import torch

import attn_ref as R
from test_attention_edges_gpu import _case

THETA = 10000.0
T_EXPLICIT = 401
SAMPLE_SHIFT = 7

Geo = collections.namedtuple("Geo", "S H Hkv causal lens cu_lens mode")

SIZES = (1, 63, 64, 65, 127, 129, 255, 257)             # either side of 64 (key tile, natural dK/dV block), 128 (natural dQ block), 256 (transposed dQ block)
PAD_S, PAD_LENS = 200, ((1, 200), (63, 64), (199, 64))
PACKED = ((130, 1, 64, 65), (300, 129))
GQA_HEADS, GQA_SIZES = ((4, 2), (6, 1)), (129, 257)
GQA_LAYOUTS = ("null", "explicit", "packed")
BITS_SIZES = (65, 257)


def size_geo(S, causal, mode):
    return Geo(S, 2, 2, causal, None, None, mode)


def padding_geo(lens, causal, mode):
    return Geo(PAD_S, 2, 2, causal, tuple(lens), None, mode)


def packed_geo(cu_lens, causal, H=2, Hkv=2):
    return Geo(None, H, Hkv, causal, None, tuple(cu_lens), "packed")


def gqa_geo(H, Hkv, S, layout):
    return packed_geo((S, 66), True, H, Hkv) if layout == "packed" else Geo(S, H, Hkv, True, None, None, layout)


def all_geometries():
    """Every geometry some GPU test runs (each at head_dim 64 and 128), without repeats."""
    g = [size_geo(S, causal, mode) for S in SIZES for causal in (True, False) for mode in ("null", "explicit")]
    g += [padding_geo(lens, causal, mode) for lens in PAD_LENS for causal in (True, False) for mode in ("null", "explicit")]
    g += [packed_geo(cu, causal) for cu in PACKED for causal in (True, False)]
    g += [gqa_geo(H, Hkv, S, layout) for H, Hkv in GQA_HEADS for S in GQA_SIZES for layout in GQA_LAYOUTS]
    return list(dict.fromkeys(g))


def geo_id(g):
    shape = "cu" + "-".join(map(str, g.cu_lens)) if g.cu_lens else f"S{g.S}" + ("-lens" + "-".join(map(str, g.lens)) if g.lens else "")
    return f"{shape}-H{g.H}k{g.Hkv}-{'causal' if g.causal else 'full'}-{g.mode}"


def case_of(g, hd):
    """The cached inputs and un-rotated reference (test_attention_edges_gpu.Case; never modified)."""
    if g.cu_lens is not None:
        return _case("rand", None, None, g.H, g.Hkv, hd, g.causal, cu_lens=g.cu_lens)
    return _case("rand", 2, g.S, g.H, g.Hkv, hd, g.causal, lens=g.lens)


def table(rows, hd):
    """fp32 [rows, hd/2, 2] (cos, sin) of angle position * THETA^(-2 e / hd), from float64 trig, values rounded through bf16."""
    inv = THETA ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd)
    ang = torch.outer(torch.arange(rows, dtype=torch.float64), inv)
    return torch.stack((ang.cos(), ang.sin()), -1).to(R.BF16).float().contiguous()


def row_positions(c, mode):
    """int64 [M]: the table row of every token row of Case c."""
    if mode == "null":
        return R.positions(c.B, c.S, c.cu)
    if mode == "explicit":
        assert c.cu is None
        return (7 * np.arange(c.M) + 3) % T_EXPLICIT
    assert mode == "packed" and c.cu is not None
    return np.concatenate([SAMPLE_SHIFT * b + np.arange(n) for b, (_, n) in enumerate(c.spans)])


def table_rows(c, mode):
    """Rows of the table in use: exactly what the positions can reach."""
    return T_EXPLICIT if mode == "explicit" else int(row_positions(c, mode).max()) + 1


@functools.lru_cache(maxsize=None)
def rope_reference(g, hd):
    """{cs, pos, dq, A_dq, dk, A_dk, dv, A_dv, valid}: the float64 reference of one backward call with rope=(cs, pos).  Computed once per
    (geometry, head_dim) and shared; do not modify."""
    c = case_of(g, hd)
    pos, cs = row_positions(c, g.mode), table(table_rows(c, g.mode), hd)
    dq, A_dq = R.unrope(c.ref["dq"], c.ref["A_dq"], cs, pos, c.H, hd)
    dk, A_dk = R.unrope(c.ref["dk"], c.ref["A_dk"], cs, pos, c.Hkv, hd)
    return dict(cs=cs, pos=pos, dq=dq, A_dq=A_dq, dk=dk, A_dk=A_dk, dv=c.ref["dv"], A_dv=c.ref["A_dv"], valid=c.valid)

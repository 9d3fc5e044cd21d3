"""GPU tests of the data-movement and optimizer kernels of radvlm_amd/csrc/ops.hip -- gather / segment sum / 2x2 max over rows, the CLIP
embedding kernels, the image normalisation, the transposes, the dropout mask and its consumers, the casts and AdamW -- at the widths, strides
and values where they can go wrong: the second trip of the 8-wide row loops (d > 2048), leading dimensions wider than the data, scattered and
aliased output rows, ties / signed zeros / NaN in the max, ragged and zero-length transposes, rounding ties of the casts, and AdamW steps that
eps or the weight decay dominates.

Nearly all of these kernels have one right answer and are compared BIT FOR BIT with tests/dataops_ref.py (its own CPU checks:
tests/test_dataops_ref_host.py); the summing kernels and AdamW are held per element to gates derived in their tests.  Every output buffer
carries a NaN sentinel in one extra row and in the columns beyond d, compared bit for bit afterwards; everything a kernel must not read is NaN.
Layouts the ops wrappers do not offer go through the C ABI (radvlm_amd.lib.call).  Each test appends its worst ratio of the gate (0 for exact
tests) to the measurement log (conftest.record_measurement)."""
import ctypes

import numpy as np
import pytest
import torch

import dataops_ref as D
from dataops_ref import BF16

pytestmark = pytest.mark.gpu

F32 = torch.float32
ROW_DS = (8, 2048, 2056)          # one vector; the last width one trip of 256 threads x 8 covers; one vector into the second trip
SEEDS = (0, (1 << 32) + 5, (1 << 63) - 1)
NAN, INF = float("nan"), float("inf")


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _call(name, *args):
    from radvlm_amd import lib
    lib.call(name, *args)


def _record(test, worst=0.0, **kw):
    from conftest import record_measurement
    record_measurement(test, worst_ratio_of_gate=worst, **kw)


_INT = {BF16: torch.int16, F32: torch.int32, torch.uint8: torch.uint8}
_SENT = {BF16: 0x7fc5, F32: 0x7fc5a5a5, torch.uint8: 0xAB}


def _bits(t):
    return t.contiguous().view(_INT[t.dtype]).cpu()


def _sent(shape, dtype=BF16, device="cuda"):
    """A buffer of one NaN bit pattern (bf16 0x7fc5 / fp32 0x7fc5a5a5; uint8 0xAB): no kernel here produces it, and a read of it shows."""
    return torch.full(tuple(shape), _SENT[dtype], dtype=_INT[dtype], device=device).view(dtype)


def _assert_bits(got, want, what, any_nan=False):
    """got (GPU) == want (CPU) bit for bit, shape and dtype included.  any_nan: where want is a NaN other than the sentinel, got may be any NaN
    other than the sentinel (a conversion may quieten a NaN or drop its payload)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = _bits(got), _bits(want)
    bad = g != w
    if any_nan:
        s = _SENT[want.dtype]
        bad &= ~(torch.isnan(want) & (w != s) & torch.isnan(got.cpu()) & (g != s))
    if bool(bad.any()):
        i = int(bad.reshape(-1).int().argmax())
        msg = f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat {i}: got bits {int(g.reshape(-1)[i]) & 0xffffffff:#x}, want {int(w.reshape(-1)[i]) & 0xffffffff:#x}"
        print(msg)
        raise AssertionError(msg)


def _randn(shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


def _nonzero(shape, seed, std=1.0):
    """bf16 values with |x| >= 0.25 std: no zeros, so a zero in an output is the kernel's."""
    x = _randn(shape, seed, std)
    return (x + torch.sign(x) * 0.25 * std + (x == 0) * std).to(BF16)


def _rand_bits(shape, seed):
    """Random finite bf16 bit patterns (any sign, exponent and mantissa; no inf / NaN): a copy that misplaces one element shows."""
    b = torch.randint(0, 1 << 16, tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    b = torch.where((b >> 7) & 0xFF == 0xFF, b & ~0x4000, b)
    return (b - ((b >= 1 << 15).int() << 16)).to(torch.int16).view(BF16)


def _padded(t, ld, extra_rows=1):
    """t (CPU [rows, d]) on the GPU inside a sentinel buffer [rows + extra_rows, ld]: (buffer, its [rows, d] view with row stride ld)."""
    rows, d = t.shape
    buf = _sent((rows + extra_rows, ld), t.dtype)
    buf[:rows, :d] = t.cuda()
    return buf, buf[:rows, :d]


def _expect(shape, rows, ref, dtype=BF16):
    """The expected content of an output buffer (CPU): the sentinel everywhere but ref ([len(rows), d]) in the named rows' first d columns."""
    e = _sent(shape, dtype, "cpu")
    e[torch.as_tensor(list(rows), dtype=torch.int64), :ref.shape[1]] = ref
    return e


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("d", ROW_DS)
def test_gather_rows_three_index_kinds_and_wide_strides(d):
    ops = _ops()
    ta, tb = _rand_bits((6, d), d + 1), _rand_bits((4, d), d + 2)
    _, tav = _padded(ta, d + 8)
    _, tbv = _padded(tb, d + 16)
    idx = [0, 5, -1, -2, -5, 3, 3, 5, 0, -5, -1, -3]                    # first / last row of each table, zero rows, repeats
    out = _sent((len(idx) + 1, d + 24))
    ops.gather_rows(_i32(idx), d, tav, tbv, out=out[:len(idx), :d])
    _assert_bits(out, _expect(out.shape, range(len(idx)), D.gather_rows(idx, d, ta, tb)), f"gather_rows d={d}")
    idx = [5, -1, 0, 0, 2]                                              # no second table
    out = _sent((len(idx) + 1, d + 24))
    ops.gather_rows(_i32(idx), d, tav, None, out=out[:len(idx), :d])
    _assert_bits(out, _expect(out.shape, range(len(idx)), D.gather_rows(idx, d, ta)), f"gather_rows d={d}, table_b None")
    _record("dataops_gather_rows", d=d)


# ------------------------------------------------------------------------------------------------ max of four rows
# (slot 0, 1, 2, 3) of one column; the expected winner is the reference's scan rule (its own CPU test states them)
MAX4_PLANTED = [(1, 1, 0, 0), (0, 1, 1, -1), (0, 2, 2, 2), (2, 2, 2, 2), (0.0, -0.0, -1, -1), (-0.0, 0.0, -1, -1), (-INF, -INF, -INF, -INF),
                (NAN, 5, 6, 7), (5, NAN, 6, 7), (5, 6, NAN, 7), (5, 6, 7, NAN), (NAN, 5, NAN, 9), (3, NAN, 9, NAN)]
MAX4_IDX = [[0, 1, 2, 3], [9, 4, 7, 5], [10, 6, 8, 11], [12, 12, 12, 12]]          # the last window: one row four times; row 13 in no window


def _max4_src(d):
    src = _nonzero((14, d), 3 * d)
    for k, vals in enumerate(MAX4_PLANTED):
        win, col = MAX4_IDX[k % 3], k // 3
        for c in {col, d - 8 + col}:                                   # also in the last vector of the row (the second trip at d = 2056)
            for j in range(4):
                src[win[j], c] = vals[j]
    src[12, 1], src[12, 2] = NAN, -0.0
    return src


@pytest.mark.parametrize("d", ROW_DS)
def test_max4_rows_fwd_ties_zeros_nans_and_in_place(d):
    _ops()
    src = _max4_src(d)
    n, out_row = len(MAX4_IDX), [5, 0, 3, 2]
    ref, which_ref = D.max4_fwd(src, MAX4_IDX)
    for k, vals in enumerate(MAX4_PLANTED):                             # the planted columns are where they are meant to be
        assert int(which_ref[k % 3, k // 3]) == D.max4_fwd(torch.tensor(vals).to(BF16)[:, None], [[0, 1, 2, 3]])[1].item()
    idx4 = _i32(MAX4_IDX)
    _, srcv = _padded(src, d + 8)
    out, which = _sent((7, d + 16)), _sent((n + 1, d), torch.uint8)
    _call("rv_max4_rows_fwd", srcv, d + 8, idx4, _i32(out_row), n, out, d + 16, which, d)
    _assert_bits(out, _expect(out.shape, out_row, ref), f"max4_rows_fwd d={d}", any_nan=True)
    _assert_bits(which, _expect(which.shape, range(n), which_ref, torch.uint8), f"max4_rows_fwd which d={d}")
    # in place, as the engine pools its feature table: out is src, the pooled rows lie behind the source rows
    table, _ = _padded(src, d + 8, extra_rows=n + 1)
    rows2 = [16, 14, 17, 15]
    which2 = _sent((n + 1, d), torch.uint8)
    _call("rv_max4_rows_fwd", table, d + 8, idx4, _i32(rows2), n, table, d + 8, which2, d)
    want = _sent(table.shape, BF16, "cpu")
    want[:14, :d] = src
    want[torch.tensor(rows2), :d] = ref
    _assert_bits(table, want, f"max4_rows_fwd in place d={d}", any_nan=True)
    assert torch.equal(_bits(table[rows2, :d]), _bits(out[out_row, :d])) and torch.equal(which2.cpu(), which.cpu())
    _record("dataops_max4_rows_fwd", d=d)


@pytest.mark.parametrize("d", ROW_DS)
def test_max4_rows_bwd_routes_each_gradient_and_in_place(d):
    _ops()
    src = _max4_src(d)
    idx = MAX4_IDX[:3]                                                  # every source row in exactly one window
    n = len(idx)
    dout = _nonzero((n, d), 5 * d)
    dout[1, 0] = -0.0
    e = torch.arange(d)
    hand = torch.stack([(e + s) % 4 for s in range(n)]).to(torch.uint8)                 # every slot, in every lane position
    dout_row = [2, 0, 4]
    dbuf = _sent((6, d + 8))
    dbuf[dout_row, :d] = dout.cuda()
    for name, which in (("forward", D.max4_fwd(src, idx)[1]), ("hand-made", hand)):
        dsrc = _sent((15, d + 16))
        _call("rv_max4_rows_bwd", dbuf, d + 8, _i32(idx), _i32(dout_row), n, which.cuda(), dsrc, d + 16, d)
        ref = D.max4_bwd(dout, idx, range(n), which, _sent((12, d), BF16, "cpu"))
        _assert_bits(dsrc, _expect(dsrc.shape, range(12), ref), f"max4_rows_bwd d={d} which={name}")          # rows 12.. keep the sentinel
        each = torch.stack([ref[idx[s][j]] for s in range(n) for j in range(4)]).view(n, 4, d)
        assert torch.equal((each != 0).sum(1), (dout != 0).long())     # one of the four rows took the gradient, the others +0
        # in place (the engine's dfeat): the pooled rows' gradients lie behind the source rows of the same buffer
        buf = _sent((16, d + 8))
        rows2 = [13, 12, 14]
        buf[rows2, :d] = dout.cuda()
        _call("rv_max4_rows_bwd", buf, d + 8, _i32(idx), _i32(rows2), n, which.cuda(), buf, d + 8, d)
        want = _sent(buf.shape, BF16, "cpu")
        want[:12, :d] = ref
        want[torch.tensor(rows2), :d] = dout
        _assert_bits(buf, want, f"max4_rows_bwd in place d={d} which={name}")
    _record("dataops_max4_rows_bwd", d=d)


# ------------------------------------------------------------------------------------------------ segment sums
SEG_LENS = (0, 1, 2, 4, 5, 33)
SEG_OUT = (7, 2, 9, 0, 4, 5)                                            # of 11 rows: 1, 3, 6, 8, 10 are named by no segment


def _segments(d, weighted):
    nsrc = 40
    scale = torch.tensor([(1e-3, 1.0, 300.0)[r % 3] for r in range(nsrc)])
    src = (_randn((nsrc, d), 7 * d + 1) * scale[:, None]).to(BF16)
    off = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int32)
    g = torch.Generator().manual_seed(11)
    pos = torch.randint(0, nsrc, (int(off[-1]),), generator=g).tolist()
    pos[1:3] = [6, 6]                                                   # the segment of two: one row twice
    pos[3:7] = [0, 1, 2, 0]                                             # scales 1e-3, 1, 300 in one segment, and a repeat
    w = None
    if weighted:
        w = torch.rand(len(pos), generator=g) * 2 - 1
        w[1], w[2] = 0.75, -0.75                                        # (w, -w) on the same source row
        w[3], w[4], w[5] = 0.0, 1.0, -1.5
        w = w.float()
    return src, off, pos, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", ROW_DS)
def test_segment_sum_rows_per_element_and_in_place(d, weighted):
    """Gate per element: |got - ref| <= ulp_bf16(ref) / 2 + J 2^-23 A, A = sum_j |w_j| |src_j|: J fp32 accumulations each cost at most
    2^-24 A (2x margin), then one bf16 store."""
    ops = _ops()
    src, off, pos, w = _segments(d, weighted)
    ref, A, J = D.segment_sum(src, off, pos, w)
    nseg = len(SEG_LENS)
    _, srcv = _padded(src, d + 8)
    out = _sent((12, d + 16))
    args = (_i32(off), _i32(pos)) + ((w.cuda(),) if weighted else ()) + (_i32(SEG_OUT),)
    fn = ops.weighted_segment_sum_rows if weighted else ops.segment_sum_rows
    fn(srcv, *args, out[:11, :d])
    got = out[list(SEG_OUT), :d]
    bound = D.ulp_bf16(ref) / 2 + J[:, None].double() * 2.0 ** -23 * A
    worst = D.assert_within(got, ref, bound, f"segment_sum d={d} weighted={weighted}")
    want = _expect(out.shape, SEG_OUT, got.cpu())                       # the values are gated above; here: nothing else was written
    _assert_bits(out, want, f"segment_sum guards d={d} weighted={weighted}")
    assert int(_bits(got[0]).abs().max()) == 0                          # the empty segment: +0, bit for bit
    if not weighted:
        _assert_bits(got[1], src[pos[0]], "a one-row segment is a copy")
    # in place, as the engine resamples its feature table and takes the adjoint in dfeat: outputs behind every source row, out is src
    table, _ = _padded(src, d + 8, extra_rows=nseg + 1)
    rows2 = [45, 40, 43, 41, 44, 42]
    args2 = args[:-1] + (_i32(rows2),)
    fn(table[:, :d], *args2, table[:, :d])
    want = _sent(table.shape, BF16, "cpu")
    want[:40, :d] = src
    want[torch.tensor(rows2), :d] = got.cpu()
    _assert_bits(table, want, f"segment_sum in place d={d} weighted={weighted}")
    _record("dataops_segment_sum_rows", worst, d=d, weighted=weighted)


# ------------------------------------------------------------------------------------------------ CLIP embeddings
@pytest.mark.parametrize("n,P,d", [(1, 1, 8), (3, 5, 136), (3, 43, 16), (2, 3, 2056)])
def test_add_pos_rows(n, P, d):
    """(3, 5, 136) is 255 vectors and (3, 43, 16) 258: either side of one 256-thread block."""
    ops = _ops()
    x, pos = _nonzero((n * P, d), n + P + d), _nonzero((P, d), n + P + d + 1, 0.1)
    xb, pb = _sent((n * P + 1, d)), _sent((P + 1, d))
    xb[:n * P], pb[:P] = x.cuda(), pos.cuda()
    ops.add_pos_rows(xb[:n * P], pb[:P], n, P)
    _assert_bits(xb, _expect(xb.shape, range(n * P), D.add_pos(x, pos, n, P)), f"add_pos_rows {(n, P, d)}")
    _assert_bits(pb, _expect(pb.shape, range(P), pos), "pos is read only")
    _record("dataops_add_pos_rows", n=n, P=P, d=d)


@pytest.mark.parametrize("n,P,d", [(1, 1, 8), (3, 4, 136), (2, 5, 2056)])
def test_clip_embed(n, P, d):
    _ops()
    po, cls, pos = _nonzero((n * P, d), n + d), _nonzero((d,), n + d + 1, 0.1), _nonzero((P + 1, d), n + d + 2, 0.1)
    pob, posb, clsb = _sent((n * P + 1, d)), _sent((P + 2, d)), _sent((2, d))
    pob[:n * P], posb[:P + 1], clsb[0] = po.cuda(), pos.cuda(), cls.cuda()
    out = _sent((n * (P + 1) + 1, d))
    _call("rv_clip_embed", pob, clsb, posb, out, n, P, d)
    _assert_bits(out, _expect(out.shape, range(n * (P + 1)), D.clip_embed(po, cls, pos, n, P)), f"clip_embed {(n, P, d)}")
    _record("dataops_clip_embed", n=n, P=P, d=d)


@pytest.mark.parametrize("n,H,W,p,kp", [(1, 2, 2, 2, 16), (2, 28, 42, 14, 592), (1, 30, 17, 14, 588)])
def test_im2col_patches_non_square_ragged_and_padded(n, H, W, p, kp):
    _ops()
    pix = _rand_bits((n, 3, H, W), H * W)
    pb = _sent((n * 3 * H * W + 8,))
    pb[:pix.numel()] = pix.reshape(-1).cuda()
    rows = n * (H // p) * (W // p)
    out = _sent((rows + 1, kp))
    _call("rv_im2col_patches", pb, out, n, H, W, p, kp)
    ref = D.im2col(pix, p, kp)
    assert kp == 3 * p * p or int(_bits(ref[:, 3 * p * p:]).abs().max()) == 0          # the padded columns: +0
    _assert_bits(out, _expect(out.shape, range(rows), ref), f"im2col {(n, H, W, p, kp)}")
    _record("dataops_im2col_patches", n=n, H=H, W=W, p=p, kp=kp)


@pytest.mark.parametrize("kind", ["clip", "siglip"])
def test_normalize_tiles_u8_every_byte_value(kind):
    _ops()
    from radvlm_amd.llava.mm_utils import ClipImageProcessor, SigLipImageProcessor
    tile, n, gh, gw = 16, 2, 2, 3
    proc = ClipImageProcessor(tile) if kind == "clip" else SigLipImageProcessor(size=(tile, tile), crop_size={"height": tile, "width": tile})
    factor = getattr(proc, "rescale_factor", 1.0 / 255)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(n, gh * tile, gw * tile, 3), dtype=np.uint8)
    for c in range(3):                                                  # every byte value in every channel, in a different tile each
        img[c % n, tile:2 * tile, c * tile:(c + 1) * tile, c] = rng.permutation(256).astype(np.uint8).reshape(tile, tile)
    ib = torch.full((img.size + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    ib[:img.size] = torch.from_numpy(img).reshape(-1).cuda()
    per = 3 * tile * tile
    out = _sent((n * gh * gw + 1, per))
    m3, s3 = (ctypes.c_float * 3)(*proc.image_mean), (ctypes.c_float * 3)(*proc.image_std)
    _call("rv_normalize_tiles_u8", ib, out, n, gh, gw, tile, proc.normalize_mode, float(factor), m3, s3)
    ref = D.normalize_tiles(img, tile, proc.image_mean, proc.image_std, proc.normalize_mode, factor, gh, gw)
    _assert_bits(out, _expect(out.shape, range(n * gh * gw), ref.reshape(n * gh * gw, per)), f"normalize_tiles_u8 {kind}")
    _record("dataops_normalize_tiles_u8", kind=kind)


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("R,C,r_pad", [(1, 1, 8), (63, 7, 64), (64, 64, 64), (65, 72, 72), (70, 65, 200)])
def test_transpose_plain_scalar_columns_wide_strides_and_padding(R, C, r_pad):
    """C % 8 != 0 takes the scalar loads; r_pad = 200 leaves two whole 64-row tiles of zeros past R = 70."""
    _ops()
    x = _rand_bits((R, C), R * C)
    in_ld, out_ld = (C + 7) // 8 * 8 + 8, r_pad + 8
    xb, _ = _padded(x, in_ld)                                           # NaN beyond column C and in the row after R
    out = _sent((C + 1, out_ld))
    _call("rv_transpose_bf16", xb, in_ld, 0, 0, out, out_ld, 0, 0, R, C, r_pad, 1, 1, 0)
    _assert_bits(out, _expect(out.shape, range(C), D.transpose(x, r_pad)[0, 0]), f"transpose {(R, C, r_pad)}")
    _record("dataops_transpose_plain", R=R, C=C, r_pad=r_pad)


@pytest.mark.parametrize("perm32", [False, True])
@pytest.mark.parametrize("S,s_pad", [(50, 64), (70, 128)])
def test_transpose_heads_from_a_fused_buffer(S, s_pad, perm32):
    ops = _ops()
    B, H, hd = 2, 3, 64
    k = _rand_bits((B * S, H * hd), S + s_pad)
    qkv = _sent((B * S + 1, 3 * H * hd))                                # q and v stay NaN: only the k columns may be read
    qkv[:B * S, H * hd:2 * H * hd] = k.cuda()
    out = _sent((B * H * hd + 1, s_pad))
    ops.transpose_heads(qkv[:B * S, H * hd:2 * H * hd], B, S, H, hd, s_pad, out=out, perm32=perm32)
    ref = D.transpose(k, s_pad, perm32=perm32, B=B, H=H).reshape(B * H * hd, s_pad)
    _assert_bits(out, _expect(out.shape, range(B * H * hd), ref), f"transpose_heads S={S} s_pad={s_pad} perm32={perm32}")
    _record("dataops_transpose_heads", S=S, s_pad=s_pad, perm32=perm32)


@pytest.mark.parametrize("perm32", [False, True])
def test_transpose_heads_varlen_with_an_empty_sample(perm32):
    ops = _ops()
    B, H, hd, S, s_pad = 3, 3, 64, 70, 128
    cu = [0, 0, 37, 107]
    k = _rand_bits((cu[-1], H * hd), 77)
    kb = _sent((cu[-1] + 3, H * hd + 8))                                # the rows after the last sample and the columns beyond H hd are NaN
    kb[:cu[-1], :H * hd] = k.cuda()
    out = _sent((B * H * hd + 1, s_pad))
    ops.transpose_heads(kb[:, :H * hd], B, S, H, hd, s_pad, out=out, perm32=perm32, cu=_i32(cu))
    ref = D.transpose(k, s_pad, perm32=perm32, cu=cu, B=B, H=H)
    assert int(_bits(ref[0]).abs().max()) == 0                          # the sample without rows: all +0
    _assert_bits(out, _expect(out.shape, range(B * H * hd), ref.reshape(B * H * hd, s_pad)), f"transpose_heads varlen perm32={perm32}")
    _record("dataops_transpose_heads_varlen", perm32=perm32)


# ------------------------------------------------------------------------------------------------ casts, add
def _f32_bits(words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).view(F32)


CAST_WORDS = [0x3F808000, 0x3F818000,               # exact ties: the even neighbour is below / above
              0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,      # just above and below each
              0xBF808000, 0xBF818000, 0xBF808001, 0xBF817FFF,
              0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7FA00000,
              0x7F7F7FFF,                           # the largest value that still rounds to the finite maximum 0x7F7F
              0x7F7F8000, 0xFF7F8000,               # the tie above it: to even, which is inf
              0x00000001, 0x007FFFFF, 0x00400000, 0x80000001, 0x00008000, 0x00018000, 0x00807FFF]          # denormals, and ties among them


@pytest.mark.parametrize("n", [1, 7, 257])
def test_cast_f32_to_bf16_round_to_nearest_even(n):
    _ops()
    vals = torch.cat((_f32_bits(CAST_WORDS), torch.tensor([3.4e38, -3.4e38], dtype=F32), _randn((257,), 5)))
    assert float(vals[len(CAST_WORDS)].to(BF16)) == INF               # 3.4e38 lies above the last tie: it overflows
    for start in range(0, len(CAST_WORDS) + 2, n):                    # every special value at n = 1 and 7 too (random values follow them)
        x = vals[start:start + n]
        xb, out = _sent((n + 1,), F32), _sent((n + 1,))
        xb[:n] = x.cuda()
        _call("rv_cast_f32_to_bf16", xb, out, n)
        want = _sent((n + 1,), BF16, "cpu")
        want[:n] = x.to(BF16)
        _assert_bits(out, want, f"cast_f32_to_bf16 n={n} start={start}", any_nan=True)
    _record("dataops_cast_f32_to_bf16", n=n)


def test_cast_bf16_to_f32_every_bit_pattern():
    _ops()
    n = 1 << 16
    x = (torch.arange(n, dtype=torch.int32) - ((torch.arange(n) >= 1 << 15).int() << 16)).to(torch.int16).view(BF16)
    xb, out = _sent((n + 1,)), _sent((n + 1,), F32)
    xb[:n] = x.cuda()
    _call("rv_cast_bf16_to_f32", xb, out, n)
    want = _sent((n + 1,), F32, "cpu")
    want[:n] = x.float()
    _assert_bits(out, want, "cast_bf16_to_f32", any_nan=True)
    finite = ~torch.isnan(x)
    assert torch.equal(_bits(out[:n])[finite], (x.view(torch.int16).int() << 16)[finite])      # a widening: the pattern, shifted
    _record("dataops_cast_bf16_to_f32")


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2049])
def test_add_bf16_vector_body_and_scalar_tail(n):
    _ops()
    a = (_randn((n,), n) * torch.tensor([(1.0, 2.0 ** 20, 2.0 ** -20, 1e-3)[i % 4] for i in range(n)])).to(BF16)
    b = (_randn((n,), n + 1) * torch.tensor([(2.0 ** -20, 1.0, 1.0, 300.0)[i % 4] for i in range(n)])).to(BF16)       # 20 binary orders apart
    b[::5] = -a[::5]                                                    # exact cancellation: +0
    ab, bb, y = _sent((n + 1,)), _sent((n + 1,)), _sent((n + 1,))
    ab[:n], bb[:n] = a.cuda(), b.cuda()
    _call("rv_add_bf16", ab, bb, y, n)
    want = _sent((n + 1,), BF16, "cpu")
    want[:n] = (a.float() + b.float()).to(BF16)
    _assert_bits(y, want, f"add_bf16 n={n}")
    _record("dataops_add_bf16", n=n)


# ------------------------------------------------------------------------------------------------ dropout
DROP_PS = (0.0, 2.0 ** -18, 2.0 ** -17, 0.05, 0.5, 0.99999)


@pytest.mark.parametrize("n", ROW_DS)
def test_dropout_is_bit_identical_to_the_stated_mask(n):
    ops = _ops()
    x = _nonzero((n,), n)
    xb = _sent((n + 8,))
    xb[:n] = x.cuda()
    for p in DROP_PS:
        for seed in SEEDS:
            y = _sent((n + 8,))
            ops.dropout(xb[:n], p, seed, y=y[:n])
            want = _sent((n + 8,), BF16, "cpu")
            want[:n] = D.dropout(x, p, seed)
            _assert_bits(y, want, f"dropout n={n} p={p} seed={seed}")
            assert np.array_equal((y[:n] != 0).cpu().numpy(), D.keep_mask(seed, n, p))        # x holds no zero: the mask, read off the output
    _record("dataops_dropout", n=n)


@pytest.mark.parametrize("n,p,seed", [(8, 0.05, 0), (2048, 0.5, (1 << 32) + 5), (2056, 0.99999, (1 << 63) - 1), (2056, 2.0 ** -17, 0),
                                      (2048, 0.0, (1 << 63) - 1), (2056, 0.05, (1 << 32) + 5)])
def test_dropout_add_keeps_dropped_bits_and_adds_one_of_two_candidates(n, p, seed):
    ops = _ops()
    x, y0 = _nonzero((n,), n + 1), _nonzero((n,), n + 2)
    xb, yb = _sent((n + 8,)), _sent((n + 8,))
    xb[:n], yb[:n] = x.cuda(), y0.cuda()
    ops.dropout_add(xb[:n], yb[:n], p, seed)
    ref, alt = D.dropout_add(x, y0, p, seed)
    keep = torch.from_numpy(D.keep_mask(seed, n, p))
    got = _bits(yb[:n])
    assert torch.equal(got[~keep], _bits(y0)[~keep]), "dropped positions keep their bits"
    ok = (got == _bits(ref)) | (got == _bits(alt))
    assert bool(ok.all()), (int((~ok).sum()), int((~ok).int().argmax()))
    assert bool((_bits(yb[n:]) == _bits(_sent((8,), BF16, "cpu"))).all()) and torch.equal(_bits(xb[:n]), _bits(x))
    _record("dataops_dropout_add", n=n, p=p, seed=seed, fused_form=int((got != _bits(ref)).sum()))


@pytest.mark.parametrize("p,seed", [(0.25, 0), (0.5, (1 << 32) + 5), (0.05, (1 << 63) - 1)])
def test_lora_down_applies_the_stated_mask(p, seed):
    """Adapters [I | 0] and [0 | I] read the two halves of K back: t[m, r] is zero exactly where element m K + k of x is dropped."""
    ops = _ops()
    M, K, R = 130, 128, 64
    x = _nonzero((M, K), 41).cuda()
    keep = torch.from_numpy(D.keep_mask(seed, M * K, p)).view(M, K)
    for half in (0, 1):
        a = torch.zeros(R, K, dtype=BF16)
        a[torch.arange(R), half * R + torch.arange(R)] = 1.0
        t = ops.lora_down(x, a.cuda(), 1.0, p, seed)
        assert t.shape == (M, R) and torch.equal((t != 0).cpu(), keep[:, half * R:(half + 1) * R]), half
    _record("dataops_mask_lora_down", p=p)


@pytest.mark.parametrize("p,seed", [(0.25, 0), (0.5, (1 << 32) + 5), (0.05, (1 << 63) - 1)])
def test_lora_a_grad_applies_the_stated_mask(p, seed):
    """A selector dT (one 1 per adapter row) reads masked token rows of x back: row r of gA is zero exactly where its token row is dropped."""
    ops = _ops()
    M, K, R = 130, 136, 8
    x = _nonzero((M, K), 43).cuda()
    tok = [0, 5, 63, 64, 65, 127, 128, 129]
    sel = torch.zeros(M, R, dtype=BF16)
    sel[torch.tensor(tok), torch.arange(R)] = 1.0
    ws = torch.empty(1 << 20, dtype=F32, device="cuda")
    ga = ops.lora_a_grad(sel.cuda(), x, torch.empty(R, K, dtype=BF16, device="cuda"), p, seed, False, ws)
    keep = torch.from_numpy(D.keep_mask(seed, M * K, p)).view(M, K)
    assert torch.equal((ga != 0).cpu(), keep[torch.tensor(tok)])
    _record("dataops_mask_lora_a_grad", p=p)


@pytest.mark.parametrize("M,N,K", [(130, 72, 64), (130, 264, 64)])
def test_gemm_dropout_add_applies_the_stated_mask(M, N, K):
    """All-positive operands: no product is zero, so y (accumulate=False) is zero exactly where element m N + n is dropped."""
    ops = _ops()
    a, b = _nonzero((M, K), 45).abs().cuda(), _nonzero((K, N), 46).abs().cuda()
    for p, seed in ((0.25, 0), (0.5, (1 << 32) + 5), (0.05, (1 << 63) - 1)):
        y = ops.gemm_dropout_add(a, b, torch.full((M, N), 7.0, dtype=BF16, device="cuda"), p, seed, accumulate=False)
        assert torch.equal((y != 0).cpu(), torch.from_numpy(D.keep_mask(seed, M * N, p)).view(M, N)), (p, seed)
    _record("dataops_mask_gemm_dropout_add", M=M, N=N, K=K)


# ------------------------------------------------------------------------------------------------ AdamW
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
ADAM_N = 1028


def _adam_state(kind):
    """(master, m, v, step), ADAM_N elements each (a test takes a prefix, so element k is the same in every n).  master cycles through the
    scales 0.02, 2^-50 and exactly 0, so that a step of any size shows against it."""
    sc = torch.tensor([(0.02, 2.0 ** -50, 0.0)[k % 3] for k in range(ADAM_N)])
    master = (_randn((ADAM_N,), 61) * sc).float()
    if kind == "fresh":
        return master, torch.zeros(ADAM_N), torch.zeros(ADAM_N), 1
    m = _randn((ADAM_N,), 62, 0.01).float()
    v = (_randn((ADAM_N,), 63, 0.01) ** 2 + 1e-12).float()
    return master, m, v, (1000 if kind == "warm" else 10 ** 6)


def _adam_grad(kind):
    if kind == "ordinary":
        return _randn((ADAM_N,), 64, 0.01).to(BF16)
    if kind == "zero":
        return torch.zeros(ADAM_N, dtype=BF16)
    sign = torch.where(_randn((ADAM_N,), 65) >= 0, 1.0, -1.0)
    return (sign * (2.0 ** -40 if kind == "2^-40" else 2.0 ** -70)).to(BF16)


def _adam_run(n, state, grad, wd, gscale, step=None):
    master, m, v, st = state
    bufs = [_sent((n + 4,), F32) for _ in range(3)]
    for b, t in zip(bufs, (master, m, v)):
        b[:n] = t[:n].cuda()
    pb, gb = _sent((n + 4,)), _sent((n + 4,))
    gb[:n] = grad[:n].cuda()
    gs = None if gscale is None else torch.tensor([gscale], dtype=F32, device="cuda")
    _ops().adamw(pb[:n], bufs[0][:n], gb[:n], bufs[1][:n], bufs[2][:n], LR, B1, B2, EPS, wd, st, gscale=gs)
    return pb, bufs


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027])
def test_adamw_single_steps_per_element(n):
    """One step from a given state (fp32 state error cannot compound), per element against float64:
    |got - ref| <= 2^-20 A + 2^-126 for master, m and v, each against its own A.  2^-20 is 8 fp32 ulps: the update is a handful of correctly
    rounded fp32 operations (sqrtf and / are correctly rounded in the default build: no fast-math) plus rsqrtf(bc2) at 1-2 ulp; the floor
    accepts a flushed denormal (g^2 at g = 2^-70).  The reference takes the hyperparameters as the fp32 values the C ABI receives."""
    _ops()
    worst = 0.0
    for skind in ("fresh", "warm", "late"):
        state = _adam_state(skind)
        for gkind in ("ordinary", "zero", "2^-40", "2^-70"):
            grad = _adam_grad(gkind)
            for wd in (0.0, 0.1):
                for gscale in (None, 0.37):
                    what = f"adamw n={n} state={skind} grad={gkind} wd={wd} gscale={gscale}"
                    pb, bufs = _adam_run(n, state, grad, wd, gscale)
                    ref = D.adamw_step(state[0][:n], state[1][:n], state[2][:n], grad[:n], LR, B1, B2, EPS, wd, state[3], gscale=gscale)
                    for name, buf, r, A in zip(("master", "m", "v"), bufs, ref[:3], ref[3:]):
                        worst = max(worst, D.assert_within(buf[:n], r, 2.0 ** -20 * A + 2.0 ** -126, f"{what}: {name}"))
                        assert bool((_bits(buf[n:]) == _bits(_sent((4,), F32, "cpu"))).all()), what + f": {name} guard"
                    want = _sent((n + 4,), BF16, "cpu")
                    want[:n] = bufs[0][:n].cpu().to(BF16)
                    _assert_bits(pb, want, what + ": p is the kernel's own master, rounded")
                    if gkind == "zero" and skind == "fresh":        # nothing but the weight decay moves the parameter
                        assert float(bufs[1][:n].abs().max()) == 0.0 and float(bufs[2][:n].abs().max()) == 0.0, what
                        if wd == 0.0:
                            assert torch.equal(_bits(bufs[0][:n]), _bits(state[0][:n])), what
    _record("dataops_adamw", worst, n=n)


def test_adamw_body_and_tail_agree():
    """An element gets the same master, m, v and p, bit for bit, whether the 4-wide body updates it or the scalar tail of another n: both
    call one function whose fused multiply-adds are written out (the source comment), so nothing is left to the compiler's contraction."""
    _ops()
    for skind, gkind, wd, gscale in (("warm", "ordinary", 0.1, 0.37), ("fresh", "2^-40", 0.0, None), ("late", "ordinary", 0.1, None),
                                     ("fresh", "ordinary", 0.1, 0.37)):
        state, grad = _adam_state(skind), _adam_grad(gkind)
        body = _adam_run(1028, state, grad, wd, gscale)                 # every element in the 4-wide body
        for n, tail in ((3, range(0, 3)), (1023, range(1020, 1023)), (1027, range(1024, 1027)), (5, range(4, 5))):
            run = _adam_run(n, state, grad, wd, gscale)
            t = torch.tensor(list(tail))
            for name, a, b in (("p", run[0], body[0]), ("master", run[1][0], body[1][0]), ("m", run[1][1], body[1][1]), ("v", run[1][2], body[1][2])):
                assert torch.equal(_bits(a)[t], _bits(b)[t]), (skind, gkind, n, name)
    _record("dataops_adamw_body_tail")


# ------------------------------------------------------------------------------------------------ argument checks
def _refused(name, good, bad_sets):
    """Every argument list in bad_sets (the good one with some positions replaced) is refused on the host, before any launch."""
    from radvlm_amd import lib
    for repl in bad_sets:
        args = list(good)
        for i, val in repl.items():
            args[i] = val
        with pytest.raises(lib.RadvlmHipError, match=f"{name} failed with code -1"):             # RV_ERR_ARG, not a launch error
            lib.call(name, *args)


def test_argument_checks_refuse_before_any_launch():
    _ops()
    bf = torch.zeros(64, 64, dtype=BF16, device="cuda")
    bf2, bf3 = torch.zeros_like(bf), torch.zeros_like(bf)
    odd = bf.reshape(-1)[1:]                                            # 2 bytes off a 16-byte boundary
    f32 = torch.zeros(64, dtype=F32, device="cuda")
    f32b, f32c = torch.zeros_like(f32), torch.zeros_like(f32)
    i32 = torch.zeros(64, dtype=torch.int32, device="cuda")
    u8 = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    nulls = lambda *pos: [{i: None} for i in pos]
    each = lambda pos, vals: [{i: v} for i in pos for v in vals]
    # (dst, ld_dst, ta, ld_a, tb, ld_b, idx, rows, d)
    _refused("rv_gather_rows", (bf, 64, bf2, 64, bf3, 64, i32, 4, 8),
             nulls(0, 6) + each((7,), (0, -1)) + each((8,), (0, -8, 12)) + each((1, 3, 5), (68,)))
    # (src, ld_src, seg_off, pos, out_row, nseg, out, ld_out, d)
    _refused("rv_segment_sum_rows", (bf, 64, i32, i32, i32, 2, bf2, 64, 8),
             nulls(0, 2, 3, 4, 6) + each((5,), (0, -1)) + each((8,), (0, -8, 12)) + each((1, 7), (68,)))
    # (src, ld_src, seg_off, pos, w, out_row, nseg, out, ld_out, d)
    _refused("rv_weighted_segment_sum_rows", (bf, 64, i32, i32, f32, i32, 2, bf2, 64, 8),
             nulls(0, 2, 3, 4, 5, 7) + each((6,), (0, -1)) + each((9,), (0, -8, 12)) + each((1, 8), (68,)) + [{0: odd}, {7: odd}])
    # (src, ld_src, idx4, out_row, n, out, ld_out, which, d)
    _refused("rv_max4_rows_fwd", (bf, 64, i32, i32, 2, bf2, 64, u8, 8),
             nulls(0, 2, 3, 5, 7) + each((4,), (0, -1)) + each((8,), (0, -8, 12)) + each((1, 6), (68,)))
    # (dout, ld_dout, idx4, dout_row, n, which, dsrc, ld_dsrc, d)
    _refused("rv_max4_rows_bwd", (bf, 64, i32, i32, 2, u8, bf2, 64, 8),
             nulls(0, 2, 3, 5, 6) + each((4,), (0, -1)) + each((8,), (0, -8, 12)) + each((1, 7), (68,)))
    # (x, pos, n, P, d)
    _refused("rv_add_pos_rows", (bf, bf2, 2, 2, 8), nulls(0, 1) + each((2, 3), (0, -1)) + each((4,), (0, -8, 12)) + [{0: odd}, {1: odd}])
    # (pix, out, n, H, W, p, Kp)
    _refused("rv_im2col_patches", (bf, bf2, 1, 4, 4, 2, 16),
             nulls(0, 1) + each((2,), (0, -1)) + each((5,), (0, -2)) + [{3: 1}, {4: 1}, {6: 11}, {6: 8}])
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    # (img, out, n, gh, gw, tile, mode, factor, mean3, std3)
    _refused("rv_normalize_tiles_u8", (u8, bf, 1, 1, 1, 4, 0, 1.0 / 255, m3, m3),
             nulls(0, 1, 8, 9) + each((2, 3, 4, 5), (0, -1)) + each((6,), (2, -1, 3)))
    # (patch_out, cls, pos, out, n, P, d)
    _refused("rv_clip_embed", (bf, bf2, bf3, torch.zeros_like(bf), 2, 2, 8), nulls(0, 1, 2, 3) + each((4, 5), (0, -1)) + each((6,), (0, -8, 12)))
    # (in, in_ld, in_bs0, in_bs1, out, out_ld, out_bs0, out_bs1, R, C, R_pad, nb0, nb1, perm32)
    _refused("rv_transpose_bf16", (bf, 64, 0, 0, bf2, 64, 0, 0, 16, 16, 64, 1, 1, 0),
             nulls(0, 4) + each((8, 9, 11, 12), (0, -1)) + [{10: 8}, {10: 20}, {10: 0}] + each((1, 2, 3, 5, 6, 7), (68,)) + [{0: odd}, {4: odd}]
             + [{13: 1, 10: 32}, {13: 1, 10: 72}])
    # (in, in_ld, cu_rows, in_bs1, out, out_ld, out_bs0, out_bs1, R_max, C, R_pad, nb0, nb1, perm32)
    _refused("rv_transpose_bf16_varlen", (bf, 64, i32, 0, bf2, 64, 0, 0, 16, 16, 64, 1, 1, 0),
             nulls(0, 2, 4) + each((8, 9, 11, 12), (0, -1)) + [{10: 8}, {10: 20}] + each((1, 3, 5, 6, 7), (68,)) + [{0: odd}, {4: odd}]
             + [{13: 1, 10: 32}, {13: 1, 10: 72}])
    for name in ("rv_dropout_bf16", "rv_dropout_add_bf16"):             # (x, y, n, p, seed)
        _refused(name, (bf, bf2, 64, 0.25, 1), nulls(0, 1) + each((2,), (0, -8, 12, 7)) + each((3,), (1.0, 1.5, -0.25)))
    fodd = f32[1:]                                                      # 4 bytes off a 16-byte boundary
    # (p, master, g, m, v, n, lr, b1, b2, eps, wd, bc1, bc2, gscale)
    _refused("rv_adamw", (bf, f32, bf2, f32b, f32c, 8, LR, B1, B2, EPS, 0.0, 0.1, 0.001, None),
             nulls(0, 1, 2, 3, 4) + each((5,), (0, -4)) + [{0: odd}, {2: odd}, {1: fodd}, {3: fodd}, {4: fodd}])
    _refused("rv_cast_f32_to_bf16", (f32, bf, 8), nulls(0, 1) + each((2,), (0, -1)))
    _refused("rv_cast_bf16_to_f32", (bf, f32, 8), nulls(0, 1) + each((2,), (0, -1)))
    _refused("rv_add_bf16", (bf, bf2, bf3, 8), nulls(0, 1, 2) + each((3,), (0, -1)))
    torch.cuda.synchronize()
    for t in (bf, bf2, bf3, f32, f32b, f32c):                           # nothing was launched: every buffer is as it was
        assert float(t.float().abs().max()) == 0.0
    _record("dataops_argument_checks")

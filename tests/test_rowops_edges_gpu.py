"""GPU tests of the row and elementwise training kernels (radvlm_amd/csrc/ops.hip) at the sizes, strides and values where they can go wrong:
every pass boundary of the row kernels (d = 8 .. 8192), grid-stride loops that take a second trip or leave blocks idle, rows of very
different scale in one tensor, eps 1e-5 and 1e-6, vocabularies that are no multiple of 8, -inf logits, explicit RoPE positions, leading
dimensions wider than the data with sentinel columns, saturating activation inputs, and the argument checks.

Every output element is compared with the float64 reference of tests/rowops_ref.py (its own CPU checks: tests/test_rowops_ref_host.py)
under the per-element gate |got - ref| <= 2^-7 A + 1e-30 (rowops_ref.assert_close_elementwise); fp32 per-row outputs are held to 1e-5
relative (rstd, LayerNorm stats) and 1e-4 max(1, |lse| + |target|) (loss rows).  Buffers a kernel must not touch carry a NaN sentinel and are
compared bit for bit afterwards; inputs it must not read are NaN.  Layouts the ops wrappers do not offer (a chosen block count, NULL
dlogits, a separate dlogits stride) go through the C ABI (radvlm_amd.lib.call).  Each test appends its worst measured ratio to
the measurement log (conftest.record_measurement)."""
import pytest
import torch

import rowops_ref as R
from rowops_ref import BF16, assert_close_elementwise, assert_rows_close

pytestmark = pytest.mark.gpu

NORM_DS = (8, 512, 520, 2048, 2056, 4096, 8184, 8192)
PLANTED = (0.0, -0.0, 2.0 ** -20, -2.0 ** -20, 10.0, -10.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4)


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _call(name, *args):
    from radvlm_amd import lib
    lib.call(name, *args)


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


def _randn(shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def _guarded(t, dtype=BF16):
    """t (CPU, [rows, ...]) on the GPU as the first rows of a buffer with one more row of sentinel: (buffer, view of the first rows)."""
    buf = _sentinel((t.shape[0] + 1,) + tuple(t.shape[1:]), dtype)
    buf[:-1] = t.to(dtype).cuda()
    return buf, buf[:-1]


def _norm_inputs(rows, d, scales, seed, offset=0.0):
    sc = torch.tensor([scales[i % len(scales)] for i in range(rows)])
    x = ((_randn((rows, d), seed) + offset) * sc[:, None]).to(BF16)
    w = (1 + _randn((d,), seed + 1, 0.1)).to(BF16)
    b = _randn((d,), seed + 2, 0.1).to(BF16)
    dy = _randn((rows, d), seed + 3).to(BF16)
    return x, w, b, dy


ROW_SETS = ((1, (1.0,)), (3, (1e-3, 1.0, 30.0)), (3, (1.0, 0.0, 30.0)))       # (rows, scale of each row); 0.0: an all-zero row


# ------------------------------------------------------------------------------------------------ RMSNorm / LayerNorm forward
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("d", NORM_DS)
def test_rmsnorm_fwd_every_pass_boundary(d, eps):
    ops = _ops()
    worst = worst_rstd = 0.0
    for rows, scales in ROW_SETS:
        x, w, _, _ = _norm_inputs(rows, d, scales, seed=d + rows)
        _, xg = _guarded(x)
        ybuf, rbuf = _sentinel((rows + 1, d)), _sentinel((rows + 1,), torch.float32)
        ops.rmsnorm_fwd(xg, w.cuda(), eps, y=ybuf[:rows], rstd=rbuf[:rows])
        ref, A, alt, rstd = R.rmsnorm_fwd(x, w, eps)
        worst = max(worst, assert_close_elementwise(ybuf[:rows], ref, A, f"rmsnorm y d={d} rows={rows} scales={scales}", alt=alt))
        worst_rstd = max(worst_rstd, assert_rows_close(rbuf[:rows], rstd, rstd.abs(), 1e-5, f"rmsnorm rstd d={d} scales={scales}"))
        assert _is_sentinel(ybuf[rows:]) and _is_sentinel(rbuf[rows:])
        for r, s in enumerate(scales[:rows]):
            if s == 0.0:                                    # the all-zero row: rstd = eps^-1/2 (within the row gate above), y exactly zero
                assert abs(float(rbuf[r]) - eps ** -0.5) <= 1e-5 * eps ** -0.5 and float(ybuf[r].float().abs().max()) == 0.0
    _record("rowops_rmsnorm_fwd", worst, d=d, eps=eps, worst_rstd_ratio_of_1e_5=worst_rstd)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("d", NORM_DS)
def test_layernorm_fwd_every_pass_boundary(d, eps):
    ops = _ops()
    worst = worst_stats = 0.0
    for rows, scales in ROW_SETS:
        x, w, b, _ = _norm_inputs(rows, d, scales, seed=2 * d + rows, offset=0.5)
        _, xg = _guarded(x)
        ybuf = _sentinel((rows + 1, d))
        _, stats = ops.layernorm_fwd(xg, w.cuda(), b.cuda(), eps, y=ybuf[:rows], save_stats=True)
        ref, A, mean, rstd = R.layernorm_fwd(x, w, b, eps)
        worst = max(worst, assert_close_elementwise(ybuf[:rows], ref, A, f"layernorm y d={d} rows={rows} scales={scales}"))
        # the saved mean is a sum that may cancel: held to 1e-5 of the row's mean |x| (A of a mean); rstd to 1e-5 relative
        worst_stats = max(worst_stats, assert_rows_close(stats[:, 0], mean, x.double().abs().mean(-1), 1e-5, f"layernorm mean d={d} scales={scales}"),
                          assert_rows_close(stats[:, 1], rstd, rstd.abs(), 1e-5, f"layernorm rstd d={d} scales={scales}"))
        assert _is_sentinel(ybuf[rows:])
        y2 = ops.layernorm_fwd(xg, w.cuda(), b.cuda(), eps)                       # stats == NULL: the same y
        assert _same_bits(y2, ybuf[:rows])
        for r, s in enumerate(scales[:rows]):
            if s == 0.0:
                assert abs(float(stats[r, 1]) - eps ** -0.5) <= 1e-5 * eps ** -0.5 and float(stats[r, 0]) == 0.0 and _same_bits(ybuf[r], b.cuda())
    _record("rowops_layernorm_fwd", worst, d=d, eps=eps, worst_stats_ratio_of_1e_5=worst_stats)


# ------------------------------------------------------------------------------------------------ RMSNorm / LayerNorm backward
BWD_GRIDS = ((3, 8), (5, 3), (1, 4))          # (nblk, rows): uneven trips / idle blocks / one block walks every row
BWD_SCALES = (1e-3, 1.0, 30.0, 0.0)


def _bwd_buffers(rows, d, dx_add, seed):
    dx_in = _randn((rows, d), seed + 7).to(BF16) if dx_add else None
    dxbuf = _sentinel((rows + 1, d))
    if dx_add:
        dxbuf[:rows] = dx_in.cuda()
    return dx_in, dxbuf


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("d", NORM_DS)
def test_rmsnorm_bwd_block_counts_and_partials(d, eps):
    _ops()
    worst = worst_dw = 0.0
    for nblk, rows in BWD_GRIDS:
        for dx_add in (False, True):
            x, w, _, dy = _norm_inputs(rows, d, BWD_SCALES, seed=3 * d + rows)
            _, xg = _guarded(x)
            _, dyg = _guarded(dy)
            dx_in, dxbuf = _bwd_buffers(rows, d, dx_add, 3 * d + rows)
            rstd = R.rmsnorm_fwd(x, w, eps)[3].float().cuda()
            part = _sentinel((nblk + 1, d), torch.float32)
            _call("rv_rmsnorm_bwd", dyg, xg, w.cuda(), rstd, dxbuf, int(dx_add), part, nblk, rows, d)
            dx, A, dw, Aw = R.rmsnorm_bwd(dy, x, w, eps, dx_in=dx_in)
            what = f"rmsnorm d={d} nblk={nblk} rows={rows} dx_add={dx_add}"
            worst = max(worst, assert_close_elementwise(dxbuf[:rows], dx, A, what + " dx"))
            assert _is_sentinel(dxbuf[rows:]) and _is_sentinel(part[nblk:])
            p = part[:nblk].cpu().double()
            assert bool(torch.isfinite(p).all()), what
            if nblk > rows:
                assert float(p[rows:].abs().max()) == 0.0, what + ": idle blocks write zero partials"
            worst_dw = max(worst_dw, assert_close_elementwise(p.sum(0), dw, Aw, what + " dw partial column sum"))
    _record("rowops_rmsnorm_bwd", worst, d=d, eps=eps, worst_dw_ratio_of_gate=worst_dw)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("d", NORM_DS)
def test_layernorm_bwd_block_counts_and_partials(d, eps):
    _ops()
    worst = worst_dw = 0.0
    for nblk, rows in BWD_GRIDS:
        for dx_add in (False, True):
            x, w, _, dy = _norm_inputs(rows, d, BWD_SCALES, seed=5 * d + rows, offset=0.5)
            _, xg = _guarded(x)
            _, dyg = _guarded(dy)
            dx_in, dxbuf = _bwd_buffers(rows, d, dx_add, 5 * d + rows)
            _, _, mean, rstd = R.layernorm_fwd(x, w, torch.zeros(d), eps)
            stats = torch.stack((mean, rstd), dim=1).float().contiguous().cuda()
            part = _sentinel((nblk + 1, 2 * d), torch.float32)
            _call("rv_layernorm_bwd", dyg, xg, w.cuda(), stats, dxbuf, int(dx_add), part, nblk, rows, d)
            dx, A, dw, Aw, db, Ab = R.layernorm_bwd(dy, x, w, eps, dx_in=dx_in)
            what = f"layernorm d={d} nblk={nblk} rows={rows} dx_add={dx_add}"
            worst = max(worst, assert_close_elementwise(dxbuf[:rows], dx, A, what + " dx"))
            assert _is_sentinel(dxbuf[rows:]) and _is_sentinel(part[nblk:])
            p = part[:nblk].cpu().double()
            assert bool(torch.isfinite(p).all()), what
            if nblk > rows:
                assert float(p[rows:].abs().max()) == 0.0, what + ": idle blocks write zero partials"
            worst_dw = max(worst_dw, assert_close_elementwise(p[:, :d].sum(0), dw, Aw, what + " dw partial column sum"),
                           assert_close_elementwise(p[:, d:].sum(0), db, Ab, what + " db partial column sum"))
    _record("rowops_layernorm_bwd", worst, d=d, eps=eps, worst_dw_db_ratio_of_gate=worst_dw)


@pytest.mark.parametrize("accumulate", [False, True])
def test_rmsnorm_bwd_more_rows_than_blocks(accumulate):
    """ops.rmsnorm_bwd launches min(rows, 1024) blocks: at 1027 rows three of them take a second trip through the prefetch pipeline."""
    ops = _ops()
    rows, d, eps = 1027, 64, 1e-6
    x, w, _, dy = _norm_inputs(rows, d, (1e-3, 1.0, 30.0), seed=71)
    rstd = R.rmsnorm_fwd(x, w, eps)[3].float().cuda()
    dx_in = _randn((rows, d), 72).to(BF16) if accumulate else None
    dw_in = _randn((d,), 73, 30.0).to(BF16) if accumulate else None
    dxbuf = _sentinel((rows + 1, d))
    if accumulate:
        dxbuf[:rows] = dx_in.cuda()
    dwbuf = _sentinel((d + 8,))
    if accumulate:
        dwbuf[:d] = dw_in.cuda()
    ops.rmsnorm_bwd(dy.cuda(), x.cuda(), w.cuda(), rstd, dx=dxbuf[:rows], dx_add=accumulate, dw=dwbuf[:d], dw_accumulate=accumulate)
    dx, A, dw, Aw = R.rmsnorm_bwd(dy, x, w, eps, dx_in=dx_in, dw_in=dw_in)
    worst = assert_close_elementwise(dxbuf[:rows], dx, A, "rmsnorm 1027 rows dx")
    worst_dw = assert_close_elementwise(dwbuf[:d], dw, Aw, "rmsnorm 1027 rows dw")
    assert _is_sentinel(dxbuf[rows:]) and _is_sentinel(dwbuf[d:])
    _record("rowops_rmsnorm_bwd_1027_rows", worst, accumulate=accumulate, worst_dw_ratio_of_gate=worst_dw)


@pytest.mark.parametrize("accumulate", [False, True])
def test_layernorm_bwd_more_rows_than_blocks(accumulate):
    """ops.layernorm_bwd launches min(rows, 512) blocks: at 515 rows three of them take a second trip."""
    ops = _ops()
    rows, d, eps = 515, 64, 1e-6
    x, w, _, dy = _norm_inputs(rows, d, (1e-3, 1.0, 30.0), seed=81, offset=0.5)
    _, _, mean, rstd = R.layernorm_fwd(x, w, torch.zeros(d), eps)
    stats = torch.stack((mean, rstd), dim=1).float().contiguous().cuda()
    dx_in = _randn((rows, d), 82).to(BF16) if accumulate else None
    dw_in = _randn((d,), 83, 30.0).to(BF16) if accumulate else None
    db_in = _randn((d,), 84, 30.0).to(BF16) if accumulate else None
    dxbuf = _sentinel((rows + 1, d))
    wb = _sentinel((2, d + 8))
    if accumulate:
        dxbuf[:rows] = dx_in.cuda()
        wb[0, :d], wb[1, :d] = dw_in.cuda(), db_in.cuda()
    ops.layernorm_bwd(dy.cuda(), x.cuda(), w.cuda(), stats, wb[0, :d], wb[1, :d], dx=dxbuf[:rows], dx_add=accumulate, accumulate=accumulate)
    dx, A, dw, Aw, db, Ab = R.layernorm_bwd(dy, x, w, eps, dx_in=dx_in, dw_in=dw_in, db_in=db_in)
    worst = assert_close_elementwise(dxbuf[:rows], dx, A, "layernorm 515 rows dx")
    worst_dw = max(assert_close_elementwise(wb[0, :d], dw, Aw, "layernorm 515 rows dw"), assert_close_elementwise(wb[1, :d], db, Ab, "layernorm 515 rows db"))
    assert _is_sentinel(dxbuf[rows:]) and _is_sentinel(wb[:, d:])
    _record("rowops_layernorm_bwd_515_rows", worst, accumulate=accumulate, worst_dw_db_ratio_of_gate=worst_dw)


# ------------------------------------------------------------------------------------------------ argument contract
@pytest.mark.parametrize("d", [12, 8200, 0, -8])
def test_norm_entry_points_refuse_a_bad_width(d):
    """d % 8 != 0, d > 8192 and d <= 0 are refused by all four norm entry points before any launch (every buffer is valid and large enough
    for 2 rows of 8208, so nothing can fault whatever a launcher lets through)."""
    _ops()
    from radvlm_amd.lib import RadvlmHipError
    rows, cap = 2, 8208
    x, dy, y = (torch.zeros(rows, cap, dtype=BF16, device="cuda") for _ in range(3))
    w, b = torch.ones(cap, dtype=BF16, device="cuda"), torch.zeros(cap, dtype=BF16, device="cuda")
    rstd, stats = torch.ones(rows, dtype=torch.float32, device="cuda"), torch.ones(rows, 2, dtype=torch.float32, device="cuda")
    part = torch.zeros(rows, 2 * cap, dtype=torch.float32, device="cuda")
    with pytest.raises(RadvlmHipError):
        _call("rv_rmsnorm_fwd", x, w, y, rstd, rows, d, 1e-5)
    with pytest.raises(RadvlmHipError):
        _call("rv_rmsnorm_bwd", dy, x, w, rstd, y, 0, part, rows, rows, d)
    with pytest.raises(RadvlmHipError):
        _call("rv_layernorm_fwd", x, w, b, y, stats, rows, d, 1e-5)
    with pytest.raises(RadvlmHipError):
        _call("rv_layernorm_bwd", dy, x, w, stats, y, 0, part, rows, rows, d)
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0 and float(part.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ cross entropy
CE_VS = (8, 9, 15, 1001, 2047, 2049, 32003)


def _ceil8(v):
    return (v + 7) // 8 * 8


def _ce_rows(V):
    """(bf16 logits [7, V], labels): N(0,2) rows with labels 0, V-1, one ignored; rows offset by +300 and -200; a planted dominant label
    logit (40 above the rest, p ~ 1)."""
    z = _randn((7, V), 900 + V, 2.0)
    z[2] += 300
    z[3] -= 200
    dom = min(5, V - 1)
    z[5, dom] = z[5].max() + 40
    labels = torch.tensor([0, V - 1, V // 2, V // 3, -100, dom, V - 1])
    return z.to(BF16), labels


def _ce_launch(logits, ld, labels, dl, ld_d, rows, V, inv):
    loss = _sentinel((rows + 1,), torch.float32)
    _call("rv_cross_entropy", logits, ld, labels, loss, dl, ld_d, rows, V, inv)
    assert _is_sentinel(loss[rows:])
    return loss[:rows]


def _ce_packed(z, V):
    """z [rows, V] as the first rows of a [rows + 1, ceil8(V)] buffer: NaN in the pad columns (never read) and in the row past the end."""
    buf = _sentinel((z.shape[0] + 1, _ceil8(V)))
    buf[:-1, :V] = z.cuda()
    return buf


def _ce_check_all_forms(z, labels, V, inv, what):
    """The four buffer forms on one input; returns (worst gradient ratio, worst loss ratio)."""
    rows, ld8 = z.shape[0], _ceil8(V)
    lab = labels.cuda()
    loss_ref, scale, g_ref, A = R.cross_entropy(z, labels, V, inv)
    # (a) in place, ld = ceil8(V)
    a = _ce_packed(z, V)
    loss_a = _ce_launch(a, ld8, lab, a, ld8, rows, V, inv)
    worst_l = assert_rows_close(loss_a, loss_ref, scale, 1e-4, what + " loss rows")
    worst_g = assert_close_elementwise(a[:rows, :V], g_ref, A, what + " in-place gradient")
    assert float(a[:rows, V:].float().abs().max() if ld8 > V else 0.0) == 0.0, what + ": gradient pad columns are zero"
    assert _is_sentinel(a[rows:])
    ignored = (labels < 0)
    if bool(ignored.any()):
        assert float(a[:rows][ignored.cuda()].float().abs().max()) == 0.0 and float(loss_a[ignored.cuda()].abs().max()) == 0.0
    # (b) in place in a column slice of a wider buffer
    wide = _sentinel((rows, 8 + ld8 + 24))
    wide[:, 8:8 + V] = z.cuda()
    loss_b = _ce_launch(wide[:, 8:], wide.stride(0), lab, wide[:, 8:], wide.stride(0), rows, V, inv)
    assert _same_bits(loss_b, loss_a) and _same_bits(wide[:, 8:8 + ld8], a[:rows]), what + ": slice form"
    assert _is_sentinel(wide[:, :8]) and _is_sentinel(wide[:, 8 + ld8:]), what + ": columns outside the slice"
    # (c) out of place, ld_d != ld; the logits stay as they are
    src = _ce_packed(z, V)
    keep = src.clone()
    dl = _sentinel((rows, ld8 + 16))
    loss_c = _ce_launch(src, ld8, lab, dl, dl.stride(0), rows, V, inv)
    assert _same_bits(src, keep), what + ": logits unchanged"
    assert _same_bits(loss_c, loss_a) and _same_bits(dl[:, :ld8], a[:rows]), what + ": out-of-place gradient bit-identical to in-place"
    assert _is_sentinel(dl[:, ld8:])
    # (d) dlogits == NULL
    loss_d = _ce_launch(src, ld8, lab, None, 0, rows, V, inv)
    assert _same_bits(src, keep) and _same_bits(loss_d, loss_a), what + ": dlogits NULL"
    return worst_g, worst_l


@pytest.mark.parametrize("V", CE_VS)
def test_cross_entropy_ragged_vocabulary_and_buffer_forms(V):
    _ops()
    z, labels = _ce_rows(V)
    worst_g, worst_l = _ce_check_all_forms(z, labels, V, 1.0 / 6, f"ce V={V}")
    # a whole batch of ignored labels (the engine passes inv_count = NaN then): zeros, not 0 * NaN
    a = _ce_packed(z, V)
    none = torch.full((z.shape[0],), -100, dtype=torch.int64, device="cuda")
    loss = _ce_launch(a, _ceil8(V), none, a, _ceil8(V), z.shape[0], V, float("nan"))
    assert float(loss.abs().max()) == 0.0 and float(a[:-1].float().abs().max()) == 0.0 and _is_sentinel(a[-1:])
    _record("rowops_cross_entropy", worst_g, V=V, worst_loss_ratio_of_1e_4=worst_l)


@pytest.mark.parametrize("V", CE_VS)
def test_cross_entropy_masked_logits(V):
    """-inf logits (masked tokens), none at the label: p = 0 there, loss and gradient finite and equal to the reference.  A run of eight
    -inf that is the FIRST vector a thread sees, followed by finite ones on a later trip (columns 0..7 at V > 2048), used to leave NaN in
    that thread's running sum."""
    _ops()
    z = _randn((5, V), 950 + V, 2.0)
    lab = torch.tensor([0, 0, V - 1, 0, V - 1])
    z[0, 3::5] = float("-inf")                                 # scattered
    z[1, 1::2] = float("-inf")                                 # every other column: each vector half masked
    if V > 8:
        z[2, :8] = float("-inf")                               # an aligned run: the first vector thread 0 sees
    if V > 2048:
        z[3, 2048:2056] = float("-inf")                        # the first vector of thread 0's second trip (all of its real columns at V = 2049)
        z[4, :16] = float("-inf")                              # both: the running sum stays empty through the first trip
        z[4, 2048:min(V - 1, 2056)] = float("-inf")
    z = z.to(BF16)
    assert bool(torch.isfinite(z[torch.arange(5), lab].float()).all())
    worst_g, worst_l = _ce_check_all_forms(z, lab, V, 0.2, f"ce -inf V={V}")
    a = _ce_packed(z, V)
    _ce_launch(a, _ceil8(V), lab.cuda(), a, _ceil8(V), 5, V, 0.2)
    assert float(a[:5, :V][torch.isinf(z).cuda()].float().abs().max()) == 0.0          # p = 0 at a masked logit
    _record("rowops_cross_entropy_masked", worst_g, V=V, worst_loss_ratio_of_1e_4=worst_l)


# ------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("nsec", [1, 2])
@pytest.mark.parametrize("hd", [16, 64, 128])
def test_rope_positions_sections_and_strides(hd, nsec, heads):
    ops = _ops()
    n, left, vcols, right, S = nsec * heads * hd, 8, 16, 8, 5
    worst = worst_back = 0.0
    for rows in (1, 37):
        explicit = torch.tensor([44] if rows == 1 else [(13 * i + 7) % 61 for i in range(rows)])
        if rows > 1:
            explicit[5] = explicit[4]                                        # repeated; the sequence is non-monotone and exceeds `rows`
            assert int(explicit.max()) > rows
        for pos in (None, explicit):
            table = ops.rope_table(S if pos is None else int(pos.max()) + 1, hd)
            p_ref = torch.arange(rows) % S if pos is None else pos
            x = _randn((rows, n + vcols), 1000 + hd + rows).to(BF16)
            buf = _sentinel((rows + 1, left + n + vcols + right))
            buf[:rows, left:left + n + vcols] = x.cuda()
            before = buf.clone()
            view = buf[:rows, left:]
            pg = None if pos is None else pos.to(torch.int32).cuda()
            ops.rope_inplace(view, table, S, heads, hd, nsec, 1, positions=pg)
            ref, A = R.rope(x, table.cpu(), p_ref, heads, hd, nsec, 1)
            what = f"rope hd={hd} nsec={nsec} heads={heads} rows={rows} positions={'explicit' if pos is not None else 'row % S'}"
            worst = max(worst, assert_close_elementwise(buf[:rows, left:left + n], ref, A, what))
            untouched = torch.ones_like(buf, dtype=torch.bool)
            untouched[:rows, left:left + n] = False
            assert torch.equal(_bits(buf)[untouched.cpu()], _bits(before)[untouched.cpu()]), what + ": V columns, sentinel columns and the row past the end"
            ops.rope_inplace(view, table, S, heads, hd, nsec, -1, positions=pg)
            xs = x[:, :n].double().view(rows, nsec * heads, 2, hd // 2).abs()
            pair = (xs[:, :, 0] + xs[:, :, 1])[:, :, None].expand(-1, -1, 2, -1).reshape(rows, n)
            worst_back = max(worst_back, assert_close_elementwise(buf[:rows, left:left + n], x[:, :n].double(), 2 * pair, what + " there and back"))
            assert torch.equal(_bits(buf)[untouched.cpu()], _bits(before)[untouched.cpu()])
    _record("rowops_rope", worst, hd=hd, nsec=nsec, heads=heads, worst_round_trip_ratio_of_2x_gate=worst_back)


# ------------------------------------------------------------------------------------------------ SwiGLU / GELUs
def _plant(flat, shift):
    k = min(flat.numel(), len(PLANTED))
    flat[:k] = torch.tensor([PLANTED[(i + shift) % len(PLANTED)] for i in range(k)])
    return flat


@pytest.mark.parametrize("F", [8, 2048, 2056])
def test_swiglu_strides_and_saturating_inputs(F):
    ops = _ops()
    worst = 0.0
    for rows in ((1, 259) if F == 8 else (1, 3)):        # 259 x 1 and 3 x 257 threads: a partial last block; 3 x 256: exact blocks
        for shift in ((0, 8) if rows * F < len(PLANTED) else (0,)):
            g = _plant(_randn((rows, F), 1100 + F + rows).reshape(-1), shift).reshape(rows, F).to(BF16)
            u = _plant(_randn((rows, F), 1101 + F + rows).reshape(-1).flip(0), shift + 4).flip(0).reshape(rows, F).to(BF16)
            da = _randn((rows, F), 1102 + F + rows).to(BF16)
            gu_buf, act_buf = _sentinel((rows, 8 + 2 * F + 8)), _sentinel((rows, 8 + F + 24))
            da_buf, dgu_buf = _sentinel((rows, 8 + F + 40)), _sentinel((rows, 8 + 2 * F + 48))
            gu_buf[:, 8:8 + F], gu_buf[:, 8 + F:8 + 2 * F], da_buf[:, 8:8 + F] = g.cuda(), u.cuda(), da.cuda()
            assert len({gu_buf.stride(0), act_buf.stride(0), da_buf.stride(0), dgu_buf.stride(0)}) == 4
            keep_gu, keep_da = gu_buf.clone(), da_buf.clone()
            what = f"swiglu F={F} rows={rows} shift={shift}"
            ops.swiglu_fwd(gu_buf[:, 8:], F, act=act_buf[:, 8:])
            ref, A, alt = R.swiglu_fwd(g, u)
            worst = max(worst, assert_close_elementwise(act_buf[:, 8:8 + F], ref, A, what + " act", alt=alt))
            assert _is_sentinel(act_buf[:, :8]) and _is_sentinel(act_buf[:, 8 + F:]), what
            ops.swiglu_bwd(da_buf[:, 8:], gu_buf[:, 8:], F, dgu=dgu_buf[:, 8:])
            dg, Ag, du, Au = R.swiglu_bwd(da, g, u)
            worst = max(worst, assert_close_elementwise(dgu_buf[:, 8:8 + F], dg, Ag, what + " dg"),
                        assert_close_elementwise(dgu_buf[:, 8 + F:8 + 2 * F], du, Au, what + " du"))
            assert _is_sentinel(dgu_buf[:, :8]) and _is_sentinel(dgu_buf[:, 8 + 2 * F:]), what
            assert _same_bits(gu_buf, keep_gu) and _same_bits(da_buf, keep_da), what + ": inputs unchanged"
    _record("rowops_swiglu", worst, F=F)


GELUS = {"quick_gelu": (R.quick_gelu_fwd, R.quick_gelu_bwd), "gelu": (R.gelu_fwd, R.gelu_bwd), "gelu_tanh": (R.gelu_tanh_fwd, R.gelu_tanh_bwd)}


@pytest.mark.parametrize("n", [8, 2048, 2056])
@pytest.mark.parametrize("kind", sorted(GELUS))
def test_gelus_sizes_and_saturating_inputs(kind, n):
    ops = _ops()
    fwd, bwd = getattr(ops, kind + "_fwd"), getattr(ops, kind + "_bwd")
    worst = 0.0
    for shift in ((0, 8) if n < len(PLANTED) else (0,)):
        x = _plant(_randn((n,), 1200 + n), shift).to(BF16)
        dy = _randn((n,), 1201 + n).to(BF16)
        xb, dyb = _sentinel((n + 8,)), _sentinel((n + 8,))                 # NaN past n: never read
        xb[:n], dyb[:n] = x.cuda(), dy.cuda()
        yb, dxb = _sentinel((n + 8,)), _sentinel((n + 8,))
        fwd(xb[:n], y=yb[:n])
        bwd(dyb[:n], xb[:n], dx=dxb[:n])
        ref, A = GELUS[kind][0](x)
        dref, Ad = GELUS[kind][1](dy, x)
        worst = max(worst, assert_close_elementwise(yb[:n], ref, A, f"{kind} fwd n={n} shift={shift}"),
                    assert_close_elementwise(dxb[:n], dref, Ad, f"{kind} bwd n={n} shift={shift}"))
        assert _is_sentinel(yb[n:]) and _is_sentinel(dxb[n:])
    _record("rowops_" + kind, worst, n=n)


def test_saturated_activation_values_are_exact():
    """At -100 the fast exp overflows (or erf / tanh reach -1): quick_gelu, gelu, gelu_tanh and silu are exactly 0 or -0.  At +100 each
    forward output is x and each backward output is dy."""
    ops = _ops()
    x = torch.tensor([-100.0, 100.0] * 4).to(BF16).cuda()
    dy = torch.tensor([0.75, -1.5, 3.0, 0.0078125, -0.3125, 2.5, 1.0, -7.0]).to(BF16).cuda()
    lo, hi = slice(0, 8, 2), slice(1, 8, 2)
    for kind in sorted(GELUS):
        y, dx = getattr(ops, kind + "_fwd")(x), getattr(ops, kind + "_bwd")(dy, x)
        assert float(y[lo].float().abs().max()) == 0.0, kind
        assert _same_bits(y[hi], x[hi]) and _same_bits(dx[hi], dy[hi]), kind
    gu = torch.cat((x, torch.ones_like(x)))[None].contiguous()               # g = +-100, u = 1
    act = ops.swiglu_fwd(gu, 8)
    assert float(act[0, lo].float().abs().max()) == 0.0 and _same_bits(act[0, hi], x[hi])
    dgu = ops.swiglu_bwd(dy[None].contiguous(), gu, 8)
    assert _same_bits(dgu[0, :8][hi], dy[hi])                                   # dg = da u = da


# ------------------------------------------------------------------------------------------------ column sums / gradient norm
@pytest.mark.parametrize("cols", [8, 40, 2056])
@pytest.mark.parametrize("rows", [1, 31, 33, 259])
def test_bias_grad_strided_rows(rows, cols):
    """bias_grad launches min(rows, 256) partial rows: at 259 three of them take a second trip."""
    ops = _ops()
    dy = _randn((rows, cols), 1300 + rows + cols).to(BF16)
    dy[rows // 2] *= 1000.0
    wide = _sentinel((rows, 8 + cols + 16))                                   # NaN beside the view: never read
    wide[:, 8:8 + cols] = dy.cuda()
    out = ops.bias_grad(wide[:, 8:8 + cols])
    s, A = R.colsum(dy)
    worst = assert_close_elementwise(out, s, A, f"bias_grad rows={rows} cols={cols}")
    out_in = _randn((cols,), 1301 + rows, 100.0).to(BF16)
    ob = _sentinel((cols + 8,))
    ob[:cols] = out_in.cuda()
    ops.bias_grad(wide[:, 8:8 + cols], out=ob[:cols], accumulate=True)
    s, A = R.colsum(dy, out_in)
    worst = max(worst, assert_close_elementwise(ob[:cols], s, A, f"bias_grad accumulate rows={rows} cols={cols}"))
    assert _is_sentinel(ob[cols:])
    _record("rowops_bias_grad", worst, rows=rows, cols=cols)


@pytest.mark.parametrize("cols", [1, 31, 33])
@pytest.mark.parametrize("rows", [1, 33])
def test_colsum_f32_odd_sizes(rows, cols):
    _ops()
    x = _randn((rows, cols), 1400 + rows + cols)
    xb, xg = _guarded(x, torch.float32)
    worst = 0.0
    for acc in (0, 1):
        out_in = _randn((cols,), 1401 + cols, 3.0).to(BF16)
        ob = _sentinel((cols + 8,))
        if acc:
            ob[:cols] = out_in.cuda()
        _call("rv_colsum_f32", xg, rows, cols, ob, acc)
        s, A = R.colsum(x, out_in if acc else None)
        worst = max(worst, assert_close_elementwise(ob[:cols], s, A, f"colsum_f32 rows={rows} cols={cols} accumulate={acc}"))
        assert _is_sentinel(ob[cols:])
    _record("rowops_colsum_f32", worst, rows=rows, cols=cols)


@pytest.mark.parametrize("n", [1, 7, 8, 2_097_152 + 13])
def test_grad_norm_tail_and_second_trip(n):
    """1024 blocks x 256 threads x 8 elements = 2,097,152 per grid-stride trip: the last size adds one vector of a second trip and a
    five-element tail.  One entry of 1e4 among 1e-3 carries the whole norm, so it is placed in turn at the start, in the second trip's
    vector and in the tail; a run of N(0,1) makes every element count."""
    ops = _ops()
    big_at = sorted({0, n - 1, n // 2} | ({2_097_152 + 2} if n > 2_097_152 else set()))
    cases = [("1e4 at %d" % i, i) for i in big_at] + [("normal", None)]
    worst = 0.0
    for name, i in cases:
        g = _randn((n,), 1500 + n) if i is None else torch.full((n,), 1e-3)
        if i is not None:
            g[i] = 1e4
        g = g.to(BF16)
        gb = _sentinel((n + 8,))
        gb[:n] = g.cuda()
        for max_norm in (1.0, 1e9):
            out = ops.grad_norm_clip_coef(gb[:n], max_norm).cpu().double()
            norm = g.double().pow(2).sum().sqrt()
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            ref = torch.stack((norm, coef))
            worst = max(worst, assert_rows_close(out, ref, ref.abs(), 1e-5, f"grad norm n={n} {name} max_norm={max_norm}"))
    _record("rowops_grad_norm", worst, n=n)

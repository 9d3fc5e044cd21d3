"""GPU tests of the scoring kernels (radvlm_amd/csrc/score.hip).  rv_attn_extend_prefix_bf16: bit for bit against rv_attn_extend_bf16 on
the cache materialised as prefix ++ tail, over both head sizes and group sizes 1 .. 8, with prefix lengths around the 64-key stage, shared
prefix rows, a sequence without rows and NaN wherever the kernel must not read; strides and refused arguments.
rv_token_logprob_rows_f32: the int32 bits of rv_log_softmax_rows_f32 followed by a gather, rv_argmax_rows_f32's argmax, the special rows
and src_row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (hd, H, Hkv): toy_qwen, Qwen2-7B, Llama-7B (heads cut to 4: the kernel's work split is per kv head), G = 8
SHAPES = [(64, 4, 2), (128, 28, 4), (128, 4, 4), (128, 8, 1)]
PLEN = [1, 63, 64, 65, 130, 130, 64]
TAILS = [1, 2, 15, 16, 17, 40, 0]
PROW = [0, 1, 1, 2, 3, 3, 1]                     # rows 1 and 3 are shared, row 1 at two lengths; row 4 belongs to nobody
P_ROWS, P_MAX, T_MAX = 5, 133, 43
NAN = float("nan")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _case(H, Hkv, hd, seed=0):
    """(q, prefix, tail, materialised cache): NaN in every prefix position past the largest prefix_len that uses the row, in the whole
    unreferenced row, in the tail rows past n_b and in the materialised cache past each sequence's keys."""
    g = torch.Generator().manual_seed(seed)
    kvd = Hkv * hd
    col = torch.linspace(0.5, 1.5, 2 * kvd)
    prefix = (torch.randn(P_ROWS, P_MAX, 2 * kvd, generator=g) * col).to(torch.bfloat16)
    tail = (torch.randn(len(TAILS), T_MAX, 2 * kvd, generator=g) * col).to(torch.bfloat16)
    used = [0] * P_ROWS
    for row, n in zip(PROW, PLEN):
        used[row] = max(used[row], n)
    assert used == [1, 64, 65, 130, 0]
    for row in range(P_ROWS):
        prefix[row, used[row]:] = NAN
    for b, n in enumerate(TAILS):
        tail[b, n:] = NAN
    L_max = max(p + n for p, n in zip(PLEN, TAILS)) + 5
    mat = torch.full((len(TAILS), L_max, 2 * kvd), NAN, dtype=torch.bfloat16)
    for b, (row, p, n) in enumerate(zip(PROW, PLEN, TAILS)):
        mat[b, :p] = prefix[row, :p]
        mat[b, p:p + n] = tail[b, :n]
    q = (torch.randn(sum(TAILS), H * hd, generator=g) * 1.3).to(torch.bfloat16)
    return q.cuda(), prefix.cuda(), tail.cuda(), mat.cuda()


def _cu():
    return _i32(np.concatenate([[0], np.cumsum(TAILS)]).tolist())


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("chunk", [64, 256])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"hd{s[0]}_H{s[1]}_Hkv{s[2]}" for s in SHAPES])
def test_extend_prefix_bit_identical_to_extend_on_the_materialised_cache(shape, chunk):
    _need_gpu()
    from radvlm_amd import ops
    assert ops.EXTEND_CHUNK == 256
    hd, H, Hkv = shape
    q, prefix, tail, mat = _case(H, Hkv, hd, seed=hd + H)
    cu, plen, prow = _cu(), _i32(PLEN), _i32(PROW)
    want = ops.attn_extend(q, mat, cu, plen, H, Hkv, hd, Hkv * hd, max(TAILS), chunk=chunk)
    got = ops.attn_extend_prefix(q, prefix, tail, cu, prow, plen, H, Hkv, hd, Hkv * hd, max(TAILS), chunk=chunk)
    assert torch.isfinite(want.float()).all()
    assert torch.equal(_bits(got), _bits(want))


def test_sharing_reads_the_shared_row():
    _need_gpu()
    from radvlm_amd import ops
    hd, H, Hkv = 128, 28, 4
    q, prefix, tail, mat = _case(H, Hkv, hd, seed=11)
    cu, plen, prow = _cu(), _i32(PLEN), _i32(PROW)
    run = lambda p: ops.attn_extend_prefix(q, p, tail, cu, prow, plen, H, Hkv, hd, Hkv * hd, max(TAILS), chunk=64)
    want = ops.attn_extend(q, mat, cu, plen, H, Hkv, hd, Hkv * hd, max(TAILS), chunk=64)
    mat[5] = NAN                                       # the copy the prefix kernel never had
    got = run(prefix)
    assert torch.equal(_bits(got), _bits(want))
    p2 = prefix.clone()
    p2[1, 0] = (p2[1, 0].float() * -1.5 + 0.25).to(torch.bfloat16)      # position 0 of row 1: inside every length it is used at
    got2 = run(p2)
    starts = np.concatenate([[0], np.cumsum(TAILS)])
    for b, row in enumerate(PROW):
        a, c = got[starts[b]:starts[b + 1]], got2[starts[b]:starts[b + 1]]
        if TAILS[b] == 0:
            continue
        if row == 1:
            assert not torch.equal(_bits(a), _bits(c)), b
        else:
            assert torch.equal(_bits(a), _bits(c)), b


def test_strided_q_and_out_keep_the_guard_columns():
    _need_gpu()
    from radvlm_amd import ops
    hd, H, Hkv = 64, 4, 2
    kvd = Hkv * hd
    q, prefix, tail, _ = _case(H, Hkv, hd, seed=7)
    cu, plen, prow = _cu(), _i32(PLEN), _i32(PROW)
    M = q.shape[0]
    want = ops.attn_extend_prefix(q, prefix, tail, cu, prow, plen, H, Hkv, hd, kvd, max(TAILS))
    qkv = torch.randn(M, H * hd + 2 * kvd, device="cuda").to(torch.bfloat16)               # q as a slice of a wider q|k|v row
    qkv[:, :H * hd] = q
    wide = torch.full((M, H * hd + 16), 77.0, dtype=torch.bfloat16, device="cuda")         # out inside wider rows
    got = ops.attn_extend_prefix(qkv[:, :H * hd], prefix, tail, cu, prow, plen, H, Hkv, hd, kvd, max(TAILS), out=wide[:, 8:8 + H * hd])
    torch.cuda.synchronize()
    assert got.data_ptr() == wide[:, 8:].data_ptr()
    assert torch.equal(_bits(wide[:, 8:8 + H * hd]), _bits(want))
    assert (wide[:, :8] == 77.0).all() and (wide[:, 8 + H * hd:] == 77.0).all()


def test_a_sequence_with_a_bad_prefix_entry_is_zeros_and_the_rest_is_unchanged():
    _need_gpu()
    from radvlm_amd import ops
    hd, H, Hkv = 64, 4, 2
    q, prefix, tail, _ = _case(H, Hkv, hd, seed=9)
    cu, plen = _cu(), _i32(PLEN)
    want = ops.attn_extend_prefix(q, prefix, tail, cu, _i32(PROW), plen, H, Hkv, hd, Hkv * hd, max(TAILS), chunk=64)
    starts = np.concatenate([[0], np.cumsum(TAILS)])
    for bad_row, bad_len in ((P_ROWS, PLEN[3]), (-1, PLEN[3]), (PROW[3], P_MAX + 1), (PROW[3], -1)):
        prow2, plen2 = list(PROW), list(PLEN)
        prow2[3], plen2[3] = bad_row, bad_len
        got = ops.attn_extend_prefix(q, prefix, tail, cu, _i32(prow2), _i32(plen2), H, Hkv, hd, Hkv * hd, max(TAILS), chunk=64)
        assert (got[starts[3]:starts[4]] == 0).all()
        assert torch.equal(_bits(got[:starts[3]]), _bits(want[:starts[3]]))
        assert torch.equal(_bits(got[starts[4]:]), _bits(want[starts[4]:]))


def test_extend_prefix_rejects_bad_arguments():
    _need_gpu()
    from radvlm_amd import lib
    hd, H, Hkv = 64, 4, 2
    kvd, w = Hkv * hd, 2 * Hkv * hd
    q, prefix, tail, _ = _case(H, Hkv, hd, seed=1)
    cu, plen, prow = _cu(), _i32(PLEN), _i32(PROW)
    M, B, chunk = q.shape[0], len(TAILS), 64
    out = torch.zeros(M, H * hd, dtype=torch.bfloat16, device="cuda")
    nch = (P_MAX + T_MAX + chunk - 1) // chunk
    part = torch.zeros(M * H * nch * (hd + 2), dtype=torch.float32, device="cuda")
    good = dict(q=q, ld_q=H * hd, prefix=prefix, ld_p=w, bs_p=P_MAX * w, P_rows=P_ROWS, P_max=P_MAX, tail=tail, ld_t=w, bs_t=T_MAX * w,
                T_max=T_MAX, v_off=kvd, cu_q=cu, prefix_row=prow, prefix_len=plen, out=out, ld_o=H * hd, part=part,
                part_bytes=part.numel() * 4, B=B, M=M, max_q=max(TAILS), H=H, Hkv=Hkv, hd=hd, chunk=chunk, scale=0.125)

    def call(**kw):
        a = dict(good, **kw)
        lib.call("rv_attn_extend_prefix_bf16", *[a[k] for k in good])

    call()
    bad = [dict(prefix_row=None), dict(prefix_len=None), dict(prefix=None), dict(tail=None), dict(P_rows=0), dict(P_max=0), dict(T_max=0),
           dict(chunk=100), dict(chunk=0), dict(H=18), dict(hd=96), dict(ld_q=H * hd - 8), dict(ld_o=H * hd - 8), dict(ld_p=w - 8),
           dict(ld_t=w - 8), dict(bs_p=P_MAX * w - 8), dict(bs_t=T_MAX * w - 8), dict(part_bytes=part.numel() * 4 - 4), dict(max_q=0),
           dict(max_q=T_MAX + 1), dict(B=0), dict(M=0), dict(v_off=kvd + 4)]
    for kw in bad:
        with pytest.raises(lib.RadvlmHipError):
            call(**kw)
    with pytest.raises(lib.RadvlmHipError):                                                # B * tiles > 65535
        call(B=70000)


# ------------------------------------------------------------------------------------------------ token log-prob
def _rows(rows, n, seed, pad=13):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, n + pad), NAN)
    x[:, :n] = torch.randn(rows, n, generator=g) * 3.0
    return x.cuda()


def _reference(ops, x, n):
    """(log-softmax of every row by rv_log_softmax_rows_f32 on a clone, argmax by rv_argmax_rows_f32)"""
    ls = ops.log_softmax_rows(x.clone(), n)
    return ls, ops.argmax_rows(x, n)


def _ibits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n,rows", [(1, 5), (255, 5), (256, 5), (257, 5), (2048, 5), (2049, 5), (32000, 3), (152064, 3)])
def test_token_logprob_is_log_softmax_rows_then_gather(n, rows):
    _need_gpu()
    from radvlm_amd import ops
    x = _rows(rows, n, seed=n)
    keep = x.clone()
    ls, am = _reference(ops, x, n)
    rng = np.random.default_rng(n)
    kinds = np.stack([np.zeros(rows, np.int64), np.full(rows, n - 1), am.cpu().numpy(), rng.integers(0, n, rows)], axis=1)   # [rows, 4]
    # every row with every kind of target, through src_row
    src = np.repeat(np.arange(rows), 4)
    tgt = kinds.reshape(-1)
    lp, got_am = ops.token_logprob_rows(x, n, _i32(tgt.tolist()), src_row=_i32(src.tolist()))
    want = ls[torch.tensor(src).cuda(), torch.tensor(tgt).cuda()]
    assert torch.equal(_ibits(lp), _ibits(want))
    assert torch.equal(got_am, am[torch.tensor(src).cuda()])
    # and without src_row: row r takes kind r % 4
    t1 = np.array([kinds[r, r % 4] for r in range(rows)])
    lp1, am1 = ops.token_logprob_rows(x, n, _i32(t1.tolist()))
    assert torch.equal(_ibits(lp1), _ibits(ls[torch.arange(rows).cuda(), torch.tensor(t1).cuda()]))
    assert torch.equal(am1, am)
    assert torch.equal(_ibits(x), _ibits(keep))                                           # x is only read, guard columns included
    # a row alone gives the bits it has inside the launch
    for r in range(rows):
        one, a = ops.token_logprob_rows(x[r:r + 1], n, _i32([int(t1[r])]))
        assert torch.equal(_ibits(one), _ibits(lp1[r:r + 1])) and int(a) == int(am[r])
    lp_none, no_am = ops.token_logprob_rows(x, n, _i32(t1.tolist()), want_argmax=False)
    assert no_am is None and torch.equal(_ibits(lp_none), _ibits(lp1))


def test_token_logprob_special_rows():
    _need_gpu()
    from radvlm_amd import ops
    n = 300
    x = _rows(6, n, seed=3)
    x[0, 17] = NAN
    x[1, 200] = float("inf")
    x[2, :n] = float("-inf")
    x[3, 5] = float("-inf")
    target = [40, 40, 40, 5, -100, n]
    ls, am = _reference(ops, x, n)
    lp, got_am = ops.token_logprob_rows(x, n, _i32(target))
    lp, ls = lp.cpu(), ls.cpu()
    assert torch.isnan(lp[0]) and torch.isnan(ls[0, 40])
    assert torch.isnan(lp[1]) and torch.isnan(ls[1, 40])
    assert torch.isnan(lp[2]) and torch.isnan(ls[2, 40])
    assert lp[3] == float("-inf") and ls[3, 5] == float("-inf")
    assert _ibits(lp[4:5]).item() == 0                                                     # +0.0
    assert torch.isnan(lp[5])
    assert torch.equal(got_am, am)                                                         # written whatever the target
    assert int(got_am[0]) == 17 and int(got_am[1]) == 200 and int(got_am[2]) == 0


def test_token_logprob_src_row():
    _need_gpu()
    from radvlm_amd import ops
    n = 2049
    x = _rows(4, n, seed=5)
    ls, am = _reference(ops, x, n)
    lp, got_am = ops.token_logprob_rows(x, n, _i32([3, 1000, 2048, 7, 7]), src_row=_i32([2, 2, 2, 4, -1]))
    assert torch.equal(_ibits(lp[:3]), _ibits(ls[2, [3, 1000, 2048]]))
    assert (got_am[:3] == am[2]).all()
    assert torch.isnan(lp[3:]).all()                                                       # a source row outside x: NaN, nothing read
    assert (got_am[3:] == -1).all()

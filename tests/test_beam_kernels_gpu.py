"""GPU tests of the beam-search kernels (radvlm_amd/csrc/beam.hip): rv_attn_decode_beam_bf16 bit for bit against rv_attn_decode_bf16 on
the gathered cache, rv_log_softmax_rows_f32 against float64 within the bound its comment derives, rv_beam_topk_f32 exactly against
np.lexsort."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGPROB_TOL = 1e-5                # tests/test_sample_gpu.py: the tolerance generate_batch's log-softmax is tested to
CHUNK = 128
NS = (1000, 1001, 32000, 152064)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------ 5. attention lookup, bit-exact
ROWS, NB = 6, 3
OUT_OF_RANGE = 10 ** 6


def _tables(kind, tail, ld_t):
    """tail_src int32 [ROWS, ld_t]: rows 3g .. 3g + 2 are the beams of prompt g.  Columns >= tail hold an index far outside the cache:
    they lie past every kv_len and must never be read."""
    t = np.full((ROWS, ld_t), OUT_OF_RANGE, dtype=np.int32)
    for r in range(ROWS):
        base = r // NB * NB
        for i in range(tail):
            if kind == "shared":            # the group's beams descend from one ancestor for the first half, then live in their own row
                t[r, i] = base + 1 if i < tail // 2 else r
            else:                           # ancestry switches rows at every position
                t[r, i] = base + (r + i) % NB
    return t


@pytest.mark.parametrize("H,Hkv,hd", [(2, 2, 128), (4, 2, 64), (8, 1, 128)])
def test_attn_decode_beam_bit_identical_to_gathered_cache(H, Hkv, hd):
    _need_gpu()
    from radvlm_amd import ops
    kvd = Hkv * hd
    L_max = 129 + 130 + 13
    g = torch.Generator().manual_seed(H * 1000 + hd)
    cache = torch.randn(ROWS, L_max, 2 * kvd, generator=g).to(torch.bfloat16).cuda()
    q = torch.randn(ROWS, H * hd, generator=g).to(torch.bfloat16).cuda()
    prefix_row = np.array([3, 3, 3, 0, 0, 0], dtype=np.int32)                 # never the row's own
    for plen in (1, 127, 128, 129):
        for tail in (0, 1, 130):
            for kind in (("none",) if tail == 0 else ("shared", "switch")):
                kv_len = np.full(ROWS, plen + tail, dtype=np.int32)
                kv_len[4] = plen + max(tail - 1, 0)                           # a row that stops one key earlier
                kv_len[5] = 0                                                 # a row without keys: zeros out
                ld_t = tail + 5
                tab = _tables(kind, tail, ld_t) if tail else None
                src = np.tile(np.arange(ROWS)[:, None], (1, L_max))            # positions >= kv_len: anything, they are not read
                src[:, :plen] = prefix_row[:, None]
                if tail:
                    src[:, plen:plen + tail] = tab[:, :tail]
                gathered = cache[torch.from_numpy(src).cuda(), torch.arange(L_max, device="cuda")[None, :]].contiguous()
                kv_d = torch.from_numpy(kv_len).cuda()
                want = ops.attn_decode(q, gathered, kv_d, H, Hkv, hd, kvd, chunk=CHUNK)
                tab_d = None if tab is None else torch.from_numpy(tab).cuda()
                got = ops.attn_decode_beam(q, cache, kv_d, torch.from_numpy(prefix_row).cuda(),
                                           torch.full((ROWS,), plen, dtype=torch.int32, device="cuda"), tab_d, H, Hkv, hd, kvd,
                                           tail_cols=None if tab is None else tail + 3, chunk=CHUNK)     # ld_t > tail_cols > tail
                torch.cuda.synchronize()
                assert torch.equal(got, want), (plen, tail, kind, float((got.float() - want.float()).abs().max()))
                assert not got[5].any() and got[:5].float().abs().max() > 0


def test_attn_decode_beam_refuses_short_rows():
    _need_gpu()
    from radvlm_amd import lib
    H, Hkv, hd, L_max = 2, 2, 64, 64
    cache = torch.zeros(2, L_max, 2 * Hkv * hd, dtype=torch.bfloat16, device="cuda")
    q = torch.zeros(2, H * hd, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(2, H * hd, dtype=torch.bfloat16, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    part = torch.zeros(2 * H * (hd + 2), dtype=torch.float32, device="cuda")

    def call(ld_q, ld_o):
        lib.call("rv_attn_decode_beam_bf16", q, ld_q, cache, cache.shape[2], L_max * cache.shape[2], Hkv * hd, i32([1, 1]), L_max,
                 i32([0, 0]), i32([1, 1]), None, 0, 0, 2, out, ld_o, part, part.numel() * 4, 2, H, Hkv, hd, 64, 0.125)

    call(H * hd, H * hd)
    with pytest.raises(lib.RadvlmHipError):
        call(H * hd, H * hd - 8)
    with pytest.raises(lib.RadvlmHipError):
        call(H * hd - 8, H * hd)


# ------------------------------------------------------------------------------------------------ 6. row log-softmax
def lsm_bound(out64, n):
    """csrc/beam.hip: |out_i - exact_i| <= 2^-24 (2 |out_i| + 4 ln n + 3)."""
    return 2.0 ** -24 * (2 * np.abs(out64) + 4 * np.log(n) + 3)


def lsm_exact(x):
    x = np.asarray(x, dtype=np.float64)
    d = x - x.max()
    with np.errstate(divide="ignore"):
        return d - np.log(np.exp(d).sum())


def _lsm_rows(n, rng):
    base = rng.standard_normal((4, n)).astype(np.float32)
    rows = np.empty((4, n + 8), dtype=np.float32)
    rows[:, n:] = 777.0
    rows[0, :n] = 0.25                                   # flat
    rows[1, :n] = base[1]
    rows[1, rng.integers(0, n)] = 80.0                   # peaked
    rows[2, :n] = base[2] * 8                            # scaled
    rows[3, :n] = base[3] * 3
    rows[3, rng.integers(0, n, 20)] = -np.inf
    rows[3, :3] = -np.inf
    return rows


@pytest.mark.parametrize("n", NS)
def test_log_softmax_rows_within_derived_bound(n):
    _need_gpu()
    from conftest import record_measurement
    from radvlm_amd import ops
    rows = _lsm_rows(n, np.random.default_rng(n))
    xd = torch.from_numpy(rows).cuda()
    ops.log_softmax_rows(xd[:, :n], n)                   # rows of stride n + 8
    got = xd.cpu().numpy()
    assert (got[:, n:] == 777.0).all()                   # columns >= n are never touched
    worst = {}
    for r, name in enumerate(("flat", "peaked", "scaled", "neg_inf")):
        want = lsm_exact(rows[r, :n])
        fin = np.isfinite(want)
        assert (got[r, :n][~fin] == -np.inf).all() and np.isfinite(got[r, :n][fin]).all(), name
        err = np.abs(got[r, :n][fin].astype(np.float64) - want[fin])
        bound = lsm_bound(want[fin], n)
        worst[name] = dict(err=float(err.max()), bound_there=float(bound[err.argmax()]), bound_max=float(bound.max()),
                           min_logprob=float(want[fin].min()))
        assert (err <= bound).all(), (name, float(err.max()), float(bound[err.argmax()]))
    # the bound against the 1e-5 that generate_batch's logprobs are tested to (tests/test_sample_gpu.py LOGPROB_TOL).  That tolerance is
    # applied to the log-prob of an emitted token, i.e. near the row's maximum, where |out| <= ln n: there the bound is below it for
    # every n the kernel accepts.  Further down it grows with the value itself, 2 ulp of it (1.2e-5 at the peaked row's -80).
    assert 2.0 ** -24 * (6 * np.log(262144) + 3) < LOGPROB_TOL
    for name, v in worst.items():
        v["bound_below_logprob_tol_down_to"] = -(LOGPROB_TOL * 2.0 ** 24 - 4 * np.log(n) - 3) / 2
    assert worst["flat"]["bound_max"] < LOGPROB_TOL, worst["flat"]
    record_measurement("beam_log_softmax_rows", n=n, logprob_tol=LOGPROB_TOL, **{f"{k}_{f}": v[f] for k, v in worst.items() for f in v})


def test_log_softmax_row_bits_do_not_depend_on_the_launch():
    _need_gpu()
    from radvlm_amd import ops
    n = 152064
    rng = np.random.default_rng(9)
    row = (rng.standard_normal(n) * 4).astype(np.float32)
    alone = torch.from_numpy(row[None].copy()).cuda()
    ops.log_softmax_rows(alone, n)
    many = (rng.standard_normal((32, n)) * 6).astype(np.float32)
    many[17] = row
    md = torch.from_numpy(many).cuda()
    ops.log_softmax_rows(md, n)
    assert torch.equal(md[17], alone[0])


# ------------------------------------------------------------------------------------------------ 7. grouped top-K, exact
def topk_ref(x, score, nb, n, K):
    rows = x.shape[0]
    v = (np.float32(x[:, :n]) + np.float32(score)[:, None]).reshape(rows // nb, nb * n)
    vals, idx = [], []
    for g in range(v.shape[0]):
        order = np.lexsort((np.arange(nb * n), -v[g]))[:K]
        vals.append(v[g][order])
        idx.append(order)
    return np.stack(vals), np.stack(idx)


def _topk_inputs(kind, groups, nb, n, K, rng):
    rows = groups * nb
    if kind == "ints":                                   # integer-valued rows: ties everywhere, also across beams
        x = rng.integers(-3, 4, (rows, n + 8)).astype(np.float32)
        score = np.zeros(rows, dtype=np.float32)
    elif kind == "inf_runs":                             # runs of -inf, HF's starting scores [0, -1e9, ...]
        x = (rng.standard_normal((rows, n + 8)) * 3).astype(np.float32)
        for r in range(rows):
            a = int(rng.integers(0, n - 300))
            x[r, a:a + 300] = -np.inf
        x[:, :5] = -np.inf
        score = np.tile(np.array([0.0] + [-1e9] * (nb - 1), dtype=np.float32), groups)
    else:                                                # fewer finite candidates than K in the last group
        x = (rng.standard_normal((rows, n + 8)) * 3).astype(np.float32)
        x[rows - nb:, :n] = -np.inf
        keep = rng.choice(nb * n, size=max(K // 2, 1), replace=False)
        for f in keep:
            x[rows - nb + f // n, f % n] = np.float32(rng.standard_normal())
        score = (rng.standard_normal(rows) * 2).astype(np.float32)
    x[:, n:] = 1e30                                      # columns >= n would win every comparison if they were read
    return x, score


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("groups,nb,K", [(1, 1, 2), (3, 3, 6), (2, 5, 15), (1, 16, 64)])
def test_beam_topk_exact(groups, nb, K, n):
    _need_gpu()
    from radvlm_amd import ops
    rng = np.random.default_rng(n + 7 * nb)
    for kind in ("ints", "inf_runs", "few_finite"):
        x, score = _topk_inputs(kind, groups, nb, n, K, rng)
        xd = torch.from_numpy(x).cuda()
        top = ops.beam_topk(xd[:, :n], n, nb, torch.from_numpy(score).cuda(), K).cpu()
        vals, idx = top[0].view(torch.float32).numpy(), top[1].numpy()
        want_v, want_i = topk_ref(x, score, nb, n, K)
        assert (idx == want_i).all(), (kind, np.argwhere(idx != want_i)[:4])
        assert (vals.view(np.uint32) == want_v.view(np.uint32)).all(), kind
        if kind == "few_finite":
            assert np.isneginf(vals[-1, -1]) and np.isfinite(vals[-1, 0])


def test_beam_topk_same_bits_among_other_groups():
    _need_gpu()
    from radvlm_amd import ops
    n, nb, K = 32000, 4, 8
    rng = np.random.default_rng(2)
    x = rng.integers(-2, 3, (3 * nb, n)).astype(np.float32)
    score = rng.integers(-2, 3, 3 * nb).astype(np.float32)
    xd, sd = torch.from_numpy(x).cuda(), torch.from_numpy(score).cuda()
    all3 = ops.beam_topk(xd, n, nb, sd, K).cpu()
    alone = ops.beam_topk(xd[nb:2 * nb], n, nb, sd[nb:2 * nb].contiguous(), K).cpu()
    assert torch.equal(all3[:, 1], alone[:, 0])


def test_beam_topk_refuses_bad_sizes():
    _need_gpu()
    from radvlm_amd import lib, ops
    x = torch.zeros(17, 64, device="cuda")
    s = torch.zeros(17, device="cuda")
    out = torch.zeros(2, 1, 64, dtype=torch.int32, device="cuda")
    ws = ops.beam_topk_workspace(1, 16, 64, 64, "cuda")
    for nb, K in ((17, 4), (1, 65), (1, 0)):
        with pytest.raises(lib.RadvlmHipError):
            lib.call("rv_beam_topk_f32", x, 64, 1, nb, 64, s, K, out[0], out[1], ws, ws.numel() * 8)
    small = torch.zeros(1, 3, device="cuda")
    with pytest.raises(lib.RadvlmHipError):              # K above the number of candidates
        lib.call("rv_beam_topk_f32", small, 3, 1, 1, 3, s, 4, out[0], out[1], ws, ws.numel() * 8)

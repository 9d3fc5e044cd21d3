"""GPU tests of rv_spec_accept_rows_f32 and rv_sample_rows_tagged_f32 against the float64 restatements (tests/spec_ref.py,
tests/sample_ref.py): accept tests outside the band, the drawn token against the reference CDF of the row the kernel stopped at, the
log-probability; the exact edge rows; bit-reproducibility across launches, group positions and workspace contents; the tagged sampler
against the plain one and against its stream; refused arguments."""
import numpy as np
import pytest
import torch

import sample_ref
import spec_ref
from test_sample_gpu import LOGPROB_TOL
from test_spec_host import KERNEL_GROUPS, KERNEL_N, KERNEL_R

pytestmark = pytest.mark.gpu
DELTA = spec_ref.DELTA
POISON = float("nan")                            # past column n: a kernel that read it would find an unusable row


def _dev_rows(a, pad=5):
    """Rows on the device with ld > n and poison behind column n; returns the [rows, n] view."""
    a = np.asarray(a, dtype=np.float32)
    full = torch.full((max(a.shape[0], 1), a.shape[1] + pad), POISON, dtype=torch.float32, device="cuda")
    full[:a.shape[0], :a.shape[1]] = torch.from_numpy(a)
    return full[:a.shape[0], :a.shape[1]]


def _launch(p, q, draft, seeds, t0, ws=None):
    from radvlm_amd import ops
    p = np.asarray(p, dtype=np.float32)
    n, groups = p.shape[1], len(seeds)
    R = p.shape[0] // groups
    pd = _dev_rows(p)
    qd = _dev_rows(q) if R > 1 else None
    dd = torch.from_numpy(np.asarray(draft, dtype=np.int32).reshape(groups, R - 1)).cuda() if R > 1 else None
    sd = torch.from_numpy(np.asarray(seeds, dtype=np.int64)).cuda()
    td = torch.from_numpy(np.asarray(t0, dtype=np.int32)).cuda()
    a, tok, lp = ops.spec_accept_rows(pd, qd, dd, sd, td, n, ws=ws)
    return a.cpu().numpy(), tok.cpu().numpy(), lp.cpu().numpy()


def _check_group(p, q, draft, seed, t0, ka, ktok, klp):
    """The kernel's (n_accept, token, logprob) of one group against the reference; returns how many decisions sat in the band."""
    R, band = len(p), 0
    for i in range(min(ka + 1, R - 1)):
        ok, margin = spec_ref.accept_test(p[i], q[i], int(draft[i]), seed, t0 + i)
        band += margin <= DELTA
        assert margin <= DELTA or ok == (i < ka), (i, ka, ok, margin)
    cdf, logp = spec_ref.draw_cdf(p, q, ka)
    u = spec_ref.uniform(seed, spec_ref.TAG_DRAW, t0 + ka)
    j = int(ktok)
    assert 0 <= j < p.shape[1] and (cdf[j] - (cdf[j - 1] if j else 0.0)) > 0, (j, "a token without weight")
    assert (cdf[j - 1] if j else 0.0) - DELTA <= u <= cdf[j] + DELTA, (j, u, cdf[j - 1] if j else 0.0, cdf[j])
    assert abs(float(klp) - float(logp[j])) <= LOGPROB_TOL, (klp, logp[j])
    return band


@pytest.mark.parametrize("groups", KERNEL_GROUPS)
@pytest.mark.parametrize("R", KERNEL_R)
@pytest.mark.parametrize("n", KERNEL_N)
def test_against_reference(n, R, groups):
    p, q, draft, seeds, t0 = spec_ref.kernel_case(n, R, groups)
    ka, ktok, klp = _launch(p, q, draft, seeds, t0)
    for g in range(groups):
        _check_group(p[g * R:(g + 1) * R], q[g * (R - 1):(g + 1) * (R - 1)], draft[g], int(seeds[g]), int(t0[g]), int(ka[g]), ktok[g], klp[g])


def test_equal_rows_accept_every_draft():
    n, R = 1000, 5
    p = spec_ref.warped_rows(3, R, n, top=40)
    for seed in range(256):
        draft = [int(np.flatnonzero(np.isfinite(p[i]))[(seed + 7 * i) % 40]) for i in range(R - 1)]
        a, tok, lp = _launch(p, p[:R - 1].copy(), draft, [seed], [seed % 5])
        assert a[0] == R - 1 and np.isfinite(p[R - 1, tok[0]]), (seed, a, tok)


def test_edge_rows():
    n = 64
    ninf = -np.inf
    rng = np.random.default_rng(5)
    base = rng.standard_normal((2, n)).astype(np.float32)
    for seed in range(32):
        # q one-hot on x where p(x) = -inf: always rejected, the token drawn from p (the residual is p itself)
        p = base.copy()
        p[0, 9] = ninf
        q = np.full((1, n), ninf, dtype=np.float32)
        q[0, 9] = 0.5
        a, tok, lp = _launch(p, q, [9], [seed], [3])
        assert a[0] == 0
        _check_group(p, q, [9], seed, 3, 0, tok[0], lp[0])
        # p one-hot on y != x: the token is y
        p1 = np.full((2, n), ninf, dtype=np.float32)
        p1[:, 20] = 1.0
        a, tok, lp = _launch(p1, base[:1], [9], [seed], [0])
        assert (a[0], tok[0]) == (0, 20) and abs(lp[0]) <= LOGPROB_TOL
        # ... and on x itself with q spread out: accepted, then the bonus draw from the one-hot row
        a, tok, lp = _launch(p1, base[:1], [20], [seed], [0])
        assert (a[0], tok[0]) == (1, 20)
        # a draft id at -1 and at n: rejected, never used as an index
        for x in (-1, n):
            a, tok, lp = _launch(base, base[1:], [x], [seed], [1])
            assert a[0] == 0
            _check_group(base, base[1:], [x], seed, 1, 0, tok[0], lp[0])
        # r identically 0 after a rejection (equal rows, a draft outside the kept set): the draw falls back to p
        p2 = base.copy()
        p2[0, 11] = ninf
        a, tok, lp = _launch(p2, p2[:1].copy(), [11], [seed], [2])
        assert a[0] == 0 and tok[0] != 11
        _check_group(p2, p2[:1].copy(), [11], seed, 2, 0, tok[0], lp[0])


@pytest.mark.parametrize("where", [0, 2, 4])
@pytest.mark.parametrize("what", ["nan", "inf", "empty"])
def test_unusable_row_on_the_path(where, what):
    n, R = 200, 5
    p = spec_ref.warped_rows(11, R, n, top=30)
    bad = p.copy()
    if what == "empty":
        bad[where] = -np.inf
    else:
        bad[where, 77] = np.nan if what == "nan" else np.inf
    for seed in range(8):
        draft = [int(np.flatnonzero(np.isfinite(p[i]))[seed % 30]) for i in range(R - 1)]
        a, tok, lp = _launch(bad, p[:R - 1].copy(), draft, [seed], [0])      # equal rows before `where`: all accepted up to it
        assert (a[0], tok[0]) == (where, -1) and np.isnan(lp[0]), (a, tok, lp)
    # a row behind the first rejection is not on the path
    if where > 0:
        q = p[:R - 1].copy()
        a, tok, lp = _launch(bad, q, [-1] * (R - 1), [1], [0])
        assert a[0] == 0 and tok[0] >= 0 and np.isfinite(lp[0])


def test_n_equal_one():
    for R in (1, 3):
        p = np.full((R, 1), 0.25, dtype=np.float32)
        q = np.full((R - 1, 1), -3.0, dtype=np.float32)
        a, tok, lp = _launch(p, q, [0] * (R - 1), [4], [0])
        assert (a[0], tok[0]) == (R - 1, 0) and abs(lp[0]) <= LOGPROB_TOL


def test_bit_reproducible_across_launches_groups_and_workspace():
    from radvlm_amd import ops
    for n, R in ((1000, 5), (32003, 2), (7, 32)):
        p, q, draft, seeds, t0 = spec_ref.kernel_case(n, R, 3, seed=1)
        alone = _launch(p[2 * R:], q[2 * (R - 1):], draft[2:], seeds[2:], t0[2:])
        ws = ops.spec_accept_workspace(3, R, "cuda")
        ws.fill_(-0x0123456789ABCDEF)                                    # garbage: nothing of it may be read before it is written
        three = _launch(p, q, draft, seeds, t0, ws=ws)
        again = _launch(p, q, draft, seeds, t0, ws=ws)
        first = _launch(np.concatenate([p[2 * R:], p[:2 * R]]), np.concatenate([q[2 * (R - 1):], q[:2 * (R - 1)]]),
                        np.concatenate([draft[2:], draft[:2]]), np.concatenate([seeds[2:], seeds[:2]]), np.concatenate([t0[2:], t0[:2]]))
        for k in range(3):
            want = alone[k].view(np.uint32 if alone[k].dtype == np.float32 else alone[k].dtype)[0]
            for got, g in ((three, 2), (again, 2), (first, 0)):
                assert got[k].view(np.uint32 if got[k].dtype == np.float32 else got[k].dtype)[g] == want, (n, R, k, g)
        for x, y in zip(three, again):
            assert x.tobytes() == y.tobytes()


def test_tagged_sampler():
    from radvlm_amd import ops
    n, rows = 1000, 6
    x = spec_ref.warped_rows(2, rows, n, None)
    seeds = np.arange(rows, dtype=np.int64) * 977 + 5
    ts = np.arange(rows, dtype=np.int32) * 3
    sd, td = torch.from_numpy(seeds).cuda(), torch.from_numpy(ts).cuda()
    st = dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.0)
    out = {}
    for tag in (None, 0, 1, 2):
        xd = _dev_rows(x)
        lp = torch.empty(rows, dtype=torch.float32, device="cuda")
        tok = ops.sample_rows(xd, n, sd, td, write_scores=True, logprob=lp, **st, **({} if tag is None else dict(tag=tag)))
        out[tag] = (tok.cpu().numpy(), lp.cpu().numpy(), xd.cpu().numpy())
    # tag 0 is rv_sample_rows_f32 bit for bit, through the tagged entry point as well
    from radvlm_amd import lib
    xd = _dev_rows(x)
    lp = torch.empty(rows, dtype=torch.float32, device="cuda")
    tok = torch.empty(rows, dtype=torch.int64, device="cuda")
    ws = ops.sample_rows_workspace(rows, "cuda")
    lib.call("rv_sample_rows_tagged_f32", xd, xd.stride(0), rows, n, sd, td, 0, 0.8, 40, 0.9, 0.0, 1, tok, lp, ws, ws.numel() * 8)
    for got in (out[0], (tok.cpu().numpy(), lp.cpu().numpy(), xd.cpu().numpy())):
        for a, b in zip(got, out[None]):
            assert a.tobytes() == b.tobytes()
    # the warped rows do not depend on the stream; the draws follow their own stream's uniform
    for tag in (1, 2):
        assert out[tag][2].tobytes() == out[None][2].tobytes()
        for r in range(rows):
            s, kept, _, q = sample_ref.warp_row(x[r], 0.8, 40, 0.9, 0.0)
            c = np.cumsum(np.where(kept, q, 0.0))
            u = spec_ref.uniform(int(seeds[r]), tag, int(ts[r]))
            j = int(out[tag][0][r])
            assert kept[j] and (c[j - 1] if j else 0.0) - sample_ref.DELTA <= u <= c[j] + sample_ref.DELTA, (tag, r, j)
    assert any((out[1][0] != out[None][0]).tolist()) and any((out[2][0] != out[1][0]).tolist())


def test_bad_arguments():
    from radvlm_amd import lib
    n, R = 16, 3
    p = torch.zeros(R, n, device="cuda")
    q = torch.zeros(R - 1, n, device="cuda")
    d = torch.zeros(R - 1, dtype=torch.int32, device="cuda")
    s = torch.zeros(1, dtype=torch.int64, device="cuda")
    t = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = torch.zeros(1, dtype=torch.int32, device="cuda")
    tok = torch.zeros(1, dtype=torch.int64, device="cuda")
    lp = torch.zeros(1, dtype=torch.float32, device="cuda")
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")
    good = dict(p=p, ld_p=n, q=q, ld_q=n, draft=d, seed=s, t0=t, groups=1, R=R, n=n, a=a, tok=tok, lp=lp, ws=ws, ws_bytes=ws.numel() * 8)
    L = lib.load()

    def call(**kw):
        v = dict(good, **kw)
        ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
        return L.rv_spec_accept_rows_f32(ptr(v["p"]), v["ld_p"], ptr(v["q"]), v["ld_q"], ptr(v["draft"]), ptr(v["seed"]), ptr(v["t0"]),
                                         v["groups"], v["R"], v["n"], ptr(v["a"]), ptr(v["tok"]), ptr(v["lp"]), ptr(v["ws"]), v["ws_bytes"],
                                         None)
    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(p=None), dict(q=None), dict(draft=None), dict(seed=None), dict(t0=None), dict(a=None), dict(tok=None), dict(lp=None),
                dict(ws=None), dict(R=0), dict(R=33), dict(n=0), dict(n=262145), dict(ld_p=n - 1), dict(ld_q=n - 1), dict(groups=0),
                dict(ws_bytes=L.rv_spec_ws_bytes(1, R) - 8), dict(ws=ws.data_ptr() + 4)):
        assert call(**bad) == -1, bad
    assert call(R=1, q=None, draft=None) == 0                             # no drafts: the plain draw needs neither
    torch.cuda.synchronize()

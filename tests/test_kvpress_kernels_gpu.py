"""GPU tests of the three SnapKV kernels at ABI level (radvlm_amd/csrc/kvpress.hip through ops.kv_votes / kv_select / kv_gather) against
tests/kvpress_ref.py.  Every output buffer, every padding column and V are pre-filled with a NaN (or a marker int) sentinel, so a
stray read shows as a NaN vote and a stray write as a missing sentinel."""
import math

import numpy as np
import pytest
import torch

import kvpress_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 128                     # KP_CHUNK of kvpress.hip: keys per vote workgroup
U = 2.0 ** -23                  # one fp32 ulp, relative: covers rounding to nearest and truncation
MARK = -12345


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _pack(seqs, H, Hkv, hd, pad=8):
    """(q [P, H, hd], k [P, Hkv, hd]) fp32 per sequence -> the packed bf16 q|k|v rows as a column view of a wider buffer (row stride
    larger than the width), V and the padding columns NaN, and cu."""
    width = (H + 2 * Hkv) * hd
    M = sum(q.shape[0] for q, _ in seqs)
    buf = torch.full((M, width + pad), float("nan"), dtype=torch.bfloat16)
    r = 0
    for q, k in seqs:
        P = q.shape[0]
        buf[r:r + P, :H * hd] = torch.from_numpy(q.reshape(P, -1)).bfloat16()
        buf[r:r + P, H * hd:(H + Hkv) * hd] = torch.from_numpy(k.reshape(P, -1)).bfloat16()
        r += P
    cu = np.concatenate([[0], np.cumsum([q.shape[0] for q, _ in seqs])]).astype(np.int32)
    return buf.to(DEV)[:, :width], torch.from_numpy(cu).to(DEV)


def _rounded(x):
    return torch.from_numpy(x).bfloat16().float().numpy().astype(np.float64)


def _votes(ops, seqs, H, Hkv, hd, w, scale=None, flags=None):
    qkv, cu = _pack(seqs, H, Hkv, hd)
    max_P = max(q.shape[0] for q, _ in seqs)
    out = torch.full((len(seqs), Hkv, max(max_P - w, 1)), float("nan"), dtype=torch.float32, device=DEV)
    ops.kv_votes(qkv, cu, H, Hkv, hd, w, max_P, scale=scale, out=out, flags=flags)
    return out


def _bound(q, k, w, scale, hd):
    """The relative error bound of one sequence's votes (test_votes_against_fp64 derives it)."""
    P, H, _ = q.shape
    Hkv = k.shape[1]
    G, n = H // Hkv, P - w
    A = S = 0.0
    for h in range(H):
        qa, ka = q[n:, h], k[:, h // G]
        A = max(A, float((np.abs(qa) @ np.abs(ka).T).max()) * scale)
        S = max(S, float(np.abs(qa @ ka.T).max()) * scale)
    ds = (hd + 1) * U * A
    nch = (P + CHUNK - 1) // CHUNK
    return 2.0 * (2.0 * ds + 2.0 * U * S + 2.0 * U) + (12 + nch + 1 + w * G + 5) * U


@pytest.mark.parametrize("heads", [(4, 4), (4, 2), (14, 2)])
@pytest.mark.parametrize("hd", [64, 128])
def test_votes_against_fp64(hd, heads):
    """Votes against kvpress_ref.votes in fp64 on the same bf16 inputs; every sequence alone has the bits it has in the batch; columns
    [n, ld_v) keep the sentinel.

    The gate, relative to the fp64 vote (a sum of positive terms, so relative bounds of the terms carry over), first order in
    u = 2^-23 (one fp32 ulp: it covers an accumulation that truncates instead of rounding):
      score s = scale * sum_i q_i k_i: the hd products of bf16 values are exact in fp32 (16 significant bits); hd - 1 additions and the
        multiplication by scale each err by at most u of a partial sum of magnitude <= A / scale, A = max over (row, key) of
        scale * sum_i |q_i k_i| (computed here from the inputs): |ds| <= (hd + 1) u A.
      exp(s - M): M is the score of some key (error ds again), the subtraction rounds by u |s - M| <= 2 u S, S = max |s|, and expf
        errs by at most 2 ulp: relative error <= 2 ds + 2 u S + 2 u.
      L = sum_c l_c exp(m_c - M): every term carries the same relative error; a chunk's l passes 8 sequential additions and a 4-level
        tree (12 u), the merge adds nch chunks in order (nch u); the division adds u.
      vote = sum over R = w G rows: a term passes fewer than R + 5 additions.
    Together: E = 2 (2 ds + 2 u S + 2 u) + (12 + nch + 1 + R + 5) u, about 7e-4 at hd 128 and 3e-4 at hd 64 on N(0, 1) inputs, an
    order below what a bf16-rounded score or probability would cost (4e-3).  The worst measured error / E over all shapes is printed;
    on one MI355X it was 0.0025 (hd 64, (4, 4)), 0.0013, 0.0008 (hd 64) and 0.0010, 0.0008, 0.0006 (hd 128): the bound is a worst-case
    linear one, and the gate is left as derived."""
    ops = _ops()
    H, Hkv = heads
    scale = 1.0 / math.sqrt(hd)
    rng = np.random.default_rng(hd * 100 + H * 10 + Hkv)
    worst = 0.0
    for w in (1, 5, 16, 32, 64):
        for ns in ((1, 2 * CHUNK + 1), (63, 2 * CHUNK - 1), (64, 65)):
            seqs = []
            for n in ns:
                P = n + w
                seqs.append((rng.standard_normal((P, H, hd)).astype(np.float32), rng.standard_normal((P, Hkv, hd)).astype(np.float32)))
            got = _votes(ops, seqs, H, Hkv, hd, w)
            for b, (q, k) in enumerate(seqs):
                n = ns[b]
                q64, k64 = _rounded(q), _rounded(k)
                ref = R.votes(q64, k64, w, scale)
                g = got[b, :, :n].double().cpu().numpy()
                assert np.isfinite(g).all()
                E = _bound(q64, k64, w, scale, hd)
                rel = np.abs(g - ref) / ref
                worst = max(worst, float(rel.max()) / E)
                assert (rel <= E).all(), (w, n, float(rel.max()), E)
                assert torch.isnan(got[b, :, n:]).all()                     # columns [n, ld_v) are not touched
                alone = _votes(ops, [seqs[b]], H, Hkv, hd, w)
                assert torch.equal(_bits(alone[0, :, :n]), _bits(got[b, :, :n]))
    print(f"kv_votes hd={hd} heads={heads}: worst error / bound = {worst:.3g}")
    assert worst < 1.0


def test_votes_flags_and_short_sequences():
    """A sequence with flags 0 and one no longer than the window are skipped: their rows keep the sentinel; the others' bits stay."""
    ops = _ops()
    H, Hkv, hd, w = 4, 2, 64, 5
    rng = np.random.default_rng(5)
    seqs = [(rng.standard_normal((P, H, hd)).astype(np.float32), rng.standard_normal((P, Hkv, hd)).astype(np.float32)) for P in (40, 5, 200, 3)]
    flags = torch.tensor([1, 1, 0, 1], dtype=torch.int32, device=DEV)
    got = _votes(ops, seqs, H, Hkv, hd, w, flags=flags)
    full = _votes(ops, seqs, H, Hkv, hd, w)
    assert torch.isnan(got[1]).all() and torch.isnan(got[2]).all() and torch.isnan(got[3]).all() and torch.isnan(full[1]).all()
    assert torch.equal(_bits(got[0, :, :35]), _bits(full[0, :, :35])) and not torch.isnan(full[2, :, :195]).any()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("j_star", [3, CHUNK - 1, CHUNK, 300])
def test_needle_is_kept(hd, j_star):
    """The needle input of test_kvpress_host.py (first chunk, the two sides of a chunk edge, the last chunk): every kv head keeps it
    at N - w = 1."""
    ops = _ops()
    w, P, H, Hkv = 8, 330, 4, 2
    per = [R.needle(P, w, hd, j_star, seed=j_star + 1000 * g) for g in range(Hkv)]
    q = np.concatenate([np.repeat(qg, H // Hkv, axis=1) for qg, _ in per], axis=1)
    k = np.concatenate([kg for _, kg in per], axis=1)
    qkv, cu = _pack([(q, k)], H, Hkv, hd)
    votes = torch.full((1, Hkv, P - w), float("nan"), dtype=torch.float32, device=DEV)
    ops.kv_votes(qkv, cu, H, Hkv, hd, w, P, scale=1.0, out=votes)
    keep = ops.kv_select(votes, cu, w + 1, w, 1).cpu().numpy()
    assert keep[0, :, 0].tolist() == [j_star] * Hkv
    assert keep[0, :, 1:].tolist() == [list(range(P - w, P))] * Hkv
    v = votes.cpu().numpy()[0]
    assert (v[:, j_star] > 10.0 * np.delete(v, j_star, axis=1).max(1)).all()


def _select_case(ops, rows, N, w, k, flags=None):
    """rows: per sequence a list of Hkv fp32 vote rows (equal length n_b).  Returns (device keep with MARK sentinel, cu)."""
    B, Hkv = len(rows), len(rows[0])
    ns = [len(r[0]) for r in rows]
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum([n + w for n in ns])]).astype(np.int32)).to(DEV)
    votes = torch.full((B, Hkv, max(ns)), float("nan"), dtype=torch.float32)
    for b, r in enumerate(rows):
        for g in range(Hkv):
            votes[b, g, :ns[b]] = torch.from_numpy(np.asarray(r[g], dtype=np.float32))
    keep = torch.full((B, Hkv, N), MARK, dtype=torch.int32, device=DEV)
    ops.kv_select(votes.to(DEV), cu, N, w, k, flags=flags, out=keep)
    return keep.cpu().numpy()


@pytest.mark.parametrize("k", [1, 3, 7, 63])
def test_select_exact_small(k):
    """Ties, plateaus that straddle the cut, all-equal rows, N - w = 1 and n - 1, denormal and huge votes; a sequence of P <= N and a
    flagged-off one keep the sentinel."""
    ops = _ops()
    rng = np.random.default_rng(k)
    w = 4
    for n, N in ((9, w + 1), (9, w + 8), (300, w + 37), (513, w + 256), (1025, w + 1024)):
        rows = [[rng.integers(0, 4, n).astype(np.float32) * 0.25, np.full(n, 0.5, np.float32)],            # few distinct values: ties
                [np.repeat(rng.random((n + 15) // 16).astype(np.float32), 16)[:n], np.zeros(n, np.float32)],    # plateaus of 16
                [rng.random(n).astype(np.float32), (rng.random(n) * 1e-42).astype(np.float32)],            # distinct; denormals
                [np.exp(rng.standard_normal(n) * 20).astype(np.float32), rng.random(n).astype(np.float32)]]
        short = [[rng.random(N - w).astype(np.float32)] * 2]                                             # P = N: not compressed
        flags = torch.tensor([1, 1, 1, 1, 1, 0], dtype=torch.int32, device=DEV)
        got = _select_case(ops, rows + short + rows[:1], N, w, k, flags=flags)
        for b in range(4):
            for g in range(2):
                assert got[b, g].tolist() == R.select(rows[b][g], N, w, k).tolist(), (n, N, b, g)
        assert (got[4] == MARK).all() and (got[5] == MARK).all()


def test_select_exact_long():
    """n = 7,571 (a 7,603-position prompt, w = 32), N = 1024, k = 7: random votes, a row of few distinct values, a one-hot row."""
    ops = _ops()
    rng = np.random.default_rng(7)
    n, w, N, k = 7571, 32, 1024, 7
    hot = np.zeros(n, np.float32)
    hot[5000] = 1.0
    rows = [[rng.random(n).astype(np.float32) ** 8, rng.integers(0, 3, n).astype(np.float32)], [hot, np.full(n, 1e-30, np.float32)]]
    got = _select_case(ops, rows, N, w, k)
    for b in range(2):
        for g in range(2):
            assert np.array_equal(got[b, g], R.select(rows[b][g], N, w, k)), (b, g)


@pytest.mark.parametrize("hd,Hkv", [(64, 2), (128, 1), (128, 3)])
def test_gather_exact(hd, Hkv):
    """Every kept slot holds its position's K and V per kv head; every other element of the cache keeps the sentinel; a sequence of
    P <= N and a flagged-off one write nothing; cache rows are taken from seq."""
    ops = _ops()
    rng = np.random.default_rng(hd + Hkv)
    N, kvd, L_max, rows = 11, Hkv * hd, 17, 6
    Ps = [30, 11, 12, 25]
    cu = np.concatenate([[0], np.cumsum(Ps)]).astype(np.int32)
    buf = torch.from_numpy(rng.standard_normal((cu[-1], 2 * kvd + 16)).astype(np.float32)).bfloat16().to(DEV)
    kv = buf[:, 8:8 + 2 * kvd]                                              # a column view: row stride larger than the width
    keep = np.stack([np.stack([np.sort(rng.choice(P, N, replace=False)) for _ in range(Hkv)]) for P in Ps]).astype(np.int32)
    seq = np.array([4, 1, 0, 3], dtype=np.int32)
    flags = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=DEV)
    sent = torch.full((rows, L_max, 2 * kvd), float("nan"), dtype=torch.bfloat16, device=DEV)
    cache = sent.clone()
    ops.kv_gather(kv, torch.from_numpy(cu).to(DEV), torch.from_numpy(keep).to(DEV), torch.from_numpy(seq).to(DEV), cache, Hkv, hd, flags=flags)
    want = sent.clone()
    for b in (0, 2):                                                        # 1: P = N; 3: flagged off
        for g in range(Hkv):
            src = kv[torch.from_numpy(cu[b] + keep[b, g]).long().to(DEV)]
            for off in (0, kvd):
                want[seq[b], :N, off + g * hd:off + (g + 1) * hd] = src[:, off + g * hd:off + (g + 1) * hd]
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))
    assert not torch.isnan(cache[4, :N]).any() and torch.isnan(cache[4, N:]).all()


def test_refused_arguments():
    """Each bad argument gives RV_ERR_ARG (-1) before any launch -- the outputs keep their sentinels -- and a good call follows."""
    ops = _ops()
    from radvlm_amd import lib
    H, Hkv, hd, w, P, N = 4, 2, 64, 4, 40, 12
    rng = np.random.default_rng(0)
    seqs = [(rng.standard_normal((P, H, hd)).astype(np.float32), rng.standard_normal((P, Hkv, hd)).astype(np.float32))]
    qkv, cu = _pack(seqs, H, Hkv, hd)
    ld = qkv.stride(0)
    votes = torch.full((1, Hkv, P - w), float("nan"), dtype=torch.float32, device=DEV)
    wsb = lib.load().rv_kv_votes_ws_bytes(1, H, Hkv, w, P)
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=DEV)
    kq = qkv[:, H * hd:]

    def v_args(**o):
        a = dict(q=qkv, ld_q=ld, k=kq, ld_k=ld, cu=cu, flags=None, max_P=P, votes=votes, ld_v=P - w, ws=ws, wsb=wsb, B=1, H=H, Hkv=Hkv, hd=hd,
                 w=w, scale=0.125)
        a.update(o)
        return list(a.values())
    for bad in (dict(q=None), dict(k=None), dict(cu=None), dict(votes=None), dict(ws=None), dict(B=0), dict(B=65536), dict(H=5), dict(H=18),
                dict(Hkv=0), dict(hd=96), dict(w=0), dict(w=65), dict(max_P=w), dict(ld_q=ld + 4), dict(ld_q=H * hd - 8), dict(ld_k=ld + 4),
                dict(ld_k=Hkv * hd - 8), dict(ld_v=P - w - 1), dict(wsb=wsb - 4), dict(q=qkv.data_ptr() + 2)):
        with pytest.raises(lib.RadvlmHipError, match="rv_kv_votes_f32 failed with code -1"):
            lib.call("rv_kv_votes_f32", *v_args(**bad))
    torch.cuda.synchronize()
    assert torch.isnan(votes).all()
    lib.call("rv_kv_votes_f32", *v_args())
    assert torch.isfinite(votes).all()

    keep = torch.full((1, Hkv, N), MARK, dtype=torch.int32, device=DEV)
    sb = lib.load().rv_kv_select_ws_bytes(1, Hkv, P - w)
    sws = torch.empty(sb // 4, dtype=torch.int32, device=DEV)

    def s_args(**o):
        a = dict(votes=votes, ld_v=P - w, cu=cu, flags=None, keep=keep, ws=sws, wsb=sb, B=1, Hkv=Hkv, N=N, w=w, k=3)
        a.update(o)
        return list(a.values())
    for bad in (dict(votes=None), dict(cu=None), dict(keep=None), dict(ws=None), dict(wsb=sb - 4), dict(B=0), dict(Hkv=0), dict(N=w), dict(w=0),
                dict(w=65, N=70), dict(k=0), dict(k=4), dict(k=65), dict(k=-1), dict(ld_v=0)):
        with pytest.raises(lib.RadvlmHipError, match="rv_kv_select_i32 failed with code -1"):
            lib.call("rv_kv_select_i32", *s_args(**bad))
    torch.cuda.synchronize()
    assert (keep == MARK).all()
    lib.call("rv_kv_select_i32", *s_args())
    ref = [R.select(votes[0, g].cpu().numpy(), N, w, 3).tolist() for g in range(Hkv)]
    assert keep[0].cpu().tolist() == ref

    kvd, L_max = Hkv * hd, N + 3
    cache = torch.full((2, L_max, 2 * kvd), float("nan"), dtype=torch.bfloat16, device=DEV)
    seq = torch.tensor([1], dtype=torch.int32, device=DEV)
    kv = qkv[:, H * hd:]

    def g_args(**o):
        a = dict(kv=kv, ld_kv=ld, v_off=kvd, cu=cu, flags=None, keep=keep, seq=seq, cache=cache, ld_c=2 * kvd, L_max=L_max, n_rows=2, B=1,
                 Hkv=Hkv, hd=hd, N=N)
        a.update(o)
        return list(a.values())
    for bad in (dict(kv=None), dict(cu=None), dict(keep=None), dict(seq=None), dict(cache=None), dict(B=0), dict(Hkv=0), dict(hd=32),
                dict(N=L_max + 1), dict(N=1), dict(n_rows=0), dict(v_off=kvd + 4), dict(v_off=kvd - 8), dict(ld_kv=ld + 4),
                dict(ld_kv=2 * kvd - 8), dict(ld_c=2 * kvd - 8), dict(ld_c=2 * kvd + 4)):
        with pytest.raises(lib.RadvlmHipError, match="rv_kv_gather_bf16 failed with code -1"):
            lib.call("rv_kv_gather_bf16", *g_args(**bad))
    torch.cuda.synchronize()
    assert torch.isnan(cache).all()
    lib.call("rv_kv_gather_bf16", *g_args())
    assert torch.isnan(cache[0]).all() and torch.isnan(cache[1, N:]).all() and not torch.isnan(cache[1, :N, :kvd]).any()     # V is the NaN sentinel

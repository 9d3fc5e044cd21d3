"""GPU tests of seeded sampling: rv_sample_rows_f32 against the float64 restatement (tests/sample_ref.py) -- kept sets within the band
the kernel's documented summation order allows, the draw against the float64 CDF, the distribution of many draws, determinism,
independence of the launch, the limits that reduce to argmax, logprobs, bad arguments, unusable rows -- and generate() /
generate_batch() with do_sample=True, seed=... end to end on the toy goldens."""
import numpy as np
import pytest
import torch

import sample_ref
from logits_ref import has_repeated_ngram
from radvlm_amd import portable_rng
from sample_ref import DELTA
from test_generate_batch_gpu import _alone, _batch, _requests
from test_generate_gpu import CASES, LOGITS_FP32_TOL, _engine, _load, _model, _prompt

pytestmark = pytest.mark.gpu

LOGPROB_TOL = 1e-5                # the absolute tolerance of test_generate_batch_gpu.test_rows_kernel_logprob for its log-softmax
STEPS = 64
PAD = 5                           # columns beyond n: the rows are strided [:, :n] views and start at every alignment
SENTINEL = np.float32(777.0)
BASE_T = (0, 1, 2, 4, 17, 48, 3)

# name -> (temperature, top_k, top_p, min_p); top_k "n+5" is resolved per row length
SETTINGS = {
    "temperature": (0.7, 0, 1.0, 0.0),
    "top_k_1": (1.0, 1, 1.0, 0.0),
    "top_k_50": (1.0, 50, 1.0, 0.0),
    "top_k_above_n": (1.0, "n+5", 1.0, 0.0),
    "top_p_0.9": (1.0, 0, 0.9, 0.0),
    "top_p_0.5": (1.0, 0, 0.5, 0.0),
    "min_p_0.05": (1.0, 0, 1.0, 0.05),
    "chat_default": (0.2, 50, 0.7, 0.0),
    "everything": (0.7, 50, 0.9, 0.05),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _setting(name, n):
    T, k, p, mp = SETTINGS[name]
    return T, (n + 5 if k == "n+5" else k), p, mp


def _rows(n, scale, rows, seed0=1):
    x = np.full((rows, n + PAD), SENTINEL, dtype=np.float32)
    for r in range(rows):
        x[r, :n] = portable_rng.normal(seed0 + r, n, (n,), scale)
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(xd, n, seeds, ts, st, write=False, logprob=False):
    """rv_sample_rows_f32 on the device rows xd[:, :n] -> (tokens, logprobs or None), numpy."""
    from radvlm_amd import ops
    sd = torch.tensor([int(s) for s in seeds], dtype=torch.int64, device="cuda")
    td = torch.tensor([int(t) for t in ts], dtype=torch.int32, device="cuda")
    lpo = torch.empty(xd.shape[0], dtype=torch.float32, device="cuda") if logprob else None
    tok = ops.sample_rows(xd[:, :n], n, sd, td, st[0], st[1], st[2], st[3], write_scores=write, logprob=lpo)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), None if lpo is None else lpo.cpu().numpy()


def _check_kept(x, got, st):
    """x: the fp32 row given to the kernel, got: the row it wrote (write_scores).  Asserts the contract of the kept set; returns its mask."""
    T, k, p, mp = st
    n = x.size
    s, ref_kept, tail, _ = sample_ref.warp_row(x, T, k, p, mp)
    kept = np.isfinite(got)
    assert DELTA <= 1e-4
    assert np.array_equal(_bits(got[kept]), _bits(s[kept])), "kept scores are the fp32 quotient x / T"
    assert (got[~kept] == -np.inf).all()
    tk = np.ones(n, dtype=bool)
    if k and k < n:
        tk = s >= np.partition(s, n - k)[n - k]
    assert not kept[~tk].any(), "top-k is exact: nothing below the k-th largest survives"
    if (~kept).any():
        assert s[kept].min() > s[~kept].max(), "the kept set is an upper set in value"
    s64 = s.astype(np.float64)
    e = np.exp(s64 - s64.max())
    must_keep, must_drop = tk.copy(), ~tk
    if p < 1.0:
        cut = 1.0 - p
        top = tail > cut + DELTA
        top[np.argmax(s)] = True
        must_keep &= top
        must_drop |= tk & (tail < cut - DELTA)
    if mp > 0.0:
        # p_i against min_p * max p, with the band taken on the ratio e_i = p_i / max p (the maximum always survives, so the ratio does
        # not depend on what else does).  That is at least as strict on the kernel as a band of DELTA on p_i itself (max p <= 1), and
        # the looser band would hold up to 2.4 % of a 152,064-entry row of scale 1 (its Z is in the thousands), against the 0.1 %
        # condition below; on the ratio it holds 0 - 2 entries.
        must_keep &= e > mp + DELTA
        must_drop |= e < mp - DELTA
    band = ~(must_keep | must_drop)
    assert band.sum() <= max(1, n // 1000), ("the band holds more than 0.1 % of the row", int(band.sum()), n)
    assert kept[must_keep].all(), np.flatnonzero(must_keep & ~kept)[:8]
    assert not kept[must_drop].any(), np.flatnonzero(must_drop & kept)[:8]
    if p >= 1.0 and mp <= 0.0:
        assert np.array_equal(kept, tk)
    return kept, int(band.sum())


def _check_draw(C, kept, tok, u):
    """C: the float64 CDF over the kernel's kept set.  Returns (identical to the float64 draw, distance of u to the nearest boundary)."""
    j = int(tok)
    assert 0 <= j < C.size and kept[j], j
    lo = C[j - 1] if j > 0 else 0.0
    assert lo - DELTA <= u <= C[j] + DELTA, (j, lo, u, C[j])
    ref = min(int(np.searchsorted(C, u, side="right")), int(np.flatnonzero(kept)[-1]))
    return j == ref, min(abs(u - lo), abs(u - C[j]))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("n", [1000, 32000, 152064])
def test_kept_set_draw_and_logprob(n, scale, rows):
    _need_gpu()
    from conftest import record_measurement
    x = _rows(n, scale, rows)
    seeds = [1000 + 7 * r for r in range(rows)]
    base_t = [BASE_T[r % 7] for r in range(rows)] if rows > 1 else [17]
    worst_flip, flips, worst_lp, worst_band = 0.0, 0, 0.0, 0
    for name in SETTINGS:
        st = _setting(name, n)
        xd = torch.from_numpy(x).cuda()
        tok_w, lp_w = _launch(xd, n, seeds, base_t, st, write=True, logprob=True)
        got = xd.cpu().numpy()
        assert np.array_equal(got[:, n:], x[:, n:]), "columns >= n are never touched"
        xr = torch.from_numpy(x).cuda()                                   # read-only launches on the rows as given
        toks = np.stack([_launch(xr, n, seeds, [b + i for b in base_t], st)[0] for i in range(STEPS)])
        assert np.array_equal(_bits(xr.cpu().numpy()), _bits(x)), "write_scores = 0 leaves the row as it is"
        assert np.array_equal(toks[0], tok_w), "the token does not depend on write_scores"
        for r in range(rows):
            kept, nband = _check_kept(x[r, :n], got[r, :n], st)
            worst_band = max(worst_band, nband)
            C = sample_ref.cdf(got[r, :n], kept)
            for i in range(STEPS):
                same, dist = _check_draw(C, kept, toks[i, r], sample_ref.uniform(seeds[r], base_t[r] + i))
                if not same:
                    flips, worst_flip = flips + 1, max(worst_flip, dist)
            s64 = got[r, :n].astype(np.float64)
            e = np.where(kept, np.exp(s64 - s64[kept].max()), 0.0)
            ref_lp = s64[tok_w[r]] - s64[kept].max() - np.log(e.sum())
            worst_lp = max(worst_lp, abs(float(lp_w[r]) - ref_lp))
            assert abs(float(lp_w[r]) - ref_lp) <= LOGPROB_TOL, (name, r, float(lp_w[r]), ref_lp)
    record_measurement("sample_rows_draw", n=n, scale=scale, rows=rows, draws=len(SETTINGS) * rows * STEPS, non_identical=flips,
                       worst_boundary_distance=worst_flip, worst_logprob_err=worst_lp, worst_band_entries=worst_band, delta=DELTA)


def test_distribution_of_many_draws():
    """20,000 steps of one seed on one row (n = 64, top_k = 10, T = 1): chi-square of the counts against the float64 q, df = 9, below
    33.72 = scipy.stats.chi2.isf(1e-4, 9).  Seeds and inputs are fixed, so the outcome is."""
    _need_gpu()
    n, N = 64, 20000
    x = portable_rng.normal(5, n, (n,), 1.0)
    s, kept, _, q = sample_ref.warp_row(x, 1.0, 10, 1.0, 0.0)
    assert kept.sum() == 10
    xd = torch.from_numpy(np.tile(x, (N, 1))).cuda()
    tok, _ = _launch(xd, n, [42] * N, range(N), (1.0, 10, 1.0, 0.0))
    assert kept[tok].all()
    counts = np.bincount(tok, minlength=n)[kept].astype(np.float64)
    chi2 = float((((counts - N * q[kept]) ** 2) / (N * q[kept])).sum())
    from conftest import record_measurement
    record_measurement("sample_rows_chi2", chi2=chi2, df=9, draws=N)
    assert chi2 < 33.72, chi2


@pytest.mark.parametrize("n", [1000, 152064])
def test_determinism_and_independence_of_the_launch(n):
    _need_gpu()
    x = _rows(n, 4.0, 7, seed0=20)
    seeds = [3, 3, 99, 12345678901, 5, 0, 77]
    ts = list(BASE_T)
    for name in ("temperature", "chat_default", "everything", "top_p_0.9"):
        st = _setting(name, n)
        runs = []
        for _ in range(2):
            xd = torch.from_numpy(x).cuda()
            tok, lp = _launch(xd, n, seeds, ts, st, write=True, logprob=True)
            runs.append((tok, _bits(lp), _bits(xd.cpu().numpy())))
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), name
        for r in (0, 3, 6):                                               # the row alone: another base address, another grid
            xd = torch.from_numpy(np.ascontiguousarray(x[r:r + 1])).cuda()
            tok, lp = _launch(xd, n, seeds[r:r + 1], ts[r:r + 1], st, write=True, logprob=True)
            assert int(tok[0]) == int(runs[0][0][r]) and _bits(lp)[0] == runs[0][1][r], (name, r)
            assert np.array_equal(_bits(xd.cpu().numpy())[0], runs[0][2][r]), (name, r)


@pytest.mark.parametrize("n", [1000, 32000, 152064])
def test_limits_reduce_to_argmax(n):
    _need_gpu()
    from radvlm_amd import ops
    x = _rows(n, 1.0, 7, seed0=40)
    xd = torch.from_numpy(x).cuda()
    want = ops.argmax_rows(xd[:, :n], n).cpu().numpy()
    srt = np.sort(x[:, :n], axis=1)
    gap = srt[:, -1] - srt[:, -2]
    assert (gap > 0).all()                                                # rows without ties
    for i in range(8):
        tok, _ = _launch(xd, n, [50 + r for r in range(7)], [i] * 7, (1.0, 1, 1.0, 0.0))
        assert np.array_equal(tok, want)
    # T = 1e-3: where the runner-up's share is below the resolution of u (gap / T > 30: e^-30 n < 2^-25) every u gives the argmax
    sure = gap / 1e-3 > 30.0
    assert int(sure.sum()) == {1000: 7, 32000: 6, 152064: 6}[n]           # the rows are fixed: counted on the CPU from portable_rng
    for i in range(8):
        tok, _ = _launch(xd, n, [60 + r for r in range(7)], [i] * 7, (1e-3, 0, 1.0, 0.0))
        assert np.array_equal(tok[sure], want[sure])


def test_bad_arguments_launch_nothing():
    _need_gpu()
    from radvlm_amd import lib, ops
    x = torch.zeros(2, ops.LOGITS_PROCESS_MAX_N + 8, device="cuda")      # wider than the limit: only the limit itself rejects n above it
    out = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")
    t = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.load().rv_sample_ws_bytes(2) // 8, dtype=torch.int64, device="cuda")
    ok = dict(n=64, seed=seed, T=1.0, k=0, p=1.0, mp=0.0, ws=ws, ws_bytes=ws.numel() * 8)
    for bad in (dict(n=ops.LOGITS_PROCESS_MAX_N + 1), dict(n=0), dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(p=1.5), dict(p=-0.1),
                dict(mp=1.5), dict(k=-1), dict(seed=None), dict(ws=None), dict(ws_bytes=ws.numel() * 8 - 8)):
        a = {**ok, **bad}
        with pytest.raises(lib.RadvlmHipError):
            lib.call("rv_sample_rows_f32", x, x.stride(0), 2, a["n"], a["seed"], t, a["T"], a["k"], a["p"], a["mp"], 1, out, None, a["ws"],
                     a["ws_bytes"])
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all() and (x.cpu() == 0).all()


def test_unusable_rows_give_minus_one():
    _need_gpu()
    from radvlm_amd.generation import _check_sampled
    n = 1000
    x = _rows(n, 1.0, 5, seed0=70)
    x[1, :n] = -np.inf
    x[2, 17] = np.nan
    x[3, 900] = np.inf
    x[4, :n] = -np.inf
    x[4, 123] = 0.25                                                      # one finite entry: usable
    for name in ("temperature", "everything"):
        xd = torch.from_numpy(x).cuda()
        tok, lp = _launch(xd, n, [1, 2, 3, 4, 5], [0, 1, 2, 3, 4], _setting(name, n), write=True, logprob=True)
        assert tok.tolist()[1:4] == [-1, -1, -1] and tok[0] >= 0 and tok[4] == 123
        assert np.isnan(lp[1:4]).all() and abs(lp[4]) <= LOGPROB_TOL
        after = xd.cpu().numpy()
        assert np.array_equal(_bits(after[1:4]), _bits(x[1:4])), "an unusable row is left as it is"
        with pytest.raises(ValueError):
            _check_sampled(tok)
        _check_sampled(tok, [0, 4])


# ------------------------------------------------------------------------------------------------ generate() end to end
def _gen(model, p, image, size, n, **kw):
    return model.generate(torch.from_numpy(p[None]), images=None if image is None else [image], image_sizes=None if size is None else [size],
                          max_new_tokens=n, eos_token_id=None, **kw)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_top_k_1_is_greedy(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p = _prompt(g, 0)
    want = _gen(model, p, images[0], sizes[0], 12)
    got = _gen(model, p, images[0], sizes[0], 12, do_sample=True, seed=5, top_k=1, temperature=0.7)
    assert torch.equal(got, want)


def test_generate_scores_tokens_and_seeds(golden_dir):
    differs = False
    for case in ("toy", "toy_qwen"):
        g, images, sizes, kw = _load(golden_dir, case)
        model = _model(CASES[case]["geo"], kw)
        V = model.engine.vocab
        prompts = [_prompt(g, 0), _prompt(g, 1)[:-2]]
        T = max(p.size for p in prompts)
        ids, am = np.zeros((2, T), dtype=np.int64), np.zeros((2, T), dtype=bool)
        for b, p in enumerate(prompts):
            ids[b, T - p.size:], am[b, T - p.size:] = p, True
        args = dict(images=images[:2], image_sizes=sizes[:2], attention_mask=torch.from_numpy(am), max_new_tokens=10, eos_token_id=None,
                    do_sample=True, temperature=0.7, top_p=0.9, output_scores=True, output_logits=True, return_dict_in_generate=True)
        seed = 31
        out = model.generate(torch.from_numpy(ids), seed=seed, **args)
        assert tuple(out.sequences.shape) == (2, 10) and len(out.scores) == len(out.logits) == 10
        st = (0.7, 50, 0.9, 0.0)                                          # top_k: HF's default of 50
        for t in range(10):
            for b in range(2):
                raw, warped = out.logits[t][b, :V].cpu().numpy(), out.scores[t][b, :V].cpu().numpy()
                kept, _ = _check_kept(raw, warped, st)
                _check_draw(sample_ref.cdf(warped, kept), kept, int(out.sequences[b, t]), sample_ref.uniform(seed + b, t))
        again = model.generate(torch.from_numpy(ids), seed=seed, **args)
        assert torch.equal(again.sequences, out.sequences)
        assert all(torch.equal(a, b) for a, b in zip(again.scores, out.scores))
        lst = model.generate(torch.from_numpy(ids), seed=[seed, seed + 1], **args)            # the list form of the same seeds
        assert torch.equal(lst.sequences, out.sequences)
        other = model.generate(torch.from_numpy(ids), seed=seed + 1000, **args)
        differs |= not torch.equal(other.sequences, out.sequences)
    assert differs, "another seed gave the same tokens on every case"


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_processors_run_before_the_sampler(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p = _prompt(g, 0)
    for seed in (1, 2, 3):
        out = _gen(model, p, images[0], sizes[0], 24, do_sample=True, seed=seed, repetition_penalty=1.3, no_repeat_ngram_size=2)
        assert not has_repeated_ngram(out[0].cpu().tolist(), 2), (seed, out[0].tolist())


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_processors_run_before_the_sampler_in_generate_batch(golden_dir, case):
    """DevicePicker with an active processor: rv_logits_process_argmax_rows_f32, then the sampler, the drawn token into the history."""
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    reqs = _requests(g, images, sizes, case)
    budgets = [24, 7, 16, 24, 12, 24, 9, 20][:len(reqs)] + [10] * max(0, len(reqs) - 8)
    kws = dict(max_batch_size=3, max_new_tokens=budgets, do_sample=True, seed=40, top_p=0.9, repetition_penalty=1.3, no_repeat_ngram_size=2,
               eos_token_id=None)
    out = _batch(model, reqs, **kws)
    for i in range(len(reqs)):
        toks = out[f"req_{i}"].generated_tokens
        assert len(toks) == budgets[i] and not has_repeated_ngram(toks, 2), (i, toks)
    again = _batch(model, reqs, **kws)
    assert all(again[k].generated_tokens == out[k].generated_tokens for k in out)
    plain = _batch(model, reqs, **{**kws, "repetition_penalty": 1.0, "no_repeat_ngram_size": 0})
    assert any(plain[k].generated_tokens != out[k].generated_tokens for k in out), "the processors changed nothing"


def _own_draws(tokens, scores, seed, logprobs=None):
    """Every token is the draw, with u(seed, t), from the warped scores its own run had at step t (-inf: removed)."""
    for t, (tok, sc) in enumerate(zip(tokens, scores)):
        s1 = sc.astype(np.float64)
        kept = np.isfinite(s1)
        _check_draw(sample_ref.cdf(s1, kept), kept, int(tok), sample_ref.uniform(seed, t))
        if logprobs is not None:
            ref = s1[tok] - s1[kept].max() - np.log(np.exp(s1[kept] - s1[kept].max()).sum())
            assert abs(logprobs[t] - ref) <= LOGPROB_TOL, (t, logprobs[t], ref)


def _compare_draws(tok_a, sc_a, tok_b, sc_b, seed, score_tol=None):
    """The rule of test_generate_batch_gpu._compare, restated for draws.  Two runs' scores agree only up to rounding (another prefill
    group, the cached path).  _compare excuses a near tie of the argmax; a draw is decided by where u falls in the CDF, so here the near
    tie is u within `margin` of a boundary of its token's interval, and the margin is what the two runs' difference can move a boundary
    by: if every kept score differs by at most d, every q_i changes by a factor within e^(+-2d), so a partial sum C and its complement
    1 - C do too and C moves by at most expm1(2d); the kernel's own band delta is added on each side.  With the same bits in both runs
    d = 0 and the margin is 2 delta.  Kept sets that differ are a near tie at the cut, and the entries they differ in must lie there.  While the two histories agree every step is
    checked: the tokens are equal, or the step is a near tie and the comparison ends there (anything else fails).  score_tol: the scores
    of every such step are also within it (relative to max |score|, as test_generate_cache_gpu does for logits).  Returns the steps
    whose tokens were equal."""
    n = min(len(tok_a), len(tok_b))
    for t in range(n):
        a, b = sc_a[t].astype(np.float64), sc_b[t].astype(np.float64)
        ka, kb = np.isfinite(a), np.isfinite(b)
        both = ka & kb
        d = float(np.abs(a[both] - b[both]).max())
        if score_tol is not None:
            assert d / float(np.abs(b[kb]).max()) <= score_tol, (t, d)
        if int(tok_a[t]) == int(tok_b[t]):
            continue
        margin = float(np.expm1(2.0 * d)) + 2.0 * DELTA
        C, u, tok = sample_ref.cdf(b, kb), sample_ref.uniform(seed, t), int(tok_b[t])
        dist = min(u - (C[tok - 1] if tok > 0 else 0.0), C[tok] - u)
        print("tokens part at step", t, "d", d, "margin", margin, "u to the boundary", dist)
        if np.array_equal(ka, kb):
            assert dist <= margin, (t, list(tok_a), list(tok_b), dist, margin)
        else:
            # an entry one run kept and the other removed lies at the cut: the kept set is an upper set in value, so in the run that
            # removed it it is below every kept score, and in the run that kept it it is therefore within 2 d of the lowest score
            # both runs kept
            for s, k in ((a, ka), (b, kb)):
                only = k & ~both
                assert not only.any() or float(s[only].max()) <= float(s[both].min()) + 2.0 * d + 1e-12, (t, d)
        return t
    return n


class _Recorder:
    """A stopping criterion that stops nothing and keeps the scores each request was drawn from (generate_batch calls it per request
    with [1, t] ids and the warped [1, vocab] scores).  It is not told which request it is called for, so the scores are filed under
    the tokens generated before the step, and a request finds its own among them: the scores that give the logprob generate_batch
    returned for the token AND from which u(the request's seed, t) draws that token.  None found: the request was not drawn as promised."""

    def __init__(self, V):
        self.V, self.seen = V, {}

    def __call__(self, ids, scores):
        self.seen.setdefault(tuple(ids[0].tolist()[:-1]), []).append(scores[0, :self.V].cpu().numpy().copy())
        return False

    def scores_of(self, tokens, logprobs, seed):
        out = []
        for t, tok in enumerate(tokens):
            hits = []
            for sc in self.seen[tuple(tokens[:t])]:
                s1 = sc.astype(np.float64)
                k = np.isfinite(s1)
                if not (k[tok] and abs(s1[tok] - s1[k].max() - np.log(np.exp(s1[k] - s1[k].max()).sum()) - logprobs[t]) <= LOGPROB_TOL):
                    continue
                C = sample_ref.cdf(s1, k)
                u = sample_ref.uniform(seed, t)
                if (C[tok - 1] if tok > 0 else 0.0) - DELTA <= u <= C[tok] + DELTA:
                    hits.append(sc)
            assert hits, (t, tok, logprobs[t], len(self.seen[tuple(tokens[:t])]))
            out.append(hits[0])
        return out


BATCH_SETTINGS = {"temperature": dict(temperature=0.8, top_k=0), "warpers": dict(temperature=0.7, top_k=20, top_p=0.9)}


@pytest.mark.parametrize("setting", list(BATCH_SETTINGS))
@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_batch_request_draws_what_it_draws_alone(golden_dir, case, setting):
    from conftest import record_measurement
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    V = model.engine.vocab
    reqs = _requests(g, images, sizes, case)
    budgets = [6, 0, 9, 1, 12, 4, 7, 10][:len(reqs)] + [5] * max(0, len(reqs) - 8)
    seed = 900
    settings = dict(do_sample=True, eos_token_id=None, **BATCH_SETTINGS[setting])
    steps = {}
    runs = {}
    for slots in (3, 1):                                                  # 1 slot: every request is prefilled and decoded alone
        rec = _Recorder(V)
        out = _batch(model, reqs, max_batch_size=slots, max_new_tokens=budgets, seed=seed, return_logprobs=True, stopping_criteria=[rec],
                     **settings)
        runs[slots] = out
        steps[slots] = 0
        for i, r in enumerate(reqs):
            o = out[f"req_{i}"]
            assert len(o.generated_tokens) == len(o.logprobs) == budgets[i]
            if not budgets[i]:
                continue
            sc = rec.scores_of(o.generated_tokens, o.logprobs, seed + i)
            _own_draws(o.generated_tokens, sc, seed + i, o.logprobs)     # request i's own seed and its own step, whatever the slot
            one = _alone(model, r, budgets[i], seed=seed + i, **settings)
            _own_draws(one.sequences[0].cpu().tolist(), [s[0, :V].cpu().numpy() for s in one.scores], seed + i)
            alone = one.sequences[0].cpu().tolist()
            steps[slots] += _compare_draws(o.generated_tokens, sc, alone, [s[0, :V].cpu().numpy() for s in one.scores], seed + i)
    again = _batch(model, reqs, max_batch_size=3, max_new_tokens=budgets, seed=[seed + i for i in range(len(reqs))], **settings)
    for k in again:                                                       # the list form of the same seeds, a second run: the same tokens
        assert again[k].generated_tokens == runs[3][k].generated_tokens
    record_measurement("sample_batch_vs_alone", case=case, setting=setting, requests=len(reqs), total_steps=int(sum(budgets)),
                       steps_compared_3_slots=steps[3], steps_compared_1_slot=steps[1])
    print("sample_batch_vs_alone", case, setting, "steps", int(sum(budgets)), "compared", steps)
    # 1 slot: every request is prefilled alone and decoded at B = 1, the kernels and shapes of generate() alone, so the scores are the
    # same bits, the margin is 2 delta and no step is a near tie: all of them are compared.  3 slots: the floor of the greedy
    # test_generate_batch_equals_generate_alone, one step per request on average.
    assert steps[1] == sum(budgets)
    assert steps[3] >= len(reqs)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_sampled_conversation_through_the_cache(golden_dir, case):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    V = model.engine.vocab
    p1 = _prompt(g, 0)
    settings = dict(do_sample=True, temperature=0.8, top_k=0, output_scores=True, return_dict_in_generate=True)
    cache = GenerationCache()
    a1 = _gen(model, p1, images[0], sizes[0], 8, seed=4, past_key_values=cache, **settings)
    b1 = _gen(model, p1, images[0], sizes[0], 8, seed=4, **settings)
    assert torch.equal(a1.sequences, b1.sequences)                        # an empty cache changes nothing
    assert all(torch.equal(x, y) for x, y in zip(a1.scores, b1.scores))
    follow = np.random.default_rng(11).integers(3, V, 20).astype(np.int64)
    p2 = np.concatenate([p1, a1.sequences[0].cpu().numpy(), follow])
    a2 = _gen(model, p2, images[0], sizes[0], 8, seed=5, past_key_values=cache, **settings)
    b2 = _gen(model, p2, images[0], sizes[0], 8, seed=5, **settings)
    assert cache.get_seq_length() > p2.size                               # the second turn went through the cache
    # the cached turn agrees with the fresh one up to rounding (tests/test_generate_cache_gpu.py: LOGITS_FP32_TOL on the first step's
    # scores); each run's tokens are the draws from its own scores, and equal to the other run's up to the first near tie
    s_a, s_b = a2.scores[0][0, :V].cpu(), b2.scores[0][0, :V].cpu()
    assert float((s_a - s_b).abs().max() / s_b.abs().max()) <= LOGITS_FP32_TOL
    for o in (a2, b2):
        _own_draws(o.sequences[0].cpu().tolist(), [s[0, :V].cpu().numpy() for s in o.scores], 5)
    n = _compare_draws(a2.sequences[0].cpu().tolist(), [s[0, :V].cpu().numpy() for s in a2.scores], b2.sequences[0].cpu().tolist(),
                       [s[0, :V].cpu().numpy() for s in b2.scores], 5, score_tol=LOGITS_FP32_TOL)
    from conftest import record_measurement
    record_measurement("sample_cache_two_turn", case=case, steps_compared=n)
    print("sample_cache_two_turn", case, "compared", n)
    assert n >= 1                                                         # the first token of the cached turn is the fresh turn's


def test_unusable_scores_raise_in_generate(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    eng = model.engine
    orig = eng.prefill

    def poisoned(*a, **k):
        cache, logits = orig(*a, **k)
        logits[0, 3] = float("nan")
        return cache, logits

    eng.prefill = poisoned
    try:
        with pytest.raises(ValueError):
            _gen(model, _prompt(g, 0), images[0], sizes[0], 4, do_sample=True, seed=1)
    finally:
        del eng.prefill
    assert tuple(_gen(model, _prompt(g, 0), images[0], sizes[0], 4, do_sample=True, seed=1).shape) == (1, 4)


def test_sampling_leaves_training_state_unchanged(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    reqs = _requests(g, images, sizes, "toy")

    def step(with_generate):
        eng = _engine("toy")
        if with_generate:
            from radvlm_amd.generation import generate_batch, greedy_generate, parse_batch_kwargs, parse_generate_kwargs
            greedy_generate(eng, g["input_ids"], g["attention_mask"], images, sizes,
                            parse_generate_kwargs(dict(max_new_tokens=6, attention_mask=g["attention_mask"], do_sample=True, seed=3,
                                                       temperature=0.7, top_p=0.9, repetition_penalty=1.2)))
            generate_batch(eng, [r[0] for r in reqs], [r[1] for r in reqs], None,
                           parse_batch_kwargs(dict(max_new_tokens=6, do_sample=True, seed=3, min_p=0.05), len(reqs)), max_batch_size=3,
                           return_logprobs=True)
        loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return float(loss), eng.lm.flat.clone(), eng.grads.clone(), eng.lora_step

    a, b = step(False), step(True)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]

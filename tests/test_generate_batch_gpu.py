"""GPU tests of generate_batch() (continuous batching): rv_logits_process_argmax_rows_f32 against the numpy restatement and against
rv_logits_process_argmax_f32 at a uniform step, its logprobs against a float64 log-softmax, prefill into slots of a shared KVCache,
decode over a shared cache, and generate_batch end to end against generate() run alone per request."""
import numpy as np
import pytest
import torch

from logits_ref import argmax, process_row, same_values
from test_generate_gpu import CASES, LOGITS_FP32_TOL, _engine, _load, _model, _pad_batch, _prompt
from test_logits_process_gpu import SETTINGS, _hist, _ref_kwargs, _rows
from test_logits_process_gpu import _run as _run_uniform

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _run_rows(x_full, n, hist, slot, t, min_new, cfg, logprobs=False):
    """rv_logits_process_argmax_rows_f32 on a copy of x_full (rows strided: the [:, :n] view) -> (x after, tokens, logprobs, lp)."""
    from radvlm_amd import ops
    from radvlm_amd.generation import LogitsProcessors
    lp = LogitsProcessors(cfg, n)
    xd = torch.from_numpy(x_full).cuda()
    hd = torch.from_numpy(np.ascontiguousarray(hist, dtype=np.int32)).cuda()
    info = torch.from_numpy(np.stack([slot, t, min_new]).astype(np.int32)).cuda()
    i32 = lambda ids: torch.tensor(ids, dtype=torch.int32, device="cuda") if ids else None
    tok_b, off_b = lp.bad_csr()
    bad = (torch.from_numpy(tok_b).cuda(), torch.from_numpy(off_b).cuda()) if lp.multi else (None, None)
    lpo = torch.empty(x_full.shape[0], dtype=torch.float32, device="cuda") if logprobs else None
    tok = ops.logits_process_argmax_rows(xd[:, :n], n, hd, info[0], info[1], info[2], lp.penalty, lp.ngram,
                                         i32(sorted(set(lp.suppress) | set(lp.one))), i32(lp.begin), i32(lp.eos), *bad, logprob=lpo)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), tok.cpu().numpy(), None if lpo is None else lpo.cpu().numpy(), lp


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", [1000, 32000, 152064])
@pytest.mark.parametrize("rows", [1, 7, 32])
def test_rows_kernel_matches_restatement(n, rows):
    _need_gpu()
    from radvlm_amd.generation import parse_generate_kwargs
    rng = np.random.default_rng(n + rows)
    S, T = rows + 3, 48                                               # more history rows than launch rows: rows map to slots
    for name in SETTINGS:
        cfg = parse_generate_kwargs(SETTINGS[name])
        x = _rows(rng, rows, n)
        hist = _hist(rng, S, T, n)
        slot = rng.permutation(S)[:rows]
        t = np.array([(0, 1, 2, 4, 17, 48, 3)[r % 7] for r in range(rows)]) if rows > 1 else np.array([17])
        min_new = rng.integers(0, 60, rows)
        got, tok, _, lp = _run_rows(x, n, hist, slot, t, min_new, cfg)
        assert np.array_equal(got[:, n:], x[:, n:], equal_nan=True)  # columns >= n are never touched
        for r in range(rows):
            kw = _ref_kwargs(cfg, lp)
            kw["min_new"] = int(min_new[r])
            want = process_row(x[r, :n], hist[slot[r], :t[r]], **kw)
            assert same_values(got[r, :n], want), (name, r, int(t[r]))
            assert int(tok[r]) == argmax(want), (name, r, int(t[r]))


@pytest.mark.parametrize("n,rows", [(1000, 7), (32000, 32), (152064, 32)])
@pytest.mark.parametrize("t", [0, 1, 5, 40])
def test_rows_kernel_bit_identical_to_uniform_kernel(n, rows, t):
    """Every row at the same step: the processed rows and tokens are the bits of rv_logits_process_argmax_f32."""
    _need_gpu()
    from radvlm_amd.generation import parse_generate_kwargs
    rng = np.random.default_rng(10 * n + t)
    for name in SETTINGS:
        cfg = parse_generate_kwargs(SETTINGS[name])
        x = _rows(rng, rows, n)
        h = _hist(rng, rows, max(t, 1), n)
        old_x, old_tok, lp = _run_uniform(x, n, h[:, :t], t, cfg)
        new_x, new_tok, _, _ = _run_rows(x, n, h, np.arange(rows), np.full(rows, t), np.full(rows, lp.min_new), cfg)
        assert np.array_equal(_bits(new_x), _bits(old_x)), name
        assert np.array_equal(new_tok, old_tok), name


@pytest.mark.parametrize("n", [1000, 32000, 152064])
def test_rows_kernel_logprob(n):
    _need_gpu()
    from conftest import record_measurement
    from radvlm_amd.generation import parse_generate_kwargs
    rng = np.random.default_rng(n)
    rows, T = 32, 40
    worst = 0.0
    for kw in ({}, SETTINGS["penalty_up"], SETTINGS["all"], SETTINGS["suppress"]):
        cfg = parse_generate_kwargs(kw)
        x = (rng.standard_normal((rows, n + 8)) * 5).astype(np.float32)
        x[0, :] = 0.0                                                 # flat: log(1 / n)
        x[1, 7] = 80.0                                                # peaked: ~0
        x[2, :] *= 8.0
        hist = _hist(rng, rows, T, n)
        t = rng.integers(0, T + 1, rows)
        min_new = rng.integers(0, 60, rows)
        got, tok, lpv, _ = _run_rows(x, n, hist, np.arange(rows), t, min_new, cfg, logprobs=True)
        plain_x, plain_tok, _, _ = _run_rows(x, n, hist, np.arange(rows), t, min_new, cfg)
        assert np.array_equal(_bits(got), _bits(plain_x)) and np.array_equal(tok, plain_tok)
        for r in range(rows):
            p = got[r, :n].astype(np.float64)
            m = p.max()
            ref = p[tok[r]] - (m + np.log(np.exp(p - m).sum()))
            err = abs(float(lpv[r]) - ref)
            worst = max(worst, err)
            assert err <= 1e-5, (kw, r, float(lpv[r]), ref)
    record_measurement("logits_rows_logprob", n=n, worst_abs_err=worst)


def test_rows_kernel_rejects_bad_arguments():
    _need_gpu()
    from radvlm_amd import lib, ops
    x = torch.zeros(2, 64, device="cuda")
    out = torch.empty(2, dtype=torch.int64, device="cuda")
    info = torch.zeros(3, 2, dtype=torch.int32, device="cuda")
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_logits_process_argmax_rows_f32", x, x.stride(0), 2, ops.LOGITS_PROCESS_MAX_N + 1, None, 0, 0, 0, info[0], info[1], info[2],
                 1.0, 0, None, 0, None, 0, None, 0, None, None, 0, out, None)
    with pytest.raises(lib.RadvlmHipError):                           # history without a pointer
        lib.call("rv_logits_process_argmax_rows_f32", x, x.stride(0), 2, 64, None, 8, 2, 8, info[0], info[1], info[2],
                 1.0, 0, None, 0, None, 0, None, 0, None, None, 0, out, None)


# ------------------------------------------------------------------------------------------------ engine: prefill into slots, decode
def _two_prompts(g):
    p = [_prompt(g, 0), _prompt(g, 1)]
    p[1] = p[1][:-2]
    return p


@pytest.mark.parametrize("case", list(CASES))
def test_prefill_into_slots_is_bit_identical(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    prompts = _two_prompts(g)
    ids, am = _pad_batch(prompts, "right")
    ids, am = ids.numpy(), am.numpy()
    lens = eng.plan(ids, am, None, images[:2], sizes[:2])["lens"]
    L_max = int(lens.max()) + 9
    ref, ref_logits = eng.prefill(ids, am, images[:2], sizes[:2], max_new_tokens=9)
    shared = eng.new_kv_cache(4, L_max)
    for t in shared.layers:
        t.copy_(torch.randn(t.shape, device=t.device).to(t.dtype))   # stale contents everywhere
    before = [t.clone() for t in shared.layers]
    _, logits = eng.prefill(ids, am, images[:2], sizes[:2], cache=shared, slots=[3, 1])
    assert torch.equal(logits, ref_logits)
    assert shared.lens.tolist() == [0, int(lens[1]), 0, int(lens[0])]
    for i in range(len(shared.layers)):
        for b, s in enumerate((3, 1)):
            n = int(lens[b])
            assert torch.equal(shared.layers[i][s, :n], ref.layers[i][b, :n]), (i, b)
            assert torch.equal(shared.layers[i][s, n:], before[i][s, n:])
        for s in (0, 2):
            assert torch.equal(shared.layers[i][s], before[i][s])
    with pytest.raises(ValueError):
        eng.prefill(ids, am, images[:2], sizes[:2], cache=shared, slots=[1, 1])
    with pytest.raises(ValueError):
        eng.prefill(ids, am, images[:2], sizes[:2], cache=shared, slots=[0, 4])


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_decode_on_shared_cache_equals_own_cache(golden_dir, case):
    """Rows admitted at different times into a shared 4-slot cache (idle slots fed token 0 at position 0) give the logits, bit for bit,
    of decode_step on a KVCache holding that row alone."""
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    prompts = _two_prompts(g)
    lens = [int(eng.plan(p[None], None, None, [images[b]], [sizes[b]])["lens"][0]) for b, p in enumerate(prompts)]
    L_max = max(lens) + 12
    toks = np.random.default_rng(3).integers(0, eng.vocab, (2, 12))
    own = []
    for b, p in enumerate(prompts):
        c, lg = eng.prefill(p[None], None, [images[b]], [sizes[b]], max_new_tokens=L_max - lens[b])
        seq = [lg[0].clone()]
        for k in range(8 if b == 0 else 5):
            seq.append(eng.decode_step(c, [int(toks[b, k])])[0].clone())
        own.append(seq)
    shared = eng.new_kv_cache(4, L_max)

    def step(feed):
        idle = np.array([s not in feed for s in range(4)])
        shared.lens[idle] = 0
        out = eng.decode_step(shared, [feed.get(s, 0) for s in range(4)])
        shared.lens[idle] = 0
        return out

    _, lg = eng.prefill(prompts[0][None], None, [images[0]], [sizes[0]], cache=shared, slots=[2])
    assert torch.equal(lg[0], own[0][0])
    for k in range(3):                                               # slot 2 alone decodes
        assert torch.equal(step({2: int(toks[0, k])})[2], own[0][k + 1])
    _, lg = eng.prefill(prompts[1][None], None, [images[1]], [sizes[1]], cache=shared, slots=[0])   # admission while slot 2 decodes
    assert torch.equal(lg[0], own[1][0])
    for k in range(5):
        out = step({2: int(toks[0, k + 3]), 0: int(toks[1, k])})
        assert torch.equal(out[2], own[0][k + 4]) and torch.equal(out[0], own[1][k + 1]), k


# ------------------------------------------------------------------------------------------------ generate_batch end to end
def _requests(g, images, sizes, case):
    """At least 7 requests: golden prompts, truncated variants, a text-only prompt, one image used twice."""
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    B = g["input_ids"].shape[0]
    reqs = []
    for b in range(min(B, 2)):
        p = _prompt(g, b)
        reqs.append((p, images[b], sizes[b]))
        reqs.append((p[:-2], images[b], sizes[b]))
    p0 = _prompt(g, 0)
    text = p0[p0 != IMAGE_TOKEN_INDEX]
    reqs.insert(2, (text, None, None))
    reqs.append((p0[:-4], images[0], sizes[0]))                       # images[0] a third time
    reqs.append((text[:6], None, None))
    reqs.append((_prompt(g, 1)[:-1], images[1], sizes[1]))
    return reqs


def _batch(model, reqs, max_batch_size=3, **kw):
    return model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs],
                                max_batch_size=max_batch_size, **kw)


def _alone(model, req, budget, **kw):
    p, im, s = req
    return model.generate(torch.from_numpy(p[None]), images=None if im is None else [im], image_sizes=None if s is None else [s],
                          max_new_tokens=budget, output_scores=True, return_dict_in_generate=True, **kw)


def _compare(got, one, logprobs=None):
    """Tokens equal to the alone run up to its first near tie (the rule of test_batch_rows_generate_as_if_alone).  Returns the steps
    compared and whether the whole output was equal."""
    seq = one.sequences[0].cpu().tolist()
    if not one.scores:
        assert got == [] and seq == []
        return 0, True
    n = len(seq)
    for t in range(n):
        s1 = one.scores[t][0].cpu()
        fin = s1[torch.isfinite(s1)]
        if logprobs is not None and t < len(got) and got[t] == seq[t]:
            ref = float(torch.log_softmax(s1.double(), 0)[seq[t]])
            assert abs(logprobs[t] - ref) <= 2 * LOGITS_FP32_TOL * float(fin.abs().max()), (t, logprobs[t], ref)
        top = torch.topk(fin, 2).values
        if float(top[0] - top[1]) < 3 * LOGITS_FP32_TOL * float(fin.abs().max()):
            return t, got == seq
        assert t < len(got) and got[t] == seq[t], (t, got, seq)
    assert got == seq
    return n, True


@pytest.mark.parametrize("case", list(CASES))
def test_generate_batch_equals_generate_alone(golden_dir, case):
    from conftest import record_measurement
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    reqs = _requests(g, images, sizes, case)
    budgets = [6, 0, 9, 1, 12, 4, 7, 10][:len(reqs)] + [5] * max(0, len(reqs) - 8)
    out = _batch(model, reqs, max_new_tokens=budgets, eos_token_id=None)
    assert list(out) == [f"req_{i}" for i in range(len(reqs))]
    steps, exact = 0, 0
    for i, r in enumerate(reqs):
        o = out[f"req_{i}"]
        assert o.prompt_ids == r[0].tolist() and o.error is None and o.is_finished() and o.logprobs == []
        assert len(o.generated_tokens) == budgets[i]
        n, eq = _compare(o.generated_tokens, _alone(model, r, budgets[i], eos_token_id=None))
        steps, exact = steps + n, exact + int(eq)
    assert out["req_1"].generated_tokens == []
    record_measurement("generate_batch_vs_alone", case=case, requests=len(reqs), steps_compared=steps, requests_equal=exact)
    assert steps >= len(reqs)


def test_eos_and_stopping_criteria(golden_dir):
    """EOS taken from a free-running output and a criterion that stops one request at t = 3: early finishers free their slots (3 slots,
    8 requests) and every request, later admissions included, equals generate() alone with the same settings."""
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    reqs = _requests(g, images, sizes, "toy")
    free = _batch(model, reqs, max_new_tokens=12, eos_token_id=None)
    f0 = free["req_0"].generated_tokens
    k = next((i for i in range(1, 12) if f0[i] not in f0[:i]), 0)    # random weights may loop: the first new token
    eos = f0[k]
    out = _batch(model, reqs, max_new_tokens=12, eos_token_id=eos)
    assert out["req_0"].generated_tokens == f0[:k + 1]              # the first group is admitted identically in both runs
    for i, r in enumerate(reqs):
        got = out[f"req_{i}"].generated_tokens
        assert eos not in got[:-1] and (got[-1] == eos or len(got) == 12)
        _compare(got, _alone(model, r, 12, eos_token_id=eos))
    seen = []
    stop_prefix = f0[:3]

    def crit(ids, scores):
        seen.append((tuple(ids.shape), tuple(scores.shape)))
        return ids.shape[1] == 3 and ids[0].tolist() == stop_prefix

    out = _batch(model, reqs, max_new_tokens=12, eos_token_id=None, stopping_criteria=[crit])
    assert all(a[0] == 1 and b == (1, model.engine.vocab) for a, b in seen)
    assert sum(len(o.generated_tokens) for o in out.values()) == len(seen)
    assert out["req_0"].generated_tokens == stop_prefix
    for i, r in enumerate(reqs):
        _compare(out[f"req_{i}"].generated_tokens, _alone(model, r, 12, eos_token_id=None, stopping_criteria=[crit]))


def test_reused_slot_never_reads_stale_rows(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p = _prompt(g, 0)
    reqs = [(p, images[0], None), (p[:-4], images[0], None), (p[:-9], images[0], None)]
    out = _batch(model, reqs, max_batch_size=1, max_new_tokens=10, eos_token_id=None)
    for i, r in enumerate(reqs):
        _compare(out[f"req_{i}"].generated_tokens, _alone(model, r, 10, eos_token_id=None))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_processor_settings_equal_generate_alone(golden_dir, name):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    reqs = _requests(g, images, sizes, "toy")[:5]
    settings = dict(SETTINGS[name])
    settings.setdefault("eos_token_id", None)
    out = _batch(model, reqs, max_batch_size=2, max_new_tokens=16, **settings)
    for i, r in enumerate(reqs):
        _compare(out[f"req_{i}"].generated_tokens, _alone(model, r, 16, **settings))


def test_logprobs_and_determinism(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    reqs = _requests(g, images, sizes, "toy_qwen")
    settings = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=None)
    a = _batch(model, reqs, max_new_tokens=10, return_logprobs=True, **settings)
    b = _batch(model, reqs, max_new_tokens=10, return_logprobs=True, **settings)
    for k in a:
        assert a[k].generated_tokens == b[k].generated_tokens
        assert np.array_equal(np.float32(a[k].logprobs).view(np.uint32), np.float32(b[k].logprobs).view(np.uint32))
    for i, r in enumerate(reqs):
        o = a[f"req_{i}"]
        assert len(o.logprobs) == len(o.generated_tokens) == 10 and all(v <= 1e-6 for v in o.logprobs)
        _compare(o.generated_tokens, _alone(model, r, 10, **settings), logprobs=o.logprobs)


def test_generate_batch_leaves_training_state_unchanged(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    reqs = _requests(g, images, sizes, "toy")

    def step(with_generate):
        eng = _engine("toy")
        if with_generate:
            from radvlm_amd.generation import generate_batch, parse_batch_kwargs
            generate_batch(eng, [r[0] for r in reqs], [r[1] for r in reqs], None,
                           parse_batch_kwargs(dict(max_new_tokens=6, repetition_penalty=1.2), len(reqs)), max_batch_size=3,
                           return_logprobs=True)
        loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return float(loss), eng.lm.flat.clone(), eng.grads.clone(), eng.lora_step

    a, b = step(False), step(True)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]


def test_generate_batch_argument_errors(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p = _prompt(g, 0)
    assert model.generate_batch([]) == {}
    for bad in (dict(do_sample=True), dict(num_beams=2), dict(streamer=object())):
        with pytest.raises(NotImplementedError):
            model.generate_batch([p], images=[images[0]], **bad)
    with pytest.raises(TypeError):
        model.generate_batch([p], images=[images[0]], attention_mask=torch.ones(1, p.size))
    with pytest.raises(ValueError):
        model.generate_batch([p, p], images=[images[0]])
    with pytest.raises(ValueError):
        model.generate_batch([p])

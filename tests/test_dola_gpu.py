"""GPU tests of DoLa (dola_layers=) in the engine, generate() and generate_batch() on the toy goldens (2 decoder layers, vocab 1000).

The reference leg runs none of the DoLa loop: the run's tokens are replayed through prefill / decode_step with tap_layers=, and per
step the chain log-softmax kernel -> float64 divergence and selection of dola_ref -> dola_ref.contrast -> the CPU processors of
logits_ref.py -> argmax must give the run's layers, scores and tokens without a tolerance.  A step whose two largest float64
divergences are closer than the sum of their error bounds ends the comparison for that row; at most one row in ten may end early."""
import numpy as np
import pytest
import torch

import dola_ref
from logits_ref import argmax, process_row, same_values
from test_generate_batch_gpu import _compare
from test_generate_gpu import CASES, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu
T_NEW = 8
EARLY = dict(rows=0, ended=0)            # rows replayed / rows whose comparison ended early, over the whole module


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ taps
def _spy(eng, name):
    """Record (args, result) of every call of eng.<name> until the returned undo() runs."""
    orig, calls = getattr(eng, name), []

    def wrapped(*a, **k):
        r = orig(*a, **k)
        calls.append((a, k, r))
        return r

    setattr(eng, name, wrapped)
    return calls, lambda: delattr(eng, name)


def _check_taps(model, prompts, images, sizes, taps):
    eng = model.engine
    ids, am = _pad_batch(prompts, "left")
    B, V, d = len(prompts), eng.vocab, eng.l["d"]
    head = eng.W("lm_head.weight")
    n = len(taps)
    # prefill: mature logits and K|V rows are the bits of the call without taps
    c0, l0 = eng.prefill(ids.numpy(), am.numpy(), images, sizes, max_new_tokens=4)
    calls, undo = _spy(eng, "_layer_forward")
    try:
        c1, l1, cand = eng.prefill(ids.numpy(), am.numpy(), images, sizes, max_new_tokens=4, tap_layers=taps)
    finally:
        undo()
    assert torch.equal(_bits(l0), _bits(l1)) and all(torch.equal(a, b) for a, b in zip(c0.layers, c1.layers))
    assert tuple(cand.shape) == (n, B, V) and cand.dtype == torch.float32 and torch.isfinite(cand).all()
    lens = eng.plan(ids.numpy(), am.numpy(), None, list(images), sizes)["lens"].astype(np.int64)
    last = torch.from_numpy(np.cumsum(lens) - 1).cuda()
    entering = {i: a[1] for (a, k, r) in calls for i in [a[0]]}              # x as it enters layer i
    hs = torch.cat([entering[c][last] for c in taps], 0)
    want = eng._decode_linear(hs, head, out_dtype=torch.float32).view(n, B, -1)[:, :, :V]
    assert torch.equal(_bits(cand), _bits(want))
    assert not torch.equal(cand[0], l1)                                      # a candidate is not the mature row
    # decode_step
    tok = torch.arange(B, dtype=torch.int64) + 5
    d0 = eng.decode_step(c0, tok).clone()
    calls, undo = _spy(eng, "_decode_linear")
    try:
        d1, dc = eng.decode_step(c1, tok, tap_layers=taps)
    finally:
        undo()
    assert torch.equal(_bits(d0), _bits(d1)) and all(torch.equal(a, b) for a, b in zip(c0.layers, c1.layers))
    assert tuple(dc.shape) == (n, B, V) and torch.isfinite(dc).all() and np.array_equal(c0.lens, c1.lens)
    from radvlm_amd import ops
    x = {0: ops.gather_rows(tok.to("cuda", torch.int32), d, eng.W("model.embed_tokens.weight"))}
    for i in range(eng.l["layers"] - 1):
        x[i + 1] = calls[4 * i + 3][2]                                       # q|k|v, o, gate|up, down: the down projection's output
    want = eng._decode_linear(torch.cat([x[c] for c in taps], 0), head, out_dtype=torch.float32).view(n, B, -1)[:, :, :V]
    assert torch.equal(_bits(dc), _bits(want))
    return d1, dc


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_taps_keep_the_mature_bits_and_are_lm_head_of_the_tapped_rows(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    eng = model.engine
    assert eng.l["layers"] == 2
    _check_taps(model, [_prompt(gd, 0)], images[:1], sizes[:1], (0, 1))
    _check_taps(model, [_prompt(gd, 0)], images[:1], sizes[:1], (1,))
    six = [_prompt(gd, b % 3)[:len(_prompt(gd, b % 3)) - b // 3] for b in range(6)]
    im6, sz6 = [images[b % 3] for b in range(6)], [sizes[b % 3] for b in range(6)]
    _check_taps(model, six, im6, sz6, (1, 0))
    one = _check_taps(model, [_prompt(gd, 0)], images[:1], sizes[:1], (0, 1))
    try:                                 # B = 6 past the skinny kernel's row limit: the mature rows and the candidates take the GEMM
        eng.gemv_max_m = 4
        _check_taps(model, six, im6, sz6, (0, 1))
    finally:
        del eng.gemv_max_m
    assert eng.tap_lm_head == "stacked"
    try:                                 # the two-launch arrangement gives the same bits
        eng.tap_lm_head = "second"
        two = _check_taps(model, [_prompt(gd, 0)], images[:1], sizes[:1], (0, 1))
    finally:
        del eng.tap_lm_head
    assert torch.equal(_bits(one[0]), _bits(two[0])) and torch.equal(_bits(one[1]), _bits(two[1]))
    with pytest.raises(ValueError):
        eng.prefill(np.asarray([[1, 2, 3]]), None, None, None, tap_layers=(0, 2))
    with pytest.raises(ValueError):
        eng.prefill(np.asarray([[1, 2, 3]]), None, None, None, tap_layers=(1, 1))
    with pytest.raises(ValueError):
        eng.prefill(np.asarray([[1, 2, 3]]), None, None, None, tap_layers=())


# ------------------------------------------------------------------------------------------------ generate() against a host loop
def _replay(model, prompts, images, sizes, layers, out, side="left", settings=None, kv_dtype=None, sampling=None):
    """Teacher-forced replay of a generate(dola_layers=layers) run `out` (dict output with scores and logits)."""
    from radvlm_amd import ops
    eng = model.engine
    V, B = eng.vocab, len(prompts)
    layers = list(layers)
    ids, am = _pad_batch(prompts, side)
    seq = out.sequences
    T = seq.shape[1]
    settings = dict(settings or {})
    eos = settings.get("eos_token_id")
    pk = dict(penalty=settings.get("repetition_penalty"), ngram=settings.get("no_repeat_ngram_size", 0),
              eos=[] if eos is None else [eos], min_new=settings.get("min_new_tokens", 0) if eos is not None else 0)
    plain = pk == dict(penalty=None, ngram=0, eos=[], min_new=0)
    kv = {} if kv_dtype is None else dict(kv_dtype=kv_dtype)
    cache, f, c = eng.prefill(ids.numpy(), am.numpy(), images, sizes, max_new_tokens=T, tap_layers=tuple(layers), **kv)
    toks = seq.cpu().numpy()
    lay = out.dola_premature_layers.cpu().numpy()
    assert lay.shape == toks.shape and lay.dtype == np.int64
    comparing, finished = [True] * B, [False] * B
    EARLY["rows"] += B
    for t in range(T):
        assert torch.equal(_bits(out.logits[t]), _bits(f)), t               # the raw mature rows, cloned before the transform
        lf = ops.log_softmax_rows(f.clone(), V)
        lq = torch.stack([ops.log_softmax_rows(c[k].clone(), V) for k in range(len(layers))])
        if len(layers) == 1:
            ch, sure = np.zeros(B, dtype=np.int64), np.ones(B, dtype=bool)
        else:
            lf64, lq64 = torch.log_softmax(f.double(), -1), torch.log_softmax(c.double(), -1)
            J = torch.stack([dola_ref.jsd64(lf64, lq64[k]) for k in range(len(layers))], 1)
            bound = torch.stack([dola_ref.jsd_error_bound(lf64, lq64[k]) for k in range(len(layers))], 1)
            top = torch.topk(J, 2, dim=1)
            sure = ((top.values[:, 0] - top.values[:, 1]) > bound.gather(1, top.indices).sum(1)).cpu().numpy()
            ch = dola_ref.select(J.cpu().numpy())
        want = dola_ref.contrast(lf, lq[torch.from_numpy(ch).cuda(), torch.arange(B, device="cuda")])
        if sampling is not None:
            sd, sk = sampling
            rows = want.clone()
            tok = ops.sample_rows(rows, V, torch.tensor(sd, dtype=torch.int64, device="cuda"), torch.full((B,), t, dtype=torch.int32, device="cuda"),
                                  sk["temperature"], sk["top_k"], sk["top_p"], 0.0).cpu().numpy()
        got = out.scores[t].cpu().numpy()
        want = want.cpu().numpy()
        for b in range(B):
            if comparing[b] and not finished[b] and not sure[b]:
                comparing[b] = False
                EARLY["ended"] += 1
            if not comparing[b]:
                continue
            if finished[b]:
                assert lay[b, t] == -1
                continue
            assert lay[b, t] == layers[ch[b]], (t, b)
            if sampling is not None:
                assert int(toks[b, t]) == int(tok[b]), (t, b)
            else:
                w = process_row(want[b], toks[b, :t], **pk)
                assert same_values(got[b], w), (t, b)
                if plain:
                    assert np.array_equal(got[b].view(np.int32), w.view(np.int32)), (t, b)
                assert int(toks[b, t]) == argmax(w), (t, b)
            finished[b] = eos is not None and int(toks[b, t]) == eos
        if t < T - 1:
            f, c = eng.decode_step(cache, seq[:, t].cpu(), tap_layers=tuple(layers))
    return comparing


def _generate(model, prompts, images, sizes, side="left", T=T_NEW, **kw):
    ids, am = _pad_batch(prompts, side)
    return model.generate(ids, images=images, image_sizes=sizes, attention_mask=am, max_new_tokens=T, output_scores=True, output_logits=True,
                          return_dict_in_generate=True, **dict({"eos_token_id": None}, **kw))


def _three(gd, images, sizes):
    p = [_prompt(gd, 0), _prompt(gd, 1)[:-3], _prompt(gd, 2)[:-1]]
    return p, images[:3], sizes[:3]


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
@pytest.mark.parametrize("B,side", [(1, "right"), (3, "left")])
def test_generate_equals_the_replayed_chain(golden_dir, case, B, side):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _three(gd, images, sizes)
    p, im, sz = p[:B], im[:B], sz[:B]
    out = _generate(model, p, im, sz, side, dola_layers=[0, 1])
    assert tuple(out.sequences.shape) == (B, T_NEW) and tuple(out.dola_premature_layers.shape) == (B, T_NEW)
    _replay(model, p, im, sz, [0, 1], out, side)
    out = _generate(model, p, im, sz, side, dola_layers=(1, 0))             # the list's order is the tie order and the index base
    _replay(model, p, im, sz, [1, 0], out, side)
    settings = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4)
    free = _generate(model, p, im, sz, side, dola_layers=[0, 1], **settings)
    _replay(model, p, im, sz, [0, 1], free, side, settings=dict(settings, eos_token_id=None))
    eos = int(free.sequences[0, 5])                                         # banned for 4 steps, then live: rows finish, layers become -1
    out = _generate(model, p, im, sz, side, dola_layers=[0, 1], **dict(settings, eos_token_id=eos))
    _replay(model, p, im, sz, [0, 1], out, side, settings=dict(settings, eos_token_id=eos))
    hit = (out.sequences[0] == eos).nonzero()
    assert hit.numel() > 0
    first = int(hit[0])
    assert (out.dola_premature_layers[0, :first + 1] >= 0).all() and (out.dola_premature_layers[0, first + 1:] == -1).all()


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_seeded_sampling_on_the_contrasted_rows(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _three(gd, images, sizes)
    seeds, sk = [11, 29, 5], dict(temperature=0.9, top_k=40, top_p=0.95)
    a = _generate(model, p, im, sz, dola_layers=[0, 1], do_sample=True, seed=seeds, **sk)
    b = _generate(model, p, im, sz, dola_layers=[0, 1], do_sample=True, seed=seeds, **sk)
    greedy = _generate(model, p, im, sz, dola_layers=[0, 1])
    assert torch.equal(a.sequences, b.sequences) and not torch.equal(a.sequences, greedy.sequences)
    _replay(model, p, im, sz, [0, 1], a, sampling=(seeds, sk))


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_single_candidate(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _three(gd, images, sizes)
    out = _generate(model, p, im, sz, dola_layers="high")                   # 2 layers: "high" is [1]
    assert (out.dola_premature_layers == 1).all()
    assert all(_replay(model, p, im, sz, [1], out))
    low = _generate(model, p, im, sz, dola_layers="low")                    # and "low" is [0]
    assert (low.dola_premature_layers == 0).all()
    assert all(_replay(model, p, im, sz, [0], low))


def test_dola_changes_the_scores_and_off_is_off(golden_dir):
    from radvlm_amd import ops
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p, im, sz = _three(gd, images, sizes)
    base = _generate(model, p, im, sz, repetition_penalty=1.2)              # before any DoLa call on this model
    assert not hasattr(base, "dola_premature_layers")
    on = _generate(model, p, im, sz, dola_layers=[0, 1])
    V = model.engine.vocab
    assert any(not torch.equal(on.scores[t], ops.log_softmax_rows(on.logits[t].clone(), V)) for t in range(T_NEW))
    assert torch.equal(_bits(on.logits[0]), _bits(base.logits[0]))          # the same prompt pass
    for off in (dict(), dict(dola_layers=None)):
        again = _generate(model, p, im, sz, repetition_penalty=1.2, **off)
        assert torch.equal(again.sequences, base.sequences)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again.logits + again.scores, base.logits + base.scores))
    reqs = [p[0], p[1]]
    b0 = model.generate_batch(reqs, images=im[:2], image_sizes=sz[:2], max_new_tokens=5, eos_token_id=None, return_logprobs=True)
    b1 = model.generate_batch(reqs, images=im[:2], image_sizes=sz[:2], max_new_tokens=5, eos_token_id=None, return_logprobs=True, dola_layers=None)
    assert {k: (v.generated_tokens, v.logprobs) for k, v in b0.items()} == {k: (v.generated_tokens, v.logprobs) for k, v in b1.items()}


def test_int8_cache_and_quantized_decoders_compose(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    p, im, sz = _three(gd, images, sizes)
    model = _model("toy", kw)
    out = _generate(model, p, im, sz, dola_layers=[0, 1], kv_cache_dtype="int8")
    _replay(model, p, im, sz, [0, 1], out, kv_dtype="int8")
    model.quantize_decoder_()
    out = _generate(model, p, im, sz, dola_layers=[0, 1])
    _replay(model, p, im, sz, [0, 1], out)
    model4 = _model("toy", kw)
    model4.quantize_decoder_("mxfp4")
    out = _generate(model4, p, im, sz, dola_layers=[1, 0])
    _replay(model4, p, im, sz, [1, 0], out)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_batch_equals_generate_alone(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    p0, p1, p2 = _prompt(gd, 0), _prompt(gd, 1), _prompt(gd, 2)
    reqs = [(p0, images[0], sizes[0]), (p1[:-2], images[1], sizes[1]), (p0[p0 != IMAGE_TOKEN_INDEX], None, None), (p2[:-1], None, None),
            (p1[:-3], images[1], sizes[1])]
    budgets = [3, 8, 6, 7, 5]            # three slots for five requests: slots are reused, and free slots exist while the last ones decode
    settings = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=None)
    out = model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=3,
                               max_new_tokens=budgets, return_logprobs=True, dola_layers=[0, 1], **settings)
    for i, r in enumerate(reqs):
        o = out[f"req_{i}"]
        assert len(o.generated_tokens) == len(o.logprobs) == budgets[i]
        one = model.generate(torch.from_numpy(r[0][None]), images=None if r[1] is None else [r[1]], image_sizes=None if r[2] is None else [r[2]],
                             max_new_tokens=budgets[i], output_scores=True, return_dict_in_generate=True, dola_layers=[0, 1], **settings)
        _compare(o.generated_tokens, one, logprobs=o.logprobs)
    plain = model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=3,
                                 max_new_tokens=budgets, return_logprobs=True, **settings)
    assert any(plain[k].logprobs != out[k].logprobs for k in out)


def test_refusals_through_the_model(golden_dir):
    from radvlm_amd.generation import GenerationCache
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p = _prompt(gd, 0)
    ids = torch.from_numpy(p[None])
    call = lambda **extra: model.generate(ids, images=images[:1], image_sizes=sizes[:1], max_new_tokens=3, **extra)
    for bad in ("middle", [], [0, 0], [1.0], [True], [2], [-1], list(range(17)), 1):
        with pytest.raises(ValueError):
            call(dola_layers=bad)
    with pytest.raises(ValueError):
        model.generate_batch([p], images=[images[0]], max_new_tokens=3, dola_layers=[0, 2])
    with pytest.raises(NotImplementedError, match="dola_layers"):
        call(dola_layers="high", guidance_scale=1.5)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        call(dola_layers="high", past_key_values=GenerationCache())
    with pytest.raises(NotImplementedError, match="dola_layers"):
        call(dola_layers="high", prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        model.generate_batch([p, p], images=[images[0], images[0]], max_new_tokens=3, dola_layers="high", share_prefix=True)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        model.generate_beams(ids, images=images[:1], image_sizes=sizes[:1], num_beams=2, max_new_tokens=3, dola_layers="high")
    cache = model.engine.new_kv_cache(1, 64)
    model.engine.prefill(p[None], None, images[:1], sizes[:1], cache=cache, slots=[0])
    with pytest.raises(TypeError):
        model.engine.verify_step(cache, np.asarray([1, 2]), tap_layers=(0,))
    assert call(dola_layers="low").shape == (1, 3)                          # and a good call follows


def test_at_most_one_row_in_ten_ended_early(golden_dir):
    """Over every replay of this module (run alone: over two replays of its own), the rows whose comparison stopped at a float64
    near tie of the divergences."""
    if EARLY["rows"] == 0:
        for case in ("toy", "toy_qwen"):
            gd, images, sizes, kw = _load(golden_dir, case)
            model = _model(CASES[case]["geo"], kw)
            p, im, sz = _three(gd, images, sizes)
            _replay(model, p, im, sz, [0, 1], _generate(model, p, im, sz, dola_layers=[0, 1]))
    print(f"dola replays: {EARLY['rows']} rows, {EARLY['ended']} ended early")
    assert EARLY["rows"] > 0 and EARLY["ended"] * 10 <= EARLY["rows"], EARLY

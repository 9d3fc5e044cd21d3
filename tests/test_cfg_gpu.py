"""GPU tests of classifier-free guidance in generate() and generate_batch() on the toy goldens.  The reference leg runs none of the
guided loop: both branches are replayed on a plain engine (new_kv_cache of the same L_max, prefill into slots, decode_step teacher-forced
with the guided run's tokens), and the guided run's logits, scores and tokens must equal -- without a tolerance -- the chain
log-softmax kernel -> cfg_ref.combine (HF's processor, tests/test_cfg_host.py) -> the CPU processors of logits_ref.py -> argmax."""
import numpy as np
import pytest
import torch

from cfg_ref import bits, combine
from logits_ref import argmax, process_row, same_values
from test_generate_batch_gpu import _compare
from test_generate_gpu import CASES, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu
T_NEW = 10
PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4)


def _text(p):
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    return p[p != IMAGE_TOKEN_INDEX]


def _variant(g, images, sizes, name):
    """(ids, mask, images, sizes) of the prompts and of the negative prompts (None: the default rule) of a replay case."""
    p0, p1 = _prompt(g, 0), _prompt(g, 1)[:-2]
    if name == "vcd_b1":                       # the same prompt without its image
        return ([p0], images[:1], sizes[:1]), ([_text(p0)], [], None)
    if name == "image_b1":                     # a negative prompt that carries another image
        return ([p0], images[:1], sizes[:1]), ([p1], [images[1]], [sizes[1]])
    if name == "text_b2":                      # a different short text prompt per row, different lengths
        return ([p0, p1], images[:2], sizes[:2]), ([_text(p1)[:5], _text(p0)[2:11]], [], None)
    if name == "default_b2":                   # each row's last prompt token
        return ([p0, p1], images[:2], sizes[:2]), None
    if name == "vcd_b2":
        return ([p0, p1], images[:2], sizes[:2]), ([_text(p0), _text(p1)], [], None)
    raise KeyError(name)


def _kwargs(cond, neg):
    ids, am = _pad_batch(cond[0], "right")
    kw = dict(images=cond[1], image_sizes=cond[2], attention_mask=am)
    if neg is not None:
        nids, nam = _pad_batch(neg[0], "right")
        kw.update(negative_prompt_ids=nids, negative_prompt_attention_mask=nam)
        if neg[1]:
            kw.update(negative_images=neg[1], negative_image_sizes=neg[2])
    return ids, kw


def _neg_rows(cond, neg):
    """The negative prompts as the replay feeds them: the default is each row's last prompt token."""
    if neg is None:
        return [p[-1:] for p in cond[0]], [], None
    return neg


def _replay(eng, prompts, images, sizes, L_max, tokens, kv_dtype=None):
    """Prefill the prompts into a fresh cache of L_max positions and feed `tokens` [B, T]: the raw logits of every step, [T][B, vocab]."""
    ids, am = _pad_batch(prompts, "right")
    B = len(prompts)
    cache = eng.new_kv_cache(B, L_max) if kv_dtype is None else eng.new_kv_cache(B, L_max, kv_dtype)
    _, lg = eng.prefill(ids.numpy(), am.numpy(), images or None, sizes, cache=cache, slots=list(range(B)))
    out = [lg.clone()]
    for t in range(tokens.shape[1] - 1):
        out.append(eng.decode_step(cache, tokens[:, t].cpu()).clone())
    return out


def _L_max(eng, cond, negr, T):
    n = 0
    for prompts, images, sizes in (cond, negr):
        ids, am = _pad_batch(prompts, "right")
        n = max(n, int(eng.plan(ids.numpy(), am.numpy(), None, list(images), sizes)["lens"].max()))
    return n + T


def _guided_rows(eng, c, u, g):
    """log-softmax kernel on copies, then HF's combine on the host: fp32 numpy [B, vocab]."""
    from radvlm_amd import ops
    V = eng.vocab
    lc, lu = ops.log_softmax_rows(c.clone(), V), ops.log_softmax_rows(u.clone(), V)
    return combine(lc.cpu().numpy(), lu.cpu().numpy(), g)


def _check_replay(model, cond, neg, g, settings=None, kv_dtype=None, T=T_NEW):
    eng = model.engine
    ids, kw = _kwargs(cond, neg)
    settings = dict(settings or {})
    eos = settings.get("eos_token_id")
    out = model.generate(ids, guidance_scale=g, max_new_tokens=T, output_scores=True, output_logits=True, return_dict_in_generate=True,
                         **({} if kv_dtype is None else dict(kv_cache_dtype=kv_dtype)), **dict({"eos_token_id": None}, **settings), **kw)
    seq = out.sequences
    B = len(cond[0])
    assert tuple(seq.shape) == (B, len(out.scores)) and len(out.logits) == len(out.scores) and out.past_key_values is None
    if eos is None:
        assert seq.shape[1] == T
    negr = _neg_rows(cond, neg)
    L_max = _L_max(eng, cond, negr, T)
    rc = _replay(eng, cond[0], cond[1], cond[2], L_max, seq, kv_dtype)
    ru = _replay(eng, negr[0], negr[1], negr[2], L_max, seq, kv_dtype)
    pk = dict(penalty=settings.get("repetition_penalty"), ngram=settings.get("no_repeat_ngram_size", 0),
              eos=[] if eos is None else [eos], min_new=settings.get("min_new_tokens", 0) if eos is not None else 0)
    finished = [False] * B
    toks = seq.cpu().numpy()
    for t in range(seq.shape[1]):
        assert torch.equal(out.logits[t], rc[t]), t                     # raw conditional logits, cloned before the guide ran
        guided = _guided_rows(eng, rc[t], ru[t], g)
        got = out.scores[t].cpu().numpy()
        for b in range(B):
            want = process_row(guided[b], toks[b, :t], **pk)
            assert same_values(got[b], want), (t, b)
            if pk == dict(penalty=None, ngram=0, eos=[], min_new=0):
                assert np.array_equal(bits(got[b]), bits(want))
            if finished[b]:
                continue
            assert int(toks[b, t]) == argmax(want) == int(torch.argmax(out.scores[t][b])), (t, b)
            finished[b] = eos is not None and int(toks[b, t]) == eos
    return out


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
@pytest.mark.parametrize("name,g", [("vcd_b1", 1.5), ("image_b1", 2.0), ("text_b2", 7.5), ("default_b2", 0.5), ("vcd_b2", -1.0)])
def test_guided_generate_equals_the_replayed_chain(golden_dir, case, name, g):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    cond, neg = _variant(gd, images, sizes, name)
    _check_replay(model, cond, neg, g)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_guided_generate_with_processors_equals_the_replayed_chain(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    cond, neg = _variant(gd, images, sizes, "vcd_b2")
    free = _check_replay(model, cond, neg, 2.0, dict(PROCESSORS, eos_token_id=None))
    eos = int(free.sequences[0, 5])                                     # an EOS id the free run emits: banned for 4 steps, then live
    _check_replay(model, cond, neg, 2.0, dict(PROCESSORS, eos_token_id=eos))


def test_off_means_off(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    ids, am = _pad_batch([_prompt(gd, 0), _prompt(gd, 1)[:-2]], "right")
    call = lambda **extra: model.generate(ids, images=images[:2], image_sizes=sizes[:2], attention_mask=am, max_new_tokens=6, eos_token_id=None,
                                          output_scores=True, output_logits=True, return_dict_in_generate=True, repetition_penalty=1.2, **extra)
    base = call()
    for off in (None, 1, 1.0):
        out = call(guidance_scale=off)
        assert torch.equal(out.sequences, base.sequences)
        assert all(torch.equal(a, b) for a, b in zip(out.logits, base.logits)) and len(out.logits) == len(base.logits)
        assert all(torch.equal(a, b) for a, b in zip(out.scores, base.scores)) and len(out.scores) == len(base.scores)
    assert not torch.equal(call(guidance_scale=1.5).scores[0], base.scores[0])     # on: log-probabilities, not raw scores
    reqs = [_prompt(gd, 0), _prompt(gd, 1)[:-2]]
    b0 = model.generate_batch(reqs, images=images[:2], image_sizes=sizes[:2], max_new_tokens=5, eos_token_id=None, return_logprobs=True)
    for off in (None, 1.0):
        b1 = model.generate_batch(reqs, images=images[:2], image_sizes=sizes[:2], max_new_tokens=5, eos_token_id=None, return_logprobs=True,
                                  guidance_scale=off)
        assert {k: (v.generated_tokens, v.logprobs) for k, v in b0.items()} == {k: (v.generated_tokens, v.logprobs) for k, v in b1.items()}


def test_refusals_through_the_model(golden_dir):
    from radvlm_amd.generation import GenerationCache
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p = _prompt(gd, 0)
    ids = torch.from_numpy(p[None])
    call = lambda **extra: model.generate(ids, images=images[:1], image_sizes=sizes[:1], max_new_tokens=3, **extra)
    with pytest.raises(ValueError):                                     # a wrongly built negative prompt is rejected, not ignored
        call(guidance_scale=1.5, negative_prompt_ids=ids)               # placeholders without negative_images
    with pytest.raises(ValueError):
        call(guidance_scale=1.5, negative_prompt_ids=torch.from_numpy(_text(p)[None]), negative_images=images[:1])
    with pytest.raises(ValueError):
        call(negative_prompt_ids=torch.from_numpy(_text(p)[None]))      # a negative prompt without guidance
    with pytest.raises(ValueError):
        call(guidance_scale=1.5, negative_prompt_ids=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        call(guidance_scale=float("nan"))
    with pytest.raises(ValueError):
        call(guidance_scale=True)
    with pytest.raises(NotImplementedError, match="guidance"):
        call(guidance_scale=1.5, past_key_values=GenerationCache())
    with pytest.raises(NotImplementedError, match="guidance"):
        call(guidance_scale=1.5, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="guidance"):
        model.generate_beams(ids, images=images[:1], image_sizes=sizes[:1], num_beams=2, max_new_tokens=3, guidance_scale=1.5)
    with pytest.raises(NotImplementedError, match="guidance"):
        model.generate_beams(ids, images=images[:1], image_sizes=sizes[:1], num_beams=2, max_new_tokens=3, negative_prompt_ids=ids)
    with pytest.raises(ValueError):
        model.generate_batch([p], images=[images[0]], guidance_scale=1.5, negative_prompt_ids=[p])
    with pytest.raises(TypeError):
        model.generate_batch([p], images=[images[0]], guidance_scale=1.5, negative_prompt_attention_mask=[[1]])
    with pytest.raises(ValueError):
        model.generate_batch([p], images=[images[0]], negative_prompt_ids=[_text(p)])


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_neutral_contrast_gives_the_log_softmax(golden_dir, case):
    """A negative prompt equal to the prompt, with the same image: both branches hold the same bits, so every g gives log_softmax(raw)."""
    from radvlm_amd import ops
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    ids = torch.from_numpy(_prompt(gd, 0)[None])
    first = None
    for g in (0, 0.5, 2.0, 7.5, -1.0):
        out = model.generate(ids, images=images[:1], image_sizes=sizes[:1], max_new_tokens=5, eos_token_id=None, guidance_scale=g,
                             negative_prompt_ids=ids, negative_images=images[:1], negative_image_sizes=sizes[:1], output_scores=True,
                             output_logits=True, return_dict_in_generate=True)
        for t in range(5):
            assert torch.equal(out.scores[t], ops.log_softmax_rows(out.logits[t].clone(), model.engine.vocab)), (g, t)
        first = out if first is None else first
        assert torch.equal(out.sequences, first.sequences)


def test_quantized_weights_and_int8_cache_compose(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    cond, neg = _variant(gd, images, sizes, "vcd_b2")
    ids, gkw = _kwargs(cond, neg)
    call = lambda **extra: model.generate(ids, guidance_scale=2.0, max_new_tokens=8, eos_token_id=None, output_scores=True,
                                          return_dict_in_generate=True, **gkw, **extra)
    eng = model.engine
    runs = []
    for flag in (True, False):                                          # the two int8-cache routes are bit-identical
        eng.kv8_decode = flag
        try:
            runs.append(call(kv_cache_dtype="int8"))
        finally:
            eng.kv8_decode = True
    assert torch.equal(runs[0].sequences, runs[1].sequences) and all(torch.equal(a, b) for a, b in zip(runs[0].scores, runs[1].scores))
    _check_replay(model, cond, neg, 2.0, kv_dtype="int8", T=8)
    model.quantize_decoder_()
    runs = []
    for flag in (True, False):                                          # and so are the two int8-weight routes
        eng.w8_decode = flag
        try:
            runs.append(call())
        finally:
            eng.w8_decode = True
    assert torch.equal(runs[0].sequences, runs[1].sequences) and all(torch.equal(a, b) for a, b in zip(runs[0].scores, runs[1].scores))
    _check_replay(model, cond, neg, 2.0, T=8)


def test_seeded_sampling_on_the_guided_rows(golden_dir):
    from radvlm_amd import ops
    gd, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    eng = model.engine
    cond, neg = _variant(gd, images, sizes, "vcd_b2")
    ids, gkw = _kwargs(cond, neg)
    T, g, seeds = 8, 1.5, [11, 29]
    sk = dict(temperature=0.9, top_k=40, top_p=0.95)
    call = lambda **extra: model.generate(ids, guidance_scale=g, max_new_tokens=T, eos_token_id=None, **gkw, **extra)
    a, b, greedy = call(do_sample=True, seed=seeds, **sk), call(do_sample=True, seed=seeds, **sk), call()
    assert torch.equal(a, b) and not torch.equal(a, greedy)
    negr = _neg_rows(cond, neg)
    L_max = _L_max(eng, cond, negr, T)
    rc, ru = _replay(eng, cond[0], cond[1], cond[2], L_max, a), _replay(eng, negr[0], negr[1], negr[2], L_max, a)
    sd = torch.tensor(seeds, dtype=torch.int64, device="cuda")
    for t in range(T):
        rows = torch.from_numpy(_guided_rows(eng, rc[t], ru[t], g)).cuda()
        tok = ops.sample_rows(rows, eng.vocab, sd, torch.full((2,), t, dtype=torch.int32, device="cuda"), sk["temperature"], sk["top_k"],
                              sk["top_p"], 0.0)
        assert torch.equal(tok, a[:, t]), t


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_batch_equals_guided_generate_alone(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p0, p1 = _prompt(gd, 0), _prompt(gd, 1)
    # (prompt, image, size, negative prompt or None, negative image, negative size)
    reqs = [(p0, images[0], sizes[0], _text(p0), None, None),
            (p1[:-2], images[1], sizes[1], None, None, None),                      # the default: its last prompt token
            (_text(p0), None, None, p1, images[1], sizes[1]),                      # a text request against an image prompt
            (p0[:-3], images[0], sizes[0], _text(p1)[:4], None, None)]
    budgets = [3, 9, 6, 7]                                              # request 0 finishes first: request 3 reuses its pair of rows
    g, settings = 1.5, dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=None)
    out = model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=3,
                               max_new_tokens=budgets, return_logprobs=True, guidance_scale=g, negative_prompt_ids=[r[3] for r in reqs],
                               negative_images=[r[4] for r in reqs], negative_image_sizes=[r[5] for r in reqs], **settings)
    for i, r in enumerate(reqs):
        o = out[f"req_{i}"]
        assert len(o.generated_tokens) == len(o.logprobs) == budgets[i]
        neg = {} if r[3] is None else dict(negative_prompt_ids=torch.from_numpy(r[3][None]))
        if r[4] is not None:
            neg.update(negative_images=[r[4]], negative_image_sizes=[r[5]])
        one = model.generate(torch.from_numpy(r[0][None]), images=None if r[1] is None else [r[1]], image_sizes=None if r[2] is None else [r[2]],
                             max_new_tokens=budgets[i], output_scores=True, return_dict_in_generate=True, guidance_scale=g, **neg, **settings)
        _compare(o.generated_tokens, one, logprobs=o.logprobs)

"""GPU tests of constrained decoding (constraint=) in generate() and generate_batch() on the toy goldens (vocab 1000).  Every
comparison is exact: the replay rebuilds each step's score row from the run's own raw row and the automaton's allowed set (walk), bit
for bit, and a request of generate_batch equals generate() on it alone token for token."""
import numpy as np
import pytest
import torch

from radvlm_amd.constraints import FREE, TokenConstraint
from test_generate_gpu import CASES, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu
T_NEW = 6
NEG_INF = float("-inf")


def _bits(x):
    return x.contiguous().view(torch.int32)


def _generate(model, prompts, images, sizes, T=T_NEW, side="left", **kw):
    ids, am = _pad_batch(prompts, side)
    return model.generate(ids, images=images, image_sizes=sizes, attention_mask=am, max_new_tokens=T, output_scores=True, output_logits=True,
                          return_dict_in_generate=True, **kw)


def _replay(out, cons, greedy=True):
    """scores[t] == where(allowed_t, logits[t], -inf) bit for bit with allowed_t from walk, the token is its argmax, and rows after
    the EOS edge (free) and unconstrained rows are untouched.  Returns the steps at which a mask applied."""
    seq = out.sequences.cpu().numpy()
    masked = 0
    for b, c in enumerate(cons):
        states, allowed = (np.full(seq.shape[1], FREE), [None] * seq.shape[1]) if c is None else c.walk(seq[b])
        for t in range(len(out.scores)):
            raw, got = out.logits[t][b], out.scores[t][b]
            if states[t] == FREE:
                if greedy:                                       # no processor or warper ran: the raw row's bits
                    assert torch.equal(_bits(raw), _bits(got)), (b, t)
                continue
            keep = torch.zeros(raw.numel(), dtype=torch.bool, device=raw.device)
            keep[torch.from_numpy(allowed[t].astype(np.int64)).to(raw.device)] = True
            assert keep.any(), (b, t)                            # never a dead state
            masked += 1
            if greedy:
                want = torch.where(keep, raw, torch.full_like(raw, NEG_INF))
                assert torch.equal(_bits(want), _bits(got)), (b, t)
                assert int(seq[b, t]) == int(torch.argmax(got)), (b, t)
            else:
                assert bool(torch.isneginf(got[~keep]).all()), (b, t)
            assert bool(keep[int(seq[b, t])]), (b, t)
    return masked


def _lowest(out, k):
    """The k ids the step-0 raw logits of row 0 rank lowest."""
    return torch.argsort(out.logits[0][0])[:k].cpu().tolist()


def _two(gd, images, sizes):
    return [_prompt(gd, 0), _prompt(gd, 1)[:-2]], images[:2], sizes[:2]


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_choices_change_the_answer(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _two(gd, images, sizes)
    low = _lowest(_generate(model, p, im, sz), 6)
    eos = low[5]
    free = _generate(model, p, im, sz, eos_token_id=eos)
    choices = [[low[0]], [low[1], low[2]], [low[1], low[3], low[4]]]          # lengths 1, 2, 3; two share their first token
    c = TokenConstraint.from_choices(choices, eos=[eos])
    assert int(free.sequences[0, 0]) not in c.allowed(c.start).tolist()       # so the mask must change step 0
    out = _generate(model, p, im, sz, eos_token_id=eos, constraint=[c, None])
    row = out.sequences[0].cpu().tolist()
    hit = [ch for ch in choices if row[:len(ch) + 1] == ch + [eos]]
    assert len(hit) == 1 and all(v == eos for v in row[len(hit[0]) + 1:])     # a choice, EOS, then pads (the pad is the EOS id)
    assert torch.equal(out.sequences[1], free.sequences[1])                   # the unconstrained row is the unconstrained call's
    assert torch.equal(_bits(out.logits[0]), _bits(free.logits[0]))           # output_logits: the raw rows of the same prompt pass
    assert _replay(out, [c, None]) == len(hit[0]) + 1
    assert len(out.scores) == T_NEW                                           # row 1 ran on: row 0's rows after its EOS were replayed too
    both = _generate(model, p, im, sz, eos_token_id=eos, constraint=c)        # one constraint for every row
    steps = both.sequences.shape[1]                                           # both rows finish, so the call ends with the longer choice
    assert both.sequences[0].cpu().tolist() == row[:steps] and len(hit[0]) + 1 <= steps <= 4
    assert _replay(both, [c, c]) > len(hit[0]) + 1


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_an_automaton_that_allows_everything_changes_no_bit(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _two(gd, images, sizes)
    V = model.engine.vocab
    base = _generate(model, p, im, sz)
    eos = int(base.sequences[0, 3])                                           # row 0 finishes at step 3 at the latest
    edges = {i: 0 for i in range(V)}
    edges[eos] = FREE
    c = TokenConstraint._from_edges([edges])
    for settings in (dict(), dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2)):
        a = _generate(model, p, im, sz, eos_token_id=eos, **settings)
        b = _generate(model, p, im, sz, eos_token_id=eos, constraint=c, **settings)
        assert torch.equal(a.sequences, b.sequences) and len(a.scores) == len(b.scores)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a.scores + a.logits, b.scores + b.logits))
    off = _generate(model, p, im, sz, eos_token_id=eos, constraint=None)
    none = _generate(model, p, im, sz, eos_token_id=eos, constraint=[None, None])
    plain = _generate(model, p, im, sz, eos_token_id=eos)
    for o in (off, none):
        assert torch.equal(o.sequences, plain.sequences)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(o.scores + o.logits, plain.scores + plain.logits))


def _random_choices(V, seed, k=8, length=4, avoid=()):
    ids = [int(v) for v in np.random.default_rng(seed).permutation(np.arange(1, V)) if int(v) not in avoid]
    return [ids[i * length:(i + 1) * length] for i in range(k)], ids[k * length]


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_processors_and_seeded_sampling_stay_inside_the_automaton(golden_dir, case):
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p, im, sz = _two(gd, images, sizes)
    choices, eos = _random_choices(model.engine.vocab, 5)
    c = TokenConstraint.from_choices(choices + [choices[0][:2]], eos=[eos])
    settings = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, do_sample=True, seed=[7, 19], temperature=1.5, eos_token_id=eos,
                    constraint=c)
    a = _generate(model, p, im, sz, **settings)
    b = _generate(model, p, im, sz, **settings)
    assert torch.equal(a.sequences, b.sequences)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a.scores + a.logits, b.scores + b.logits))
    assert _replay(a, [c, c], greedy=False) >= 6
    for row in a.sequences.cpu().tolist():
        assert any(row[:len(ch) + 1] == ch + [eos] for ch in choices + [choices[0][:2]]), row
    greedy = _generate(model, p, im, sz, repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=eos, constraint=c)
    assert _replay(greedy, [c, c], greedy=False) >= 6                          # processed rows: -inf outside the allowed set, tokens inside


def test_int8_cache_and_quantized_decoder_compose(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p, im, sz = _two(gd, images, sizes)
    choices, eos = _random_choices(model.engine.vocab, 9)
    c = TokenConstraint.from_choices(choices, eos=[eos])
    assert _replay(_generate(model, p, im, sz, eos_token_id=eos, constraint=c, kv_cache_dtype="int8"), [c, c]) == 10
    model.quantize_decoder_()
    assert _replay(_generate(model, p, im, sz, eos_token_id=eos, constraint=[None, c]), [None, c]) == 5


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_second_turn_of_a_conversation_restarts_at_start(golden_dir, case):
    from radvlm_amd.generation import GenerationCache
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p1 = _prompt(gd, 0)
    choices, eos = _random_choices(model.engine.vocab, 11, k=4, length=2)
    c = TokenConstraint.from_choices(choices, eos=[eos])
    cache = GenerationCache()
    gen = lambda p: model.generate(torch.from_numpy(p[None]), images=images[:1], image_sizes=sizes[:1], max_new_tokens=4, output_scores=True,
                                   output_logits=True, return_dict_in_generate=True, eos_token_id=eos, constraint=c, past_key_values=cache)
    t1 = gen(p1)
    assert _replay(t1, [c]) == 3
    follow = np.random.default_rng(11).integers(3, model.engine.vocab, 9).astype(np.int64)
    t2 = gen(np.concatenate([p1, t1.sequences[0].cpu().numpy()[:3], follow]))
    assert cache.get_seq_length() > len(p1)                                    # the second turn extended the first turn's cache
    assert _replay(t2, [c]) == 3                                               # from the start state again: a choice, then EOS
    assert t2.sequences[0, :3].cpu().tolist() in [ch + [eos] for ch in choices]


def _requests(gd, images, sizes):
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    p0, p1, p2 = _prompt(gd, 0), _prompt(gd, 1), _prompt(gd, 2)
    return [(p0, images[0], sizes[0]), (p1[:-2], images[1], sizes[1]), (p0[p0 != IMAGE_TOKEN_INDEX], None, None), (p2[:-1], None, None),
            (p1[:-3], images[1], sizes[1])]


def _alone(model, r, budget, c, **kw):
    return model.generate(torch.from_numpy(r[0][None]), images=None if r[1] is None else [r[1]], image_sizes=None if r[2] is None else [r[2]],
                          max_new_tokens=budget, output_scores=True, output_logits=True, return_dict_in_generate=True, constraint=c, **kw)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
@pytest.mark.parametrize("sampled", [False, True])
def test_generate_batch_equals_generate_alone(golden_dir, case, sampled):
    """Five requests on two slots (slots are reused), three different automata and two unconstrained requests, mixed budgets.  A
    request's tokens are those of generate() on it alone with its constraint; its logprobs are those of generate_batch on it alone
    (generate() returns scores, not logprobs), and exactly 0.0 where its state allows a single id: the logprob is the processed row's,
    so it is renormalised over the allowed set."""
    gd, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    V = model.engine.vocab
    reqs = _requests(gd, images, sizes)
    ch_a, eos = _random_choices(V, 21, k=6, length=2)
    ch_b, _ = _random_choices(V, 22, k=5, length=4, avoid=(eos,))
    every = {i: 0 for i in range(V)}
    every[eos] = FREE
    cons = [TokenConstraint.from_choices(ch_a, eos=[eos]), None, TokenConstraint.from_choices(ch_b + [ch_b[0][:1]], eos=[eos]), None,
            TokenConstraint._from_edges([every])]
    budgets = [3, 8, 6, 7, 5]
    settings = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=eos)
    if sampled:
        settings.update(do_sample=True, temperature=1.3, top_k=20)
    seeds = [3, 14, 15, 92, 65]
    batch = lambda **extra: model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs],
                                                 max_batch_size=2, max_new_tokens=budgets, return_logprobs=True, constraint=cons,
                                                 **dict(settings, **({"seed": seeds} if sampled else {})), **extra)
    out = batch()
    shared = batch(share_prefix=True)
    for i, r in enumerate(reqs):
        o = out[f"req_{i}"]
        sd = dict(seed=[seeds[i]]) if sampled else {}
        one = _alone(model, r, budgets[i], cons[i], **settings, **sd)
        seq = one.sequences[0].cpu().tolist()
        n = len(o.generated_tokens)
        assert o.generated_tokens == seq[:n] and (n == len(seq) or seq[n - 1] == eos), (i, o.generated_tokens, seq)
        assert shared[f"req_{i}"].generated_tokens == o.generated_tokens
        _replay(one, [cons[i]], greedy=False)
        solo = model.generate_batch([r[0]], images=[r[1]], image_sizes=[r[2]], max_batch_size=1, max_new_tokens=budgets[i],
                                    return_logprobs=True, constraint=[cons[i]], **settings, **sd)["req_0"]
        assert solo.generated_tokens == o.generated_tokens and solo.logprobs == o.logprobs, (i, solo.logprobs, o.logprobs)
        if cons[i] is not None:                                  # renormalised over the allowed set: a state that allows one id gives log 1
            _, allowed = cons[i].walk(o.generated_tokens)
            single = [t for t in range(n) if allowed[t] is not None and allowed[t].size == 1]
            assert all(o.logprobs[t] == 0.0 for t in single), (i, o.logprobs)
            assert single or i == 4
    assert cons[0].accepts(out["req_0"].generated_tokens)          # a choice of length 2 and its EOS fit the budget of 3


def test_dead_end_raises_and_names_the_row_and_the_step(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p, im, sz = _two(gd, images, sizes)
    c = TokenConstraint.from_choices([[11, 12]], eos=[13])
    with pytest.raises(RuntimeError, match=r"row 1 reached a dead end at step 1"):
        _generate(model, p, im, sz, eos_token_id=13, constraint=[None, c], bad_words_ids=[[12]])
    with pytest.raises(RuntimeError, match=r"row 0 reached a dead end at step 2"):
        _generate(model, p, im, sz, eos_token_id=13, constraint=c, min_new_tokens=4)           # only EOS is allowed, and it is banned
    with pytest.raises(RuntimeError, match=r"row 0 reached a dead end at step 1"):
        _generate(model, p, im, sz, eos_token_id=13, constraint=c, bad_words_ids=[[12]], do_sample=True, seed=1)
    z = TokenConstraint.from_choices([[11, 0]], eos=[13])                      # token 0 is what the argmax of an all -inf row gives
    with pytest.raises(RuntimeError, match=r"row 0 reached a dead end at step 1"):
        _generate(model, p, im, sz, eos_token_id=13, constraint=z, bad_words_ids=[[0]])
    reqs = [p[0], p[1], p[0]]
    call = lambda **kw_: model.generate_batch(reqs, images=[im[0], im[1], im[0]], image_sizes=[sz[0], sz[1], sz[0]], max_batch_size=2,
                                               max_new_tokens=5, eos_token_id=13, **kw_)
    with pytest.raises(RuntimeError, match=r"request 2 reached a dead end at step 1"):
        call(constraint=[None, None, c], bad_words_ids=[[12]])
    with pytest.raises(RuntimeError, match=r"request 1 reached a dead end at step 2"):
        call(constraint=[None, c, None], min_new_tokens=4, do_sample=True, seed=5)
    good = call(constraint=[c, None, c])                                       # and a good call follows
    assert good["req_0"].generated_tokens == [11, 12, 13] == good["req_2"].generated_tokens


def test_other_errors_through_the_model(golden_dir):
    gd, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p = _prompt(gd, 0)
    ids = torch.from_numpy(p[None])
    c = TokenConstraint.from_choices([[11, 12]], eos=[13])
    call = lambda **extra: model.generate(ids, images=images[:1], image_sizes=sizes[:1], max_new_tokens=3, **extra)
    with pytest.raises(NotImplementedError, match="constraint with prompt_lookup_num_tokens"):
        call(constraint=c, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="constraint with guidance_scale"):
        call(constraint=c, guidance_scale=1.5)
    with pytest.raises(NotImplementedError, match="constraint with dola_layers"):
        call(constraint=c, dola_layers="high")
    beyond = TokenConstraint.from_choices([[11, model.engine.vocab]], eos=[13])
    with pytest.raises(ValueError, match="vocabulary"):
        call(constraint=beyond)
    with pytest.raises(ValueError, match="vocabulary"):
        model.generate_batch([p], images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=3, constraint=[beyond])
    with pytest.raises(ValueError, match="2 entries for 1"):
        call(constraint=[c, None])
    with pytest.raises(ValueError, match="constraint"):
        call(constraint="yes")
    with pytest.raises(TypeError, match="constraint"):
        model.generate_beams(ids, images=images[:1], image_sizes=sizes[:1], num_beams=2, max_new_tokens=3, constraint=c)
    assert call(constraint=c, eos_token_id=13).cpu().tolist() == [[11, 12, 13]]

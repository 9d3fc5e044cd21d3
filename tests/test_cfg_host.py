"""CPU tests of classifier-free guidance's host side: the numpy restatement against the installed HF processor bit for bit, HF's
default negative prompt, every argument rule of generate(guidance_scale=) / generate_batch() / generate_beams(), and the continuous
batching scheduler with paired rows on the fake engine of tests/test_generate_batch_host.py."""
import numpy as np
import pytest
import torch

import cfg_ref
from cfg_ref import G_LIST, bits, combine, hf_guided, torch_log_softmax32
from logits_ref import argmax, process_row
from radvlm_amd.generation import (BatchScheduler, batch_requests, parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs,
                                   resolve_negative_prompts)
from radvlm_amd.splice import IMAGE_TOKEN_INDEX
from test_generate_batch_host import IMG_ROWS, V, FakeEngine, HostPicker, _prompts

NAMES = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "negative_image_sizes")


# ------------------------------------------------------------------------------------------------ the rule, against HF's own code
@pytest.mark.parametrize("n", [1, 2, 1000, 32000])
@pytest.mark.parametrize("kind", ["flat", "peaked"])
def test_combine_is_hf_processor_bit_for_bit(n, kind):
    rng = np.random.default_rng(n)
    c, u = cfg_ref.logits_rows(rng, 3, n, kind), cfg_ref.logits_rows(rng, 3, n, kind)
    lc, lu = torch_log_softmax32(c), torch_log_softmax32(u)
    for g in G_LIST:
        want = hf_guided(c, u, g, torch.float32).numpy()
        assert np.array_equal(bits(combine(lc, lu, g)), bits(want)), g


def test_contraction_would_be_visible():
    """g = 1/3 on random rows: a fused multiply-add (one rounding of g * d + lu) differs from HF's two roundings somewhere."""
    rng = np.random.default_rng(7)
    lc, lu = torch_log_softmax32(cfg_ref.logits_rows(rng, 1, 32000, "flat")), torch_log_softmax32(cfg_ref.logits_rows(rng, 1, 32000, "flat"))
    d = lc - lu
    fma = (np.float64(np.float32(1 / 3)) * d.astype(np.float64) + lu.astype(np.float64)).astype(np.float32)   # exact product: one rounding
    assert not np.array_equal(bits(fma), bits(combine(lc, lu, 1 / 3)))


def test_hf_scale_one_is_plain_log_softmax_and_never_calls_the_model():
    rng = np.random.default_rng(1)
    c, u = cfg_ref.logits_rows(rng, 2, 1000, "flat"), cfg_ref.logits_rows(rng, 2, 1000, "flat")
    stub = cfg_ref.StubModel(None)
    out = hf_guided(c, u, 1, torch.float32, stub=stub)
    assert stub.calls == [] and np.array_equal(bits(out.numpy()), bits(torch_log_softmax32(c)))
    out = hf_guided(c, u, 1.0, torch.float32, stub=stub)
    assert stub.calls == []


def test_default_negative_prompt_is_hfs_last_prompt_token():
    rng = np.random.default_rng(2)
    ids = rng.integers(1, V, (3, 7))
    c, u = cfg_ref.logits_rows(rng, 3, V, "flat"), cfg_ref.logits_rows(rng, 3, V, "flat")
    stub = cfg_ref.StubModel(None)
    hf_guided(c, u, 2.0, input_ids=torch.from_numpy(ids), stub=stub)
    first = stub.calls[0]
    assert first["input_ids"].tolist() == ids[:, -1:].tolist() and first["attention_mask"].tolist() == [[1]] * 3
    cfg = parse_generate_kwargs(dict(guidance_scale=2.0))
    nid, nam, imgs, sizes = resolve_negative_prompts(cfg.guidance, ids, None)
    assert nid.tolist() == first["input_ids"].tolist() and nam.all() and imgs == [] and sizes is None
    reqs = batch_requests([row for row in ids], guidance=parse_batch_kwargs(dict(guidance_scale=2.0), 3).guidance)
    assert [r.neg_ids.tolist() for r in reqs] == first["input_ids"].tolist()
    # right padding: the last REAL token of each row
    am = np.ones((3, 7), dtype=bool)
    am[1, 4:] = False
    nid, nam, _, _ = resolve_negative_prompts(cfg.guidance, ids, am)
    assert nid[:, 0].tolist() == [int(ids[0, 6]), int(ids[1, 3]), int(ids[2, 6])]
    # an explicit negative prompt reaches the model as given
    neg = torch.tensor([[4, 5], [6, 7], [8, 9]])
    stub = cfg_ref.StubModel(None)
    hf_guided(c, u, 2.0, input_ids=torch.from_numpy(ids), negative_prompt_ids=neg, stub=stub)
    cfg = parse_generate_kwargs(dict(guidance_scale=2.0, negative_prompt_ids=neg))
    assert resolve_negative_prompts(cfg.guidance, ids, None)[0].tolist() == stub.calls[0]["input_ids"].tolist()


# ------------------------------------------------------------------------------------------------ arguments
def test_off_values_leave_the_config_as_it_was():
    base = dict(max_new_tokens=5, repetition_penalty=1.2, eos_token_id=3)
    plain = parse_generate_kwargs(dict(base))
    assert plain.guidance is None
    for off in (None, 1, 1.0, np.float32(1)):
        assert parse_generate_kwargs(dict(base, guidance_scale=off)) == plain
        assert parse_batch_kwargs(dict(base, guidance_scale=off), 2) == parse_batch_kwargs(dict(base), 2)
    for on in (0, 0.0, 0.5, 1.5, -1, 7.5, np.float32(2)):
        c = parse_generate_kwargs(dict(base, guidance_scale=on))
        assert c.guidance is not None and c.guidance.scale == float(on)
        c.guidance = None
        assert c == plain


def test_bad_scale_and_negative_arguments_without_guidance():
    for bad in (True, False, "2", float("nan"), float("inf"), -float("inf"), 1e39, [2.0], 2 + 0j):
        with pytest.raises(ValueError):
            parse_generate_kwargs(dict(guidance_scale=bad))
        with pytest.raises(ValueError):
            parse_batch_kwargs(dict(guidance_scale=bad), 2)
    img = torch.zeros(3, 4, 4)
    for off in ({}, dict(guidance_scale=None), dict(guidance_scale=1), dict(guidance_scale=1.0)):
        for name, v in (("negative_prompt_ids", [[1, 2]]), ("negative_prompt_attention_mask", [[1, 1]]), ("negative_images", [img]),
                        ("negative_image_sizes", [(4, 4)])):
            with pytest.raises(ValueError):
                parse_generate_kwargs(dict(off, **{name: v}))
    for name, v in (("negative_prompt_ids", [[1, 2], [3]]), ("negative_images", [img, None]), ("negative_image_sizes", [(4, 4), None])):
        with pytest.raises(ValueError):
            parse_batch_kwargs({name: v}, 2)


def test_negative_prompt_rules_of_generate():
    ids = np.array([[1, 2, 3], [4, 5, 6]])
    img = torch.zeros(3, 4, 4)
    g = lambda **kw: parse_generate_kwargs(dict(guidance_scale=2.0, **kw)).guidance
    with pytest.raises(ValueError):                                   # a row count other than B
        resolve_negative_prompts(g(negative_prompt_ids=[[1, 2]]), ids, None)
    with pytest.raises(ValueError):
        resolve_negative_prompts(g(negative_prompt_ids=[[1], [2], [3]]), ids, None)
    with pytest.raises(ValueError):                                   # an empty row after masking
        resolve_negative_prompts(g(negative_prompt_ids=[[1, 2], [3, 4]], negative_prompt_attention_mask=[[1, 1], [0, 0]]), ids, None)
    with pytest.raises(ValueError):                                   # no columns at all
        resolve_negative_prompts(g(negative_prompt_ids=np.zeros((2, 0), np.int64)), ids, None)
    with pytest.raises(ValueError):                                   # a mask of another shape
        resolve_negative_prompts(g(negative_prompt_ids=[[1, 2], [3, 4]], negative_prompt_attention_mask=[[1], [1]]), ids, None)
    with pytest.raises(ValueError):                                   # a mask without ids
        resolve_negative_prompts(g(negative_prompt_attention_mask=[[1], [1]]), ids, None)
    with pytest.raises(ValueError):                                   # not ids
        resolve_negative_prompts(g(negative_prompt_ids=[[0.5, 1.0], [1.0, 2.0]]), ids, None)
    with pytest.raises(ValueError):                                   # placeholders without negative_images
        resolve_negative_prompts(g(negative_prompt_ids=[[1, IMAGE_TOKEN_INDEX], [3, 4]]), ids, None)
    with pytest.raises(ValueError):                                   # negative_images without a placeholder
        resolve_negative_prompts(g(negative_prompt_ids=[[1, 2], [3, 4]], negative_images=[img]), ids, None)
    with pytest.raises(ValueError):                                   # ... also under the default negative prompt
        resolve_negative_prompts(g(negative_images=[img]), ids, None)
    with pytest.raises(ValueError):                                   # two placeholders, one image
        resolve_negative_prompts(g(negative_prompt_ids=[[IMAGE_TOKEN_INDEX, 2], [IMAGE_TOKEN_INDEX, 4]], negative_images=[img]), ids, None)
    with pytest.raises(ValueError):                                   # a masked placeholder does not count
        resolve_negative_prompts(g(negative_prompt_ids=[[IMAGE_TOKEN_INDEX, 2], [3, 4]], negative_prompt_attention_mask=[[0, 1], [1, 1]],
                                   negative_images=[img]), ids, None)
    with pytest.raises(ValueError):                                   # the default rule on a row whose last token is a placeholder
        resolve_negative_prompts(g(), np.array([[1, IMAGE_TOKEN_INDEX]]), None)
    nid, nam, imgs, sizes = resolve_negative_prompts(
        g(negative_prompt_ids=torch.tensor([[1, IMAGE_TOKEN_INDEX, 0], [3, 4, 5]]), negative_prompt_attention_mask=torch.tensor([[1, 1, 0], [1, 1, 1]]),
          negative_images=[img], negative_image_sizes=[(4, 4)]), ids, None)
    assert nid.dtype == np.int64 and nam.dtype == bool and nam.tolist() == [[True, True, False], [True, True, True]]
    assert len(imgs) == 1 and sizes == [(4, 4)]


def test_refusals_name_guidance():
    from radvlm_amd.generation import GenerationCache
    with pytest.raises(NotImplementedError, match="guidance"):
        parse_generate_kwargs(dict(guidance_scale=2.0, past_key_values=GenerationCache()))
    with pytest.raises(NotImplementedError, match="guidance"):
        parse_generate_kwargs(dict(guidance_scale=2.0, prompt_lookup_num_tokens=4), lookup=True)
    values = dict(guidance_scale=2.0, negative_prompt_ids=[[1]], negative_prompt_attention_mask=[[1]], negative_images=[torch.zeros(3, 4, 4)],
                  negative_image_sizes=[(4, 4)])
    for name in NAMES:
        with pytest.raises(NotImplementedError, match="guidance"):
            parse_beam_kwargs({name: values[name], "num_beams": 2})
    # off, both still work as they did
    parse_generate_kwargs(dict(guidance_scale=1.0, past_key_values=GenerationCache()))
    parse_generate_kwargs(dict(guidance_scale=None, prompt_lookup_num_tokens=4), lookup=True)
    parse_beam_kwargs(dict(num_beams=2))


def test_batch_argument_rules():
    img = torch.zeros(3, 4, 4)
    with_img = np.array([1, IMAGE_TOKEN_INDEX, 2])
    gd = lambda n, **kw: parse_batch_kwargs(dict(guidance_scale=1.5, **kw), n).guidance
    with pytest.raises(TypeError):
        parse_batch_kwargs(dict(guidance_scale=1.5, negative_prompt_attention_mask=[[1]]), 1)
    with pytest.raises(ValueError):                                   # a list of another length
        parse_batch_kwargs(dict(guidance_scale=1.5, negative_prompt_ids=[[1]]), 2)
    with pytest.raises(ValueError):                                   # not a list
        parse_batch_kwargs(dict(guidance_scale=1.5, negative_prompt_ids=np.array([[1], [2]])), 2)
    with pytest.raises(ValueError):                                   # an empty negative prompt
        batch_requests([[1, 2]], guidance=gd(1, negative_prompt_ids=[[]]))
    with pytest.raises(ValueError):                                   # not 1-D
        batch_requests([[1, 2]], guidance=gd(1, negative_prompt_ids=[[[1, 2]]]))
    with pytest.raises(ValueError):                                   # placeholder, no image
        batch_requests([[1, 2]], guidance=gd(1, negative_prompt_ids=[with_img]))
    with pytest.raises(ValueError):                                   # image, no placeholder
        batch_requests([[1, 2]], guidance=gd(1, negative_prompt_ids=[[3]], negative_images=[img]))
    with pytest.raises(ValueError):                                   # ... under the default rule too
        batch_requests([[1, 2]], guidance=gd(1, negative_images=[img]))
    with pytest.raises(ValueError):                                   # sizes that do not match the images
        batch_requests([[1, 2]], guidance=gd(1, negative_prompt_ids=[with_img], negative_images=[img], negative_image_sizes=[[(4, 4), (4, 4)]]))
    with pytest.raises(ValueError):                                   # sizes for some requests only
        batch_requests([[1, 2], [3]], guidance=gd(2, negative_prompt_ids=[with_img, with_img], negative_images=[img, img],
                                                  negative_image_sizes=[(4, 4), None]))
    r = batch_requests([[1, 2], with_img, [5]], images=[None, img, None],
                       guidance=gd(3, negative_prompt_ids=[None, torch.tensor([7, 8]), with_img], negative_images=[None, None, img],
                                   negative_image_sizes=[None, None, (4, 5)]))
    assert [q.neg_ids.tolist() for q in r] == [[2], [7, 8], with_img.tolist()]
    assert [len(q.neg_images) for q in r] == [0, 0, 1] and r[2].neg_sizes == [(4, 5)] and r[0].neg_sizes is None
    assert not hasattr(batch_requests([[1, 2]])[0], "neg_ids")       # without guidance a request is what it was


# ------------------------------------------------------------------------------------------------ the scheduler on the fake engine
class PairEngine(FakeEngine):
    """The fake engine, recording what the scheduler asks of the cache."""

    def __init__(self, free=None):
        super().__init__(free)
        self.sized, self.made, self.filled = [], [], []

    def kv_cache_bytes(self, B, L):
        self.sized.append((B, L))
        return super().kv_cache_bytes(B, L)

    def new_kv_cache(self, B, L):
        self.made.append((B, L))
        return super().new_kv_cache(B, L)

    def prefill(self, ids, am, images, sizes, max_new_tokens=0, cache=None, slots=None):
        out = super().prefill(ids, am, images, sizes, max_new_tokens, cache, slots)
        self.filled.append({int(s): int(cache.lens[s]) for s in slots})          # the spliced length each row now holds
        return out


def host_guide(g):
    def guide(c, u):
        out = combine(torch_log_softmax32(c), torch_log_softmax32(u), g)
        c.copy_(torch.from_numpy(out))
    return guide


def guided_alone(eng, ids, images, neg, neg_images, budget, g):
    seq, nseq, out = eng._splice(ids, images), eng._splice(neg, neg_images), []
    for _ in range(budget):
        x = combine(torch_log_softmax32(eng.logits_of(seq)), torch_log_softmax32(eng.logits_of(nseq)), g)[0]
        k = argmax(process_row(x, out))
        out.append(k)
        seq, nseq = seq + [k], nseq + [k]
    return out


def _guided_run(n=7, slots=3, g=1.5, free=None, budgets=None, eng=None):
    ps, ims = _prompts(n, 3)
    rng = np.random.default_rng(11)
    negs, nims = [], []
    for i in range(n):
        if i % 4 == 0:
            negs.append(None), nims.append(None)                     # the default: the last prompt token
        elif i % 4 == 1:
            negs.append(ps[i][ps[i] != IMAGE_TOKEN_INDEX]), nims.append(None)      # the prompt without its image
        elif i % 4 == 2:
            q = rng.integers(0, V, 14).astype(np.int64)              # longer than the prompt, with another image
            q[2] = IMAGE_TOKEN_INDEX
            negs.append(q), nims.append(torch.full((3, 4, 4), 9.0 + i))
        else:
            negs.append(rng.integers(0, V, 2).astype(np.int64)), nims.append(None)
    budgets = budgets or [5, 9, 2, 7, 3, 6, 4][:n]
    cfg = parse_batch_kwargs(dict(max_new_tokens=budgets, guidance_scale=g, negative_prompt_ids=negs, negative_images=nims), n)
    eng = eng or PairEngine(free=free)
    sch = BatchScheduler(eng, batch_requests(ps, ims, guidance=cfg.guidance), cfg, slots, admit_free=1, picker=HostPicker(cfg), guide=host_guide(g))
    return sch.run(), sch, eng, ps, ims, negs, nims, budgets


def test_scheduler_pairs_rows_and_equals_the_guided_alone_run():
    out, sch, eng, ps, ims, negs, nims, budgets = _guided_run()
    S = sch.slots
    assert S == 3 and eng.made == [(2 * S, sch.L_max)] and eng.sized == [(2 * S, sch.L_max)]     # both halves are counted
    for i, p in enumerate(ps):
        neg = p[-1:] if negs[i] is None else negs[i]
        want = guided_alone(eng, p, [] if ims[i] is None else [ims[i]], neg, [] if nims[i] is None else [nims[i]], budgets[i], 1.5)
        assert out[f"req_{i}"].generated_tokens == want, i
    # L_max covers the longer prompt of each pair plus the budget
    assert sch.L_max == max(max(sch.spliced[i], sch.neg_spliced[i]) + budgets[i] for i in range(len(ps)))
    assert sch.neg_spliced[2] == 14 + IMG_ROWS - 1 and sch.neg_spliced[2] > sch.spliced[2]
    # an admitted group is two prefills: the prompts into their slots, then the negative prompts into rows slots + s
    admits = [ev for ev in sch.events if ev[0] == "admit"]
    assert len(eng.prefills) == 2 * len(admits)
    for k, ev in enumerate(admits):
        cond, neg = eng.filled[2 * k], eng.filled[2 * k + 1]
        assert sorted(cond) == sorted(ev[2]) and sorted(neg) == sorted(S + s for s in ev[2])
        for q, s in zip(ev[1], ev[2]):
            assert cond[s] == sch.spliced[q] and neg[S + s] == sch.neg_spliced[q]      # request q's negative prompt is in row slots + s
    # slots were reused: a finished request frees both rows and the next request takes both
    taken = [s for ev in admits for s in ev[2]]
    assert len(taken) > len(set(taken))
    # every decode step runs all 2 * slots rows; both rows of a slot get the same token; idle pairs: token 0 at length 0
    decodes = [ev for ev in sch.events if ev[0] == "decode"]
    assert len(decodes) == len(eng.decodes)
    for ev, (lens, toks) in zip(decodes, eng.decodes):
        assert lens.shape == (2 * S,) and toks[:S].tolist() == toks[S:].tolist()
        for s in range(S):
            if s in ev[1]:
                assert lens[s] > 0 and lens[S + s] > 0
            else:
                assert lens[s] == lens[S + s] == 0 and toks[s] == 0


def test_scheduler_scale_zero_follows_the_negative_prompt_alone():
    """g = 0: the scores are the unconditional log-softmax, so the tokens are those of the negative prompt's own greedy run."""
    out, sch, eng, ps, ims, negs, nims, budgets = _guided_run(n=4, slots=2, g=0)
    for i, p in enumerate(ps):
        neg = p[-1:] if negs[i] is None else negs[i]
        nseq, want = eng._splice(neg, [] if nims[i] is None else [nims[i]]), []
        for _ in range(budgets[i]):
            want.append(argmax(torch_log_softmax32(eng.logits_of(nseq + want))[0]))
        assert out[f"req_{i}"].generated_tokens == want, i


def test_memory_check_counts_both_halves():
    _, sch, eng, *_ = _guided_run()
    need = eng.kv_cache_bytes(2 * sch.slots, sch.L_max)
    _guided_run(free=need)
    with pytest.raises(ValueError, match="bytes"):
        _guided_run(free=need - 1)
    with pytest.raises(ValueError, match="bytes"):                    # enough for the slots alone is not enough
        _guided_run(free=eng.kv_cache_bytes(sch.slots, sch.L_max))


def test_guidance_off_leaves_the_engine_calls_as_they_were():
    ps, ims = _prompts(7, 3)
    budgets = [5, 9, 2, 7, 3, 6, 4]
    runs = []
    for extra in ({}, dict(guidance_scale=None), dict(guidance_scale=1.0)):
        cfg = parse_batch_kwargs(dict(max_new_tokens=budgets, **extra), 7)
        eng = PairEngine()
        sch = BatchScheduler(eng, batch_requests(ps, ims, guidance=cfg.guidance), cfg, 3, picker=HostPicker(cfg))
        out = sch.run()
        runs.append((sch.events, eng.prefills, [(a.tolist(), b.tolist()) for a, b in eng.decodes], eng.made, eng.sized,
                     {k: v.generated_tokens for k, v in out.items()}))
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][3] == [(3, runs[0][3][0][1])]                      # slots rows, not twice as many


def test_symbol_declared_and_bound():
    import os
    from radvlm_amd import lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert {"rv_cfg_guide_rows_f32", "rv_cfg_guide_ws_bytes"} <= set(lib.SIGNATURES)
    assert callable(ops.cfg_guide_rows) and "cfg" in open(os.path.join(root, "radvlm_amd", "csrc", "build.sh")).read().split('SRCS="')[1].split('"')[0].split()

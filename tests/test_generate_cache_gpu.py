"""GPU tests of generate(past_key_values=GenerationCache()): an empty cache changes nothing, a continued conversation reuses the cached
prefix (LlavaEngine.extend) and matches the fp32 oracle and a fresh full call, the matching rule crops to the true common prefix, the
cache grows, batches reuse per row, a weight change empties the cache, misuse raises and training is not touched.

A continued call is not bit-identical to a fresh one: the K|V of the first call's generated tokens come from the decode path (GEMV,
decode attention) where a fresh call recomputes them in the prefill.  Its logits are compared with the fresh call's within LOGITS_FP32_TOL, and
its tokens up to the first step whose top-1 / top-2 margin (of the fresh call's logits) is below 2 x LOGITS_FP32_TOL x max |logit|:
two errors within the tolerance can close such a gap, so there a rounding may legitimately pick the other token."""
import json
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
LOGITS_FP32_TOL = 1.5e-2          # as tests/test_e2e_gpu.py and tests/test_generate_gpu.py
N1, N2 = 8, 6

CASES = {
    "toy": dict(golden="toy_e2e", geo="toy", kw={}),
    "toy_qwen": dict(golden="toy_qwen_e2e", geo="toy_qwen", kw={}),
    "toy_qwen_anyres_max": dict(golden="toy_qwen_anyres_max_e2e", geo="toy_qwen", kw=None),
}


def _load(golden_dir, case):
    c = CASES[case]
    g = np.load(os.path.join(golden_dir, c["golden"] + ".npz"))
    meta = json.load(open(os.path.join(golden_dir, c["golden"] + "_gradnorms.json")))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
    kw = c["kw"] if c["kw"] is not None else dict(merge_type=meta["merge_type"], image_aspect_ratio=meta["aspect"],
                                                  image_grid_pinpoints=meta["pinpoints"])
    sizes = [tuple(s) for s in g["image_sizes"].tolist()]
    return g, images, sizes, kw


def _model(geo, kw):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    ckw = dict(mm_patch_merge_type=kw.get("merge_type", "flat"), image_aspect_ratio=kw.get("image_aspect_ratio", "square"),
               image_grid_pinpoints=kw.get("image_grid_pinpoints"))
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0), **ckw)
    return Model(cfg, device="cuda:0", init="portable", seed=0).eval()


def _prompt(g, b):
    return g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _gen(model, ids, image, size, n, cache=None, **kw):
    ids = ids if torch.is_tensor(ids) else torch.from_numpy(np.asarray(ids)[None])
    extra = {} if cache is None else dict(past_key_values=cache)
    return model.generate(ids, images=None if image is None else [image], image_sizes=None if size is None else [size], max_new_tokens=n,
                          eos_token_id=None, output_scores=True, output_logits=True, return_dict_in_generate=True, **extra, **kw)


def _spliced_len(model, ids, image, size):
    return int(model.engine.plan(np.asarray(ids)[None], None, None, [image], [size])["lens"][0])


def _tokens_match(got, fresh, row=0):
    """Step by step while the two histories agree: got's logits are within LOGITS_FP32_TOL (relative to max |logit|) of the fresh call's,
    and unless the fresh call's top-1 / top-2 margin is below 2 x LOGITS_FP32_TOL x max |logit| (a gap two such errors can close) the
    tokens are equal.  Returns the steps whose tokens were compared."""
    for t in range(fresh.sequences.shape[1]):
        lg = fresh.logits[t][row].cpu()
        assert _rel(got.logits[t][row].cpu(), lg) <= LOGITS_FP32_TOL, (t, row)
        top = torch.topk(lg, 2).values
        if float(top[0] - top[1]) < 2 * LOGITS_FP32_TOL * float(lg.abs().max()):
            return t
        assert int(got.sequences[row, t]) == int(fresh.sequences[row, t]), (t, row)
    return fresh.sequences.shape[1]


class _Spy:
    """Counts vision-tower runs and records the reuse of every extend call of an engine."""

    def __init__(self, eng):
        self.eng, self.tower, self.reuse = eng, 0, []
        self._enc, self._ext = eng.encode_images, eng.extend

        def enc(*a, **k):
            self.tower += 1
            return self._enc(*a, **k)

        def ext(cache, *a, **k):
            self.reuse.append(None if k.get("reuse") is None else np.asarray(k["reuse"]).tolist())
            return self._ext(cache, *a, **k)

        eng.encode_images, eng.extend = enc, ext

    def close(self):
        del self.eng.encode_images, self.eng.extend


@pytest.mark.parametrize("case", list(CASES))
def test_empty_cache_is_bit_identical(golden_dir, case):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    p = _prompt(g, 0)
    plain = _gen(model, p, images[0], sizes[0], N1)
    cache = GenerationCache()
    got = _gen(model, p, images[0], sizes[0], N1, cache=cache)
    assert plain.past_key_values is None and got.past_key_values is cache
    assert torch.equal(plain.sequences, got.sequences)
    assert all(torch.equal(a, b) for a, b in zip(plain.scores, got.scores))
    assert all(torch.equal(a, b) for a, b in zip(plain.logits, got.logits))
    assert cache.get_seq_length() == _spliced_len(model, p, images[0], sizes[0]) + N1 - 1


@pytest.mark.parametrize("case", list(CASES))
def test_two_turn_continuation(golden_dir, case):
    from oracle import llava_oracle as O
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    model = _model(geo, kw)
    eng = model.engine
    p1 = _prompt(g, 0)
    cache = GenerationCache()
    t1 = _gen(model, p1, images[0], sizes[0], N1, cache=cache)
    L1 = cache.kv.L_max
    follow = np.random.default_rng(11).integers(3, eng.vocab, 40).astype(np.int64)
    p2 = np.concatenate([p1, t1.sequences[0].cpu().numpy(), follow])
    spy = _Spy(eng)
    try:
        got = _gen(model, p2, images[0], sizes[0], N2, cache=cache)
    finally:
        spy.close()
    S1 = _spliced_len(model, p1, images[0], sizes[0])
    assert spy.tower == 0                                              # every image row lies in the reused prefix
    assert spy.reuse == [[S1 + N1 - 1]]                                # all the cache holds: the prompt and N1 - 1 generated tokens
    S2 = _spliced_len(model, p2, images[0], sizes[0])
    assert cache.get_seq_length() == S2 + N2 - 1 and cache.kv.L_max > L1        # grown past the first call's headroom
    fresh = _gen(model, p2, images[0], sizes[0], N2)
    P = O.make_params(GEOMETRIES[geo], seed=0, with_newline=eng.with_newline)
    t = torch.from_numpy(p2[None])
    cfg = dict(mm_patch_merge_type=kw.get("merge_type", "flat"), image_aspect_ratio=kw.get("image_aspect_ratio", "square"),
               image_grid_pinpoints=kw.get("image_grid_pinpoints"), tower_image_size=GEOMETRIES[geo]["vision"]["image"])
    with torch.no_grad():
        _, ref, _ = O.llava_forward(P, GEOMETRIES[geo], t, torch.ones_like(t, dtype=torch.bool), torch.full_like(t, -100), [images[0]],
                                    image_sizes=[sizes[0]], cfg=cfg)
    e32 = _rel(got.logits[0][0].cpu(), ref[0][-1])
    efresh = _rel(got.logits[0][0].cpu(), fresh.logits[0][0].cpu())
    n = _tokens_match(got, fresh)
    from conftest import record_measurement
    record_measurement("generate_cache_two_turn", case=case, rel_vs_fp32=e32, rel_vs_fresh=efresh, steps_compared=n)
    assert e32 <= LOGITS_FP32_TOL, e32
    assert efresh <= LOGITS_FP32_TOL, efresh


@pytest.mark.parametrize("case", ["toy", "toy_qwen_anyres_max"])
def test_rewritten_history_and_changed_image(golden_dir, case):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    eng = model.engine
    p1 = _prompt(g, 0)
    S1 = _spliced_len(model, p1, images[0], sizes[0])
    rng = np.random.default_rng(12)
    follow = rng.integers(3, eng.vocab, 12).astype(np.int64)
    for what in ("history", "image"):
        cache = GenerationCache()
        t1 = _gen(model, p1, images[0], sizes[0], N1, cache=cache)
        ans = t1.sequences[0].cpu().numpy().copy()
        image, size = images[0], sizes[0]
        if what == "history":
            ans[3:] = (ans[3:] + 1) % eng.vocab                       # the earlier answer rewritten from its 4th token on
            want = S1 + 3
        else:
            image = images[0].flip(-1).contiguous()                   # another image, the same text
            want = int(np.nonzero(p1 == -200)[0][0])                  # only the text before the image is reused
        p2 = np.concatenate([p1, ans, follow])
        spy = _Spy(eng)
        try:
            got = _gen(model, p2, image, size, N2, cache=cache)
        finally:
            spy.close()
        assert spy.reuse == [[want]], (what, spy.reuse, want)
        assert spy.tower == (1 if what == "image" else 0)
        fresh = _gen(model, p2, image, size, N2)
        e = _rel(got.logits[0][0].cpu(), fresh.logits[0][0].cpu())
        from conftest import record_measurement
        record_measurement("generate_cache_cropped", case=case, what=what, rel_vs_fresh=e)
        assert e <= LOGITS_FP32_TOL, (what, e)
        _tokens_match(got, fresh)


def test_same_prompt_twice(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    p = _prompt(g, 0)
    cache = GenerationCache()
    first = _gen(model, p, images[0], sizes[0], N1, cache=cache)            # empty cache: the fresh call, bit for bit
    spy = _Spy(model.engine)
    try:
        again = _gen(model, p, images[0], sizes[0], N1, cache=cache)
    finally:
        spy.close()
    S = _spliced_len(model, p, images[0], sizes[0])
    assert spy.reuse == [[S - 1]] and spy.tower == 0                        # everything but the last prompt position
    assert _rel(again.logits[0][0].cpu(), first.logits[0][0].cpu()) <= LOGITS_FP32_TOL
    _tokens_match(again, first)
    assert cache.get_seq_length() == S + N1 - 1


def test_growth_beyond_first_headroom(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    p1 = _prompt(g, 0)
    cache = GenerationCache()
    t1 = _gen(model, p1, images[0], sizes[0], 2, cache=cache)
    L1 = cache.kv.L_max
    p2 = np.concatenate([p1, t1.sequences[0].cpu().numpy(), np.arange(3, 303, dtype=np.int64) % model.engine.vocab])
    got = _gen(model, p2, images[0], sizes[0], N2, cache=cache)
    assert cache.kv.L_max >= L1 + 300 and cache.kv.L_max % 256 == 0
    fresh = _gen(model, p2, images[0], sizes[0], N2)
    assert _rel(got.logits[0][0].cpu(), fresh.logits[0][0].cpu()) <= LOGITS_FP32_TOL
    _tokens_match(got, fresh)


def test_batch_of_two_left_padded_different_reuse(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    prompts = [_prompt(g, 0), _prompt(g, 1)[:-3]]

    def batch(ps):
        T = max(p.size for p in ps)
        ids, am = np.zeros((2, T), dtype=np.int64), np.zeros((2, T), dtype=bool)
        for b, p in enumerate(ps):
            ids[b, T - p.size:], am[b, T - p.size:] = p, True
        return torch.from_numpy(ids), torch.from_numpy(am)

    def gen(ps, n, **kw2):
        ids, am = batch(ps)
        return model.generate(ids, images=images[:2], image_sizes=sizes[:2], attention_mask=am, max_new_tokens=n, eos_token_id=None,
                               output_logits=True, return_dict_in_generate=True, **kw2)

    cache = GenerationCache()
    t1 = gen(prompts, N1, past_key_values=cache)
    rng = np.random.default_rng(13)
    a0 = t1.sequences[0].cpu().numpy()
    a1 = t1.sequences[1].cpu().numpy().copy()
    a1[1:] = (a1[1:] + 7) % model.engine.vocab                       # row 1's answer rewritten after its first token
    p2 = [np.concatenate([prompts[0], a0, rng.integers(3, 200, 9)]), np.concatenate([prompts[1], a1, rng.integers(3, 200, 21)])]
    spy = _Spy(model.engine)
    try:
        got = gen(p2, N2, past_key_values=cache)
    finally:
        spy.close()
    S = [_spliced_len(model, prompts[b], images[b], sizes[b]) for b in range(2)]
    assert spy.reuse == [[S[0] + N1 - 1, S[1] + 1]] and spy.tower == 0
    fresh = gen(p2, N2)
    for b in range(2):
        assert _rel(got.logits[0][b].cpu(), fresh.logits[0][b].cpu()) <= LOGITS_FP32_TOL, b
        _tokens_match(got, fresh, row=b)


@pytest.mark.parametrize("change", ["optimizer_step", "load_state_dict"])
def test_weight_change_empties_the_cache(golden_dir, change):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    eng = model.engine
    p1 = _prompt(g, 0)
    cache = GenerationCache()
    t1 = _gen(model, p1, images[0], sizes[0], N1, cache=cache)
    if change == "optimizer_step":
        eng.optimizer_step(lr=1e-3)                                 # zero gradients: the weights keep their values, the version moves
    else:
        eng.load_state_dict({k: v.clone() for k, v in eng.state_dict().items()})
    p2 = np.concatenate([p1, t1.sequences[0].cpu().numpy(), np.arange(5, 25, dtype=np.int64)])
    got = _gen(model, p2, images[0], sizes[0], N2, cache=cache)
    fresh = _gen(model, p2, images[0], sizes[0], N2)
    assert torch.equal(got.sequences, fresh.sequences)
    assert all(torch.equal(a, b) for a, b in zip(got.logits, fresh.logits))
    assert cache.get_seq_length() == _spliced_len(model, p2, images[0], sizes[0]) + N2 - 1


def test_wrong_batch_or_engine_raises(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy")
    model, other = _model("toy", kw), _model("toy", kw)
    p = _prompt(g, 0)
    cache = GenerationCache()
    _gen(model, p, images[0], sizes[0], 3, cache=cache)
    with pytest.raises(ValueError, match="another model"):
        _gen(other, p, images[0], sizes[0], 3, cache=cache)
    ids = torch.from_numpy(np.stack([p, p]))
    with pytest.raises(ValueError, match="sequences"):
        model.generate(ids, images=images[:1] * 2, image_sizes=sizes[:1] * 2, max_new_tokens=3, past_key_values=cache)
    with pytest.raises(ValueError, match="use_cache"):
        model.generate(ids, images=images[:1] * 2, image_sizes=sizes[:1] * 2, max_new_tokens=3, past_key_values=cache, use_cache=False)
    with pytest.raises(TypeError, match="GenerationCache"):
        model.generate(ids, images=images[:1] * 2, image_sizes=sizes[:1] * 2, max_new_tokens=3, past_key_values=())


def test_training_step_after_cached_generation_is_unchanged(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy")

    def step(with_generate):
        model = _model("toy", kw)
        eng = model.engine
        if with_generate:
            cache = GenerationCache()
            p = _prompt(g, 0)
            t1 = _gen(model, p, images[0], sizes[0], 4, cache=cache)
            _gen(model, np.concatenate([p, t1.sequences[0].cpu().numpy(), [5, 6, 7]]), images[0], sizes[0], 4, cache=cache)
        loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return float(loss), eng.lm.flat.clone(), eng.grads.clone(), eng.lora_step

    a, b = step(False), step(True)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]

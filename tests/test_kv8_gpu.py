"""GPU tests of the int8 KV cache at engine and model level, on the toy goldens: the int8 arm (int8 rows read by
rv_attn_decode_kv8_bf16) and the reference arm (the dequantised values kept as bf16 and read by rv_attn_decode_bf16) are bit-identical,
the default cache is untouched, and what the int8 cache does not do is refused.  Every comparison is exact."""
import copy

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES
from test_generate_gpu import CASES, _engine, _load, _model, _prompt

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_MODELS = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _setup(golden_dir, case):
    """One model per toy geometry for the whole module (generation does not change it)."""
    if case not in _MODELS:
        g, images, sizes, kw = _load(golden_dir, case)
        _MODELS[case] = (_model(CASES[case]["geo"], kw), g, images, sizes, kw)
    return _MODELS[case]


def _arms(eng, fn):
    """fn() on the int8 arm and on the reference arm of the same engine."""
    out = []
    for flag in (True, False):
        eng.kv8_decode = flag
        try:
            out.append(fn())
        finally:
            eng.kv8_decode = True
    return out


def _gen(model, g, images, sizes, b=0, n=12, **k):
    return model.generate(torch.from_numpy(_prompt(g, b)[None]), images=[images[b]], image_sizes=[sizes[b]], max_new_tokens=n,
                          eos_token_id=None, output_logits=True, return_dict_in_generate=True, **k)


def _same(a, b):
    return torch.equal(a.sequences, b.sequences) and len(a.logits) == len(b.logits) and all(torch.equal(u, v) for u, v in zip(a.logits, b.logits))


def _count(monkeypatch, name):
    from radvlm_amd import ops
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# ------------------------------------------------------------------------------------------------ both arms
@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_both_arms_bit_identical(golden_dir, case, monkeypatch):
    model, g, images, sizes, _ = _setup(golden_dir, case)
    eng = model.engine
    kv8_calls, bf_calls = _count(monkeypatch, "attn_decode_kv8"), _count(monkeypatch, "attn_decode")
    a, b = _arms(eng, lambda: _gen(model, g, images, sizes, kv_cache_dtype="int8"))
    assert len(kv8_calls) == len(bf_calls) >= 11 * eng.l["layers"]         # each arm ran its own kernel: 11 decode steps after the prompt
    assert a.sequences.shape == (1, 12) and _same(a, b)
    sa, sb = _arms(eng, lambda: _gen(model, g, images, sizes, kv_cache_dtype="int8", do_sample=True, seed=3))
    assert _same(sa, sb) and not torch.equal(sa.sequences, a.sequences)
    pa, pb = _arms(eng, lambda: _gen(model, g, images, sizes, kv_cache_dtype="int8", repetition_penalty=1.3, no_repeat_ngram_size=2,
                                     output_scores=True))
    assert _same(pa, pb) and all(torch.equal(u, v) for u, v in zip(pa.scores, pb.scores))


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_both_arms_bit_identical_on_a_quantised_decoder(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    model.quantize_decoder_()
    a, b = _arms(model.engine, lambda: _gen(model, g, images, sizes, kv_cache_dtype="int8"))
    assert _same(a, b)
    plain = _gen(model, g, images, sizes)
    assert torch.equal(plain.logits[0], a.logits[0])


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_cache_bytes_of_both_arms(golden_dir, case):
    model, g, images, sizes, _ = _setup(golden_dir, case)
    eng = model.engine
    ids = _prompt(g, 0)[None]
    l, kvd, Hkv = eng.l, eng.kvd, eng.Hkv

    def run():
        cache, _ = eng.prefill(ids, None, [images[0]], [sizes[0]], max_new_tokens=4, kv_dtype="int8")
        return cache, eng.kv_cache_bytes(1, cache.L_max, "int8"), eng.new_kv_cache(1, cache.L_max, "int8").nbytes()

    (c8, n8, m8), (cb, nb, mb) = _arms(eng, run)
    assert c8.dtype == cb.dtype == "int8" and c8.L_max == cb.L_max
    assert c8.nbytes() == n8 == m8 == l["layers"] * c8.L_max * (2 * kvd + 8 * Hkv)
    assert cb.nbytes() == nb == mb == l["layers"] * c8.L_max * 4 * kvd == eng.kv_cache_bytes(1, c8.L_max)
    assert c8.layers[0].dtype == torch.int8 and c8.scales[0].dtype == torch.float32 and cb.layers[0].dtype == BF16 and cb.scales is None
    # the public layout dequantises to the reference arm's rows with plain torch
    n = int(c8.lens[0])
    for q8, s, x in zip(c8.layers, c8.scales, cb.layers):
        deq = (q8.float() * s.repeat_interleave(eng.hd, -1)).to(BF16)
        assert torch.equal(deq[0, :n], x[0, :n])


# ------------------------------------------------------------------------------------------------ generate_batch
@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_batch_matches_generate_alone(golden_dir, case):
    model, g, images, sizes, _ = _setup(golden_dir, case)
    reqs = [(_prompt(g, b)[:len(_prompt(g, b)) - c], images[b], sizes[b]) for b, c in ((0, 0), (1, 0), (0, 3), (1, 2), (0, 5))]
    budgets = [6, 9, 4, 7, 5]

    def batch():
        return model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=2,
                                    max_new_tokens=budgets, eos_token_id=None, return_logprobs=True, kv_cache_dtype="int8")

    o8, ob = _arms(model.engine, batch)
    for i, (p, im, sz) in enumerate(reqs):
        alone = model.generate(torch.from_numpy(p[None]), images=[im], image_sizes=[sz], max_new_tokens=budgets[i], eos_token_id=None,
                               kv_cache_dtype="int8")
        k = f"req_{i}"
        assert o8[k].generated_tokens == alone[0].tolist() == ob[k].generated_tokens, i
        assert o8[k].logprobs == ob[k].logprobs and len(o8[k].logprobs) == budgets[i]


# ------------------------------------------------------------------------------------------------ defaults
@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_default_dtype_is_untouched_and_the_first_step_is_unquantised(golden_dir, case, monkeypatch):
    model, g, images, sizes, _ = _setup(golden_dir, case)
    new_calls = _count(monkeypatch, "attn_decode_kv8"), _count(monkeypatch, "kv_append_q8"), _count(monkeypatch, "kv_quantize_rows")
    base = _gen(model, g, images, sizes)
    assert _same(base, _gen(model, g, images, sizes, kv_cache_dtype=None))
    assert _same(base, _gen(model, g, images, sizes, kv_cache_dtype="bf16"))
    assert not any(new_calls)                                               # none of the new code ran
    for flag in (True, False):
        model.engine.kv8_decode = flag
        try:
            q = _gen(model, g, images, sizes, kv_cache_dtype="int8")
        finally:
            model.engine.kv8_decode = True
        assert torch.equal(q.logits[0], base.logits[0])                    # the prompt's own attention is unquantised
        assert not torch.equal(q.logits[1], base.logits[1])                # the next step reads the rounded rows
    assert all(new_calls)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        _gen(model, g, images, sizes, kv_cache_dtype="fp8")


# ------------------------------------------------------------------------------------------------ refusals
def test_model_level_refusals(golden_dir):
    from radvlm_amd.generation import GenerationCache
    model, g, images, sizes, _ = _setup(golden_dir, "toy")
    with pytest.raises(NotImplementedError, match="past_key_values"):
        _gen(model, g, images, sizes, kv_cache_dtype="int8", past_key_values=GenerationCache())
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        _gen(model, g, images, sizes, kv_cache_dtype="int8", prompt_lookup_num_tokens=3)
    kw = dict(images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=4, eos_token_id=None, num_beams=2)
    ids = torch.from_numpy(_prompt(g, 0)[None])
    with pytest.raises(NotImplementedError, match="beam"):
        model.generate_beams(ids, kv_cache_dtype="int8", **kw)
    want = model.generate_beams(ids, **kw)
    for v in (None, "bf16"):                                                # accepted no-ops
        assert torch.equal(model.generate_beams(ids, kv_cache_dtype=v, **kw), want)


def test_engine_level_refusals(golden_dir):
    model, g, images, sizes, _ = _setup(golden_dir, "toy")
    eng = model.engine
    ids = _prompt(g, 0)[None]
    for flag in (True, False):
        eng.kv8_decode = flag
        try:
            cache, _ = eng.prefill(ids, None, [images[0]], [sizes[0]], max_new_tokens=8, kv_dtype="int8")
            with pytest.raises(NotImplementedError, match="beams"):
                eng.decode_step(cache, [1], beams=object())
            with pytest.raises(NotImplementedError, match="verify_step"):
                eng.verify_step(cache, [1, 2])
            with pytest.raises(NotImplementedError, match="extend"):
                eng.extend(cache, ids, None, [images[0]], [sizes[0]], reuse=np.array([3]), max_new_tokens=2)
            with pytest.raises(ValueError, match="kv_dtype"):
                eng.prefill(ids, None, [images[0]], [sizes[0]], cache=cache, slots=[0], kv_dtype="bf16")
            assert int(cache.lens[0]) > 0 and eng.decode_step(cache, [1]).shape == (1, eng.vocab)      # the cache is still usable
        finally:
            eng.kv8_decode = True


# ------------------------------------------------------------------------------------------------ full width
@pytest.mark.parametrize("gname", ["llava15_7b", "llava_ov_qwen2_7b"])
def test_full_width_prefill_and_decode_both_arms(gname):
    """One 7B-width decoder layer + the full head: eight 48-token rows prefilled into an int8 cache, then two decode steps; the logits
    and, after dequantising, the layer's cache rows are bit-identical between the two arms."""
    _need_gpu()
    from radvlm_amd.engine import LlavaEngine
    geo = copy.deepcopy(GEOMETRIES[gname])
    geo["lm"]["layers"] = 1
    geo["vision"]["layers"] = 2
    eng = LlavaEngine(geo, device="cuda:0", init="fast", seed=0)
    ids = np.random.default_rng(0).integers(0, eng.vocab, (8, 48))
    toks = np.random.default_rng(1).integers(0, eng.vocab, (2, 8))

    def run():
        cache, lg = eng.prefill(ids, None, None, None, max_new_tokens=3, kv_dtype="int8")
        out = [lg.clone()] + [eng.decode_step(cache, toks[t].tolist()).clone() for t in range(2)]
        if cache.scales is not None:
            rows = (cache.layers[0].float() * cache.scales[0].repeat_interleave(eng.hd, -1)).to(BF16)
        else:
            rows = cache.layers[0].clone()
        return out, rows[:, :50], cache.nbytes()

    (la, kva, na), (lb, kvb, nb) = _arms(eng, run)
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and torch.equal(kva, kvb)
    assert all(bool(torch.isfinite(a).all()) for a in la) and bool(kva.float().abs().sum() > 0)
    assert na == 8 * 51 * (2 * eng.kvd + 8 * eng.Hkv) and nb == 8 * 51 * 4 * eng.kvd

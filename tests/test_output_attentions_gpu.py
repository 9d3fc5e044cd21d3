"""GPU tests of generate(output_attentions=True) on the toy goldens: the call perturbs nothing (sequences, scores and logits are the bits
of the call without it), the returned structure, the provenance of every returned entry (recomputed in float64 from the operands the
probability op received, which are bitwise the operands of the attention the model ran), the engine-level keywords and the new
refusals.  The batch is two left-padded prompts of different lengths, so cache positions rather than padded positions are pinned."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import attn_probs_ref as R
from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
CASES = {"toy": "toy_e2e", "toy_qwen": "toy_qwen_e2e"}
T_NEW = 4


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _new_model(geo):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0))
    return Model(cfg, device="cuda:0", init="portable", seed=0).eval()


@functools.lru_cache(maxsize=None)
def _model(geo):
    return _new_model(geo)


@functools.lru_cache(maxsize=None)
def _inputs(geo):
    """Two prompts of different lengths, left-padded, with their images: generate()'s arguments."""
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(golden_dir, CASES[geo] + ".npz"))
    json.load(open(os.path.join(golden_dir, CASES[geo] + "_gradnorms.json")))
    prompts = [g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64) for b in range(2)]
    prompts[1] = prompts[1][:-3]
    T = max(p.size for p in prompts)
    ids, am = np.zeros((2, T), dtype=np.int64), np.zeros((2, T), dtype=bool)
    for b, p in enumerate(prompts):
        ids[b, T - p.size:], am[b, T - p.size:] = p, True
    images = [torch.from_numpy(g[f"image{i}"]) for i in range(2)]
    sizes = [tuple(s) for s in g["image_sizes"].tolist()][:2]
    return dict(inputs=torch.from_numpy(ids), attention_mask=torch.from_numpy(am), images=images, image_sizes=sizes)


def _generate(model, geo, **kw):
    return model.generate(**_inputs(geo), max_new_tokens=T_NEW, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)


def _same_outputs(a, b):
    assert torch.equal(a.sequences, b.sequences)
    assert len(a.scores) == len(b.scores) and len(a.logits) == len(b.logits)
    for x, y in zip(a.scores + a.logits, b.scores + b.logits):
        assert torch.equal(_bits(x), _bits(y))


@functools.lru_cache(maxsize=None)
def _all_layers(geo):
    return _generate(_model(geo), geo, output_attentions=True)


MODES = {"greedy": {}, "sampled": dict(do_sample=True, seed=11, top_k=20), "processed": dict(repetition_penalty=1.3, no_repeat_ngram_size=2)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geo", list(CASES))
def test_no_perturbation(geo, mode):
    model = _model(geo)
    base = _generate(model, geo, **MODES[mode])
    assert getattr(base, "attentions", None) is None
    att = _generate(model, geo, output_attentions=True, attention_reduce="mean_heads" if mode == "sampled" else None, **MODES[mode])
    _same_outputs(base, att)
    assert len(att.attentions) == att.sequences.shape[1] == T_NEW


def test_no_perturbation_int8_weights():
    model = _new_model("toy")
    model.quantize_decoder_()
    base = _generate(model, "toy")
    att = _generate(model, "toy", output_attentions=True, attention_layers=[0, -1])
    _same_outputs(base, att)
    assert att.attention_layers == (0, model.engine.l["layers"] - 1) and len(att.attentions[0]) == 2


@pytest.mark.parametrize("geo", list(CASES))
def test_structure(geo):
    model = _model(geo)
    eng = model.engine
    L, H = eng.l["layers"], eng.l["heads"]
    out = _all_layers(geo)
    inp = _inputs(geo)
    plan = eng.plan(inp["inputs"].numpy(), inp["attention_mask"].numpy(), None, inp["images"], inp["image_sizes"])
    lens = plan["lens"].astype(np.int64)
    assert lens[0] != lens[1]
    S0 = int(lens.max())
    assert out.attention_layers == tuple(range(L)) and len(out.attentions) == T_NEW
    for t, step in enumerate(out.attentions):
        assert isinstance(step, tuple) and len(step) == L
        for a in step:
            assert a.dtype == torch.float32 and tuple(a.shape) == (2, H, 1, S0 + t)
            for b in range(2):                          # the key axis is the sequence's cache positions: zeros past its own length
                n = int(lens[b]) + t
                assert not bool(_bits(a[b, :, 0, n:]).any())
                assert float((a[b, :, 0, :n].double().sum(-1) - 1).abs().max()) <= (n + 16) * 2.0 ** -24
    last = _generate(model, geo, output_attentions=True, attention_layers=[-1])
    assert last.attention_layers == (L - 1,)
    for t in range(T_NEW):
        assert len(last.attentions[t]) == 1 and torch.equal(_bits(last.attentions[t][0]), _bits(out.attentions[t][-1]))
    mean = _generate(model, geo, output_attentions=True, attention_reduce="mean_heads")
    worst = 0.0
    for t in range(T_NEW):
        for c in range(L):
            m, a = mean.attentions[t][c], out.attentions[t][c]
            assert m.dtype == torch.float32 and tuple(m.shape) == (2, 1, 1, S0 + t)
            host = a.double().mean(1, keepdim=True).cpu()
            gate = host * (H * 2.0 ** -24) + 1e-37           # the H-term fp32 sum in head order and the division: the per-head bits are shared
            err = (m.cpu().double() - host).abs()
            assert bool((err <= gate).all()), (t, c, float((err / gate).max()))
            worst = max(worst, float((err / gate).max()))
    print(f"{geo}: mean_heads against the host mean of the per-head call: worst error / gate = {worst:.4g}")
    from radvlm_amd.attention_maps import step_image_maps
    maps = step_image_maps(out, plan, side=eng.side, image=1)
    assert maps.shape == (T_NEW, 1, eng.side, eng.side) and float(maps.min()) >= 0 and float(maps.sum(axis=(1, 2, 3)).max()) <= 1 + 1e-5
    # the device's head mean against the host's float64 one, both stored as fp32: the gate above plus the two fp32 stores
    assert np.allclose(maps, step_image_maps(mean, plan, side=eng.side, image=1), rtol=(H + 2) * 2.0 ** -24, atol=1e-37)


@pytest.mark.parametrize("geo", list(CASES))
def test_provenance(geo, monkeypatch):
    from radvlm_amd import ops
    from radvlm_amd.engine import LlavaEngine
    model = _model(geo)
    eng = model.engine
    L, H, Hkv, hd, d = eng.l["layers"], eng.l["heads"], eng.Hkv, eng.hd, eng.l["d"]
    probs_calls, decode_q, prompt_qkv = [], [], []
    real_probs, real_decode, real_layer = ops.attn_decode_probs, ops.attn_decode, LlavaEngine._layer_forward

    def probs(q, cache, kv_len, *a, **kw):
        got = real_probs(q, cache, kv_len, *a, **kw)
        probs_calls.append(dict(q=q.clone(), cache=cache.clone(), kv_len=kv_len.cpu().numpy().copy(), args=a, kw=kw, got=got))
        return got

    def decode(q, *a, **kw):
        decode_q.append(q.clone())
        return real_decode(q, *a, **kw)

    def layer(self, i, x, g, rows=None):
        out = real_layer(self, i, x, g, rows)
        prompt_qkv.append((i, out[1]["qkv"].clone()))
        return out

    monkeypatch.setattr(ops, "attn_decode_probs", probs)
    monkeypatch.setattr(ops, "attn_decode", decode)
    monkeypatch.setattr(LlavaEngine, "_layer_forward", layer)
    out = _generate(model, geo, output_attentions=True)
    monkeypatch.undo()
    _same_outputs(out, _all_layers(geo))
    assert len(probs_calls) == T_NEW * L and len(decode_q) == (T_NEW - 1) * L and [i for i, _ in prompt_qkv] == list(range(L))
    worst = 0.0
    for k, c in enumerate(probs_calls):
        t, layer_no = divmod(k, L)
        assert c["args"][:3] == (H, Hkv, hd) and c["kw"] == dict(per_head=True, mean=False)
        L_out = c["args"][3]
        entry = out.attentions[t][layer_no]
        assert c["got"][1] is None and torch.equal(_bits(entry[:, :, 0, :]), _bits(c["got"][0]))
        p64, gp, _, _ = R.reference(c["q"], c["cache"], c["kv_len"], H, Hkv, hd, L_out)
        worst = max(worst, R.assert_within_budget(entry[:, :, 0, :], p64, gp, f"{geo} step {t} layer {layer_no}"))
        if t == 0:      # the last prompt row of every sequence, from the layer's own post-RoPE q|k|v
            rows = np.cumsum(c["kv_len"]) - 1
            assert c["kv_len"][0] != c["kv_len"][1]
            want = prompt_qkv[layer_no][1][torch.from_numpy(rows).cuda(), :d]
            assert torch.equal(_bits(c["q"]), _bits(want))
        else:           # bitwise the q of the attention the step really ran in this layer
            assert torch.equal(_bits(c["q"]), _bits(decode_q[(t - 1) * L + layer_no]))
            assert np.array_equal(c["kv_len"], probs_calls[layer_no]["kv_len"] + t)
    print(f"{geo}: worst error / gate over every returned entry = {worst:.4g}")


@pytest.mark.parametrize("geo", list(CASES))
def test_engine_level(geo):
    model = _model(geo)
    eng = model.engine
    L, H = eng.l["layers"], eng.l["heads"]
    inp = _inputs(geo)
    args = (inp["inputs"].numpy(), inp["attention_mask"].numpy(), inp["images"], inp["image_sizes"])
    c0, lg0 = eng.prefill(*args, max_new_tokens=3)
    c1, lg1, at = eng.prefill(*args, max_new_tokens=3, attn_layers=(L - 1, 0))
    S0 = int(c0.lens.max())
    assert torch.equal(_bits(lg0), _bits(lg1)) and np.array_equal(c0.lens, c1.lens)
    assert len(at) == 2 and all(tuple(a.shape) == (2, H, S0) for a in at)
    tok = lg0.argmax(-1).to(torch.int32)
    for step in range(2):
        a = eng.decode_step(c0, tok)
        kw = dict(attn_layers=(L - 1, 0)) if step == 0 else dict(attn_layers=[0], attn_mean=True)
        b, at = eng.decode_step(c1, tok, **kw)
        assert torch.equal(_bits(a), _bits(b)) and np.array_equal(c0.lens, c1.lens)
        want = (2, H, S0 + 1 + step) if step == 0 else (2, S0 + 1 + step)
        assert len(at) == len(kw["attn_layers"]) and all(tuple(x.shape) == want and x.dtype == torch.float32 for x in at)
        for x, y in zip(c0.layers, c1.layers):
            assert torch.equal(_bits(x), _bits(y))
        tok = a.argmax(-1).to(torch.int32)


def test_new_refusals_and_a_good_call_after_them(monkeypatch):
    from radvlm_amd.generation import GenerationCache
    geo = "toy"
    model = _model(geo)
    eng = model.engine
    L = eng.l["layers"]
    inp = _inputs(geo)
    args = (inp["inputs"].numpy(), inp["attention_mask"].numpy(), inp["images"], inp["image_sizes"])
    cache, lg = eng.prefill(*args, max_new_tokens=2)
    tok = lg.argmax(-1).to(torch.int32)
    lens = cache.lens.copy()
    for kw, name in ((dict(beams=object()), "beams="), (dict(shared=object()), "shared="), (dict(tap_layers=(0,)), "tap_layers=")):
        with pytest.raises(NotImplementedError, match=r"attn_layers=\.\.\.\) with " + name):
            eng.decode_step(cache, tok, attn_layers=(0,), **kw)
    c8, _ = eng.prefill(*args, max_new_tokens=2, kv_dtype="int8")
    with pytest.raises(NotImplementedError, match="int8 KV cache"):
        eng.decode_step(c8, tok, attn_layers=(0,))
    with pytest.raises(NotImplementedError, match="int8 KV cache"):
        eng.prefill(*args, max_new_tokens=2, kv_dtype="int8", attn_layers=(0,))
    with pytest.raises(NotImplementedError, match="tap_layers="):
        eng.prefill(*args, max_new_tokens=2, tap_layers=(0,), attn_layers=(0,))
    with pytest.raises(NotImplementedError, match="cache= / slots="):
        eng.prefill(*args, max_new_tokens=0, cache=cache, slots=[0, 1], attn_layers=(0,))
    for bad in ((), (0, 0), (L,), (-1,), (True,), (0.0,)):
        with pytest.raises(ValueError, match="attn_layers"):
            eng.decode_step(cache, tok, attn_layers=bad)
    assert np.array_equal(cache.lens, lens)                        # a refused step appended nothing
    on = dict(output_attentions=True)
    for kw, name in ((dict(kv_cache_dtype="int8"), "kv_cache_dtype='int8'"), (dict(past_key_values=GenerationCache()), "past_key_values"),
                     (dict(prompt_lookup_num_tokens=2), "prompt_lookup_num_tokens"), (dict(guidance_scale=2.0), "guidance_scale"),
                     (dict(dola_layers="low"), "dola_layers")):
        with pytest.raises(NotImplementedError, match="output_attentions with " + name):
            _generate(model, geo, **on, **kw)
    for kw in (dict(attention_layers=[L]), dict(attention_layers=[-L - 1]), dict(attention_layers=[0, -L]), dict(attention_layers=[True]),
               dict(attention_reduce="sum"), dict(output_attentions=1)):
        with pytest.raises(ValueError):
            _generate(model, geo, **{**on, **kw})
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        model.generate(**inp, max_new_tokens=2, output_attentions=True)
    with pytest.raises(ValueError, match="without output_attentions"):
        _generate(model, geo, attention_layers=[0])
    for entry in (model.generate_batch, model.generate_beams):
        with pytest.raises(TypeError, match="output_attentions"):
            entry([inp["inputs"][0]], output_attentions=True)
    with monkeypatch.context() as m:                                # live adapters: the keyword is refused by name
        m.setattr(eng, "lora", True)
        m.setattr(eng, "adapter_decoding", True)
        with pytest.raises(NotImplementedError, match="output_attentions with LoRA adapters"):
            _generate(model, geo, **on)
    good = _generate(model, geo, **on)
    _same_outputs(good, _all_layers(geo))
    for a, b in zip(good.attentions, _all_layers(geo).attentions):
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    b, at = eng.decode_step(cache, tok, attn_layers=(0,))
    assert tuple(at[0].shape)[:2] == (2, eng.l["heads"]) and np.array_equal(cache.lens, lens + 1)

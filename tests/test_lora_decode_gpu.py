"""GPU tests of generation on live (unmerged) LoRA adapters: model.enable_adapter_decoding() and model.disable_adapter() on the toy and
toy_qwen geometries with r = 8, alpha = 16 and the non-zero adapters of test_lora_merge_gpu.  The gates are the project's existing ones:
the cached decode against the engine's own no-cache forward (1e-2) and against the fp32 oracle with apply_lora (LOGITS_FP32_TOL), the
margin rule for free-running greedy tokens, and bit-identity wherever two calls run the same arithmetic."""
import numpy as np
import pytest
import torch

from radvlm_amd.splice import IMAGE_TOKEN_INDEX
from test_generate_gpu import _oracle_logits
from test_lora_merge_gpu import LOGITS_FP32_TOL, _golden, _greedy_rows, _model, _oracle_params, _prompt, _rel, _set_adapters

pytestmark = pytest.mark.gpu
LORA = dict(r=8, alpha=16, dropout=0.0)
SCALE = 16 / 8
GEOS = [("toy", "toy_e2e"), ("toy_qwen", "toy_qwen_e2e")]
N_STEPS = 11


def _live(geo, lora=LORA, zero_b=False):
    model = _model(geo, lora=dict(lora)).enable_adapter_decoding()
    L = _set_adapters(model.engine)
    if zero_b:
        for n in model.engine.lm.names():
            if n.endswith("lora_B.weight"):
                model.engine.lm.view(n).zero_()
    return model, L


def _ids(t):
    return [int(v) for v in t]


def _teacher_forced(eng, prompt, image, size, cont):
    """(the fp32 logits of prefill and of one decode_step per continuation token but the last, the spliced prompt length)."""
    cache, lg = eng.prefill(prompt[None], None, [image], [size], max_new_tokens=cont.size)
    steps = [lg.cpu()]
    for t in range(cont.size - 1):
        steps.append(eng.decode_step(cache, [int(cont[t])]).cpu())
    return steps, int(cache.lens[0]) - (cont.size - 1)


def _no_cache(eng, full, image, size):
    eng.forward(full[None], np.ones((1, full.size), dtype=bool), np.full((1, full.size), -100), [image], image_sizes=[size], want_logits=True)
    own = eng.last_logits[0].cpu()
    eng.ctx = None
    return own


def test_opt_in(golden_dir):
    g, images = _golden(golden_dir, "toy_e2e")
    model = _model("toy", lora=dict(LORA))
    prompt = torch.from_numpy(_prompt(g, 0)[None])
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        model.generate(prompt, images=[images[0]], max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="enable_adapter_decoding"):
        model.engine.prefill(prompt.numpy(), None, [images[0]])
    assert model.enable_adapter_decoding() is model and model.engine.adapter_decoding
    assert tuple(model.generate(prompt, images=[images[0]], max_new_tokens=2).shape) == (1, 2)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):          # quantised decoders with adapters stay refused
        model.quantize_decoder_()
    model.enable_adapter_decoding(False)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        model.generate(prompt, images=[images[0]], max_new_tokens=2)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        model.score([prompt[0]], [[np.array([3, 4])]], images=[images[0]])
    plain = _model("toy")
    with pytest.raises(ValueError):
        plain.enable_adapter_decoding()
    with pytest.raises(ValueError):
        with plain.disable_adapter():
            pass
    # the prompt pass is the eval form: the adapters' dropout rate does not reach it
    a, _ = _live("toy")
    b, _ = _live("toy", lora=dict(LORA, dropout=0.5))
    _, la = a.engine.prefill(prompt.numpy(), None, [images[0]])
    _, lb = b.engine.prefill(prompt.numpy(), None, [images[0]])
    assert torch.equal(la, lb) and b.engine.lora_p == 0.5


@pytest.mark.parametrize("geo,golden", GEOS)
def test_teacher_forced_decode_and_greedy(golden_dir, geo, golden):
    g, images = _golden(golden_dir, golden)
    model, L = _live(geo)
    eng = model.engine
    prompt, size = _prompt(g, 0), tuple(g["image_sizes"][0].tolist())
    cont = np.random.default_rng(5).integers(0, eng.vocab, N_STEPS + 1).astype(np.int64)
    full = np.concatenate([prompt, cont])
    steps, S0 = _teacher_forced(eng, prompt, images[0], size, cont)
    assert len(steps) == N_STEPS + 1
    own = _no_cache(eng, full, images[0], size)
    Pe = _oracle_params(geo, L, SCALE, with_newline=eng.with_newline)
    ref = _oracle_logits(Pe, geo, full, images[0], size, {})
    e_own = max(_rel(steps[t][0], own[S0 - 1 + t]) for t in range(len(steps)))
    e_32 = max(_rel(steps[t][0], ref[S0 - 1 + t]) for t in range(len(steps)))
    # how far the base model alone is from these logits (recorded; test_disable_adapter_is_zero_b_bit_for_bit asserts they differ)
    P0 = _oracle_params(geo, None, SCALE, with_newline=eng.with_newline)
    e_base = _rel(steps[-1][0], _oracle_logits(P0, geo, full, images[0], size, {})[S0 - 1 + N_STEPS])
    n_cmp = _greedy_rows(Pe, geo, model, g, images)
    from conftest import record_measurement
    record_measurement("lora_decode_teacher_forced", geo=geo, max_rel_vs_nocache=e_own, max_rel_vs_fp32=e_32, rel_vs_base_model=e_base,
                       greedy_steps=n_cmp)
    assert e_own <= 1e-2, e_own
    assert e_32 <= LOGITS_FP32_TOL, e_32
    assert n_cmp >= 1


@pytest.mark.parametrize("geo,golden", GEOS)
def test_disable_adapter_is_zero_b_bit_for_bit(golden_dir, geo, golden):
    g, images = _golden(golden_dir, golden)
    off, _ = _live(geo)
    zero, _ = _live(geo, zero_b=True)
    prompt, size = _prompt(g, 0), tuple(g["image_sizes"][0].tolist())
    text = np.random.default_rng(7).integers(0, off.engine.vocab, 50).astype(np.int64)
    batch = (g["input_ids"], g["attention_mask"], g["labels"], images)

    def run(model, disabled):
        eng, out = model.engine, {}
        import contextlib
        with (model.disable_adapter() if disabled else contextlib.nullcontext()):
            assert eng.adapters_off == disabled
            cache, lg = eng.prefill(prompt[None], None, [images[0]], [size], max_new_tokens=8)
            out["prefill"] = lg.clone()
            out["decode"] = torch.stack([eng.decode_step(cache, [int(t)]) for t in text[:3]])
            out["verify"] = eng.verify_step(cache, text[3:8]).clone()
            tc, _ = eng.prefill(text[None, :10], max_new_tokens=0)
            _, out["extend_40_rows"] = eng.extend(tc, text[None], reuse=[10])
            tc, _ = eng.prefill(text[None, :40], max_new_tokens=0)
            _, out["extend_10_rows"] = eng.extend(tc, text[None], reuse=[40])
            out["token_logps"] = model.token_logps(*batch).clone()
        assert not eng.adapters_off
        return out

    a, b, live = run(off, True), run(zero, False), run(off, False)
    for k in a:
        assert a[k].numel() and torch.equal(a[k], b[k]), k
        assert not torch.equal(a[k], live[k]), k
    # restored on an exception as well, and no backward under it
    with pytest.raises(KeyError):
        with off.disable_adapter():
            raise KeyError("x")
    assert not off.engine.adapters_off
    with off.disable_adapter():
        off.engine.forward(*batch)
        with pytest.raises(RuntimeError, match="disable_adapter"):
            off.engine.backward()
    off.engine.ctx = None


def test_batch_lookup_score_and_int8_cache(golden_dir):
    g, images = _golden(golden_dir, "toy_e2e")
    model, L = _live("toy")
    eng = model.engine
    prompts = [_prompt(g, b) for b in range(3)]
    prompts[1] = prompts[1][:-3]
    sizes = [tuple(s) for s in g["image_sizes"].tolist()]
    has = [bool((p == IMAGE_TOKEN_INDEX).any()) for p in prompts]                  # the golden's third row is text only
    imgs, szs = [images[b] if has[b] else None for b in range(3)], [sizes[b] if has[b] else None for b in range(3)]
    alone = lambda b, **kw: model.generate(torch.from_numpy(prompts[b][None]), images=[images[b]] if has[b] else None,
                                           image_sizes=[sizes[b]] if has[b] else None, max_new_tokens=8, **kw)[0].cpu()
    greedy = [alone(b) for b in range(3)]
    out = model.generate_batch([torch.from_numpy(p) for p in prompts], images=imgs, image_sizes=szs, max_new_tokens=8)
    for b in range(3):
        assert _ids(out[f"req_{b}"].generated_tokens) == _ids(greedy[b]), b
    out = model.generate_batch([torch.from_numpy(p) for p in prompts], images=imgs, image_sizes=szs, max_new_tokens=8, do_sample=True,
                               seed=21, share_prefix=True)
    for b in range(3):
        assert _ids(out[f"req_{b}"].generated_tokens) == _ids(alone(b, do_sample=True, seed=21 + b)), b
    assert torch.equal(alone(0, prompt_lookup_num_tokens=3), greedy[0])
    assert tuple(alone(0, kv_cache_dtype="int8").shape) == (8,)
    assert tuple(model.generate_beams(torch.from_numpy(prompts[0][None]), images=[images[0]], image_sizes=[sizes[0]], num_beams=2,
                                      max_new_tokens=4).shape)[0] == 1
    # score(): every token within test_score_gpu's gate of the fp32 oracle with the adapters applied; best() is the oracle's choice
    # wherever the oracle's two best sums are further apart than the candidates' bounds
    rng = np.random.default_rng(5)
    cands = [rng.integers(0, eng.vocab, n).astype(np.int64) for n in (1, 2, 5)] + [greedy[0][:4].numpy().astype(np.int64)]
    sc = model.score([torch.from_numpy(prompts[0])], [cands], images=[images[0]], image_sizes=[sizes[0]])
    Pe = _oracle_params("toy", L, SCALE, with_newline=eng.with_newline)
    sums, slack, worst = [], [], 0.0
    for c, cand in enumerate(cands):
        ref = _oracle_logits(Pe, "toy", np.concatenate([prompts[0], cand]), images[0], sizes[0], {}).float()
        rows = ref[ref.shape[0] - cand.size - 1:ref.shape[0] - 1]
        want = torch.log_softmax(rows, dim=-1)[torch.arange(cand.size), torch.from_numpy(cand)]
        bound = 2 * LOGITS_FP32_TOL * rows.abs().amax(dim=-1)
        worst = max(worst, float(((sc.token_logprobs[0][c] - want).abs() / bound).max()))
        sums.append(float(want.double().sum()))
        slack.append(float(bound.double().sum()))
    assert worst <= 1.0, worst
    order = np.argsort(sums)[::-1]
    if sums[order[0]] - slack[order[0]] > sums[order[1]] + slack[order[1]]:
        assert int(sc.best()[0]) == int(order[0])
    assert int(sc.best()[0]) == int(np.argmax([float(v) for v in sc.logprobs[0]]))


def test_training_state_is_untouched_and_adapters_are_read_live(golden_dir):
    g, images = _golden(golden_dir, "toy_e2e")
    batch = (g["input_ids"], g["attention_mask"], g["labels"], images)
    prompt = torch.from_numpy(_prompt(g, 0)[None])

    def two_steps(with_generate):
        model, _ = _live("toy", lora=dict(LORA, dropout=0.05))
        eng = model.engine
        eng.forward(*batch)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        loss = eng.forward(*batch)
        if with_generate:
            ctx, step = eng.ctx, eng.lora_step
            before = [t.clone() for t in (eng.grads, eng.m, eng.vv, eng.master, eng.lm.flat)]
            model.generate(prompt, images=[images[0]], max_new_tokens=4)
            model.generate_batch([prompt[0]], images=[images[0]], max_new_tokens=3, do_sample=True, seed=3)
            assert eng.ctx is ctx and eng.lora_step == step and eng.lora_p == 0.05 and eng.opt_step == 1
            for t0, t1 in zip(before, (eng.grads, eng.m, eng.vv, eng.master, eng.lm.flat)):
                assert torch.equal(t0, t1)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return float(loss), eng.lm.flat.clone(), eng.m.clone(), eng.vv.clone()

    a, b = two_steps(False), two_steps(True)
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    # live: after an update the cached decode follows the new adapters
    model, _ = _live("toy")
    eng = model.engine
    size = tuple(g["image_sizes"][0].tolist())
    cont = np.random.default_rng(5).integers(0, eng.vocab, N_STEPS + 1).astype(np.int64)
    before, _ = _teacher_forced(eng, prompt[0].numpy(), images[0], size, cont)
    eng.forward(*batch)
    eng.backward()
    eng.optimizer_step(lr=2e-2, weight_decay=0.0, max_grad_norm=1.0)
    after, S0 = _teacher_forced(eng, prompt[0].numpy(), images[0], size, cont)
    own = _no_cache(eng, np.concatenate([prompt[0].numpy(), cont]), images[0], size)
    assert max(_rel(after[t][0], own[S0 - 1 + t]) for t in range(len(after))) <= 1e-2
    assert not torch.equal(after[-1], before[-1])

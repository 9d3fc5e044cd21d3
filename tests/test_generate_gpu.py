"""GPU tests of KV-cached greedy generation: the cached decode against the fp32 oracle and against the engine's own no-cache forward,
free-running greedy tokens, batch semantics, stopping, the training state and save / load."""
import json
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
LOGITS_FP32_TOL = 1.5e-2          # as tests/test_e2e_gpu.py
N_CONT = 12

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


def _engine(geo, **kw):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.engine import LlavaEngine
    return LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="portable", seed=0, **kw)


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


def _oracle_cfg(kw, geo):
    return dict(mm_patch_merge_type=kw.get("merge_type", "flat"), image_aspect_ratio=kw.get("image_aspect_ratio", "square"),
                image_grid_pinpoints=kw.get("image_grid_pinpoints"), tower_image_size=GEOMETRIES[geo]["vision"]["image"])


def _oracle_logits(P, geo, ids, image, size, kw):
    from oracle import llava_oracle as O
    t = torch.from_numpy(ids[None])
    with torch.no_grad():
        _, logits, _ = O.llava_forward(P, GEOMETRIES[geo], t, torch.ones_like(t, dtype=torch.bool), torch.full_like(t, -100), [image],
                                       image_sizes=[size], cfg=_oracle_cfg(kw, geo))
    return logits[0]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("case", list(CASES))
def test_teacher_forced_decode_parity(golden_dir, case):
    from oracle import llava_oracle as O
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    eng = _engine(geo, **kw)
    prompt = _prompt(g, 0)
    cont = np.random.default_rng(5).integers(0, eng.vocab, N_CONT).astype(np.int64)
    full = np.concatenate([prompt, cont])
    cache, lg = eng.prefill(prompt[None], None, [images[0]], [sizes[0]], max_new_tokens=N_CONT)
    steps = [lg.cpu()]
    for t in range(N_CONT - 1):
        steps.append(eng.decode_step(cache, [int(cont[t])]).cpu())
    S0 = int(cache.lens[0]) - (N_CONT - 1)                               # spliced prompt length
    P = O.make_params(GEOMETRIES[geo], seed=0, with_newline=eng.with_newline)
    ref = _oracle_logits(P, geo, full, images[0], sizes[0], kw)
    eng.forward(full[None], np.ones((1, full.size), dtype=bool), np.full((1, full.size), -100), [images[0]], image_sizes=[sizes[0]],
                want_logits=True)
    own = eng.last_logits[0].cpu()
    eng.ctx = None
    assert ref.shape[0] == own.shape[0] == S0 + N_CONT
    e32 = [_rel(steps[t][0], ref[S0 - 1 + t]) for t in range(N_CONT)]
    eown = [_rel(steps[t][0], own[S0 - 1 + t]) for t in range(N_CONT)]
    from conftest import record_measurement
    record_measurement("generate_teacher_forced", case=case, max_rel_vs_fp32=max(e32), max_rel_vs_nocache=max(eown))
    assert max(e32) <= LOGITS_FP32_TOL, e32
    assert max(eown) <= 1e-2, eown


def _oracle_greedy_check(P, geo, prompt, image, size, kw, got, n):
    """got (the engine's generated tokens) equals the oracle's greedy loop up to the first step whose top-1 / top-2 margin is below
    3 x LOGITS_FP32_TOL x max|logit| (there a bf16 rounding may legitimately pick the other token).  Returns the steps compared."""
    ids = prompt.copy()
    for t in range(n):
        lg = _oracle_logits(P, geo, ids, image, size, kw)[-1]
        top = torch.topk(lg, 2)
        if float(top.values[0] - top.values[1]) < 3 * LOGITS_FP32_TOL * float(lg.abs().max()):
            return t
        assert int(got[t]) == int(top.indices[0]), (t, int(got[t]), int(top.indices[0]))
        ids = np.concatenate([ids, [int(top.indices[0])]])
    return n


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_free_running_greedy_matches_oracle(golden_dir, case):
    from oracle import llava_oracle as O
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    model = _model(geo, kw)
    prompt = _prompt(g, 0)
    out = model.generate(torch.from_numpy(prompt[None]), images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=N_CONT)
    assert out.dtype == torch.int64 and tuple(out.shape) == (1, N_CONT)
    P = O.make_params(GEOMETRIES[geo], seed=0, with_newline=model.engine.with_newline)
    n = _oracle_greedy_check(P, geo, prompt, images[0], sizes[0], kw, out[0].cpu(), N_CONT)
    from conftest import record_measurement
    record_measurement("generate_free_running", case=case, steps_compared=n)
    assert n >= 1


def _pad_batch(prompts, side):
    T = max(p.size for p in prompts)
    ids = np.zeros((len(prompts), T), dtype=np.int64)
    am = np.zeros((len(prompts), T), dtype=bool)
    for b, p in enumerate(prompts):
        sl = slice(T - p.size, T) if side == "left" else slice(0, p.size)
        ids[b, sl], am[b, sl] = p, True
    return torch.from_numpy(ids), torch.from_numpy(am)


@pytest.mark.parametrize("side", ["right", "left"])
def test_batch_rows_generate_as_if_alone(golden_dir, side):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    prompts = [_prompt(g, b) for b in range(3)]
    prompts[1] = prompts[1][:-3]                                  # lengths differ in any case
    ids, am = _pad_batch(prompts, side)
    out = model.generate(ids, images=images[:3], image_sizes=sizes[:3], attention_mask=am, max_new_tokens=N_CONT, output_scores=True,
                         return_dict_in_generate=True)
    assert tuple(out.sequences.shape) == (3, N_CONT) and len(out.scores) == N_CONT
    for b in range(3):
        one = model.generate(torch.from_numpy(prompts[b][None]), images=[images[b]], image_sizes=[sizes[b]], max_new_tokens=N_CONT,
                             output_scores=True, return_dict_in_generate=True)
        for t in range(N_CONT):
            sb, s1 = out.scores[t][b].cpu(), one.scores[t][0].cpu()
            assert _rel(sb, s1) <= 1e-2, (b, t, _rel(sb, s1))
            top = torch.topk(s1, 2).values
            if float(top[0] - top[1]) < 3 * LOGITS_FP32_TOL * float(s1.abs().max()):
                break                                              # a near tie: the rest of the row may differ legitimately
            assert int(out.sequences[b, t]) == int(one.sequences[0, t]), (b, t)


def test_stopping_eos_max_new_tokens_and_criteria(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    ids, am = _pad_batch([_prompt(g, 0), _prompt(g, 1)], "left")
    args = dict(images=images[:2], image_sizes=sizes[:2], attention_mask=am)
    free = model.generate(ids, max_new_tokens=8, **args).cpu()
    assert tuple(free.shape) == (2, 8)
    assert tuple(model.generate(ids, max_new_tokens=3, **args).shape) == (2, 3)
    eos, pad = int(free[0, 2]), 999
    out = model.generate(ids, max_new_tokens=8, eos_token_id=[eos], pad_token_id=pad, **args).cpu()
    for b in range(2):
        hit = (free[b] == eos).nonzero()
        stop = int(hit[0]) if hit.numel() else None
        row = out[b]
        if stop is None:
            assert torch.equal(row, free[b, :row.numel()])
        else:
            assert torch.equal(row[:stop + 1], free[b, :stop + 1])
            assert (row[stop + 1:] == pad).all()
    firsts = [int((free[b] == eos).nonzero()[0]) if (free[b] == eos).any() else 7 for b in range(2)]
    assert out.shape[1] == max(firsts) + 1
    seen = []

    def crit(ids_so_far, scores):
        seen.append((tuple(ids_so_far.shape), tuple(scores.shape)))
        return ids_so_far.shape[1] >= 3

    out = model.generate(ids, max_new_tokens=8, stopping_criteria=[crit], **args)
    assert tuple(out.shape) == (2, 3) and seen[0] == ((2, 1), (2, model.engine.vocab))
    assert torch.equal(out.cpu(), free[:, :3])
    per_row = model.generate(ids, max_new_tokens=8, stopping_criteria=[lambda i, s: torch.tensor([True, i.shape[1] >= 2])],
                             pad_token_id=pad, eos_token_id=None, **args).cpu()
    assert tuple(per_row.shape) == (2, 2)
    for bad in (dict(do_sample=True), dict(num_beams=2), dict(streamer=object()), dict(inputs_embeds=torch.zeros(1, 2, 256))):
        with pytest.raises(NotImplementedError):
            model.generate(ids, **bad, **args)


def test_generate_leaves_training_state_unchanged(golden_dir):
    """A training step after generate() is bit-identical to the same step without it."""
    g, images, sizes, kw = _load(golden_dir, "toy")

    def step(with_generate):
        eng = _engine("toy")
        if with_generate:
            from radvlm_amd.generation import greedy_generate, parse_generate_kwargs
            greedy_generate(eng, g["input_ids"], g["attention_mask"], images, sizes,
                            parse_generate_kwargs(dict(max_new_tokens=6, attention_mask=g["attention_mask"])))
        loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        eng.backward()
        eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return float(loss), eng.lm.flat.clone(), eng.grads.clone(), eng.lora_step

    a, b = step(False), step(True)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]


def test_save_load_generate_roundtrip(golden_dir, tmp_path):
    from radvlm_amd.llava.model.builder import load_pretrained_model
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    prompt = torch.from_numpy(_prompt(g, 0)[None])
    want = model.generate(prompt, images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=6)
    model.save_pretrained(str(tmp_path / "ckpt"))
    tok, loaded, proc, ctx_len = load_pretrained_model(str(tmp_path / "ckpt"), device="cuda:0")
    assert tok is None and type(loaded).__name__ == "LlavaQwenForCausalLM" and ctx_len > 0
    got = loaded.generate(prompt, images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=6)
    assert torch.equal(got, want)

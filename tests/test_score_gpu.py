"""GPU tests of model.score() on the toy goldens: per-token log-probs against the fp32 oracle, one prompt pass for many candidates, equal
prompts prefilled once, the quantised decoders, the tail cache's bytes, refusals, and generate() unchanged by a score() call."""
import json
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
LOGITS_FP32_TOL = 1.5e-2          # as tests/test_e2e_gpu.py
CAND_LENS = (1, 2, 7, 12)

CASES = {
    "toy": dict(golden="toy_e2e", geo="toy"),
    "toy_qwen": dict(golden="toy_qwen_e2e", geo="toy_qwen"),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _load(golden_dir, case):
    g = np.load(os.path.join(golden_dir, CASES[case]["golden"] + ".npz"))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
    sizes = [tuple(s) for s in g["image_sizes"].tolist()]
    return g, images, sizes


def _model(geo, lora=None):
    _need_gpu()
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0),
                 mm_patch_merge_type="flat", image_aspect_ratio="square", image_grid_pinpoints=None, lora=lora)
    return Model(cfg, device="cuda:0", init="portable", seed=0).eval()


def _prompt(g, b):
    return g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)


def _oracle_logits(P, geo, ids, image, size):
    from oracle import llava_oracle as O
    t = torch.from_numpy(ids[None])
    cfg = dict(mm_patch_merge_type="flat", image_aspect_ratio="square", image_grid_pinpoints=None,
               tower_image_size=GEOMETRIES[geo]["vision"]["image"])
    with torch.no_grad():
        _, logits, _ = O.llava_forward(P, GEOMETRIES[geo], t, torch.ones_like(t, dtype=torch.bool), torch.full_like(t, -100), [image],
                                       image_sizes=[size], cfg=cfg)
    return logits[0].float()


def _candidates(vocab):
    rng = np.random.default_rng(5)
    return [[rng.integers(0, vocab, n).astype(np.int64) for n in CAND_LENS] for _ in range(2)]


def _request(golden_dir, case):
    g, images, sizes = _load(golden_dir, case)
    prompts = [torch.from_numpy(_prompt(g, b)) for b in range(2)]
    return g, prompts, [images[0], images[1]], [sizes[0], sizes[1]]


@pytest.mark.parametrize("case", list(CASES))
def test_score_matches_the_fp32_oracle(golden_dir, case):
    from oracle import llava_oracle as O
    geo = CASES[case]["geo"]
    model = _model(geo)
    g, prompts, images, sizes = _request(golden_dir, case)
    cands = _candidates(model.engine.vocab)
    P = O.make_params(GEOMETRIES[geo], seed=0, with_newline=model.engine.with_newline)
    # the greedy candidate: the engine's own tokens up to the first near tie; the unlikely one: the oracle's least likely first token
    gen = model.generate(prompts[0][None], images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=6)[0].cpu().numpy()
    ids, n_greedy = prompts[0].numpy().copy(), 0
    for t in range(gen.size):
        lg = _oracle_logits(P, geo, ids, images[0], sizes[0])[-1]
        if t == 0:
            unlikely = np.array([int(lg.argmin())], dtype=np.int64)
        top = torch.topk(lg, 2)
        if float(top.values[0] - top.values[1]) < 3 * LOGITS_FP32_TOL * float(lg.abs().max()):
            break
        assert int(gen[t]) == int(top.indices[0])
        ids = np.concatenate([ids, [int(gen[t])]])
        n_greedy = t + 1
    assert n_greedy >= 1
    cands[0] = cands[0] + [gen[:n_greedy].astype(np.int64), unlikely]
    out = model.score(prompts, cands, images=images, image_sizes=sizes)
    worst = 0.0
    for i in range(2):
        assert out.logprobs[i].dtype == torch.float64 and out.is_greedy[i].dtype == torch.bool
        for c, cand in enumerate(cands[i]):
            got = out.token_logprobs[i][c]
            assert got.dtype == torch.float32 and got.device.type == "cpu" and tuple(got.shape) == (cand.size,)
            full = np.concatenate([prompts[i].numpy(), cand])
            ref = _oracle_logits(P, geo, full, images[i], sizes[i])
            rows = ref[ref.shape[0] - cand.size - 1:ref.shape[0] - 1]                 # the rows that predict the candidate's tokens
            want = torch.log_softmax(rows, dim=-1)[torch.arange(cand.size), torch.from_numpy(cand)]
            bound = 2 * LOGITS_FP32_TOL * rows.abs().amax(dim=-1)
            ratio = float(((got - want).abs() / bound).max())
            print(f"score_vs_fp32 {case} prompt {i} candidate {c} ({cand.size} tokens): max |lp - ref| / bound = {ratio:.4f}")
            worst = max(worst, ratio)
            s = 0.0
            for v in got.tolist():
                s += v
            assert float(out.logprobs[i][c]) == s                                     # the fp64 sum of the fp32 values, in token order
    from conftest import record_measurement
    record_measurement("score_vs_fp32", case=case, max_ratio_to_bound=worst)
    assert worst <= 1.0, worst
    assert bool(out.is_greedy[0][len(CAND_LENS)]) and not bool(out.is_greedy[0][len(CAND_LENS) + 1])
    assert out.best().shape == (2,) and out.best(length_normalized=True).shape == (2,)


@pytest.mark.parametrize("case", list(CASES))
def test_one_prompt_pass_for_all_candidates(golden_dir, case, monkeypatch):
    from radvlm_amd import ops
    model = _model(CASES[case]["geo"])
    eng = model.engine
    g, prompts, images, sizes = _request(golden_dir, case)
    cands = _candidates(eng.vocab)
    seen = dict(prefill=[], encode=[], prefix=[], extend=[], decode=[])
    real_prefill, real_encode = eng.prefill, eng.encode_images
    monkeypatch.setattr(eng, "prefill", lambda ids, *a, **k: (seen["prefill"].append(np.asarray(ids).shape[0]), real_prefill(ids, *a, **k))[1])
    monkeypatch.setattr(eng, "encode_images", lambda px, *a, **k: (seen["encode"].append(len(px)), real_encode(px, *a, **k))[1])
    for key, name in (("prefix", "attn_extend_prefix"), ("extend", "attn_extend"), ("decode", "attn_decode")):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda q, *a, _r=real, _k=key, **k: (seen[_k].append(q.shape[0]), _r(q, *a, **k))[1])
    out = model.score(prompts, cands, images=images, image_sizes=sizes)
    assert seen["prefill"] == [2] and seen["encode"] == [2]                            # both prompts, once
    rows = sum(n - 1 for n in CAND_LENS) * 2
    assert seen["prefix"] == [rows] * eng.l["layers"]                                  # one launch: `layers` calls of the packed rows
    assert not seen["extend"] and not seen["decode"]
    assert [len(r) for r in out.token_logprobs] == [4, 4]

    # two requests with the same prompt and image are prefilled as one, and score the same
    for v in seen.values():
        v.clear()
    twice = model.score([prompts[0], prompts[1], prompts[0].clone()], [cands[0], cands[1], cands[0]],
                        images=[images[0], images[1], images[0].clone()], image_sizes=[sizes[0], sizes[1], sizes[0]])
    assert seen["prefill"] == [2] and seen["encode"] == [2]
    for c in range(4):
        assert torch.equal(twice.token_logprobs[0][c], twice.token_logprobs[2][c])
        assert torch.equal(twice.token_logprobs[0][c], out.token_logprobs[0][c])
        assert torch.equal(twice.token_logprobs[1][c], out.token_logprobs[1][c])


@pytest.mark.parametrize("fmt", ["int8", "mxfp4"])
def test_quantised_decoders_score_as_score_tails_by_hand(golden_dir, fmt):
    from radvlm_amd import scoring
    model = _model("toy_qwen")
    eng = model.engine
    g, prompts, images, sizes = _request(golden_dir, "toy_qwen")
    cands = _candidates(eng.vocab)
    model.quantize_decoder_(fmt) if fmt != "int8" else model.quantize_decoder_()
    assert model.is_quantized
    out = model.score(prompts[:1], cands[:1], images=images[:1], image_sizes=sizes[:1])
    ids = prompts[0].numpy()[None]
    prefix, logits = eng.prefill(ids, np.ones(ids.shape, dtype=bool), [images[0]], [sizes[0]])
    lp, am = eng.score_tails(prefix, [0] * len(CAND_LENS), cands[0], logits)
    arr = scoring.launch_arrays([0] * len(CAND_LENS), [int(prefix.lens[0])] * len(CAND_LENS), cands[0])
    lp, am = lp.cpu(), am.cpu()
    assert torch.isfinite(lp).all()
    for c, cand in enumerate(cands[0]):
        a, b = int(arr.offsets[c]), int(arr.offsets[c + 1])
        assert torch.equal(out.token_logprobs[0][c].view(torch.int32), lp[a:b].view(torch.int32))
        assert bool(out.is_greedy[0][c]) == bool((am[a:b] == torch.from_numpy(cand)).all())


def test_tail_cache_bytes_and_no_copy_of_the_prompt(golden_dir, monkeypatch):
    from radvlm_amd import scoring
    model = _model("toy_qwen")
    eng = model.engine
    g, prompts, images, sizes = _request(golden_dir, "toy_qwen")
    cands = _candidates(eng.vocab)
    plans, tails = [], []
    real_plan, real_tails = scoring.plan_group, eng.score_tails
    monkeypatch.setattr(scoring, "plan_group", lambda *a, **k: (plans.append(real_plan(*a, **k)), plans[-1])[1])

    def spy(prefix, prefix_row, tl, logits, arrays=None):
        tails.append((prefix.B, prefix.L_max, len(tl), arrays.T_max))
        return real_tails(prefix, prefix_row, tl, logits, arrays=arrays)

    monkeypatch.setattr(eng, "score_tails", spy)
    model.score(prompts, cands, images=images, image_sizes=sizes)
    assert len(plans) == 1 and len(tails) == 1
    n_cand, T_max = 2 * len(CAND_LENS), max(CAND_LENS) - 1
    assert plans[0].tail_cache_bytes == eng.l["layers"] * n_cand * T_max * 2 * eng.kvd * 2
    assert plans[0].prefix_rows == 2                                                   # the prefix cache: one row per prompt, not per candidate
    assert tails[0] == (2, plans[0].P_max, n_cand, T_max)


def test_refusals(golden_dir):
    model = _model("toy")
    g, prompts, images, sizes = _request(golden_dir, "toy")
    V = model.engine.vocab
    ok = [[np.array([1, 2])], [np.array([3])]]
    kw = dict(images=images, image_sizes=sizes)
    with pytest.raises(ValueError):
        model.score(prompts, [[np.array([1, V])], [np.array([3])]], **kw)
    with pytest.raises(ValueError):
        model.score(prompts, [[np.array([-200])], [np.array([3])]], **kw)              # an image placeholder in a candidate
    with pytest.raises(ValueError):
        model.score(prompts, [[np.array([], dtype=np.int64)], [np.array([3])]], **kw)
    with pytest.raises(ValueError):
        model.score(prompts, [[], [np.array([3])]], **kw)
    with pytest.raises(ValueError):
        model.score(prompts, ok[:1], **kw)
    with pytest.raises(ValueError):
        model.score([prompts[0], prompts[1][:0]], ok, **kw)                            # an empty prompt
    with pytest.raises(ValueError):
        model.score(prompts, ok, images=images[:1], image_sizes=sizes)
    with pytest.raises(TypeError):
        model.score(prompts, ok, temperature=0.7, **kw)
    with pytest.raises(TypeError):
        model.score(prompts, ok, kv_cache_dtype="int8", **kw)
    prefix = model.engine.new_kv_cache(1, 8, "int8")
    with pytest.raises(NotImplementedError):
        model.engine.score_tails(prefix, [0], [np.array([1, 2])], torch.zeros(1, V, device="cuda"))
    lora = _model("toy", lora=dict(r=8, alpha=16, dropout=0.0))
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        lora.score(prompts, ok, **kw)


def test_generate_is_unchanged_by_a_score_call(golden_dir):
    model = _model("toy_qwen")
    eng = model.engine
    g, prompts, images, sizes = _request(golden_dir, "toy_qwen")
    gen = lambda: model.generate(prompts[0][None], images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=8)
    before = gen()
    flat = eng.lm.flat.clone()
    model.score(prompts, _candidates(eng.vocab), images=images, image_sizes=sizes)
    assert eng.ctx is None and torch.equal(eng.lm.flat, flat)
    assert torch.equal(before, gen())

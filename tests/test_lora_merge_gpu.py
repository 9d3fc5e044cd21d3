"""GPU tests of the LoRA merge: the rv_lora_merge_bf16 contract, merge_and_unload() on a live LoRA model against the fp32 oracle's
apply_lora, the file round trip through load_pretrained_model(model_path, model_base=...), the projector-only branch, and training
after a merge (projector-only semantics)."""
import json
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
LOGITS_FP32_TOL = 1.5e-2          # as tests/test_e2e_gpu.py
N_CONT = 8
PROJ = ("model.mm_projector.0.weight", "model.mm_projector.0.bias", "model.mm_projector.2.weight", "model.mm_projector.2.bias")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ulp_check(got, W0, B, A, scale):
    """got (bf16) against bf16(W0 + scale * B @ A in fp64): every element within 1 bf16 ulp of the result -- or, where W and the update
    cancel, within 1/256 bf16 ulp of the operands' magnitude |W| + scale * sum_j |B_nj A_jk| (the reach of any fp32 sum there).
    Returns the bit-exact share."""
    ref64 = W0.double() + scale * (B.double() @ A.double())
    ref = ref64.to(torch.bfloat16)
    g, r = got.float().cpu(), ref.float()
    mag = torch.maximum(g.abs(), r.abs())
    _, e = torch.frexp(mag)
    ulp = torch.ldexp(torch.ones_like(mag), e - 8).clamp_min(2.0 ** -133)
    operands = (W0.double().abs() + scale * (B.double().abs() @ A.double().abs())).float()
    tol = torch.maximum(ulp, operands * 2.0 ** -16)
    assert bool(((g - r).abs() <= tol).all()), float(((g - r).abs() / tol).max())
    return float((got.cpu().view(torch.int16) == ref.view(torch.int16)).float().mean())


def _greedy_rows(P, geo, model, g, images, n_rows=3):
    """The margin rule of test_generate_gpu over the first golden prompts: a row whose first step is a near tie compares no step, so
    the test needs at least one compared step over the rows.  Returns the steps compared."""
    from test_generate_gpu import _oracle_greedy_check
    total = 0
    for b in range(min(n_rows, g["input_ids"].shape[0])):
        prompt = _prompt(g, b)
        size = tuple(g["image_sizes"][b].tolist())
        out = model.generate(torch.from_numpy(prompt[None]), images=[images[b]], image_sizes=[size], max_new_tokens=N_CONT)
        total += _oracle_greedy_check(P, geo, prompt, images[b], size, {}, out[0].cpu(), N_CONT)
    return total


# ------------------------------------------------------------------------------------------------ kernel contract
@pytest.mark.parametrize("r", [1, 8, 64, 128, 256])
def test_kernel_contract(r):
    _need_gpu()
    from radvlm_amd import ops
    g = torch.Generator().manual_seed(r)
    N, K, pad_rows, pad_cols = 200, 328, 24, 16           # odd multiples of 8; W is a row AND column slice of a wider store
    store = (torch.randn(N + 2 * pad_rows, K + pad_cols, generator=g) * 0.02).to(torch.bfloat16)
    A = (torch.randn(r, K, generator=g) * 0.05).to(torch.bfloat16)
    B = (torch.randn(N, r, generator=g) * 0.05).to(torch.bfloat16)
    s = 0.37
    dev = store.cuda()
    Ad, Bd = A.cuda(), B.cuda()
    W = dev[pad_rows:pad_rows + N, 8:8 + K]                 # ldw = K + 16, 16-byte aligned
    assert W.stride(0) == K + pad_cols
    ops.lora_merge(W, Ad, Bd, s)
    torch.cuda.synchronize()
    out = dev.cpu()
    exact = _ulp_check(out[pad_rows:pad_rows + N, 8:8 + K], store[pad_rows:pad_rows + N, 8:8 + K].float(), B.float(), A.float(), s)
    assert exact >= 0.99, exact
    inside = torch.zeros_like(store, dtype=torch.bool)
    inside[pad_rows:pad_rows + N, 8:8 + K] = True
    assert torch.equal(out.view(torch.int16)[~inside], store.view(torch.int16)[~inside])      # nothing outside the slice moves
    again = store.cuda()
    ops.lora_merge(again[pad_rows:pad_rows + N, 8:8 + K], Ad, Bd, s)
    assert torch.equal(again.cpu().view(torch.int16), out.view(torch.int16))                   # two launches, same bits
    # another grid (the whole store, zero adapter rows outside the slice): the slice's bits do not change
    whole = store.cuda()
    Bw = torch.zeros(N + 2 * pad_rows, r, dtype=torch.bfloat16, device="cuda")
    Bw[pad_rows:pad_rows + N] = Bd
    Aw = torch.zeros(r, K + pad_cols, dtype=torch.bfloat16, device="cuda")
    Aw[:, 8:8 + K] = Ad
    ops.lora_merge(whole, Aw, Bw, s)
    assert torch.equal(whole.cpu().view(torch.int16), out.view(torch.int16))
    from conftest import record_measurement
    record_measurement("lora_merge_kernel", r=r, bit_exact_share=exact)


def test_kernel_refuses_host_tensors_and_bad_shapes():
    _need_gpu()
    from radvlm_amd import lib, ops
    W = torch.zeros(16, 64, dtype=torch.bfloat16)
    with pytest.raises(AssertionError):
        ops.lora_merge(W, torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(16, 4, dtype=torch.bfloat16), 1.0)
    Wd = torch.zeros(16, 64, dtype=torch.bfloat16, device="cuda")
    A, B = torch.zeros(300, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(16, 300, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(lib.RadvlmHipError):          # r > 256
        ops.lora_merge(Wd, A, B, 1.0)
    with pytest.raises(lib.RadvlmHipError):          # K % 8 != 0
        ops.lora_merge(Wd[:, :60], A[:4, :60].contiguous(), B[:, :4].contiguous(), 1.0)


# ------------------------------------------------------------------------------------------------ live LoRA model
def _golden(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    return g, [torch.from_numpy(g[f"image{i}"]) for i in range(n)]


def _model(geo, lora=None, seed=0):
    _need_gpu()
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0), lora=lora)
    return Model(cfg, device="cuda:0", init="portable", seed=seed).eval()


def _set_adapters(eng, only=None):
    """Non-zero adapters (peft starts lora_B at zero) from the portable generator; modules outside `only` keep B = 0."""
    from radvlm_amd import portable_rng as prng
    L = {}
    for n in eng.lm.names():
        if ".lora_" in n:
            w = torch.from_numpy(prng.normal(3, prng.name_tag(n), eng.lm.shapes[n], 0.05)).to(torch.bfloat16)
            if only is not None and n.endswith("lora_B.weight") and not any(f".{m}." in n for m in only):
                w.zero_()
            eng.lm.view(n).copy_(w)
            L[n] = w.float()
    return L


def _oracle_params(geo, L, scale, with_newline=False):
    from oracle import llava_oracle as O
    P = O.make_params(GEOMETRIES[geo], seed=0, with_newline=with_newline)
    P = {k: v.to(torch.bfloat16).float() for k, v in P.items()}
    return O.apply_lora(P, L, GEOMETRIES[geo], scale) if L else P


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _prompt(g, b):
    return g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)


@pytest.mark.parametrize("geo,golden", [("toy", "toy_e2e"), ("toy_qwen", "toy_qwen_e2e")])
def test_merge_and_unload_live_model(golden_dir, geo, golden):
    from oracle import llava_oracle as O
    from radvlm_amd.params import LORA_TARGETS
    g, images = _golden(golden_dir, golden)
    model = _model(geo, lora=dict(r=8, alpha=16, dropout=0.0))
    eng = model.engine
    L = _set_adapters(eng)
    s = 16 / 8
    base0, vis0 = eng.base.flat.clone(), eng.vis.flat.clone()
    keep0 = {n: eng.lm.view(n).clone() for n in eng.lm.names() if ".lora_" not in n}
    lora_grads = eng.grads.numel()
    ids, am, lab = g["input_ids"], g["attention_mask"], g["labels"]
    eng.forward(ids, am, lab, images, want_logits=True)             # the unmerged adapters' eval forward (dropout 0)
    unmerged = eng.last_logits.cpu()
    eng.ctx = None
    assert model.merge_and_unload() is model
    assert eng.lora is None and model.config.lora is None
    assert not [n for n in eng.lm.names() if ".lora_" in n] and eng.grads.numel() == eng.lm.numel < lora_grads
    # merged weights: the kernel contract; every other tensor bit-identical
    adapted = set()
    shares = []
    for i in range(eng.l["layers"]):
        for t, _, _ in LORA_TARGETS:
            n = f"model.layers.{i}.{t}."
            off, cnt = eng.base.offsets[n + "weight"]
            adapted.add(n + "weight")
            W0 = base0[off:off + cnt].view(eng.base.shapes[n + "weight"]).float().cpu()
            shares.append(_ulp_check(eng.base.view(n + "weight"), W0, L[n + "lora_B.weight"], L[n + "lora_A.weight"], s))
    assert min(shares) >= 0.99, shares
    for n in eng.base.names():
        if n not in adapted:
            off, cnt = eng.base.offsets[n]
            assert torch.equal(eng.base.view(n).reshape(-1), base0[off:off + cnt]), n
    assert torch.equal(eng.vis.flat, vis0)
    for n, t in keep0.items():
        assert torch.equal(eng.lm.view(n), t), n
    # eval forward: the oracle with the adapters applied in fp32, and the unmerged engine
    Pe = _oracle_params(geo, L, s, with_newline=eng.with_newline)
    eng.forward(ids, am, lab, images, want_logits=True)
    merged = eng.last_logits.cpu()
    eng.ctx = None
    with torch.no_grad():
        _, rlog, _ = O.llava_forward(Pe, GEOMETRIES[geo], torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(lab), images)
    m = torch.from_numpy(g["splice_attention_mask"])
    e_or, e_un = _rel(merged[m], rlog[m]), _rel(merged[m], unmerged[m])
    # teacher-forced decode with the merged weights against the oracle
    prompt = _prompt(g, 0)
    size = tuple(g["image_sizes"][0].tolist())
    cont = np.random.default_rng(5).integers(0, eng.vocab, N_CONT).astype(np.int64)
    cache, lg = eng.prefill(prompt[None], None, [images[0]], [size], max_new_tokens=N_CONT)
    steps = [lg.cpu()]
    for t in range(N_CONT - 1):
        steps.append(eng.decode_step(cache, [int(cont[t])]).cpu())
    S0 = int(cache.lens[0]) - (N_CONT - 1)
    from test_generate_gpu import _oracle_logits
    ref = _oracle_logits(Pe, geo, np.concatenate([prompt, cont]), images[0], size, {})
    e_tf = max(_rel(steps[t][0], ref[S0 - 1 + t]) for t in range(N_CONT))
    # free-running greedy, margin rule of test_generate_gpu
    n_cmp = _greedy_rows(Pe, geo, model, g, images)
    from conftest import record_measurement
    record_measurement("lora_merge_live", geo=geo, rel_vs_fp32=e_or, rel_vs_unmerged=e_un, teacher_forced_rel=e_tf, greedy_steps=n_cmp,
                       min_bit_exact_share=min(shares))
    assert e_or <= LOGITS_FP32_TOL, e_or
    assert e_un <= LOGITS_FP32_TOL, e_un
    assert e_tf <= LOGITS_FP32_TOL, e_tf
    assert n_cmp >= 1


def test_unmerged_lora_generate_still_refused(golden_dir):
    g, images = _golden(golden_dir, "toy_e2e")
    model = _model("toy", lora=dict(r=8, alpha=16, dropout=0.0))
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        model.generate(torch.from_numpy(_prompt(g, 0)[None]), images=[images[0]], max_new_tokens=2)
    with pytest.raises(ValueError):
        _model("toy").merge_and_unload()


def test_training_after_merge_is_projector_only(golden_dir):
    """A step after merge_and_unload() trains the projector alone and equals the same step of a projector-only (freeze_lm) engine
    holding the merged weights, bit for bit."""
    from radvlm_amd.engine import LlavaEngine
    g, images = _golden(golden_dir, "toy_e2e")
    model = _model("toy", lora=dict(r=8, alpha=16, dropout=0.0))
    _set_adapters(model.engine)
    eng = model.merge_and_unload().engine
    ref = LlavaEngine(GEOMETRIES["toy"], device="cuda:0", init="fast", seed=3, freeze_lm=True)
    missing, unexpected = ref.load_state_dict(eng.state_dict())
    assert not missing and not unexpected
    base0, proj0 = eng.base.flat.clone(), eng.W("model.mm_projector.0.weight").clone()
    out = []
    for e in (eng, ref):
        loss = e.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        e.backward()
        e.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        out.append((float(loss), e.lm.flat.clone()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])
    assert torch.equal(eng.base.flat, base0)
    assert not torch.equal(eng.W("model.mm_projector.0.weight"), proj0)


# ------------------------------------------------------------------------------------------------ files
@pytest.mark.parametrize("geo,golden,only", [("toy_qwen", "toy_qwen_e2e", None), ("toy", "toy_e2e", ("q_proj", "v_proj"))])
def test_roundtrip_through_files(golden_dir, tmp_path, geo, golden, only):
    from radvlm_amd.llava.model.builder import load_pretrained_model
    g, images = _golden(golden_dir, golden)
    prompt = torch.from_numpy(_prompt(g, 0)[None])
    size = tuple(g["image_sizes"][0].tolist())
    gen = lambda m: m.generate(prompt, images=[images[0]], image_sizes=[size], max_new_tokens=N_CONT).cpu()
    base_dir, lora_dir, merged_dir = (str(tmp_path / n) for n in ("base", "lora", "merged"))
    _model(geo).save_pretrained(base_dir)
    lm = _model(geo, lora=dict(r=8, alpha=16, dropout=0.0))
    _set_adapters(lm.engine, only=only)
    lm.engine.W("model.mm_projector.2.bias").add_(0.5)              # a trained projector: non_lora_trainables.bin must be loaded
    lm.save_pretrained(lora_dir)
    if only:     # a q/v-only adapter as peft writes it: only those modules in the file and in target_modules
        ad = torch.load(os.path.join(lora_dir, "adapter_model.bin"), weights_only=True)
        torch.save({k: v for k, v in ad.items() if any(f".{m}." in k for m in only)}, os.path.join(lora_dir, "adapter_model.bin"))
        with open(os.path.join(lora_dir, "adapter_config.json")) as f:
            ac = json.load(f)
        ac["target_modules"] = list(only)
        with open(os.path.join(lora_dir, "adapter_config.json"), "w") as f:
            json.dump(ac, f)
    want = gen(lm.merge_and_unload())
    _, loaded, _, _ = load_pretrained_model(lora_dir, model_base=base_dir, device="cuda:0")
    assert loaded.engine.lora is None
    got = gen(loaded)
    assert torch.equal(got, want)
    sd_a, sd_b = lm.state_dict(), loaded.state_dict()
    assert set(sd_a) == set(sd_b)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    loaded.save_pretrained(merged_dir)
    assert "model.safetensors" in os.listdir(merged_dir) and "adapter_model.bin" not in os.listdir(merged_dir)
    _, again, _, _ = load_pretrained_model(merged_dir, device="cuda:0")
    assert torch.equal(gen(again), want)
    from tools.merge_lora import main as merge_main
    tool_dir = str(tmp_path / "tool")
    merge_main(["--model-path", lora_dir, "--model-base", base_dir, "--save-model-path", tool_dir, "--device", "cuda:0"])
    _, viatool, _, _ = load_pretrained_model(tool_dir, device="cuda:0")
    assert torch.equal(gen(viatool), want)


def test_projector_only_checkpoint(golden_dir, tmp_path):
    from radvlm_amd.llava.model.builder import load_pretrained_model
    g, images = _golden(golden_dir, "toy_e2e")
    base = _model("toy")
    base_dir, run_dir = str(tmp_path / "base"), str(tmp_path / "run")
    base.save_pretrained(base_dir)
    gen = torch.Generator().manual_seed(11)
    proj = {k: (base.state_dict()[k].float().cpu() + 0.02 * torch.randn(base.state_dict()[k].shape, generator=gen)).to(torch.bfloat16)
            for k in PROJ}
    base.save_config(run_dir)
    torch.save(proj, os.path.join(run_dir, "mm_projector.bin"))
    _, model, _, _ = load_pretrained_model(run_dir, model_base=base_dir, device="cuda:0")
    sd, sd0 = model.state_dict(), base.state_dict()
    for k in sd:
        assert torch.equal(sd[k].cpu(), proj[k] if k in proj else sd0[k].cpu()), k
    P = _oracle_params("toy", None, 1.0)
    P.update({k: v.float() for k, v in proj.items()})
    assert _greedy_rows(P, "toy", model, g, images) >= 1

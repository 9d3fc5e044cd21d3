"""GPU tests of the NF4 frozen base above the kernels (toy and toy_qwen, r = 16), all exact: an engine after quantize_base_() against a
plain LoRA engine loaded from its state_dict() -- losses, gradients and trainable weights bit for bit over two steps, with and without
adapter dropout, double quantisation and recompute --, what the engine stores, dequantize_base_() / merge_and_unload() / generate(),
DPO with the adapters off as reference, every refusal, and the trainer's --bits 4 run with checkpoint, resume and base_quant record."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu

CASES = {"toy": "toy_e2e", "toy_qwen": "toy_qwen_e2e"}
STEP = dict(lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)
R_LORA = 16


def _model(geo, dropout=0.0, lora=True, adapters=True):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import portable_rng as prng
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0),
                 lora=dict(r=R_LORA, alpha=16, dropout=dropout) if lora else None)
    model = Model(cfg, device="cuda:0", init="portable", seed=0).train()
    if lora and adapters:                   # non-zero adapters (peft starts lora_B at zero): every gradient is live from the first step
        eng = model.engine
        for n in eng.lm.names():
            if ".lora_" in n:
                eng.lm.view(n).copy_(torch.from_numpy(prng.normal(3, prng.name_tag(n), eng.lm.shapes[n], 0.05)).to(torch.bfloat16))
    return model


def _golden(golden_dir, geo):
    g = np.load(os.path.join(golden_dir, CASES[geo] + ".npz"))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    return g, [torch.from_numpy(g[f"image{i}"]) for i in range(n)]


def _pair(geo, dropout=0.0, dq=False):
    """A: quantize_base_(); B: a plain LoRA model loaded from A.state_dict()."""
    A = _model(geo, dropout).quantize_base_(double_quant=dq)
    B = _model(geo, dropout, adapters=False)
    missing, unexpected = B.load_state_dict(A.state_dict())
    assert not missing and not unexpected
    return A, B


def _bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("dq", [False, True])
@pytest.mark.parametrize("dropout", [0.05, 0.0])
@pytest.mark.parametrize("geo", list(CASES))
def test_nf4_base_trains_bit_for_bit_like_its_dequantised_bf16_base(golden_dir, geo, dropout, dq, recompute):
    g, images = _golden(golden_dir, geo)
    A, B = _pair(geo, dropout, dq)
    for m in (A, B):
        m.engine.recompute = recompute
    a, b = A.engine, B.engine
    assert a.nf4 is not None and a.nf4["plan"].double_quant == dq and b.nf4 is None
    for step in range(2):
        la = a.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        a.backward()
        lb = b.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
        b.backward()
        assert torch.equal(_bits(la.float()), _bits(lb.float())) and np.isfinite(float(la)), (step, float(la), float(lb))
        assert torch.equal(_bits(a.grads), _bits(b.grads)) and bool(a.grads.any()), step
        a.optimizer_step(**STEP)
        b.optimizer_step(**STEP)
        assert torch.equal(_bits(a.lm.flat), _bits(b.lm.flat)) and torch.equal(a.master, b.master), step
    assert a.lora_step == b.lora_step


# ------------------------------------------------------------------------------------------------ storage
@pytest.mark.parametrize("dq", [False, True])
@pytest.mark.parametrize("geo", list(CASES))
def test_the_engine_holds_no_bf16_matrices_beyond_one_layers_scratch(geo, dq):
    from radvlm_amd import nf4 as N
    plain = _model(geo, adapters=False)
    before = plain.engine.base.flat.untyped_storage().nbytes()
    assert plain.engine.base_weight_bytes() == N.bf16_matrix_bytes(GEOMETRIES[geo])
    A = plain.quantize_base_(double_quant=dq)
    eng, plan = A.engine, N.BasePlan(GEOMETRIES[geo], dq)
    st = eng.nf4
    assert not [n for n in eng.base.names() if n in plan.tensors] and "lm_head.weight" in eng.base.offsets
    after = eng.base.flat.untyped_storage().nbytes()
    # the frozen store shrank by the matrices (up to the 128-byte alignment of its groups) ...
    assert before - 2 * plan.weights - 128 * len(plan.tensors) <= after <= before - 2 * plan.weights + 128 * len(plan.tensors)
    # ... the only bf16 home of a matrix is the one-layer scratch, which the four views share ...
    assert st["scratch"].untyped_storage().nbytes() == plan.scratch_bytes() == 2 * plan.scratch_numel
    lv = eng._layer_views(1)
    for k in ("qkv", "o", "gu", "down"):
        assert lv[k].untyped_storage().data_ptr() == st["scratch"].untyped_storage().data_ptr() and lv[k].dtype == torch.bfloat16
    assert lv["ln1"].untyped_storage().data_ptr() == eng.base.flat.untyped_storage().data_ptr()
    assert st["resident"] == 1 and eng._layer_views(1, eng.grads) == {}
    # ... and the store is what the plan says, buffer by buffer
    held = sum(st[k].untyped_storage().nbytes() for k in ("codes", "absmax", "absmax_codes", "scale2", "offset") if st[k] is not None)
    assert eng.base_weight_bytes() == plan.base_weight_bytes() == N.base_weight_bytes(GEOMETRIES[geo], "nf4", dq) == held
    assert (st["absmax"] is None) == dq and (st["absmax_codes"] is not None) == dq
    names = [n for n, _ in eng._replica_buffers()]
    assert "nf4_codes" in names and ("nf4_absmax_codes" if dq else "nf4_absmax") in names


def test_a_repeated_request_for_the_resident_layer_launches_nothing(monkeypatch):
    from radvlm_amd import ops
    A = _model("toy", adapters=False).quantize_base_()
    calls = []
    real = ops.nf4_dequant
    monkeypatch.setattr(ops, "nf4_dequant", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    eng = A.engine
    w0 = eng._layer_views(0)["o"].clone()
    eng._layer_views(0)
    assert len(calls) == 1
    w1 = eng._layer_views(1)["o"].clone()
    assert len(calls) == 2 and not torch.equal(w0, w1)
    assert torch.equal(eng._layer_views(0)["o"], w0) and len(calls) == 3
    sd = A.state_dict()
    assert torch.equal(sd["model.layers.0.self_attn.o_proj.weight"], w0) and torch.equal(sd["model.layers.1.self_attn.o_proj.weight"], w1)
    assert eng.nf4["resident"] == 0 and torch.equal(eng._layer_views(0)["o"], w0)       # state_dict() did not touch the scratch


# ------------------------------------------------------------------------------------------------ unmerging and merging
@pytest.mark.parametrize("dq", [False, True])
@pytest.mark.parametrize("geo", list(CASES))
def test_dequantize_merge_and_generate(golden_dir, geo, dq):
    g, images = _golden(golden_dir, geo)
    A, B = _pair(geo, 0.0, dq)
    C = _model(geo).quantize_base_(double_quant=dq)
    sdA, sdB = A.state_dict(), B.state_dict()
    assert sorted(sdA) == sorted(sdB)
    for k in sdA:
        assert torch.equal(_bits(sdA[k]), _bits(sdB[k])), k
    unmerged = sdB["model.layers.0.self_attn.o_proj.weight"].clone()
    A.dequantize_base_()
    assert A.engine.nf4 is None and torch.equal(_bits(A.engine.base.flat), _bits(B.engine.base.flat))
    with pytest.raises(RuntimeError, match="not quantised"):
        A.dequantize_base_()
    for m in (A, B, C):                     # C merges straight from the NF4 store: dequantize_base_() then rv_lora_merge_bf16
        m.merge_and_unload()
        assert m.engine.nf4 is None and not m.engine.lora and m.config.lora is None
    for m in (A, C):
        assert torch.equal(_bits(m.engine.base.flat), _bits(B.engine.base.flat)) and torch.equal(_bits(m.engine.lm.flat), _bits(B.engine.lm.flat))
    assert not torch.equal(B.engine.base.view("model.layers.0.self_attn.o_proj.weight"), unmerged)       # the merge did change the weights
    prompt = torch.from_numpy(g["input_ids"][0][g["attention_mask"][0].astype(bool)].astype(np.int64)[None])
    size = [tuple(g["image_sizes"][0].tolist())] if "image_sizes" in g.files else None
    gen = lambda m: m.eval().generate(prompt, images=[images[0]], image_sizes=size, max_new_tokens=6).cpu()
    want = gen(B)
    assert want.shape[1] == 6 and torch.equal(gen(C), want) and torch.equal(gen(A), want)


# ------------------------------------------------------------------------------------------------ DPO
def test_preference_loss_on_an_nf4_base_starts_at_margin_zero(golden_dir):
    """The reference is the policy with its adapters off (disable_adapter()); peft's initial adapters (B = 0) and no dropout make the
    policy that same function, so every margin is exactly 0 -- through two forward-only passes and one training pass over the scratch."""
    from test_preference_gpu import _pairs
    g, images = _golden(golden_dir, "toy")
    model = _model("toy", dropout=0.0, adapters=False).quantize_base_(double_quant=True)
    pairs = _pairs(g, model.engine.vocab)
    sizes = [tuple(s) for s in g["image_sizes"].tolist()] if "image_sizes" in g.files else None
    from radvlm_amd import preference as PF
    ids, am, lab = PF.concatenate_pairs(*[pairs[k] for k in pairs])
    P = ids.shape[0] // 2
    with model.disable_adapter():
        ref, _ = model.sequence_logps(ids, am, lab, images + images, image_sizes=None if sizes is None else sizes + sizes)
    out = model.preference_loss(**pairs, images=images, image_sizes=sizes, ref_chosen_logps=ref[:P], ref_rejected_logps=ref[P:])
    assert torch.equal(out.margins, torch.zeros_like(out.margins)) and np.isfinite(float(out.loss.detach()))
    out.loss.backward()
    assert bool(model.engine.grads.any())
    tl = model.token_logps(ids, am, lab, images + images, image_sizes=None if sizes is None else sizes + sizes)
    ll = model.label_logits(ids, am, lab, images + images, image_sizes=None if sizes is None else sizes + sizes)
    assert tl.numel() == ll.shape[0] and bool(torch.isfinite(tl).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(golden_dir):
    from types import SimpleNamespace
    from radvlm_amd.llava.train.gkd_trainer import GKDTrainer
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images = _golden(golden_dir, "toy")
    prompt = g["input_ids"][0][g["attention_mask"][0].astype(bool)].astype(np.int64)
    model = _model("toy", adapters=False).quantize_base_()
    names = r"dequantize_base_\(\).*merge_and_unload\(\)"
    for live in (False, True):              # also with decoding on the live adapters switched on
        model.enable_adapter_decoding(live)
        with pytest.raises(NotImplementedError, match=names):
            model.generate(torch.from_numpy(prompt[None]), images=[images[0]], max_new_tokens=2)
        with pytest.raises(NotImplementedError, match=names):
            model.generate_batch([prompt], images=[images[0]], max_new_tokens=2)
        with pytest.raises(NotImplementedError, match=names):
            model.generate_beams(torch.from_numpy(prompt[None]), images=[images[0]], num_beams=2, max_new_tokens=2)
        with pytest.raises(NotImplementedError, match=names):
            model.score([prompt], [[np.array([5, 6])]], images=[images[0]])
        with pytest.raises(NotImplementedError, match=names):
            model.engine.prefill(prompt[None], images=[images[0]], max_new_tokens=2)
    model.enable_adapter_decoding(False)
    with pytest.raises(RuntimeError, match="already NF4"):
        model.quantize_base_()
    with pytest.raises(ValueError, match="only 'nf4'"):
        _model("toy", adapters=False).quantize_base_("fp4")
    with pytest.raises(ValueError, match="LoRA engine"):
        _model("toy", lora=False).quantize_base_()
    w = torch.zeros(256, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="NF4 base"):
        model.load_state_dict({"model.layers.0.self_attn.o_proj.weight": w})
    model.load_state_dict({"model.norm.weight": torch.ones(256, dtype=torch.bfloat16)})        # anything that is still bf16 loads
    with pytest.raises(NotImplementedError, match="merge_and_unload"):                          # as before this format existed
        model.quantize_decoder_()
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        _model("toy", adapters=False).quantize_decoder_()
    args = SimpleNamespace(num_generations=2, per_device_train_batch_size=1, optim="adamw_torch", lmbda=0.0)
    with pytest.raises(NotImplementedError, match="NF4"):
        GRPOTrainer(model=model, args=args, train_dataset=[], reward_funcs=lambda **k: [0.0])
    with pytest.raises(NotImplementedError, match="NF4"):
        GKDTrainer(model=model, teacher_model=model, args=args, train_dataset=[])


# ------------------------------------------------------------------------------------------------ trainer
def test_bits4_run_checkpoints_resumes_and_records_the_base(tmp_path, capsys):
    from safetensors.torch import load_file
    from radvlm_amd import nf4 as N
    from radvlm_amd.llava import conversation as conv_lib
    from radvlm_amd.llava.train.train import train
    from test_train_features_gpu import Tok, _dataset, _need_gpu, _train_args
    _need_gpu()
    data = _dataset(tmp_path, n=8)
    lora = ["--geometry", "toy", "--lora_enable", "True", "--lora_r", "16", "--lora_alpha", "16", "--lora_dropout", "0.05", "--save_steps", "2",
            "--dataloader_num_workers", "0"]
    q4 = lora + ["--bits", "4", "--quant_type", "nf4", "--double_quant", "True"]
    run = lambda extra, out, steps: train(argv=_train_args(tmp_path, data, extra + ["--max_steps", str(steps), "--output_dir", str(tmp_path / out)]),
                                          tokenizer=Tok())
    try:
        full = run(q4, "a", 3)
        said = capsys.readouterr().out
        assert said.count("the frozen decoder matrices are NF4") == 1 and "GiB saved" in said
        ts = json.load(open(tmp_path / "a" / "checkpoint-2" / "trainer_state.json"))
        assert ts["base_quant"] == {"type": "nf4", "block": 64, "double_quant": True, "codebook": N.codebook_sha()}
        assert "adapter_model.bin" in os.listdir(tmp_path / "a" / "checkpoint-2") and "model.safetensors" not in os.listdir(tmp_path / "a" / "checkpoint-2")
        # the job dies after step 2; the same command resumes from checkpoint-2, quantises the same base again and takes step 3
        os.makedirs(tmp_path / "b")
        shutil.copytree(tmp_path / "a" / "checkpoint-2", tmp_path / "b" / "checkpoint-2")
        resumed = run(q4, "b", 3)
        assert [r["step"] for r in resumed["log_history"]] == [1, 2, 3]
        assert [r["loss"] for r in resumed["log_history"]] == [r["loss"] for r in full["log_history"]]
        ad, ad2 = (torch.load(tmp_path / d / "adapter_model.bin", map_location="cpu", weights_only=True) for d in ("a", "b"))
        for k in ad:
            assert torch.equal(ad[k], ad2[k]), k
        assert any(bool(v.any()) for k, v in ad.items() if "lora_B" in k)
        # another setting of the base: the adapters were fitted to other weights
        for other in (lora + ["--bits", "4", "--quant_type", "nf4", "--double_quant", "False"], lora):
            os.makedirs(tmp_path / "c", exist_ok=True)
            shutil.rmtree(tmp_path / "c")
            os.makedirs(tmp_path / "c")
            shutil.copytree(tmp_path / "a" / "checkpoint-2", tmp_path / "c" / "checkpoint-2")
            with pytest.raises(ValueError, match="double_quant"):
                run(other, "c", 3)
        # --bits 16: the checkpoint's keys are the parent's, and nothing is said about quantisation
        capsys.readouterr()
        run(lora, "d", 2)
        said = capsys.readouterr().out
        assert "NF4" not in said and "--bits" not in said
        ck = tmp_path / "d" / "checkpoint-2"
        assert sorted(json.load(open(ck / "trainer_state.json"))) == ["global_step", "log_history", "lora_step", "opt_step"]
        assert sorted(os.listdir(ck)) == ["adapter_config.json", "adapter_model.bin", "config.json", "non_lora_trainables.bin",
                                          "optimizer.safetensors", "trainer_state.json"]
        assert sorted(load_file(str(ck / "optimizer.safetensors"))) == ["exp_avg", "exp_avg_sq", "master"]
        # every other combination trains on the bf16 base and says so once
        run(lora + ["--bits", "8"], "e", 1)
        said = capsys.readouterr().out
        assert said.count("--bits 8") == 1 and "NF4" not in said
    finally:
        conv_lib.default_conversation = conv_lib.conv_templates["v1"]

"""GPU tests of the 8-bit AdamW state above the kernels (toy geometry): the engine's state_bits=8 step against an fp32-state engine whose
8-bit tensors' moments are passed through quantise -> dequantise after every step (weights bit-identical), the trainer's --optim
adamw_bnb_8bit with checkpoint / resume / cross-format resume, the unchanged default, merge_lora() and the replica buffers on an 8-bit
state, and twenty toy steps at both widths."""
import json
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu

STEP = dict(lr=1e-3, weight_decay=0.1, max_grad_norm=1.0)


def _engine(name="toy", **kw):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.engine import LlavaEngine
    return LlavaEngine(GEOMETRIES[name], device="cuda:0", init="portable", seed=0, **kw)


def _batch(golden_dir, name="toy_e2e"):
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    return g, [torch.from_numpy(g[f"image{i}"]) for i in range(n)]


def _round(eng, g, images, **kw):
    loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
    eng.backward()
    eng.optimizer_step(**{**STEP, **kw})
    return float(loss)


def _names8(eng):
    from radvlm_amd.optim8 import StatePlan
    return StatePlan(eng.lm.offsets, eng.lm.shapes).names(8)


# ------------------------------------------------------------------------------------------------ engine
def test_engine_8bit_step_equals_the_emulated_fp32_arm(golden_dir):
    from radvlm_amd import ops
    g, images = _batch(golden_dir)
    e8, e32 = _engine(), _engine()
    e8.init_optimizer(state_bits=8)
    names8 = _names8(e32)
    assert "lm_head.weight" in names8 and "model.embed_tokens.weight" not in names8 and "model.norm.weight" not in names8
    for step in range(3):
        l8, l32 = _round(e8, g, images), _round(e32, g, images)
        for name in names8:                                  # the emulated arm: quantise -> dequantise the 8-bit tensors' moments
            off, n = e32.lm.offsets[name]
            for buf, kind in ((e32.m, 0), (e32.vv, 1)):
                codes, absmax = ops.adam8_quantize(buf[off:off + n], kind)
                ops.adam8_dequantize(codes, absmax, n, kind, buf[off:off + n])
        assert l8 == l32, (step, l8, l32)
        assert torch.equal(e8.lm.flat, e32.lm.flat) and torch.equal(e8.master, e32.master), step
    assert e8.state_bits == 8 and e32.state_bits == 32
    for name in e8.lm.names():
        off, n = e8.lm.offsets[name]
        v = e8.moment_views(name)
        if name in names8:
            assert v["exp_avg_codes"].dtype == torch.uint8 and v["exp_avg_sq_absmax"].dtype == torch.float32
            assert torch.equal(ops.adam8_dequantize(v["exp_avg_codes"], v["exp_avg_absmax"], n, 0), e32.m[off:off + n])
            assert torch.equal(ops.adam8_dequantize(v["exp_avg_sq_codes"], v["exp_avg_sq_absmax"], n, 1), e32.vv[off:off + n])
        else:                                                # the 32-bit tensors' moments are still fp32, and the same numbers
            assert v["exp_avg"].dtype == torch.float32 and torch.equal(v["exp_avg"], e32.m[off:off + n])
            assert torch.equal(v["exp_avg_sq"], e32.vv[off:off + n])
    assert bool(e8.moment_views("model.embed_tokens.weight")["exp_avg"].any())
    # converting in place to fp32 gives the state the emulated arm holds; converting that back is quantise(fp32 state) per tensor
    e8.init_optimizer(state_bits=32)
    assert e8.state_bits == 32 and e8.m8 is None and e8.m.numel() == e8.lm.numel
    assert torch.equal(e8.m, e32.m) and torch.equal(e8.vv, e32.vv)
    e8.init_optimizer(state_bits=8)
    off, n = e8.lm.offsets["lm_head.weight"]
    codes, absmax = ops.adam8_quantize(e32.vv[off:off + n], 1)
    v = e8.moment_views("lm_head.weight")
    assert torch.equal(v["exp_avg_sq_codes"], codes) and torch.equal(v["exp_avg_sq_absmax"], absmax)


def test_state_bytes_and_replica_buffers():
    """Moments only (the fp32 master copy is 4 B per parameter at either width).  A LoRA run's trainables are all 8-bit but the
    projector's biases: 2 B + 8 B / 256 per parameter against 8 B.  The full toy model is recorded, not gated: its embedding table
    (fp32 by the rule) is 14 % of its parameters, against 1.9 % of the 7B model's (tests/test_adam8_host.py holds the 7B figure < 0.3)."""
    ratios = {}
    for tag, kw in (("lora_r16", dict(lora=dict(r=16, alpha=16, dropout=0.0))), ("full_toy", {})):
        e8, e32 = _engine(**kw), _engine(**kw)
        assert e8.optimizer_state_bytes() == 0
        e8.init_optimizer(state_bits=8)
        e32.init_optimizer()
        assert e32.optimizer_state_bytes() == 8 * e32.lm.numel
        ratios[tag] = e8.optimizer_state_bytes() / e32.optimizer_state_bytes()
        names = [n for n, _ in e8._replica_buffers()]
        assert [n for n, _ in e32._replica_buffers()][-3:] == ["fp32_master", "exp_avg", "exp_avg_sq"]
        for n in ("fp32_master", "exp_avg", "exp_avg_sq", "exp_avg_codes", "exp_avg_sq_codes", "exp_avg_absmax", "exp_avg_sq_absmax"):
            assert n in names, n
        assert dict(e8._replica_buffers())["exp_avg_codes"].dtype == torch.uint8
    print("8-bit / fp32 moment bytes:", ratios)
    assert ratios["lora_r16"] < 0.3


def test_merge_lora_keeps_the_projectors_8bit_state(golden_dir):
    g, images = _batch(golden_dir)
    eng = _engine(lora=dict(r=16, alpha=16, dropout=0.0))
    eng.init_optimizer(state_bits=8)
    _round(eng, g, images)
    _round(eng, g, images)
    keep = [n for n in eng.lm.names() if ".lora_" not in n]
    before = {n: {k: v.clone() for k, v in eng.moment_views(n).items()} for n in keep}
    master = {n: eng.lm.view(n, eng.master).clone() for n in keep}
    assert "exp_avg_codes" in before["model.mm_projector.0.weight"] and bool(before["model.mm_projector.0.weight"]["exp_avg_absmax"].any())
    eng.merge_lora()
    assert eng.state_bits == 8 and eng.lm.names() == keep
    for n in keep:
        after = eng.moment_views(n)
        assert sorted(after) == sorted(before[n])
        for k in after:
            assert torch.equal(after[k], before[n][k]), (n, k)
        assert torch.equal(eng.lm.view(n, eng.master), master[n])
    assert np.isfinite(_round(eng, g, images))


# ------------------------------------------------------------------------------------------------ trainer
class _Ids:
    def __init__(self, ids):
        self.input_ids = ids


class _Tok:
    bos_token_id, pad_token_id, model_max_length, legacy, padding_side = 1, 0, 256, True, "right"

    def __call__(self, s, **kw):
        ids = [1]
        for k, piece in enumerate(s.split("</s>")):
            if k:
                ids.append(2)
            ids.extend(3 + (ord(c) % 900) for c in piece)
        return _Ids(ids)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """run(out, max_steps, save_steps, resume, optim) -> (model, state), plus the two uninterrupted 4-step runs (checkpoints at 2 and 4)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from PIL import Image
    from radvlm_amd.llava import conversation as conv_lib
    from radvlm_amd.llava.mm_utils import ClipImageProcessor
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM
    from radvlm_amd.llava.train.llava_trainer import LLaVATrainer
    from radvlm_amd.llava.train.train import DataArguments, TrainingArguments, make_supervised_data_module
    tmp = tmp_path_factory.mktemp("adam8")
    rng = np.random.default_rng(1)
    recs = []
    for i in range(8):
        Image.fromarray(rng.integers(0, 255, (64, 80, 3), dtype=np.uint8)).save(tmp / f"im{i}.png")
        recs.append({"id": f"s{i}", "image": f"im{i}.png", "conversations": [{"from": "human", "value": "<image>\nWhat is it?"},
                                                                            {"from": "gpt", "value": f"Finding number {i} " + "x" * i}]})
    (tmp / "d.json").write_text(json.dumps(recs))
    conv_lib.default_conversation = conv_lib.conv_templates["v1"]

    def run(out, max_steps, save_steps, resume, optim):
        da = DataArguments(data_path=str(tmp / "d.json"), image_folder=str(tmp), image_aspect_ratio="pad", is_multimodal=True)
        da.image_processor = ClipImageProcessor(56)
        da.mm_use_im_start_end = False
        tok = _Tok()
        model = LlavaLlamaForCausalLM(LlavaConfig(geometry=GEOMETRIES["toy"]), device="cuda:0", init="portable")
        module = make_supervised_data_module(tokenizer=tok, data_args=da)
        args = TrainingArguments(per_device_train_batch_size=2, gradient_accumulation_steps=1, max_steps=max_steps, learning_rate=1e-3,
                                 warmup_ratio=0.0, output_dir=str(tmp / out), save_steps=save_steps, optim=optim)
        state = LLaVATrainer(model=model, tokenizer=tok, args=args, **module).train(resume_from_checkpoint=resume)
        torch.cuda.synchronize()
        return model, state

    full8, s8 = run("a8", 4, 2, None, "adamw_bnb_8bit")
    full32, s32 = run("a32", 4, 2, None, "adamw_torch")
    return dict(run=run, tmp=tmp, full8=full8, s8=s8, full32=full32, s32=s32)


STATE8 = ("master", "m8", "v8", "am8", "av8", "m", "vv")


def test_trainer_8bit_checkpoint_and_resume_are_bit_identical(runs):
    from safetensors.torch import load_file
    from radvlm_amd.optim8 import codebook_sha
    tmp, full8 = runs["tmp"], runs["full8"]
    ck = tmp / "a8" / "checkpoint-2"
    assert full8.engine.state_bits == 8 and full8.engine.m8.dtype == torch.uint8
    ts = json.load(open(ck / "trainer_state.json"))
    assert ts["optim_state"] == {"bits": 8, "block": 256, "codebook": codebook_sha()}
    st = load_file(str(ck / "optimizer.safetensors"))
    assert sorted(st) == sorted(["master", "exp_avg_codes", "exp_avg_sq_codes", "exp_avg_absmax", "exp_avg_sq_absmax", "exp_avg_fp32",
                                 "exp_avg_sq_fp32"])
    assert st["exp_avg_codes"].dtype == torch.uint8 and st["master"].dtype == torch.float32
    size8, size32 = (os.path.getsize(tmp / d / "checkpoint-2" / "optimizer.safetensors") for d in ("a8", "a32"))
    print(f"optimizer.safetensors: {size8} B at 8 bits, {size32} B at 32 bits")
    assert size8 < size32
    resumed, s_res = runs["run"]("b8", 4, 0, str(ck), "adamw_8bit")
    assert s_res["global_step"] == 4 and [r["loss"] for r in s_res["log_history"]] == [r["loss"] for r in runs["s8"]["log_history"]]
    assert torch.equal(resumed.engine.lm.flat, full8.engine.lm.flat)
    for k in STATE8:
        assert torch.equal(getattr(resumed.engine, k), getattr(full8.engine, k)), k
    with pytest.raises(ValueError, match="codebook"):
        resumed.engine.load_optimizer_state_dict({k: v.cuda() for k, v in st.items()}, {"bits": 8, "block": 256, "codebook": "0" * 64})


def test_default_run_is_unchanged_fp32(runs):
    from safetensors.torch import load_file
    eng = runs["full32"].engine
    assert eng.state_bits == 32 and eng.m8 is None and eng.plan8 is None
    assert eng.m.dtype == eng.vv.dtype == eng.master.dtype == torch.float32 and eng.m.numel() == eng.lm.numel
    ck = runs["tmp"] / "a32" / "checkpoint-2"
    st = load_file(str(ck / "optimizer.safetensors"))
    assert sorted(st) == ["exp_avg", "exp_avg_sq", "master"] and all(v.dtype == torch.float32 for v in st.values())
    assert sorted(json.load(open(ck / "trainer_state.json"))) == ["global_step", "log_history", "lora_step", "opt_step"]
    assert sorted(os.listdir(ck)) == ["config.json", "mm_projector.bin", "model.safetensors", "optimizer.safetensors", "trainer_state.json"]


def test_cross_format_resume_quantises_and_dequantises_exactly(runs, capsys):
    from safetensors.torch import load_file
    from radvlm_amd import ops
    tmp = runs["tmp"]
    # fp32 file into an 8-bit run (no steps left: the state is what the load made it)
    st32 = load_file(str(tmp / "a32" / "checkpoint-2" / "optimizer.safetensors"))
    m8run, _ = runs["run"]("c8", 2, 0, str(tmp / "a32" / "checkpoint-2"), "adamw_bnb_8bit")
    assert "quantising on load" in capsys.readouterr().out
    eng = m8run.engine
    assert eng.state_bits == 8 and torch.equal(eng.master.cpu(), st32["master"])
    for name in eng.lm.names():
        off, n = eng.lm.offsets[name]
        v = eng.moment_views(name)
        for key, kind in (("exp_avg", 0), ("exp_avg_sq", 1)):
            src = st32[key][off:off + n].cuda().contiguous()
            if key in v:
                assert torch.equal(v[key], src), (name, key)
            else:
                codes, absmax = ops.adam8_quantize(src, kind)
                assert torch.equal(v[key + "_codes"], codes) and torch.equal(v[key + "_absmax"], absmax), (name, key)
    # 8-bit file into an fp32 run
    st8 = {k: t.cuda() for k, t in load_file(str(tmp / "a8" / "checkpoint-2" / "optimizer.safetensors")).items()}
    m32run, _ = runs["run"]("c32", 2, 0, str(tmp / "a8" / "checkpoint-2"), "adamw_torch")
    assert "dequantising on load" in capsys.readouterr().out
    e32 = m32run.engine
    assert e32.state_bits == 32 and e32.m8 is None and torch.equal(e32.master, st8["master"])
    plan = eng.plan8
    for name, t in plan.tensors.items():
        off, n = t["off"], t["n"]
        if t["bits"] == 8:
            b, nb = t["block"], (n + 255) // 256
            want_m = ops.adam8_dequantize(st8["exp_avg_codes"][b * 256:b * 256 + n], st8["exp_avg_absmax"][b:b + nb], n, 0)
            want_v = ops.adam8_dequantize(st8["exp_avg_sq_codes"][b * 256:b * 256 + n], st8["exp_avg_sq_absmax"][b:b + nb], n, 1)
        else:
            want_m, want_v = st8["exp_avg_fp32"][t["pos"]:t["pos"] + n], st8["exp_avg_sq_fp32"][t["pos"]:t["pos"] + n]
        assert torch.equal(e32.m[off:off + n], want_m) and torch.equal(e32.vv[off:off + n], want_v), name


def test_twenty_toy_steps_at_both_widths(golden_dir):
    """The 8-bit losses are finite and fall; both curves go to the measurement log, from which profiles/adam8_toy_losses.json was taken (the distance between them is recorded, not gated)."""
    g, images = _batch(golden_dir)
    curves = {}
    for bits in (32, 8):
        eng = _engine()
        eng.init_optimizer(state_bits=bits)
        curves[bits] = [_round(eng, g, images, lr=2e-3, weight_decay=0.0) for _ in range(20)]
    l8, l32 = np.asarray(curves[8]), np.asarray(curves[32])
    assert np.all(np.isfinite(l8)) and l8[-1] < l8[0]
    from conftest import record_measurement
    record_measurement("adam8_toy_losses", geometry="toy", batch="toy_e2e", lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, fp32=curves[32],
                       int8=curves[8], max_abs_difference=float(np.abs(l8 - l32).max()))
    print("fp32:", curves[32], "\n8-bit:", curves[8])

"""GPU tests of knowledge distillation on the toy goldens: LlavaEngine.forward(distill=) / label_logits, the model's distill_loss /
label_logits and GKDTrainer.  The anchors are bit for bit: forward KL at temperature 1 against a one-hot teacher is the SFT step;
a model distilled from itself has zero loss and zero gradient at beta 0 and 1; a seeded run repeats; a resumed run repeats."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import distill_ref as D
from radvlm_amd.config import GEOMETRIES
from radvlm_amd.policy import assemble, sample_seeds
from radvlm_amd.splice import shifted_labels
from rowops_ref import assert_rows_close
from test_generate_gpu import CASES, _load, _model, _prompt

pytestmark = pytest.mark.gpu

LAYOUTS = [(packed, head_rows) for packed in (False, True) for head_rows in ("labeled", "all")]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _batch(g, images, sizes):
    return dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"], labels=g["labels"], images=images, image_sizes=sizes)


def _make(geo, seed, geometry=None):
    """test_generate_gpu._model with a seed and an optional geometry of its own."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    geometry = GEOMETRIES[geo] if geometry is None else geometry
    l = geometry["lm"]
    cfg = Config(geometry=geometry, rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0))
    return Model(cfg, device="cuda:0", init="portable", seed=seed).eval()


def _grads(model, run):
    eng = model.engine
    eng.zero_grad()
    out = run()
    out.loss.backward()
    torch.cuda.synchronize()
    return eng.grads.clone(), out


def _scored_labels(model, batch):
    """(the labels of the scored tokens in scored order, the scored count per sample), from the spliced labels."""
    plan = model.engine.plan(batch["input_ids"], batch["attention_mask"], batch["labels"], batch["images"], batch["image_sizes"])
    tgt = shifted_labels(plan["labels"])
    return tgt[tgt != -100], (tgt != -100).sum(1)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_sft_anchor_padded_packed_and_head_rows(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw).train()
    batch = _batch(g, images, sizes)
    labels, counts = _scored_labels(model, batch)
    n, V = int(counts.sum()), model.engine.vocab
    hot = torch.zeros(n, V, dtype=torch.bfloat16, device="cuda")
    hot[torch.arange(n), torch.from_numpy(labels).cuda()] = 200.0
    for packed, head_rows in LAYOUTS:
        model.engine.packed, model.engine.head_rows = packed, head_rows
        sft, out_sft = _grads(model, lambda: model(**batch))
        assert float(sft.float().abs().max()) > 0
        for weights in (None, [1.0 / n] * len(counts)):
            got, out = _grads(model, lambda: model.distill_loss(**batch, teacher_logits=hot, beta=0.0, temperature=1.0, weights=weights))
            assert torch.equal(_bits(got), _bits(sft)), (case, packed, head_rows, weights is None)
            assert out.stats["n_scored"] == n and float(out.kl_student.abs().max()) == 0.0 and torch.equal(out.jsd, out.kl_teacher)
            # the forward KL against a one-hot teacher is the cross entropy, summed in another order
            assert abs(float(out.loss.detach()) - float(out_sft.loss.detach())) <= n * 2.0 ** -23 * max(1.0, float(out.jsd.abs().sum()) / n)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_teacher_rows_pair_with_the_students_in_every_layout(golden_dir, case):
    """.jsd per scored token against the float64 reference on the bits the two label_logits() return in that layout; the rows gate of the
    kernel tests.  A teacher row paired with the wrong student row misses it by orders of magnitude."""
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    student, teacher = _model(geo, kw).train(), _make(geo, 1)
    batch = _batch(g, images, sizes)
    _, counts = _scored_labels(student, batch)
    n, V = int(counts.sum()), student.engine.vocab
    ones = torch.ones(n)
    for packed, head_rows in LAYOUTS:
        for m in (student, teacher):
            m.engine.packed, m.engine.head_rows = packed, head_rows
        zs, zt = student.label_logits(**batch).clone(), teacher.label_logits(**batch).clone()
        assert zs.shape == zt.shape and zs.shape[0] == n and zs.shape[1] >= V and zs.dtype == torch.bfloat16
        assert teacher.engine.last_label_logits["scored"].tolist() == counts.tolist()
        for beta, tau in ((0.5, 0.9), (0.0, 1.0), (1.0, 2.0)):
            ref = D.distill_loss(zs, zt, torch.zeros(n, dtype=torch.int64), V, ones, ones, beta, tau)
            out = student.distill_loss(**batch, teacher=teacher, beta=beta, temperature=tau)
            student.engine.ctx = None
            for name, scale in (("jsd", "scale"), ("kl_teacher", "scale_t"), ("kl_student", "scale_s")):
                assert_rows_close(getattr(out, name), ref[name], ref[scale], 1e-4, f"{case} packed={packed} head_rows={head_rows} beta={beta} {name}")
            assert abs(float(out.loss.detach()) - float(ref["jsd"].mean())) <= 1e-4 * float(ref["scale"].mean())
            swapped = D.distill_loss(zs, zt.roll(1, 0), torch.zeros(n, dtype=torch.int64), V, ones, ones, beta, tau)
            assert float(((swapped["jsd"] - ref["jsd"]).abs() / (1e-4 * ref["scale"])).max()) > 1       # control: the gate sees a row mix-up


def test_self_distillation_is_a_fixed_point(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    batch = _batch(g, images, sizes)
    for packed, head_rows in ((False, "labeled"), (True, "all")):
        model.engine.packed, model.engine.head_rows = packed, head_rows
        for beta in (0.0, 1.0):
            model.engine.grads.fill_(1.0)
            grads, out = _grads(model, lambda: model.distill_loss(**batch, teacher=model, beta=beta, temperature=0.9))
            assert float(out.loss.detach()) == 0.0 and float(out.jsd.abs().max()) == 0.0 and float(grads.float().abs().max()) == 0.0
        _, out = _grads(model, lambda: model.distill_loss(**batch, teacher=model, beta=0.5, temperature=0.9))
        assert abs(float(out.loss.detach())) <= 1e-4         # the rows gate with scale 1 per token; the weights sum to 1


def test_wider_teacher_step_repeats_and_label_logits_touch_nothing(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    wide = copy.deepcopy(GEOMETRIES["toy"])
    wide["lm"].update(d=384, heads=3, ffn=640)
    teacher = _make("toy", 2, wide)
    batch = _batch(g, images, sizes)
    runs = []
    for _ in range(2):
        student = _model("toy", kw).train()
        eng = student.engine
        for step in range(2):
            eng.zero_grad()
            out = student.distill_loss(**batch, teacher=teacher, beta=0.5, temperature=0.9)
            out.loss.backward()
            eng.optimizer_step(lr=1e-3)
        torch.cuda.synchronize()
        assert float(out.loss.detach()) > 0 and bool(torch.isfinite(eng.lm.flat.float()).all())
        runs.append((eng.lm.flat.clone(), float(out.loss.detach())))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and runs[0][1] == runs[1][1]
    # label_logits on a model in the middle of a step: context, LoRA step counter and gradients stay
    out = student.distill_loss(**batch, teacher=teacher)
    ctx, lora_step, grads = eng.ctx, eng.lora_step, eng.grads.clone()
    assert ctx is not None
    a = student.label_logits(**batch).clone()
    assert eng.ctx is ctx and eng.lora_step == lora_step and torch.equal(_bits(eng.grads), _bits(grads))
    assert torch.equal(_bits(a), _bits(student.label_logits(**batch)))
    out.loss.backward()
    eng.zero_grad()


def test_errors(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model, other = _model("toy", kw).train(), _make("toy", 1)
    batch = _batch(g, images, sizes)
    _, counts = _scored_labels(model, batch)
    n, V = int(counts.sum()), model.engine.vocab
    good = torch.zeros(n, V, dtype=torch.bfloat16, device="cuda")
    model.distill_loss(**batch, teacher_logits=good[:, :V])
    model.engine.ctx = None
    for bad in (dict(), dict(teacher=other, teacher_logits=good), dict(teacher_logits=good[:-1]), dict(teacher_logits=good[:, :V - 1]),
                dict(teacher_logits=good.float()), dict(teacher_logits=good, beta=1.5), dict(teacher_logits=good, beta=-0.1),
                dict(teacher_logits=good, temperature=0.0), dict(teacher_logits=good, temperature=float("inf")),
                dict(teacher_logits=good, weights=[-1.0] * len(counts)), dict(teacher_logits=good, weights=np.ones(n + 1)),
                dict(teacher_logits=good, weights=[float("nan")] * len(counts))):
        with pytest.raises(ValueError):
            model.distill_loss(**batch, **bad)
    bigger = copy.deepcopy(GEOMETRIES["toy"])
    bigger["lm"]["vocab"] = 1008
    with pytest.raises(ValueError, match="vocabulary"):
        model.distill_loss(**batch, teacher=_make("toy", 1, bigger))
    shorter = dict(batch, labels=np.where(np.arange(g["labels"].shape[1])[None] % 2 == 0, g["labels"], -100))
    other.label_logits(**shorter)
    from radvlm_amd.distill import DistillTerms
    terms = DistillTerms(teacher_logits=good, teacher_scored=other.engine.last_label_logits["scored"])
    with pytest.raises(ValueError, match="the teacher scores"):
        model.engine.forward(batch["input_ids"], batch["attention_mask"], batch["labels"], images, image_sizes=sizes, distill=terms)
    from radvlm_amd.policy import PolicyTerms
    with pytest.raises(ValueError, match="does not combine"):
        model.engine.forward(batch["input_ids"], batch["attention_mask"], batch["labels"], images, image_sizes=sizes,
                             distill=DistillTerms(teacher_logits=good), policy=PolicyTerms(advantages=[1.0] * len(counts)))
    with pytest.raises(ValueError, match="does not combine"):
        model.engine.forward(batch["input_ids"], batch["attention_mask"], batch["labels"], images, image_sizes=sizes,
                             distill=DistillTerms(teacher_logits=good), _score_only=True)
    from radvlm_amd.llava.train.gkd_trainer import GKDTrainer
    with pytest.raises(NotImplementedError, match="seq_kd"):
        GKDTrainer(model, other, _args(seq_kd=True), [])
    with pytest.raises(NotImplementedError, match="one rank"):
        GKDTrainer(model, other, _args(world_size=2), [])


# ------------------------------------------------------------------------------------------------ the trainer
def _dataset(g, images, sizes, n=2):
    rng = np.random.default_rng(3)
    return [dict(prompt_ids=_prompt(g, b), completion_ids=rng.integers(5, 900, size=4 + b).astype(np.int64), images=images[b], image_sizes=sizes[b])
            for b in range(n)]


def _args(**kw):
    base = dict(per_device_train_batch_size=2, max_new_tokens=6, max_steps=3, learning_rate=1e-3, weight_decay=0.0, lr_scheduler_type="constant",
                seed=11, max_grad_norm=1.0, lmbda=0.5, beta=0.5, temperature=0.9)
    return SimpleNamespace(**dict(base, **kw))


def _strip_times(log):
    return [{k: v for k, v in rec.items() if not k.startswith("time/")} for rec in log]


KEYS = {"loss", "kl_teacher", "kl_student", "on_policy", "completions/mean_length", "learning_rate", "grad_norm", "step",
        "time/sampling_s", "time/assembly_s", "time/teacher_s", "time/update_s"}


@pytest.mark.parametrize("lmbda", [0.0, 1.0, 0.5])
def test_trainer_three_steps(golden_dir, lmbda):
    from radvlm_amd.distill import on_policy_step
    from radvlm_amd.llava.train.gkd_trainer import GKDTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    data, teacher = _dataset(g, images, sizes), _make("toy", 1)
    runs = []
    for r in range(2):
        model = _model("toy", kw).train()
        eng = model.engine
        trainer = GKDTrainer(model, teacher, _args(lmbda=lmbda, max_steps=3 if r == 0 else 1), data)
        state = trainer.train()
        torch.cuda.synchronize()
        assert eng.loss_scale == 1.0
        runs.append((eng.lm.flat.clone(), state["log_history"], trainer.last_completions))
    log = runs[0][1]
    assert len(log) == 3 and all(set(rec) >= KEYS for rec in log)
    assert [rec["on_policy"] for rec in log] == [int(on_policy_step(11, s, lmbda)) for s in (1, 2, 3)]
    assert all(rec["loss"] > 0 and rec["kl_teacher"] > 0 and rec["kl_student"] > 0 and rec["grad_norm"] is not None for rec in log)
    assert _strip_times(log[:1]) == _strip_times(runs[1][1])                      # a one-step run is the first step of the three
    # step 1 by hand on a fresh model: the same completions, distill_loss with the teacher, optimizer_step
    model = _model("toy", kw).train()
    eng = model.engine
    first = runs[1][2]
    order = [next(b for b in range(2) if np.array_equal(data[b]["prompt_ids"], p)) for p in _first_prompts(data, 11)]
    if log[0]["on_policy"]:
        out = model.generate_batch([data[b]["prompt_ids"] for b in order], images=[data[b]["images"] for b in order],
                                   image_sizes=[data[b]["image_sizes"] for b in order], do_sample=True, seed=sample_seeds(11, 0, 2, 1),
                                   temperature=0.9, max_new_tokens=6)
        assert first == [list(out[f"req_{i}"].generated_tokens) for i in range(2)]
    else:
        assert first == [data[b]["completion_ids"].tolist() for b in order]
    pad_id = getattr(model.config, "pad_token_id", None)
    if pad_id is None:
        eos = getattr(model.config, "eos_token_id", None)
        pad_id = 0 if eos is None else (eos if isinstance(eos, int) else list(eos)[0])
    ids, am, lab = assemble([data[b]["prompt_ids"] for b in order], first, pad_id)
    saved, eng.loss_scale = eng.loss_scale, 1.0
    eng.zero_grad()
    model.distill_loss(ids, am, lab, [data[b]["images"] for b in order], image_sizes=[data[b]["image_sizes"] for b in order], teacher=teacher,
                       beta=0.5, temperature=0.9).loss.backward()
    eng.optimizer_step(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0)
    eng.loss_scale = saved
    torch.cuda.synchronize()
    assert torch.equal(_bits(eng.lm.flat), _bits(runs[1][0])), "step 1 is the hand-made sequence"


def _first_prompts(data, seed):
    from radvlm_amd.llava.train.llava_trainer import epoch_index_batches
    it, _ = epoch_index_batches(len(data), None, seed, 2, 1, 0, 1, drop_last=False)
    return [data[i]["prompt_ids"] for i in next(it)]


def test_trainer_resume_repeats_the_run(golden_dir, tmp_path):
    from radvlm_amd.llava.train.gkd_trainer import GKDTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    data, teacher = _dataset(g, images, sizes), _make("toy", 1)
    out_dir = str(tmp_path / "run")
    model = _model("toy", kw).train()
    whole = GKDTrainer(model, teacher, _args(save_steps=2, output_dir=out_dir), data).train()
    torch.cuda.synchronize()
    want = model.engine.lm.flat.clone()
    again = _model("toy", kw).train()
    state = GKDTrainer(again, teacher, _args(save_steps=2, output_dir=out_dir), data).train(resume_from_checkpoint=os.path.join(out_dir, "checkpoint-2"))
    torch.cuda.synchronize()
    assert torch.equal(_bits(again.engine.lm.flat), _bits(want))
    assert _strip_times(state["log_history"][-1:]) == _strip_times(whole["log_history"][-1:])

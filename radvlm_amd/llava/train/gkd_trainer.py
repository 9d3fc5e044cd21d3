"""Generalised knowledge distillation (TRL's GKDTrainer restated on LlavaEngine): a student is trained to match a teacher's
distribution over the whole vocabulary at every answer token, on a mixture of the dataset's answers and the student's own samples --
sampled from the flat weights it is training, with no weight hand-over (as in grpo_trainer.py).

One optimizer step, on `per_device_train_batch_size` prompts:
  1. source   one counter-based uniform of (seed, step) (distill.on_policy_step): below `lmbda` the step is ON-POLICY and the
              completions are the student's, model.generate_batch(do_sample=True, seed=policy.sample_seeds(...), temperature=...,
              max_new_tokens=...); otherwise they are the dataset's completion_ids;
  2. assemble policy.assemble, split into `gradient_accumulation_steps` micro-batches; every scored token of the step weighs
              1 / (the step's scored tokens): TRL's batchmean over the step;
  3. update   per micro-batch the teacher's score-only pass (label_logits) and model.distill_loss(...).loss.backward(), then
              optimizer_step().  engine.loss_scale is 1: the token weights already normalise the step.
`temperature` is used twice, as in TRL: it shapes the samples and it scales both models' logits inside the loss.
"""
import math
import os
import time

import numpy as np
import torch

from ...distill import check_beta, check_lmbda, check_temperature, on_policy_step
from ...policy import assemble, sample_seeds
from .llava_trainer import LLaVATrainer, epoch_index_batches, lr_at, warmup_steps_for


class GKDTrainer(LLaVATrainer):
    """GKDTrainer(model, teacher_model, args, train_dataset, data_collator=None, tokenizer=None).
    args: TRL's names -- lmbda (0.5: the fraction of on-policy steps), beta (0.5: the JSD interpolation; 0 forward KL, 1 reverse KL),
    temperature (0.9), max_new_tokens (128), seq_kd (False; True is not built) -- and LLaVATrainer's for the optimizer, schedule,
    accumulation, logging, checkpoints and resume (per_device_train_batch_size = prompts per step, gradient_accumulation_steps =
    micro-batches per step, learning_rate, weight_decay, max_grad_norm, lr_scheduler_type, warmup_*, max_steps / num_train_epochs,
    seed, logging_steps, save_steps, output_dir, ...).
    A dataset item is a dict with prompt_ids (1-D token ids, IMAGE_TOKEN_INDEX where an image goes), completion_ids (the dataset's
    answer, its EOS included), and optional images (one tensor or a list) / image_sizes.  teacher_model: a model with the student's
    vocabulary and image-token count; it is only ever scored (label_logits), so a quantised teacher works as it is.
    Every log record lands in state["log_history"]."""

    def __init__(self, model=None, teacher_model=None, args=None, train_dataset=None, data_collator=None, tokenizer=None, **_):
        super().__init__(model=model, tokenizer=tokenizer, args=args, train_dataset=train_dataset, data_collator=data_collator)
        a = args
        if teacher_model is None:
            raise ValueError("GKDTrainer needs teacher_model")
        if getattr(a, "seq_kd", False):
            raise NotImplementedError("seq_kd=True (training on the teacher's own samples) is not built: seq_kd must be False")
        if getattr(a, "world_size", 1) > 1:
            raise NotImplementedError("GKD training runs on one rank (N > 1 untested)")
        self.lmbda = check_lmbda(getattr(a, "lmbda", 0.5))
        self.beta = check_beta(getattr(a, "beta", 0.5))
        self.temperature = check_temperature(getattr(a, "temperature", 0.9))
        self.max_new_tokens = int(getattr(a, "max_new_tokens", 128))
        if self.max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be >= 1, got {self.max_new_tokens}")
        if teacher_model.engine.vocab != model.engine.vocab:
            raise ValueError(f"the teacher's vocabulary ({teacher_model.engine.vocab}) is not the student's ({model.engine.vocab})")
        if getattr(model.engine, "nf4", None) is not None:
            raise NotImplementedError("GKD with an NF4 student: on-policy samples need generation, which has no NF4 decode kernel; "
                                      "model.dequantize_base_() or merge_and_unload() first")
        live = bool(model.engine.lora) and model.engine.adapter_decoding    # samples from the unmerged adapters
        if model.engine.lora and self.lmbda > 0 and not live:
            raise NotImplementedError("GKD with lmbda > 0 on a LoRA engine: generation refuses unmerged adapters; merge_and_unload() first, "
                                      "or model.enable_adapter_decoding() to sample from the live adapters")
        self.teacher_model = teacher_model
        self.last_completions = None

    # ------------------------------------------------------------------ the pieces of a step
    def _sample(self, items, step):
        """One seeded sample of every prompt: a list of id arrays, in the items' order."""
        a = self.args
        prompts = [np.asarray(it["prompt_ids"], dtype=np.int64).reshape(-1) for it in items]
        with_images = any(it.get("images") is not None for it in items)
        out = self.model.generate_batch(prompts, images=[it.get("images") for it in items] if with_images else None,
                                        image_sizes=[it.get("image_sizes") for it in items] if with_images else None, do_sample=True,
                                        seed=sample_seeds(int(getattr(a, "seed", 42)), step - 1, len(items), 1),
                                        temperature=self.temperature, max_new_tokens=self.max_new_tokens)
        return [np.asarray(out[f"req_{i}"].generated_tokens, dtype=np.int64) for i in range(len(items))]

    def _micro_batches(self, items, prompts, completions, pad_id):
        """The step's sequences as micro-batches: dicts of input_ids / attention_mask / labels / images / image_sizes and `rows`, the
        sequences' indices in the step.  A prompt without an image carries a zero image, as the splice expects."""
        P = len(items)
        accum = max(1, min(P, int(getattr(self.args, "gradient_accumulation_steps", 1) or 1)))
        per = -(-P // accum)
        side = self.model.engine.v["image"]
        out = []
        for p0 in range(0, P, per):
            rows = list(range(p0, min(P, p0 + per)))
            ids, am, lab = assemble([prompts[i] for i in rows], [completions[i] for i in rows], pad_id)
            images, sizes = [], []
            for i in rows:
                im, sz = items[i].get("images"), items[i].get("image_sizes")
                if im is None:
                    im, sz = [torch.zeros(3, side, side)], [(side, side)]
                elif torch.is_tensor(im):
                    im, sz = [im], [sz]
                images += list(im)
                sizes += list(sz) if sz is not None else [None] * len(im)
            out.append(dict(input_ids=ids, attention_mask=am, labels=lab, images=images,
                            image_sizes=None if any(s is None for s in sizes) else sizes, rows=rows))
        return out

    # ------------------------------------------------------------------ the loop
    def train(self, resume_from_checkpoint=None):
        a, model, eng = self.args, self.model, self.model.engine
        P, seed = int(a.per_device_train_batch_size), int(getattr(a, "seed", 42))
        it, steps_per_epoch = epoch_index_batches(len(self.train_dataset), None, seed, P, 1, 0, 1,
                                                  drop_last=bool(getattr(a, "dataloader_drop_last", False)))
        max_steps = int(getattr(a, "max_steps", -1) or -1)
        total = max_steps if max_steps > 0 else math.ceil(steps_per_epoch * float(getattr(a, "num_train_epochs", 1)))
        warm = warmup_steps_for(a, total)
        kind = getattr(a, "lr_scheduler_type", "cosine") or "cosine"
        kind = getattr(kind, "value", kind)
        start = self._maybe_resume(resume_from_checkpoint)
        for _ in range(start):
            next(it)
        pad_id = getattr(model.config, "pad_token_id", None)
        if pad_id is None:
            eos = getattr(model.config, "eos_token_id", None)
            pad_id = 0 if eos is None else (eos if isinstance(eos, int) else list(eos)[0])
        save_steps = int(getattr(a, "save_steps", 0) or 0)
        saved_scale, eng.loss_scale = eng.loss_scale, 1.0
        sync = lambda: torch.cuda.synchronize(eng.device) if eng.device.type == "cuda" else None
        batch_of = lambda m: {k: m[k] for k in ("input_ids", "attention_mask", "labels", "images", "image_sizes")}
        try:
            for step in range(start + 1, total + 1):
                items = [self.train_dataset[i] for i in next(it)]
                t0 = time.perf_counter()
                on_policy = on_policy_step(seed, step, self.lmbda)
                prompts = [np.asarray(it_["prompt_ids"], dtype=np.int64).reshape(-1) for it_ in items]
                if on_policy:
                    completions = self._sample(items, step)
                else:
                    completions = [np.asarray(it_["completion_ids"], dtype=np.int64).reshape(-1) for it_ in items]
                sync()
                t1 = time.perf_counter()
                lengths = np.array([c.size for c in completions], dtype=np.int64)
                n_step = int(lengths.sum())
                micros = self._micro_batches(items, prompts, completions, pad_id)
                t2 = time.perf_counter()
                outs, t_teacher = [], 0.0
                for j, m in enumerate(micros):
                    eng.sync_this_backward = j == len(micros) - 1
                    tt = time.perf_counter()
                    teacher_logits = self.teacher_model.label_logits(**batch_of(m))       # one micro-batch's rows alive at a time
                    sync()
                    t_teacher += time.perf_counter() - tt
                    w = [1.0 / n_step if n_step else 0.0] * len(m["rows"])
                    out = model.distill_loss(**batch_of(m), teacher_logits=teacher_logits, beta=self.beta, temperature=self.temperature,
                                             weights=w)
                    out.loss.backward()
                    outs.append(out)
                    del teacher_logits
                lr = lr_at(step, total, a.learning_rate, warm, kind)
                scale = lr / a.learning_rate if a.learning_rate else 0.0
                plr, vlr = getattr(a, "mm_projector_lr", None), getattr(a, "mm_vision_tower_lr", None)
                eng.optimizer_step(lr=lr, weight_decay=getattr(a, "weight_decay", 0.0),
                                   betas=(getattr(a, "adam_beta1", 0.9), getattr(a, "adam_beta2", 0.999)), eps=getattr(a, "adam_epsilon", 1e-8),
                                   max_grad_norm=getattr(a, "max_grad_norm", 1.0), mm_projector_lr=None if plr is None else plr * scale,
                                   mm_vision_tower_lr=None if vlr is None else vlr * scale)
                sync()
                t4 = time.perf_counter()
                n = max(1, sum(o.stats["n_scored"] for o in outs))
                mean = lambda key: float(sum(float(o.stats[key]) * o.stats["n_scored"] for o in outs) / n)
                self.state["global_step"] = step
                self.last_completions = [c.tolist() for c in completions]
                rec = {"step": step, "epoch": step / steps_per_epoch, "loss": float(sum(float(o.loss.detach()) for o in outs)),
                       "kl_teacher": mean("kl_teacher"), "kl_student": mean("kl_student"), "on_policy": int(on_policy),
                       "completions/mean_length": float(lengths.mean()), "learning_rate": lr,
                       "grad_norm": float(eng.last_grad_norm) if eng.last_grad_norm is not None else None,
                       "time/sampling_s": t1 - t0, "time/assembly_s": t2 - t1, "time/teacher_s": t_teacher,
                       "time/update_s": t4 - t2 - t_teacher}
                if step % max(1, getattr(a, "logging_steps", 1)) == 0:
                    self.state["log_history"].append(rec)
                    print(rec, flush=True)
                if save_steps and step % save_steps == 0 and getattr(a, "output_dir", None):
                    self.save_checkpoint(os.path.join(a.output_dir, f"checkpoint-{step}"), 0)
                    self._rotate_checkpoints(a.output_dir, 0)
                    eng.barrier()
        finally:
            eng.loss_scale = saved_scale
        return self.state

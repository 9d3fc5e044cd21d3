"""GRPO training (TRL's GRPOTrainer restated on LlavaEngine): sample a group of completions per prompt, score them, and take clipped
policy-gradient steps on the same flat weights the sampler reads -- no weight hand-over between a trainer and an inference engine:
optimizer_step() bumps engine.weights_version and the next generate_batch() reads the new weights.

One optimizer step, on `per_device_train_batch_size` prompts x `num_generations` completions:
  1. sample   model.generate_batch(do_sample=True, seed=policy.sample_seeds(...), share_prefix=True): a group's prompt is prefilled once;
  2. score    reward_funcs, weighted sum; policy.group_advantages; policy.token_weights over the whole step; policy.assemble;
  3. log-probs  old (num_iterations > 1) and reference (beta > 0) log-probs by token_logps(), the training path's own arithmetic, so
              the first iteration's ratio is exactly 1; a LoRA policy (model.enable_adapter_decoding()) without ref_model takes the
              reference from itself under model.disable_adapter();
  4. update   num_iterations passes over the step's micro-batches through model.policy_loss(...).loss.backward(), each followed by
              optimizer_step().  engine.loss_scale is 1: the token weights already normalise the step.
The step's groups are split into `gradient_accumulation_steps` micro-batches of whole groups (HF's meaning of the field: the number
of micro-batches per optimizer step).  Groups never straddle ranks and no collective is added; runs on more than one rank are untested.
The sampling temperature shapes the samples only: the loss scores the temperature-1 policy.
"""
import math
import os
import time

import numpy as np
import torch

from ...policy import LOSS_TYPES, SCALE_REWARDS, assemble, check_importance_sampling_level, group_advantages, sample_seeds, token_weights
from .llava_trainer import LLaVATrainer, epoch_index_batches, lr_at, warmup_steps_for

_COLUMNS_SKIPPED = ("prompt_ids", "images", "image_sizes")


class GRPOTrainer(LLaVATrainer):
    """GRPOTrainer(model, args, train_dataset, reward_funcs, tokenizer=None, ref_model=None, reward_weights=None).
    args: TRL's names -- num_generations (8), max_completion_length (256), temperature (1.0), top_p (1.0), top_k (None), min_p (None),
    epsilon (0.2), epsilon_high (None: epsilon), beta (0.0), loss_type ("dapo"; "grpo", "bnpo", "dr_grpo"), scale_rewards ("group";
    "batch", "none"), num_iterations (1), importance_sampling_level ("token"; "sequence": GSPO's one clipped ratio per completion, whose
    usual epsilon is a few 1e-4), mask_truncated_completions (False), log_completions (False) -- and LLaVATrainer's for the
    optimizer, schedule, logging and checkpoints (per_device_train_batch_size = prompts per step, learning_rate, weight_decay,
    max_grad_norm, lr_scheduler_type, warmup_*, max_steps / num_train_epochs, seed, logging_steps, save_steps, output_dir, ...).
    A dataset item is a dict with prompt_ids (1-D token ids, IMAGE_TOKEN_INDEX where an image goes), optional images (one tensor or
    a list) / image_sizes, and any further columns, which are passed to the reward functions.  A reward function is called as
    f(prompts=, completions=, completion_ids=, **columns) -> one float per completion; completions are decoded text when a tokenizer
    is given, else the id lists.  Every log record lands in state["log_history"]."""

    def __init__(self, model=None, args=None, train_dataset=None, reward_funcs=None, tokenizer=None, ref_model=None, reward_weights=None, **_):
        super().__init__(model=model, tokenizer=tokenizer, args=args, train_dataset=train_dataset)
        a = args
        self.G = int(getattr(a, "num_generations", 8))
        if self.G < 2:
            raise ValueError(f"num_generations must be at least 2 (the group is the baseline), got {self.G}")
        self.beta = float(getattr(a, "beta", 0.0) or 0.0)
        if getattr(model.engine, "nf4", None) is not None:
            raise NotImplementedError("GRPO on an NF4 base: rollouts need generation, which has no NF4 decode kernel; "
                                      "model.dequantize_base_() or merge_and_unload() first")
        live = bool(model.engine.lora) and model.engine.adapter_decoding    # rollouts on the unmerged adapters
        if self.beta > 0 and ref_model is None and not live:
            raise ValueError("beta > 0 needs ref_model (the KL term is taken against its token_logps)")
        if model.engine.lora and not live:
            raise NotImplementedError("GRPO on a LoRA engine: generation refuses unmerged adapters; merge_and_unload() first, "
                                      "or model.enable_adapter_decoding() to sample from the live adapters")
        self.loss_type, self.scale_rewards = getattr(a, "loss_type", "dapo"), getattr(a, "scale_rewards", "group")
        if self.loss_type not in LOSS_TYPES or self.scale_rewards not in SCALE_REWARDS:
            raise ValueError(f"loss_type must be one of {LOSS_TYPES} and scale_rewards one of {SCALE_REWARDS}")
        self.num_iterations = max(1, int(getattr(a, "num_iterations", 1) or 1))
        self.importance_sampling_level = check_importance_sampling_level(getattr(a, "importance_sampling_level", "token"))
        self.max_completion_length = int(getattr(a, "max_completion_length", 256))
        self.ref_model = ref_model
        funcs = list(reward_funcs) if isinstance(reward_funcs, (list, tuple)) else [reward_funcs]
        if not funcs or not all(callable(f) for f in funcs):
            raise ValueError("reward_funcs: a callable or a non-empty list of callables")
        self.reward_funcs = funcs
        self.reward_weights = [1.0] * len(funcs) if reward_weights is None else [float(w) for w in reward_weights]
        if len(self.reward_weights) != len(funcs):
            raise ValueError(f"{len(self.reward_weights)} reward_weights for {len(funcs)} reward_funcs")
        self.last_completions = None

    # ------------------------------------------------------------------ the pieces of a step
    def _sample(self, items, step):
        """G seeded samples of every prompt: (prompts, completions) as lists of P * G id arrays in [prompt][generation] order."""
        a, G = self.args, self.G
        reps = [it for it in items for _ in range(G)]
        prompts = [np.asarray(it["prompt_ids"], dtype=np.int64).reshape(-1) for it in reps]
        with_images = any(it.get("images") is not None for it in reps)
        kw = dict(do_sample=True, seed=sample_seeds(int(getattr(a, "seed", 42)), step - 1, len(items), G), share_prefix=True,
                  max_new_tokens=self.max_completion_length, temperature=float(getattr(a, "temperature", 1.0)),
                  top_p=float(getattr(a, "top_p", 1.0)), top_k=getattr(a, "top_k", None), min_p=getattr(a, "min_p", None))
        out = self.model.generate_batch(prompts, images=[it.get("images") for it in reps] if with_images else None,
                                        image_sizes=[it.get("image_sizes") for it in reps] if with_images else None, **kw)
        return prompts, [np.asarray(out[f"req_{i}"].generated_tokens, dtype=np.int64) for i in range(len(reps))]

    def _ref_logps(self, batch):
        """The reference log-probs of a micro-batch: ref_model's, or -- a LoRA policy without one -- the policy's own with the
        adapters switched off (peft's disable_adapter()): no second copy of the model."""
        if self.ref_model is not None:
            return self.ref_model.token_logps(**batch)
        with self.model.disable_adapter():
            return self.model.token_logps(**batch)

    def _rewards(self, items, prompts, completions):
        G = self.G
        ids = [c.tolist() for c in completions]
        texts = ids if self.tokenizer is None else [self.tokenizer.decode(c, skip_special_tokens=True) for c in ids]
        columns = {k: [it.get(k) for it in items for _ in range(G)] for k in items[0] if k not in _COLUMNS_SKIPPED}
        total = np.zeros(len(ids), dtype=np.float64)
        for f, w in zip(self.reward_funcs, self.reward_weights):
            r = np.asarray(f(prompts=[p.tolist() for p in prompts], completions=texts, completion_ids=ids, **columns), dtype=np.float64)
            if r.shape != total.shape:
                raise ValueError(f"reward function {getattr(f, '__name__', f)!r} returned {r.shape} values for {len(ids)} completions")
            total += w * r
        return total

    def _micro_batches(self, items, prompts, completions, pad_id):
        """The step's sequences as micro-batches of whole groups: dicts of input_ids / attention_mask / labels / images / image_sizes and
        `rows`, the sequences' indices in the step.  A prompt without an image carries a zero image, as the splice expects."""
        G, P = self.G, len(items)
        accum = max(1, min(P, int(getattr(self.args, "gradient_accumulation_steps", 1) or 1)))
        per = -(-P // accum)
        side = self.model.engine.v["image"]
        out = []
        for p0 in range(0, P, per):
            rows = list(range(p0 * G, min(P, p0 + per) * G))
            ids, am, lab = assemble([prompts[i] for i in rows], [completions[i] for i in rows], pad_id)
            images, sizes = [], []
            for i in rows:
                it = items[i // G]
                im, sz = it.get("images"), it.get("image_sizes")
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
        world, rank = getattr(a, "world_size", 1), getattr(a, "process_index", 0)
        P, G, K = int(a.per_device_train_batch_size), self.G, self.num_iterations
        it, steps_per_epoch = epoch_index_batches(len(self.train_dataset), None, getattr(a, "seed", 42), P, world, rank, 1,
                                                  drop_last=bool(getattr(a, "dataloader_drop_last", False)))
        max_steps = int(getattr(a, "max_steps", -1) or -1)
        total = max_steps if max_steps > 0 else math.ceil(steps_per_epoch * float(getattr(a, "num_train_epochs", 1)))
        warm = warmup_steps_for(a, total * K)
        kind = getattr(a, "lr_scheduler_type", "cosine") or "cosine"
        kind = getattr(kind, "value", kind)
        start = self._maybe_resume(resume_from_checkpoint)
        for _ in range(start):
            next(it)
        pad_id = getattr(model.config, "pad_token_id", None)
        if pad_id is None:
            eos = getattr(model.config, "eos_token_id", None)
            pad_id = 0 if eos is None else (eos if isinstance(eos, int) else list(eos)[0])
        eps, eps_hi = float(getattr(a, "epsilon", 0.2)), getattr(a, "epsilon_high", None)
        save_steps = int(getattr(a, "save_steps", 0) or 0)
        saved_scale, eng.loss_scale = eng.loss_scale, 1.0
        sync = lambda: torch.cuda.synchronize(eng.device) if eng.device.type == "cuda" else None
        try:
            for step in range(start + 1, total + 1):
                items = [self.train_dataset[i] for i in next(it)]
                t0 = time.perf_counter()
                prompts, completions = self._sample(items, step)
                sync()
                t1 = time.perf_counter()
                rewards = self._rewards(items, prompts, completions)
                adv = group_advantages(rewards, G, self.scale_rewards)
                lengths = np.array([c.size for c in completions], dtype=np.int64)
                truncated = np.array([c.size >= self.max_completion_length and (c.size == 0 or int(c[-1]) not in self._eos_ids()) for c in completions])
                scored = np.where(truncated, 0, lengths) if getattr(a, "mask_truncated_completions", False) else lengths
                weights = token_weights(scored, self.loss_type, self.max_completion_length)
                micros = self._micro_batches(items, prompts, completions, pad_id)
                t2 = time.perf_counter()
                batch_of = lambda m: {k: m[k] for k in ("input_ids", "attention_mask", "labels", "images", "image_sizes")}
                old = [model.token_logps(**batch_of(m)) for m in micros] if K > 1 else [None] * len(micros)
                ref = [self._ref_logps(batch_of(m)) for m in micros] if self.beta > 0 else [None] * len(micros)
                sync()
                t3 = time.perf_counter()
                iters = []
                for k in range(K):
                    outs = []
                    for j, m in enumerate(micros):
                        eng.sync_this_backward = j == len(micros) - 1
                        out = model.policy_loss(**batch_of(m), advantages=adv[m["rows"]], weights=weights[m["rows"]], old_logps=old[j],
                                                ref_logps=ref[j], epsilon=eps, epsilon_high=eps_hi, beta=self.beta,
                                                importance_sampling_level=self.importance_sampling_level)
                        out.loss.backward()
                        outs.append(out)
                    update = (step - 1) * K + k + 1
                    lr = lr_at(update, total * K, a.learning_rate, warm, kind)
                    scale = lr / a.learning_rate if a.learning_rate else 0.0
                    plr, vlr = getattr(a, "mm_projector_lr", None), getattr(a, "mm_vision_tower_lr", None)
                    eng.optimizer_step(lr=lr, weight_decay=getattr(a, "weight_decay", 0.0),
                                       betas=(getattr(a, "adam_beta1", 0.9), getattr(a, "adam_beta2", 0.999)), eps=getattr(a, "adam_epsilon", 1e-8),
                                       max_grad_norm=getattr(a, "max_grad_norm", 1.0), mm_projector_lr=None if plr is None else plr * scale,
                                       mm_vision_tower_lr=None if vlr is None else vlr * scale)
                    n = max(1, sum(o.stats["n_scored"] for o in outs))
                    mean = lambda key: float(sum(float(o.stats[key]) * o.stats["n_scored"] for o in outs) / n)
                    iters.append({"loss": float(sum(float(o.loss.detach()) for o in outs)), "kl": mean("kl"), "clip_ratio/low": mean("clip_ratio/low"),
                                  "clip_ratio/high": mean("clip_ratio/high"), "learning_rate": lr,
                                  "grad_norm": float(eng.last_grad_norm) if eng.last_grad_norm is not None else None})
                sync()
                t4 = time.perf_counter()
                self.state["global_step"] = step
                self.last_completions = [c.tolist() for c in completions]
                group_std = rewards.reshape(-1, G).std(1, ddof=1)
                rec = {"step": step, "epoch": step / steps_per_epoch, "reward": float(rewards.mean()), "reward_std": float(group_std.mean()),
                       "frac_reward_zero_std": float((group_std < 1e-6).mean()), "completions/mean_length": float(lengths.mean()),
                       "completions/clipped_ratio": float(truncated.mean()), **iters[-1],
                       "time/sampling_s": t1 - t0, "time/scoring_s": t2 - t1, "time/logps_s": t3 - t2, "time/update_s": t4 - t3}
                if K > 1:
                    rec["iterations"] = iters
                if getattr(a, "log_completions", False):
                    rec["completion_ids"] = self.last_completions
                if step % max(1, getattr(a, "logging_steps", 1)) == 0:
                    self.state["log_history"].append(rec)
                    if rank == 0:
                        print({k: v for k, v in rec.items() if k not in ("completion_ids", "iterations")}, flush=True)
                if save_steps and step % save_steps == 0 and getattr(a, "output_dir", None):
                    self.save_checkpoint(os.path.join(a.output_dir, f"checkpoint-{step}"), rank)
                    self._rotate_checkpoints(a.output_dir, rank)
                    eng.barrier()
        finally:
            eng.loss_scale = saved_scale
        return self.state

    def _eos_ids(self):
        eos = getattr(self.model.config, "eos_token_id", None)
        return set() if eos is None else ({int(eos)} if isinstance(eos, (int, np.integer)) else {int(e) for e in eos})

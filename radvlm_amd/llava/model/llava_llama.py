"""``LlavaConfig`` / ``LlavaLlamaModel`` / ``LlavaLlamaForCausalLM`` over the MI355X engine.

Mirrors the boundary class of reference finetuning/llava/model/language_model/llava_llama.py:35-156 and the
LlavaMetaModel / LlavaMetaForCausalLM glue of model/llava_arch.py:36-124, 192-196, 251-555:
same ``forward`` keyword list, ``.loss`` (fp32 scalar, mean CE over non-ignored shifted labels) and ``.logits``
(fp32 [b,S,V]) on the output, ``get_model()``, ``get_vision_tower()``, ``initialize_vision_modules`` and
``initialize_vision_tokenizer``, reference state-dict names.  ``out.loss.backward()`` runs the engine's hand-written
backward (one autograd node for the whole step), so an HF-Trainer-style ``training_step`` drives it unchanged.
"""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import torch

from ...engine import LlavaEngine


class LlavaConfig:
    model_type = "llava_llama"

    def __init__(self, geometry=None, mm_patch_merge_type="flat", image_aspect_ratio="square", image_grid_pinpoints=None,
                 tokenizer_model_max_length=None, rms_norm_eps=1e-5, rope_theta=10000.0, unfreeze_mm_vision_tower=False, lora=None, **kw):
        from ...config import GEOMETRIES
        self.geometry = geometry or GEOMETRIES["llava15_7b"]
        l, v = self.geometry["lm"], self.geometry["vision"]
        self.hidden_size, self.intermediate_size = l["d"], l["ffn"]
        self.num_hidden_layers, self.num_attention_heads, self.num_key_value_heads = l["layers"], l["heads"], l["heads"]
        self.vocab_size = l["vocab"]
        self.rms_norm_eps, self.rope_theta = rms_norm_eps, rope_theta
        self.mm_hidden_size = v["d"]
        self.mm_projector_type = "mlp2x_gelu"
        self.mm_vision_select_layer = -2
        self.mm_vision_select_feature = "patch"
        self.mm_patch_merge_type = mm_patch_merge_type
        self.image_aspect_ratio = image_aspect_ratio
        self.image_grid_pinpoints = image_grid_pinpoints
        self.tokenizer_model_max_length = tokenizer_model_max_length
        self.tokenizer_padding_side = "right"
        self.use_cache = False
        self.use_mm_proj = True
        self.unfreeze_mm_vision_tower = unfreeze_mm_vision_tower
        self.lora = lora   # {'r', 'alpha', 'dropout'} or None
        for k, val in kw.items():
            setattr(self, k, val)


class CausalLMOutputWithPast(SimpleNamespace):
    def __getitem__(self, i):
        return (self.loss, self.logits)[i]


class _StepFunction(torch.autograd.Function):
    """One autograd node for the whole training step: forward saved its context inside the engine."""

    @staticmethod
    def forward(ctx, flat_params, engine, loss):
        ctx.engine = engine
        return loss.clone().view(())

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        # d(loss)/d(params) is accumulated into engine.grads by the hand-written backward; the incoming scalar
        # multiplier (1 for plain loss.backward()) must be 1 -- loss scaling goes through forward(loss_scale=...).
        eng.backward()
        return None, None, None


class CLIPVisionTower:
    """Handle with the attributes the reference reads off its tower (clip_encoder.py:81-122)."""

    def __init__(self, engine):
        self._e = engine
        self.is_loaded = True
        self.select_layer, self.select_feature = -2, "patch"

    @property
    def config(self):
        v = self._e.v
        return SimpleNamespace(hidden_size=v["d"], image_size=v["image"], patch_size=v["patch"], num_hidden_layers=v["layers"])

    hidden_size = property(lambda s: s._e.v["d"])
    image_size = property(lambda s: s._e.v["image"])
    num_patches_per_side = property(lambda s: s._e.side)
    num_patches = property(lambda s: s._e.P)
    dtype = torch.bfloat16
    device = property(lambda s: s._e.device)

    def load_model(self, device_map=None):
        return None

    def __call__(self, images):
        """[n,3,H,W] -> [n,P,dv] patch features of hidden_states[-2] (clip_encoder.py:68-79)."""
        from ... import ops
        e = self._e
        x = images.to(e.device)
        x = x if x.dtype == torch.bfloat16 else ops.to_bf16(x.float())
        h = e.vision_forward(x.contiguous()).view(x.shape[0], e.P + 1, e.v["d"])
        return h[:, 1:]


class LlavaLlamaModel:
    def __init__(self, engine, config):
        self.engine, self.config = engine, config
        self.vision_tower = CLIPVisionTower(engine)

    def get_vision_tower(self):
        return self.vision_tower

    @property
    def embed_tokens(self):
        return self.engine.W("model.embed_tokens.weight")

    @property
    def mm_projector(self):
        e = self.engine
        return {n: e.W(f"model.mm_projector.{n}") for n in ("0.weight", "0.bias", "2.weight", "2.bias")}

    def initialize_vision_modules(self, model_args, fsdp=None):
        """Record the mm_* settings on the config (llava_arch.py:54-124); the tower/projector already live in the engine."""
        c = self.config
        c.mm_vision_tower = getattr(model_args, "vision_tower", None)
        c.mm_projector_type = getattr(model_args, "mm_projector_type", "mlp2x_gelu") or "mlp2x_gelu"
        if c.mm_projector_type not in ("mlp2x_gelu",):
            raise NotImplementedError(f"mm_projector_type={c.mm_projector_type}: only mlp2x_gelu is on the hot path")
        c.mm_vision_select_layer = getattr(model_args, "mm_vision_select_layer", -2)
        if c.mm_vision_select_layer != -2:
            raise NotImplementedError("mm_vision_select_layer must be -2 (LLaVA-1.5)")
        c.mm_vision_select_feature = getattr(model_args, "mm_vision_select_feature", "patch")
        c.mm_patch_merge_type = getattr(model_args, "mm_patch_merge_type", c.mm_patch_merge_type)
        p = getattr(model_args, "pretrain_mm_mlp_adapter", None)
        if p:
            w = torch.load(p, map_location="cpu", weights_only=True)
            self.engine.load_state_dict({("model." + k if not k.startswith("model.") else k): v for k, v in w.items() if "mm_projector" in k})


class LlavaLlamaForCausalLM:
    config_class = LlavaConfig
    model_class = LlavaLlamaModel

    def __init__(self, config, device="cuda", process_group=None, init="portable", seed=0):
        self.config = config
        self.engine = LlavaEngine(config.geometry, device=device, merge_type=config.mm_patch_merge_type,
                                  image_aspect_ratio=config.image_aspect_ratio, image_grid_pinpoints=config.image_grid_pinpoints,
                                  max_len=config.tokenizer_model_max_length, init=init, seed=seed, rms_eps=config.rms_norm_eps,
                                  rope_theta=config.rope_theta, process_group=process_group,
                                  train_vision_tower=getattr(config, "unfreeze_mm_vision_tower", False),
                                  lora=getattr(config, "lora", None), freeze_lm=getattr(config, "freeze_lm", False),
                                  train_embed_tokens=getattr(config, "train_embed_tokens", False),
                                  freeze_projector=getattr(config, "freeze_mm_mlp_adapter", False),
                                  padding_side=getattr(config, "tokenizer_padding_side", "right"),
                                  recompute=getattr(config, "activation_recompute", False))
        self.model = self.model_class(self.engine, config)
        self.training = True
        self.is_gradient_checkpointing = bool(self.engine.recompute)
        # a leaf that makes loss require grad so that `.backward()` reaches the engine
        self._anchor = torch.zeros(1, device=self.engine.device, requires_grad=True)

    def get_model(self):
        return self.model

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        """HF PreTrainedModel.gradient_checkpointing_enable (what Trainer calls for --gradient_checkpointing, reference
        train/train.py:1505-1513).  The reference re-runs EVERY decoder layer's forward in backward; here the flag selects the engine's
        "auto" policy -- the first n layers are recomputed, n taken per batch from free HBM (0 for the BASELINE batch on 288 GB), with
        bit-identical gradients either way.  LlavaEngine(recompute=True) is the explicit recompute-everything switch."""
        if self.engine.recompute is not True:
            self.engine.recompute = "auto"
        self.is_gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.engine.recompute = False
        self.is_gradient_checkpointing = False

    def get_vision_tower(self):
        return self.model.get_vision_tower()

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def parameters(self):
        return [self.engine.lm.flat]

    def state_dict(self):
        return self.engine.state_dict()

    def load_state_dict(self, sd, strict=False):
        return self.engine.load_state_dict(sd, strict=strict)

    def encode_images(self, images):
        e = self.engine
        from ... import ops
        x = images.to(e.device)
        x = x if x.dtype == torch.bfloat16 else ops.to_bf16(x.float())
        return e.encode_images(x.contiguous())[:x.shape[0] * e.P].view(x.shape[0], e.P, e.l["d"])

    def initialize_vision_tokenizer(self, model_args, tokenizer):
        """llava_arch.py:557-597: optional <im_patch> / <im_start>, <im_end> tokens are added to the tokenizer and the embedding
        tables grow by as many rows, initialised to the mean of the existing rows (:563-575).  In the pretraining stage
        (tune_mm_mlp_adapter) the INPUT embeddings then train with the projector while lm_head stays frozen (:577-581: build the
        model with config.train_embed_tokens=True, as train() does), and with pretrain_mm_mlp_adapter the two new embedding rows
        are restored from that file (:583-592)."""
        from ..constants import DEFAULT_IM_END_TOKEN, DEFAULT_IM_START_TOKEN, DEFAULT_IMAGE_PATCH_TOKEN
        e = self.engine
        if getattr(model_args, "mm_use_im_patch_token", False):
            tokenizer.add_tokens([DEFAULT_IMAGE_PATCH_TOKEN], special_tokens=True)
            e.resize_token_embeddings(max(len(tokenizer), e.vocab))
        if getattr(model_args, "mm_use_im_start_end", False):
            num_new = tokenizer.add_tokens([DEFAULT_IM_START_TOKEN, DEFAULT_IM_END_TOKEN], special_tokens=True)
            e.resize_token_embeddings(max(len(tokenizer), e.vocab))
            if getattr(model_args, "tune_mm_mlp_adapter", False) and "model.embed_tokens.weight" not in e.lm.offsets:
                raise ValueError("tune_mm_mlp_adapter + mm_use_im_start_end trains the input embeddings (llava_arch.py:577-581): "
                                 "build the model with config.train_embed_tokens=True")
            p = getattr(model_args, "pretrain_mm_mlp_adapter", None)
            if p:
                w = torch.load(p, map_location="cpu", weights_only=True)["model.embed_tokens.weight"]
                assert num_new == 2
                emb = e.W("model.embed_tokens.weight")
                if w.shape[0] in (e.vocab, emb.shape[0]) and w.shape[1] == emb.shape[1]:
                    emb[e.vocab - num_new:e.vocab].copy_(w[e.vocab - num_new:e.vocab].to(emb.dtype))
                elif w.shape[0] == num_new:
                    emb[e.vocab - num_new:e.vocab].copy_(w.to(emb.dtype))
                else:
                    raise ValueError(f"Unexpected embed_tokens_weight shape. Pretrained: {tuple(w.shape)}. Current: {(e.vocab, emb.shape[1])}. "
                                     f"Numer of new tokens: {num_new}.")
                e.weights_changed(tower=False)
                if e.master is not None:
                    from ... import ops
                    e.master.copy_(ops.to_f32(e.lm.flat))
        self.config.vocab_size = e.vocab
        self.config.mm_use_im_start_end = bool(getattr(model_args, "mm_use_im_start_end", False))

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None, labels=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, images=None, image_sizes=None, return_dict=None,
                modalities=("image",), dpo_forward=None, cache_position=None, output_logits=None):
        if past_key_values is not None or dpo_forward:
            raise NotImplementedError("forward() takes no key/value cache (generate() owns it) and returns no raw DPO logits "
                                      "(dpo_forward=True): preference training goes through preference_loss() / sequence_logps()")
        if inputs_embeds is not None:
            # llava_llama.py:83-120 with inputs_embeds given: no multimodal splice, the decoder runs on the embeddings (eval loss, the
            # per-step call of a generation loop without cache); fp32 logits, loss when labels are passed; no backward
            if input_ids is not None:
                raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
            loss, logits = self.engine.forward_embeds(inputs_embeds, attention_mask=attention_mask, labels=labels)
            return CausalLMOutputWithPast(loss=loss, logits=logits)
        if images is None:
            raise ValueError("images is required (text-only samples carry a dummy zero image, train.py:1227-1232)")
        imgs = list(images) if not torch.is_tensor(images) else [im for im in images]
        ids = input_ids.cpu().numpy() if torch.is_tensor(input_ids) else input_ids
        am = attention_mask.cpu().numpy() if torch.is_tensor(attention_mask) else attention_mask
        lab = labels.cpu().numpy() if torch.is_tensor(labels) else labels
        if lab is None:          # labels=None (llava_llama.py:69-120 returns logits only): nothing to score
            lab = np.full(np.asarray(ids).shape, -100, dtype=np.int64)
        want_logits = (labels is None or not self.training) if output_logits is None else output_logits
        loss = self.engine.forward(ids, am, lab, imgs, image_sizes=image_sizes, want_logits=want_logits)
        if self.training and labels is not None:
            loss = _StepFunction.apply(self._anchor, self.engine, loss)
        else:
            self.engine.ctx = None
        return CausalLMOutputWithPast(loss=loss if labels is not None else None, logits=self.engine.last_logits)

    __call__ = forward

    @staticmethod
    def _host_batch(input_ids, attention_mask, labels, images):
        if images is None:
            raise ValueError("images is required (text-only samples carry a dummy zero image, train.py:1227-1232)")
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
        return host(input_ids), host(attention_mask), host(labels), (list(images) if not torch.is_tensor(images) else [im for im in images])

    def policy_loss(self, input_ids, attention_mask, labels, images, image_sizes=None, *, advantages, weights=None, old_logps=None,
                    ref_logps=None, epsilon=0.2, epsilon_high=None, beta=0.0, importance_sampling_level="token"):
        """The GRPO token loss (TRL's GRPOTrainer: the clipped surrogate, plus beta times the k3 KL estimate against ref_logps) on a batch
        of prompt + completion rows; labels mark the completion tokens, as for forward().  Scored tokens of sample b: the positions of
        its spliced row whose shifted target is not -100, ascending.  advantages: one float per sample, or one array per sample, or
        the concatenation in scored order; weights likewise (None: 1 / number of scored tokens); old_logps / ref_logps per scored
        token (token_logps() gives them; None old_logps: the on-policy case, ratio exactly 1).  A shape that does not match the scored
        counts, a non-finite value, a negative epsilon / beta, or beta > 0 without ref_logps: ValueError.
        Returns an output with .loss = sum(weight * loss) (fp32 scalar; .loss.backward() runs the engine's backward, gradients scaled
        by engine.loss_scale as in forward()), .logps / .kl / .clip per scored token (device tensors) and .stats: n_scored and the
        device scalars kl, clip_ratio/low, clip_ratio/high (means over the scored tokens).
        importance_sampling_level="sequence" (TRL's keyword; GSPO): one ratio per sample, s = exp(mean over its scored tokens of logp -
        old_logp), clipped once, every token of the sample weighted alike; the KL term stays per token.  It needs one advantage per
        sample (advantages that vary inside a sample: ValueError); GSPO's usual clip range is a few 1e-4, not 0.2.  .loss and .clip
        then repeat the sample's term and clip code over its tokens, the output adds .coefs (fp32 per scored token: -dL/dlogp) and
        .seq_ratio / .seq_logratio / .seq_clip (fp64 [B], device), and clip_ratio/low and clip_ratio/high are means over the samples
        that have a scored token -- the reduction TRL uses at this level."""
        from ...policy import PolicyTerms
        ids, am, lab, imgs = self._host_batch(input_ids, attention_mask, labels, images)
        terms = PolicyTerms(advantages=advantages, weights=weights, old_logps=old_logps, ref_logps=ref_logps, epsilon=epsilon,
                            epsilon_high=epsilon_high, beta=beta, importance_sampling_level=importance_sampling_level)
        loss = self.engine.forward(ids, am, lab, imgs, image_sizes=image_sizes, policy=terms)
        lp = self.engine.last_policy
        n = int(lp["logp"].numel())
        mean = lambda t: t.float().mean() if n else torch.zeros((), device=self.engine.device)
        stats = {"n_scored": n, "kl": mean(lp["kl"]), "clip_ratio/low": mean(lp["clip"] == 1), "clip_ratio/high": mean(lp["clip"] == 2)}
        extra = {}
        if importance_sampling_level == "sequence":
            code = lp["seq_clip"][self.engine._dev(np.flatnonzero(np.asarray(lp["scored"]) > 0))]
            stats.update({"clip_ratio/low": mean(code == 1), "clip_ratio/high": mean(code == 2)})
            extra = dict(coefs=lp["coefs"], seq_ratio=lp["seq_ratio"], seq_logratio=lp["seq_logratio"], seq_clip=lp["seq_clip"])
        return SimpleNamespace(loss=_StepFunction.apply(self._anchor, self.engine, loss), logps=lp["logp"], kl=lp["kl"], clip=lp["clip"],
                               stats=stats, **extra)

    @torch.no_grad()
    def token_logps(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """log p(label) of every scored token of the batch, fp32 [n_scored] on the device, in scored order (see policy_loss), computed by
        the training path's own arithmetic (LlavaEngine.token_logps): the old / reference log-probs of policy_loss.  No gradient, and
        no training state is touched."""
        ids, am, lab, imgs = self._host_batch(input_ids, attention_mask, labels, images)
        return self.engine.token_logps(ids, am, lab, imgs, image_sizes=image_sizes)

    def distill_loss(self, input_ids, attention_mask, labels, images, image_sizes=None, *, teacher=None, teacher_logits=None, beta=0.5,
                     temperature=1.0, weights=None):
        """Knowledge distillation (TRL's GKDTrainer.generalized_jsd_loss) on a batch of prompt + completion rows; labels mark the
        completion tokens, as for forward().  At every scored token (policy_loss's order) the student's and the teacher's distributions
        over the whole vocabulary, both at `temperature`, are compared by the generalised Jensen-Shannon divergence with interpolation
        `beta` -- 0: forward KL(teacher || student), 1: reverse KL(student || teacher), between: beta KL(teacher || m) + (1 - beta)
        KL(student || m), m = (1 - beta) student + beta teacher -- and the loss is sum(weight * divergence); weights None: 1 / number
        of scored tokens (TRL's batchmean); no temperature^2 factor.
        Give exactly one of `teacher` (another model with the same vocabulary: its label_logits() on this batch are used; a quantised
        teacher works as it is) and `teacher_logits` (bf16 [n_scored, >= vocab] on the device, row j the teacher's logits at scored
        token j).  ValueError: both or neither; a vocabulary mismatch; a teacher whose scored counts per sample differ from the
        student's (another image-token count); teacher_logits of another shape or dtype; beta outside [0, 1]; a temperature that is
        not finite and positive; weights that do not match the scored counts, are negative or non-finite.
        Returns an output with .loss (fp32 scalar; .loss.backward() runs the engine's backward, gradients scaled by engine.loss_scale
        as in forward()), .jsd / .kl_teacher / .kl_student per scored token (fp32 device tensors; at beta 0 and 1 the divergence sits
        in kl_teacher / kl_student and the other is zero) and .stats: n_scored and the device scalars jsd, kl_teacher, kl_student
        (means over the scored tokens)."""
        from ...distill import DistillTerms
        if (teacher is None) == (teacher_logits is None):
            raise ValueError("distill_loss: give exactly one of teacher= and teacher_logits=")
        ids, am, lab, imgs = self._host_batch(input_ids, attention_mask, labels, images)
        terms = DistillTerms(teacher_logits=teacher_logits, beta=beta, temperature=temperature, weights=weights)
        if teacher is not None:
            if teacher.engine.vocab != self.engine.vocab:
                raise ValueError(f"the teacher's vocabulary ({teacher.engine.vocab}) is not the student's ({self.engine.vocab}): "
                                 "distillation compares the two distributions token by token")
            terms.teacher_logits = teacher.label_logits(ids, am, lab, imgs, image_sizes=image_sizes)
            terms.teacher_scored = teacher.engine.last_label_logits["scored"]      # checked against the student's counts in forward()
        loss = self.engine.forward(ids, am, lab, imgs, image_sizes=image_sizes, distill=terms)
        ld = self.engine.last_distill
        n = int(ld["jsd"].numel())
        mean = lambda t: t.mean() if n else torch.zeros((), device=self.engine.device)
        stats = {"n_scored": n, "jsd": mean(ld["jsd"]), "kl_teacher": mean(ld["kl_teacher"]), "kl_student": mean(ld["kl_student"])}
        return SimpleNamespace(loss=_StepFunction.apply(self._anchor, self.engine, loss), jsd=ld["jsd"], kl_teacher=ld["kl_teacher"],
                               kl_student=ld["kl_student"], stats=stats)

    @torch.no_grad()
    def label_logits(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """The bf16 logits of every scored token of the batch, [n_scored, >= ceil8(vocab)] on the device, in scored order (see
        policy_loss), computed by the training path's own arithmetic (LlavaEngine.label_logits): the teacher_logits of distill_loss.
        No gradient, and no training state is touched."""
        ids, am, lab, imgs = self._host_batch(input_ids, attention_mask, labels, images)
        return self.engine.label_logits(ids, am, lab, imgs, image_sizes=image_sizes)

    def preference_loss(self, chosen_input_ids, chosen_attention_mask, chosen_labels, rejected_input_ids, rejected_attention_mask,
                        rejected_labels, images, image_sizes=None, *, ref_chosen_logps=None, ref_rejected_logps=None, beta=0.1, dpo_alpha=1.0,
                        gamma=1.0, loss_type="sigmoid", label_smoothing=0.0, reference_free=False):
        """The DPO preference loss of the reference's LLaVADPOTrainer on P (chosen, rejected) pairs that share their prompts and images:
        L = dpo_alpha * mean_p l(h_p) + gamma * SFT, h = beta ((pi_c - pi_r) - (rho_c - rho_r)), pi / rho the policy's / the reference's
        summed log-prob of an answer's scored tokens (the mean for "ipo"), l the "sigmoid" (with label_smoothing), "hinge" or "ipo"
        pair loss, SFT = -(sum of the chosen scored log-probs) / (their number).  The batch runs as 2 P right-padded sequences -- the
        chosen rows, then the rejected rows, each half with the same images -- through forward()'s own path; labels mark the answer
        tokens.  ref_chosen_logps / ref_rejected_logps: P floats each, the reference's SUMMED log-probs (sequence_logps() of the
        reference model gives them), or reference_free=True.  ValueError: a pair without a scored chosen or rejected token,
        reference log-probs missing, of the wrong length or non-finite, beta <= 0, label_smoothing outside [0, 0.5) or with "ipo",
        an unknown loss_type.
        Returns an output with .loss (fp32 scalar; .loss.backward() runs the engine's backward, gradients scaled by engine.loss_scale
        as in forward()), .chosen_logps / .rejected_logps (pi), .margins (h), .pair_loss, .rewards_chosen / .rewards_rejected (fp64 [P]
        on the device), .coefs (fp32 per scored token, scored order: -dL/dlogp) and .stats under TRL's names -- rewards/chosen,
        rewards/rejected, rewards/accuracies, rewards/margins, logps/chosen, logps/rejected -- plus dpo_loss = dpo_alpha * mean pair loss and sft_loss (device
        scalars)."""
        from ...preference import PreferenceTerms, concatenate_pairs
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
        if images is None:
            raise ValueError("images is required (text-only samples carry a dummy zero image, train.py:1227-1232)")
        terms = PreferenceTerms(ref_chosen_logps=ref_chosen_logps, ref_rejected_logps=ref_rejected_logps, beta=beta, dpo_alpha=dpo_alpha,
                                gamma=gamma, loss_type=loss_type, label_smoothing=label_smoothing, reference_free=reference_free)
        terms.check()
        ids, am, lab = concatenate_pairs(host(chosen_input_ids), host(chosen_attention_mask), host(chosen_labels), host(rejected_input_ids),
                                         host(rejected_attention_mask), host(rejected_labels))
        imgs = list(images) if not torch.is_tensor(images) else [im for im in images]
        sizes = None if image_sizes is None else list(image_sizes) * 2
        loss = self.engine.forward(ids, am, lab, imgs + imgs, image_sizes=sizes, preference=terms)
        lp = self.engine.last_preference
        pl = dict(zip(("pi_c", "pi_r", "h", "loss", "reward_c", "reward_r"), lp["planes"]))
        stats = {"rewards/chosen": pl["reward_c"].mean(), "rewards/rejected": pl["reward_r"].mean(),
                 "rewards/accuracies": (pl["reward_c"] > pl["reward_r"]).double().mean(),
                 "rewards/margins": (pl["reward_c"] - pl["reward_r"]).mean(), "logps/chosen": pl["pi_c"].mean(),
                 "logps/rejected": pl["pi_r"].mean(), "dpo_loss": lp["batch"][1], "sft_loss": lp["batch"][2]}
        return SimpleNamespace(loss=_StepFunction.apply(self._anchor, self.engine, loss), chosen_logps=pl["pi_c"], rejected_logps=pl["pi_r"],
                               margins=pl["h"], pair_loss=pl["loss"], rewards_chosen=pl["reward_c"], rewards_rejected=pl["reward_r"],
                               coefs=lp["coefs"], stats=stats)

    @torch.no_grad()
    def sequence_logps(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """The summed log-prob of every sample's scored tokens, fp64 [B] on the device, and the scored counts (host int64 [B]):
        token_logps() summed per sample by rv_seq_logp_sums_f64 in its fixed order -- the reference log-probs of preference_loss.
        No gradient, and no training state is touched."""
        ids, am, lab, imgs = self._host_batch(input_ids, attention_mask, labels, images)
        return self.engine.sequence_logps(ids, am, lab, imgs, image_sizes=image_sizes)

    @torch.no_grad()
    def generate(self, inputs=None, images=None, image_sizes=None, modalities=("image",), **kwargs):
        """Greedy or seeded-sampling generation (the reference's generate(): the multimodal splice once, then HF generate on the spliced inputs_embeds).
        inputs: prompt token ids [B, T] (IMAGE_TOKEN_INDEX where an image goes); images / image_sizes as in forward (None: text only).
        Returns the NEW tokens only, LongTensor [B, T_new]; rows that finished (EOS or a stopping criterion) are filled with
        pad_token_id.  Keywords: max_new_tokens (default 20), max_length, eos_token_id, pad_token_id, attention_mask, stopping_criteria,
        use_cache (the result is the same either way), output_scores / output_logits + return_dict_in_generate (.sequences, .scores =
        the processed scores, .logits = the raw ones, .past_key_values).  past_key_values: a generation.GenerationCache() reused across
        the calls of a conversation (each with the full prompt and images; the cached common prefix is not recomputed).  HF's greedy logits processors: repetition_penalty, no_repeat_ngram_size,
        bad_words_ids, min_length, min_new_tokens, suppress_tokens, begin_suppress_tokens; as in HF generation from inputs_embeds they
        see only the generated tokens (pads included), never the prompt; a bad value raises ValueError.
        Sampling: do_sample=True together with seed= (an int s: row i draws with seed s + i; or a list with one int per row, each in
        [0, 2^63)).  After the processors HF's warpers run in HF's order -- temperature (default 1.0), top_k (50; None or 0: off),
        top_p (1.0), min_p (None) -- then one token is drawn from the softmax with a counter-based uniform of (the row's seed, the
        number of tokens the row has generated), so a call is reproducible by construction and a row draws the same alone or in any
        batch.  output_scores then returns the warped scores (-inf where a warper removed the entry), output_logits the raw ones;
        stopping criteria get the warped scores.  Scores with a NaN, +inf or no finite entry raise ValueError.  do_sample=True WITHOUT
        seed= raises NotImplementedError: draws from torch's global generator are not implemented.  With do_sample=False the sampling
        keywords are accepted and ignored, as in HF; seed= without do_sample=True is a ValueError.  typical_p, epsilon_cutoff and
        eta_cutoff (at a non-default value), beam search, num_return_sequences > 1, streamers, inputs_embeds and LoRA models raise
        NotImplementedError.
        Prompt-lookup decoding: prompt_lookup_num_tokens=k (an int, 1 .. 31; HF's name) drafts up to k tokens per step from n-gram
        repeats of the prompt and of the tokens generated so far (HF's PromptLookupCandidateGenerator rule; max_matching_ngram_size,
        default 2) and verifies them in one k + 1 row engine step (LlavaEngine.verify_step).  The result -- sequences, scores, logits,
        what a GenerationCache holds afterwards -- is bit for bit that of the same call without it, in fewer steps when the drafts
        are right; with return_dict_in_generate the output gains .lookup_stats = dict(steps=, drafted=, accepted=).  One prompt row
        only (ValueError otherwise, HF's assisted generation is batch-size-1 too); with do_sample=True NotImplementedError; k outside
        1 .. 31 or a non-int ValueError.  Every other greedy keyword keeps its meaning; stopping criteria are called once per emitted
        token, in order, with that token's own score row.
        Assisted generation: assistant_model=m (HF's name; another model of this package with the same vocabulary size and the same
        image inputs, any decoder geometry or weight format; m may be the model itself) drafts num_assistant_tokens=k tokens per
        round (an int, 1 .. 31, default 5, constant) on a KV cache of its own, prefilled with the same prompt and images, and the
        model verifies them in one k + 1 row step.  Greedy, the result is bit for bit that of the call without it.  With
        do_sample=True and seed= the round is speculative sampling (HF's _speculative_sampling on rv_spec_accept_rows_f32): the
        call is reproducible for a given (seed, assistant, k) and draws from the same distribution as the plain call, but does
        not emit the same tokens.  scores are the model's processed (warped) rows, logits its raw rows; with
        return_dict_in_generate the output gains .assist_stats = dict(steps=, drafted=, accepted=).  One prompt row only
        (ValueError); a vocabulary or image-input mismatch is a ValueError naming it, before any device work; with
        prompt_lookup_num_tokens, past_key_values, kv_cache_dtype="int8", guidance_scale, dola_layers, constraint,
        output_attentions or prompt_kv_budget NotImplementedError.
        kv_cache_dtype: None or "bf16" (today's cache) or "int8": each cached position's K and V are stored per kv head as int8 with
        one fp32 scale (s = max|x| / 127), 0.516x the cache bytes, read by an int8 decode-attention kernel.  The first token still
        comes from the unquantised prompt pass; later tokens see the rounded keys and values, so they may differ from the bf16
        cache's.  It composes with the logits processors, sampling, output_scores / output_logits and load_8bit models; it does
        NOT compose with past_key_values or prompt_lookup_num_tokens (NotImplementedError), and another value is a ValueError.
        Classifier-free guidance: guidance_scale=g (a finite number; None or 1: off, and the call is bit for bit the call without
        it) with HF's negative_prompt_ids [B, Ln] / negative_prompt_attention_mask, plus negative_images / negative_image_sizes
        (required when the negative prompt holds image placeholders, refused when it holds none); without a negative prompt each
        row's is its last real prompt token (HF).  Each step's scores become log_softmax(uncond) + g * (log_softmax(cond) -
        log_softmax(uncond)) (HF's UnbatchedClassifierFreeGuidanceLogitsProcessor, rounded as HF rounds it) before the processors and
        warpers above; the unconditional sequence -- the negative prompt, then the same generated tokens -- is one more row of the
        same decode step in a cache of 2 * B rows.  output_logits returns the raw conditional logits, output_scores and the stopping
        criteria the guided, processed scores; min_length / max_length count the conditional prompt.  It composes with sampling,
        kv_cache_dtype="int8" and load_8bit models; with past_key_values or prompt_lookup_num_tokens NotImplementedError; a bad
        scale, a negative prompt of another row count or with an empty row, images that do not match its placeholders, or any
        negative_* argument while guidance is off: ValueError.
        DoLa, decoding by contrasting layers: dola_layers="low", "high" or a list of layer numbers (HF's keyword; None: off, and the
        call is bit for bit the call without it).  Layer c is the hidden state entering decoder layer c (0: the embeddings), sent
        through lm_head without the final norm; "low" / "high" are HF's buckets (every second layer of the lower / upper half, of
        the first / last 20 for more than 40 layers).  Per step and per row the candidate whose next-token distribution has the
        largest Jensen-Shannon divergence from the last layer's is chosen (HF averages it over the batch; here every row chooses,
        which is HF at B = 1), and the scores become log_softmax(last) - log_softmax(chosen) where log_softmax(last) >= its maximum
        + ln 0.1 and -inf elsewhere (HF's relative_top = 0.1), before the processors and warpers above.  No second sequence and no
        extra cache row: the candidates' hidden rows are further rows of the step's lm_head.  output_logits returns the raw last-layer
        logits, output_scores and the stopping criteria the contrasted, processed scores; with return_dict_in_generate the output
        gains .dola_premature_layers, int64 [B, steps], the layer each row chose (-1 after the row's EOS).  It composes with
        sampling, kv_cache_dtype="int8" and quantised decoders; with guidance_scale, past_key_values or prompt_lookup_num_tokens
        NotImplementedError; another string, an empty list, a duplicate, a non-int, a bool, a layer outside [0, layers) (HF drops
        those silently) or more than 16 candidates: ValueError.
        Constrained decoding: constraint=c, a radvlm_amd.constraints.TokenConstraint for every row or a list of B with None for an
        unconstrained row (None: off, no launch added).  It is a deterministic automaton over token ids -- from_choices (a closed
        answer set), from_char_dfa (a character DFA lifted to the tokenizer's vocabulary; boxes_char_dfa gives the one of
        format_boxes' strings) -- and does what HF's prefix_allowed_tokens_fn does, without a Python callback per row and step: each
        step's raw row gets -inf outside the ids the row's state allows (rv_constrain_rows_f32, the place of HF's
        PrefixConstrainedLogitsProcessor), then the processors, the argmax or the seeded sampler run on it unchanged.  The
        constraint sees the generated tokens only and starts at its start state on every call, with past_key_values too; after an
        EOS edge the row is free.  output_logits returns the raw rows, output_scores the masked, processed ones.  When the
        processors or warpers ban everything a state allows (min_new_tokens against a state that allows only EOS), the call raises
        RuntimeError naming the row and the step.  It composes with the processors, sampling, kv_cache_dtype="int8", quantised
        decoders and past_key_values; with prompt_lookup_num_tokens, guidance_scale or dola_layers NotImplementedError; another
        type, a list of another length or an automaton naming an id beyond the vocabulary: ValueError.
        Attention maps: output_attentions=True (HF's keyword; needs return_dict_in_generate=True) returns .attentions, a tuple over
        the generated steps of a tuple over the asked layers of fp32 [B, H, 1, L_t]: softmax(q K^T / sqrt(hd)) of the step's query
        row, computed by a HIP kernel family of its own (rv_attn_decode_probs_f32) beside the unchanged decode attention, so
        .sequences, .scores and .logits are bit for bit those of the call without it.  attention_layers (ours): None = every layer, or
        a list of layer numbers, negative ones counting from the end (-1: the last layer); .attention_layers carries the resolved
        numbers.  attention_reduce (ours): None, or "mean_heads" for the mean over the heads, [B, 1, 1, L_t], taken on the device.  Two
        deviations from HF: step 0 gives only the LAST prompt row, [B, H, 1, S_0] (S_0 the longest spliced prompt), not HF's [B, H, S,
        S]; and the key axis is each sequence's cache positions 0 .. len_b - 1 whatever the padding side (position k is the k-th
        valid position of the spliced row), with zeros beyond a row's length -- L_t grows by one per step.  A finished row's entries
        at later steps are whatever the padded step computes and mean nothing; .sequences tells where each row ended.
        radvlm_amd.attention_maps turns the rows into per-image patch maps.  It composes with the processors, sampling, constraint,
        stopping_criteria and quantised decoders; with kv_cache_dtype="int8", past_key_values, prompt_lookup_num_tokens,
        guidance_scale, dola_layers or live LoRA adapters NotImplementedError; a non-bool, a missing return_dict_in_generate, a bad
        attention_reduce, attention_layers with a bool, a non-int, a duplicate or a value outside [-layers, layers), or either of
        our two keywords without output_attentions: ValueError.
        Prompt cache compression (SnapKV, Li et al. 2024; ours, lossy, opt-in): prompt_kv_budget=N keeps N of a prompt's positions per
        sequence, layer and kv head instead of all of them -- the last prompt_kv_window=w (default 32, 1 .. 64) positions, the text
        question after the image, vote with their attention for the earlier keys; the votes are max-pooled over prompt_kv_pool=k
        (default 7, odd, 1 .. 63) neighbours and the N - w best-voted positions are kept beside the window itself
        (rv_kv_votes_f32 / rv_kv_select_i32 / rv_kv_gather_bf16 inside the prompt pass: the full prompt is never cached).  A prompt of
        at most N positions is cached whole and the call is bit for bit the call without the keyword.  The first token comes from the
        uncompressed prompt pass; later ones read the compact cache with the unchanged decode kernels, each new token rotated at its
        true position.  It composes with the processors, sampling, constraint, quantised decoders and live LoRA adapters; with
        past_key_values, prompt_lookup_num_tokens, guidance_scale, dola_layers, output_attentions or kv_cache_dtype="int8"
        NotImplementedError; a bool, a non-int, N <= w, an even or out-of-range k, or window / pool without the budget: ValueError.
        The training state (weights, optimizer, RNG counters) is not touched."""
        from ...generation import greedy_generate, parse_generate_kwargs
        cfg = parse_generate_kwargs(kwargs, lora=self._lora_refused, config_eos=getattr(self.config, "eos_token_id", None),
                                    config_pad=getattr(self.config, "pad_token_id", None), lookup=True, attentions=True)
        if inputs is None:
            raise ValueError("generate() needs the prompt token ids (`inputs`)")
        imgs = None if images is None else (list(images) if not torch.is_tensor(images) else [im for im in images])
        return greedy_generate(self.engine, inputs, cfg.attention_mask, imgs, image_sizes, cfg)

    @torch.no_grad()
    def generate_batch(self, inputs, images=None, image_sizes=None, max_batch_size=32, return_logprobs=False, **kwargs):
        """Continuous batching over many independent prompts (transformers 5.x `generate_batch`), greedy or sampled.
        inputs: a list of N unpadded 1-D prompts (token ids; IMAGE_TOKEN_INDEX where an image goes).  images / image_sizes: None or a list
        of N entries, each None (text only), one tensor or a list of tensors (the request's images in image-token order) / their sizes.
        max_batch_size: requests decoded together (KV-cache slots).  Keywords: generate()'s greedy settings, applied per request
        (max_new_tokens may be a list of N budgets; pad_token_id is accepted, nothing is padded); attention_mask, past_key_values,
        position_ids, output_scores, output_logits and return_dict_in_generate raise TypeError; do_sample=True without seed=, beam
        search, streamers, inputs_embeds and LoRA models raise NotImplementedError as in generate().  Sampling: do_sample=True with
        seed= (an int s: request i draws with seed s + i; or a list of N ints) and generate()'s temperature / top_k / top_p / min_p;
        request i draws at its step t with u(seed_i, t), i.e. exactly what generate() draws for it alone with seed=seed_i, whatever
        the slot and the schedule (up to the rounding of the scores themselves).
        Returns {"req_0": GenerationOutput, ...} in input order: .generated_tokens are what generate() returns for the request alone,
        ending at its EOS token or where a stopping criterion returned True; .logprobs (return_logprobs) the log-softmax of each step's
        processed scores at the emitted token (when sampling: log q of the drawn token, q the softmax over what the warpers kept).
        kv_cache_dtype="int8" (None / "bf16": today's cache): the slots' cache holds int8 K|V rows as in generate(), so the memory
        check admits about twice the slots or positions; a request's tokens are those of generate(kv_cache_dtype="int8") on it alone.
        guidance_scale=g (one value for the call) with negative_prompt_ids (a list of N unpadded 1-D id sequences, an entry None: the
        request's last prompt token) and negative_images / negative_image_sizes (per request, as images): classifier-free guidance
        as in generate().  max_batch_size keeps counting requests; the cache holds two rows per slot (the memory check counts both)
        and a request's tokens are those of generate() on it alone with the same guidance.  negative_prompt_attention_mask: TypeError.
        share_prefix=True (default False: nothing changes): requests that begin with the same spliced positions -- equal token ids
        and image rows of bit-identical pixels with the same image_size, at least 128 of them -- share them within the call: the
        first is prefilled, a follower's cache row gets the common positions by a copy and only its suffix runs through the decoder
        (LlavaEngine.extend(slots=)), so the tower and the prompt pass run once per distinct prefix, and decode attention may read
        a group's shared keys once per step (rv_attn_decode_shared_bf16, the plain kernel's bits; LlavaEngine.shared_route).  A
        follower's tokens agree with the unshared call's within rounding; prompts with nothing in common give exactly the call
        without the keyword.  A non-bool value: ValueError; with kv_cache_dtype="int8", guidance_scale or dola_layers:
        NotImplementedError.
        dola_layers (one value for the call): DoLa as in generate().  Every request chooses its own layer at every step, so a
        request's tokens are those of generate(dola_layers=...) on it alone; the cache keeps one row per slot.
        constraint: one TokenConstraint for every request or a list of N with None entries, as in generate().  The automaton states
        live on the device, one per cache slot; an admission writes the request's start state into its slot.  A request's tokens,
        and its logprobs (of the masked, processed row, so renormalised over the allowed ids), are those of generate(constraint=)
        on it alone; it works with share_prefix=True.  A dead end raises RuntimeError naming the request and its step.
        prompt_kv_budget=N / prompt_kv_window / prompt_kv_pool (one value each for the call): prompt cache compression as in
        generate().  A request then takes min(its spliced length, N) + its budget cache positions, which is what the slots' cache
        and the memory check are sized for; a request's tokens are those of generate() on it alone with the same three values.  With
        share_prefix=True: NotImplementedError.
        The training state is not touched."""
        from ...generation import generate_batch, parse_batch_kwargs
        inputs = list(inputs)
        cfg = parse_batch_kwargs(kwargs, len(inputs), lora=self._lora_refused, config_eos=getattr(self.config, "eos_token_id", None),
                                 config_pad=getattr(self.config, "pad_token_id", None))
        return generate_batch(self.engine, inputs, images, image_sizes, cfg, max_batch_size=max_batch_size, return_logprobs=return_logprobs)

    @torch.no_grad()
    def score(self, inputs, candidates, images=None, image_sizes=None, max_batch_size=32, **kwargs):
        """Log-likelihoods of given answers (lm-evaluation-harness's `loglikelihood`, HF's compute_transition_scores on a sequence the
        caller already has): closed-ended VQA and multiple choice (log p("Yes" | image, question) against log p("No" | ...)), per-finding
        ranking scores, the perplexity of a reference report.
        inputs / images / image_sizes: generate_batch()'s request format, N unpadded 1-D prompts and per-request images.  candidates: a
        list of N lists of 1-D token-id sequences (text ids in [0, vocab)).  Each distinct prompt is prefilled once -- the tower and the
        prompt pass run once per prompt, max_batch_size prompts at a time, equal prompts of a group once -- and every candidate runs
        only its own tokens, reading the prompt's keys in place (LlavaEngine.score_tails).
        Returns a scoring.ScoreOutput: .token_logprobs[i][c] fp32 CPU tensor [len(candidate)], log_softmax(raw logits)[token] at every
        candidate position; .logprobs[i] float64 [C_i], their sums (fp64, token order); .is_greedy[i] bool [C_i], every token its row's
        argmax; .best(length_normalized=False) the best candidate's index per prompt (ties: the lower index).
        The raw distribution is the point: no logits processors, no sampling, no kv_cache_dtype (any other keyword: TypeError).
        ValueError for an empty prompt, candidate or candidate list, candidate ids outside [0, vocab) and lists of different lengths;
        NotImplementedError for LoRA models (merge_and_unload() or enable_adapter_decoding() first).  int8 / MXFP4 decoders work.
        The training state is not touched."""
        if kwargs:
            raise TypeError(f"score() got unexpected keyword arguments {sorted(kwargs)}")
        from ...scoring import score
        return score(self.engine, list(inputs), candidates, images, image_sizes, max_batch_size=max_batch_size)

    @torch.no_grad()
    def generate_beams(self, inputs=None, images=None, image_sizes=None, num_beams=1, modalities=("image",), **kwargs):
        """Beam search (HF generate(num_beams=...) on the spliced inputs_embeds: transformers 5.x GenerationMixin._beam_search, restated
        in generation.BeamState).  inputs / images / image_sizes as in generate().  Returns the NEW tokens only, LongTensor
        [B * num_return_sequences, T_out], hypothesis j of prompt b in row b * num_return_sequences + j, best first, shorter ones
        filled with pad_token_id (HF's output_fill_value).  Keywords: generate()'s max_new_tokens / max_length, eos_token_id,
        pad_token_id, attention_mask, stopping_criteria (called once per step with the K = max(2, 1 + n_eos) * num_beams candidates of
        every prompt, [B * K, t + 1]), use_cache, the logits processors (applied to the log-probs, history: the beam's own tokens),
        output_scores / output_logits + return_dict_in_generate (.sequences, .sequences_scores, .scores, .logits, .beam_indices); plus
        num_beams (1 .. 16, K <= 64), num_return_sequences (<= num_beams), length_penalty (1.0) and early_stopping (False, True,
        "never").  Ties between equal scores go to the lower beam * vocab + token (HF leaves them open).  The KV cache holds B *
        num_beams rows; the prompt is prefilled once per prompt and never copied, and no cache row is reordered (the engine's decode
        attention follows each beam's ancestry instead).  do_sample=True (beam sampling), past_key_values, streamers, inputs_embeds
        and LoRA models raise NotImplementedError, and so does kv_cache_dtype="int8" (the beam-attention kernel reads a bf16 cache;
        None and "bf16" are accepted and change nothing), and so do classifier-free guidance (guidance_scale or any negative_*
        argument) and dola_layers.  The training state is not touched."""
        from ...generation import beam_generate, parse_beam_kwargs
        cfg = parse_beam_kwargs(dict(kwargs, num_beams=num_beams), lora=self._lora_refused,
                                config_eos=getattr(self.config, "eos_token_id", None), config_pad=getattr(self.config, "pad_token_id", None))
        if inputs is None:
            raise ValueError("generate_beams() needs the prompt token ids (`inputs`)")
        imgs = None if images is None else (list(images) if not torch.is_tensor(images) else [im for im in images])
        return beam_generate(self.engine, inputs, cfg.attention_mask, imgs, image_sizes, cfg)

    def save_config(self, out_dir):
        """config.json in HF's key vocabulary (what model.config.save_pretrained leaves next to the weights), plus the tower
        geometry under 'mm_vision_geometry' so that the directory is loadable as --model_name_or_path on its own."""
        import json
        os.makedirs(out_dir, exist_ok=True)
        c, l = self.config, self.engine.l
        d = {"model_type": c.model_type, "architectures": [type(self).__name__], "hidden_size": l["d"], "intermediate_size": l["ffn"],
             "num_hidden_layers": l["layers"], "num_attention_heads": l["heads"], "num_key_value_heads": l.get("kv_heads", l["heads"]),
             "vocab_size": self.engine.vocab, "rms_norm_eps": self.engine.eps, "rope_theta": self.engine.theta, "torch_dtype": "bfloat16",
             "use_cache": False, "mm_vision_geometry": dict(self.engine.v)}
        for k, v in vars(c).items():
            if k.startswith(("mm_", "image_", "tokenizer_")) and isinstance(v, (str, int, float, bool, list, type(None))):
                d[k] = v
        with open(os.path.join(out_dir, "config.json"), "w") as f:
            json.dump(d, f, indent=2)

    def save_pretrained(self, out_dir):
        """Weights in the reference's formats.  Full fine-tune: model.safetensors under the reference state-dict names.  LoRA
        (train/train.py:1708-1717): what peft's save_pretrained(state_dict=get_peft_state_maybe_zero_3(...)) leaves --
        adapter_model.bin (torch.save; keys base_model.model.<module>.lora_{A,B}.weight, adapter name stripped) and
        adapter_config.json -- plus non_lora_trainables.bin (torch.save of the trainable non-LoRA tensors under their
        base_model.model.* names).  peft itself is not installed here: the two adapter files restate its published layout."""
        from safetensors.torch import save_file
        self.save_config(out_dir)
        cpu = lambda d: {k: v.detach().clone().contiguous().cpu() for k, v in d.items()}
        if self.engine.lora:
            import json
            adapters, others = self.engine.lora_state_dict()
            torch.save(cpu({k.replace(".default.weight", ".weight"): v for k, v in adapters.items()}), os.path.join(out_dir, "adapter_model.bin"))
            torch.save(cpu({"base_model.model." + k: v for k, v in others.items()}), os.path.join(out_dir, "non_lora_trainables.bin"))
            lo = self.engine.lora
            with open(os.path.join(out_dir, "adapter_config.json"), "w") as f:
                json.dump({"peft_type": "LORA", "task_type": "CAUSAL_LM", "base_model_name_or_path": getattr(self.config, "_name_or_path", None),
                           "r": lo["r"], "lora_alpha": lo.get("alpha", 16), "lora_dropout": lo.get("dropout", 0.0), "bias": "none",
                           "target_modules": ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"],
                           "fan_in_fan_out": False, "inference_mode": True, "init_lora_weights": True, "modules_to_save": None,
                           "layers_to_transform": None, "layers_pattern": None, "revision": None}, f, indent=2)
            return
        save_file(cpu(self.engine.state_dict()), os.path.join(out_dir, "model.safetensors"))

    def quantize_decoder_(self, fmt="int8"):
        """fmt="int8": the reference's load_8bit for decoding: row-wise int8 copies of every decoder layer's four matrices, the bf16 weights replaced by
        their dequantised values (LlavaEngine.quantize_decoder_; lm_head, embeddings, norms, projector and tower untouched).  generate(),
        generate_batch() and GenerationCache work unchanged and read half the weight bytes per generated token.  state_dict() and
        save_pretrained() then hold the dequantised bf16 weights.  A one-time act: a second call raises; models with unmerged LoRA
        adapters are refused (merge_and_unload() first).  fmt="mxfp4": the 4-bit mode, MXFP4 copies (E2M1 elements, a power-of-two scale per
        32 input features) and 0.27x the weight bytes per generated token; lossy, about 12 % relative error per matrix.  Returns self."""
        self.engine.quantize_decoder_(fmt)
        return self

    @property
    def is_quantized(self):
        return self.engine.is_quantized

    def quantize_base_(self, quant_type="nf4", double_quant=False):
        """QLoRA, the reference's --bits 4 --quant_type nf4 with --lora_enable: the frozen base's decoder matrices become NF4 codes (4.5
        bits per weight, 4.127 with double_quant) and every training pass dequantises one layer at a time into a bf16 scratch
        (LlavaEngine.quantize_base_).  Needs a model with LoRA adapters (ValueError); a one-time act (RuntimeError).  forward(),
        token_logps(), sequence_logps(), label_logits(), preference_loss() and disable_adapter() work on it; generate*, score() and
        everything built on the KV cache raise NotImplementedError until dequantize_base_() or merge_and_unload().  state_dict() holds
        the dequantised bf16 matrices.  Returns self."""
        self.engine.quantize_base_(quant_type, double_quant)
        return self

    def dequantize_base_(self):
        """Back to a plain LoRA model whose bf16 base holds exactly the dequantised weights (LlavaEngine.dequantize_base_).  Returns self."""
        self.engine.dequantize_base_()
        return self

    def merge_and_unload(self):
        """peft's merge_and_unload: W += (alpha / r) B A for every adapted linear (rv_lora_merge_bf16), the adapters are dropped and the
        model is a plain one (config.lora cleared; save_pretrained then writes the full model.safetensors).  The engine keeps the
        projector-only layout (LlavaEngine.merge_lora).  On an NF4 base it is dequantize_base_() followed by the same merge: the merged
        weight is bf16(deq(W) + (alpha / r) B A) and is NOT requantised.  Returns self."""
        if not self.engine.lora:
            raise ValueError("merge_and_unload() needs a model with LoRA adapters")
        self.engine.merge_lora()
        self.config.lora = None
        return self

    @property
    def _lora_refused(self):
        """What the generation parsers take as `lora=`: unmerged adapters that generation may not read.  Every generation entry point
        reads it first, so an NF4 base is refused here by its own row of the refusal table, before the adapters are looked at."""
        if self.engine.nf4 is not None:
            self.engine._check_generation()
        return bool(self.engine.lora) and not self.engine.adapter_decoding

    def enable_adapter_decoding(self, on=True):
        """Let generate(), generate_batch(), generate_beams(), score() and everything built on them (past_key_values,
        prompt_lookup_num_tokens, guidance, DoLa, constraints, share_prefix, kv_cache_dtype="int8") run on the UNMERGED adapters: the
        prompt pass takes the training path's adapted linears without dropout, every cached step two launches per fused projection
        (rv_lora_down_rows_bf16, rv_gemv_lora_bf16).  The adapters are read as they are at every call, so a LoRA run can sample from
        and evaluate its own policy between optimizer steps; the training state is not touched.  on=False restores the refusal.
        Needs a model with adapters (ValueError); quantised decoders with adapters stay refused.  Returns self."""
        if not self.engine.lora:
            raise ValueError("enable_adapter_decoding() needs a model with LoRA adapters")
        self.engine.adapter_decoding = bool(on)
        return self

    @contextlib.contextmanager
    def disable_adapter(self):
        """peft's disable_adapter(): inside the block every adapted linear behaves as if its lora_B were zero -- the frozen base
        model, e.g. the reference policy of GRPO / DPO on adapters -- in forward(), token_logps(), sequence_logps() and generation
        alike.  Evaluation only: loss.backward() inside the block raises.  The earlier state is restored on exit, also on an
        exception.  ValueError on a model without adapters."""
        if not self.engine.lora:
            raise ValueError("disable_adapter() needs a model with LoRA adapters")
        saved, self.engine.adapters_off = self.engine.adapters_off, True
        try:
            yield self
        finally:
            self.engine.adapters_off = saved

    def load_adapter(self, path):
        """Inverse of the LoRA branch of save_pretrained (resume / continued training): adapter_model.bin + non_lora_trainables.bin."""
        e = self.engine
        assert e.lora, "load_adapter needs a LoRA engine"
        strip = lambda k: k[len("base_model.model."):] if k.startswith("base_model.model.") else k
        sd = {}
        for name in ("adapter_model.bin", "non_lora_trainables.bin"):
            f = os.path.join(path, name)
            if os.path.exists(f):
                sd.update({strip(k).replace(".default.weight", ".weight"): v for k, v in torch.load(f, map_location="cpu", weights_only=True).items()})
        if not sd:
            raise FileNotFoundError(f"no adapter_model.bin / non_lora_trainables.bin under {path}")
        from ...params import load_named
        missing, unexpected = load_named(e.lm, sd)
        if missing or unexpected:
            raise KeyError(f"adapter checkpoint does not match the model: missing={missing[:4]} unexpected={unexpected[:4]}")
        if e.master is not None:
            from ... import ops
            e.master.copy_(ops.to_f32(e.lm.flat))

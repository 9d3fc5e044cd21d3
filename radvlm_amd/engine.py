"""LlavaEngine: the MI355X-native forward/backward/optimizer of the LLaVA training step.

No autograd graph and no tracing compiler: forward and backward are explicit sequences of C-ABI kernel launches
(radvlm_amd.ops) over flat bf16 buffers, on the current HIP stream; data-parallel gradient buckets are contiguous
slices of the flat gradient buffer, all-reduced with RCCL on a side stream while backward continues.

Reference semantics followed (paths under /root/reference/finetuning/llava):
  forward    : LlavaLlamaForCausalLM.forward model/language_model/llava_llama.py:69-120 ->
               prepare_inputs_labels_for_multimodal model/llava_arch.py:251-555 -> HF LlamaForCausalLM
               (text mirror model/language_model/modeling_llama.py:1083-1185, :1304-1337), CLIPVisionTower
               model/multimodal_encoder/clip_encoder.py:46-79, mm_projector model/multimodal_projector/builder.py:41-48
  freeze     : tower frozen (clip_encoder.py:42), projector + LM trainable (train/train.py:1613-1665)
  optimizer  : AdamW groups of LLaVATrainer.create_optimizer train/llava_trainer.py:356-433
  grad sync  : what DDP would do for the reference: mean over ranks of per-rank mean losses
"""
import contextlib
import math

import numpy as np
import torch

from . import ops
from .params import (LORA_TARGETS, VP, FlatParams, fast_random_init_, lm_param_shapes, lora_trainable_shapes, portable_init_,
                     vision_param_shapes)
from .splice import build_splice_plan, merged_feature_rows, shifted_labels

BF16 = torch.bfloat16


def _ru(x, m):
    return (x + m - 1) // m * m


class LlavaEngine:
    def __init__(self, geo, device="cuda", merge_type="flat", image_aspect_ratio="square", image_grid_pinpoints=None,
                 max_len=None, init="portable", seed=0, rms_eps=1e-5, rope_theta=10000.0, process_group=None,
                 bucket_layers=1, train_vision_tower=False, lora=None, packed="auto", freeze_lm=False, train_embed_tokens=False,
                 freeze_projector=False,
                 padding_side="right", force_grad_sync=False, recompute=False):
        self.geo = geo
        self.weights_version = 0              # bumped by every write to the weights (weights_changed): a GenerationCache of an older one is stale
        self.w4 = None                        # per layer {name: (packed nibbles, E8M0 scale bytes)} after quantize_decoder_("mxfp4"); likewise
        self.w8 = None                        # per layer {name: (packed int8, fp32 scale)} after quantize_decoder_(); dropped by weights_changed
        self.nf4 = None                       # the NF4 store of the frozen base after quantize_base_() (QLoRA); dequantize_base_() drops it
        assert recompute in (False, True, "auto")
        self.recompute = recompute            # activation recompute policy of the decoder layers (_recompute_layers)
        self.head_rows = "labeled"            # final norm + lm_head + cross entropy on the rows that carry a label ("all": every row)
        self.last_layer_rows = "labeled"      # ... and the last decoder layer's o_proj / norm / MLP (needs head_rows == "labeled")
        self._recompute_cache, self._recompute_forced = {}, False
        # packed (varlen) decoder batches: True / False / "auto" (pack when the samples of a batch differ in length): the decoder
        # then runs on sum(len_b) token rows instead of B * max(len_b) -- no padding rows through GEMMs, norms, CE
        self.packed = packed
        self.v, self.l = geo["vision"], geo["lm"]
        self.device = torch.device(device)
        self.merge_type = merge_type
        self.aspect = image_aspect_ratio
        self.pinpoints = image_grid_pinpoints
        self.max_len = max_len
        self.eps = self.l.get("rms_eps", rms_eps)
        self.theta = self.l.get("rope_theta", rope_theta)
        self.vocab = self.l["vocab"]                                # logical vocabulary (the tables may hold up to 7 zero pad rows)
        assert self.vocab % 8 == 0, "built-in geometries keep the vocabulary a multiple of 8; grow it with resize_token_embeddings"
        self.hd = self.l["d"] // self.l["heads"]
        self.Hkv = self.l.get("kv_heads", self.l["heads"])       # grouped-query attention (Qwen2)
        self.kvd = self.Hkv * self.hd
        self.siglip = self.v.get("kind") == "siglip"
        self.has_cls = not self.siglip
        self.ln_eps = 1e-6 if self.siglip else 1e-5               # siglip_encoder.py:83 / CLIP config default
        # per-channel statistics of the image processor (uint8 inputs are normalised on the device with them)
        self.image_mean = (0.5, 0.5, 0.5) if self.siglip else (0.48145466, 0.4578275, 0.40821073)
        self.image_std = (0.5, 0.5, 0.5) if self.siglip else (0.26862954, 0.26130258, 0.27577711)
        vhd = self.v["d"] // self.v["heads"]
        self.vhd_pad = vhd if vhd in (64, 128) else (64 if vhd < 64 else 128)
        assert vhd <= 128
        self._vis_pad = {}
        self.with_newline = "unpad" in merge_type
        self.side = self.v["image"] // self.v["patch"]
        self.P = self.side * self.side
        self.N_vis = self.P + (1 if self.has_cls else 0)
        self.kp = _ru(3 * self.v["patch"] ** 2, 8)
        self.train_tower = train_vision_tower
        self.lora = dict(lora) if lora else None   # {"r": 64, "alpha": 16, "dropout": 0.05}
        self.freeze_lm = bool(freeze_lm) and not self.lora
        self.base = None
        if self.lora:
            # LoRA (BASELINE config 5): the language model is a frozen bf16 store; only adapters + projector are
            # trainable, so gradients / AdamW state / the DP all-reduce cover ~2 % of the parameters
            assert not train_vision_tower
            r = self.lora["r"]
            self.lora_scale = self.lora.get("alpha", 16) / r
            self.lora_p = float(self.lora.get("dropout", 0.0))
            self.base = FlatParams(lm_param_shapes(geo, False), self.device)
            self.lm = FlatParams(lora_trainable_shapes(geo, r, self.with_newline), self.device)
            self.vis = FlatParams(vision_param_shapes(geo), self.device)
        elif freeze_lm:
            # projector-only stage (tune_mm_mlp_adapter / mm_tunable_parts="mm_mlp_adapter", train/train.py:1613-1640): tower and
            # language model are frozen stores; the trainable flat buffer holds the projector (+ image_newline) alone -- the
            # backward computes input gradients through the frozen decoder and no weight gradients for it.  With train_vision_tower
            # (mm_tunable_parts="mm_vision_tower,mm_mlp_adapter": tower + projector, frozen LM) the tower joins that buffer, in front.
            from collections import OrderedDict
            full = lm_param_shapes(geo, self.with_newline)
            self.base = FlatParams(lm_param_shapes(geo, False), self.device)
            # train_embed_tokens: tune_mm_mlp_adapter + mm_use_im_start_end makes the INPUT embeddings trainable as well
            # (llava_arch.py:577-581: get_input_embeddings requires_grad True, get_output_embeddings False)
            keep = lambda k: "mm_projector" in k or k == "model.image_newline" or (train_embed_tokens and k == "model.embed_tokens.weight")
            shapes = OrderedDict(vision_param_shapes(geo)) if train_vision_tower else OrderedDict()
            shapes.update((k, v) for k, v in full.items() if keep(k))
            self.lm = FlatParams(shapes, self.device)
            self.vis = self.lm if train_vision_tower else FlatParams(vision_param_shapes(geo), self.device)
        elif train_vision_tower:
            # mm_tunable_parts contains mm_vision_tower (train/train.py:1658-1661): the tower joins the trainable flat
            # buffer, in front (forward order), so its gradients are the last bucket of the backward pass
            from collections import OrderedDict
            shapes = OrderedDict(vision_param_shapes(geo))
            shapes.update(lm_param_shapes(geo, self.with_newline))
            self.lm = FlatParams(shapes, self.device)
            self.vis = self.lm
        else:
            self.lm = FlatParams(lm_param_shapes(geo, self.with_newline), self.device)
            self.vis = FlatParams(vision_param_shapes(geo), self.device)
        # Tensors of the trainable buffer that stay FROZEN (any subset of mm_tunable_parts, train/train.py:1613-1665): their gradients are
        # still computed where a kernel produces them anyway, then zeroed before the norm / clip, and AdamW skips them.
        #   * mm_mlp_adapter absent  -> the projector;
        #   * mm_language_model absent -> image_newline too (a parameter of the LM group there: no 'mm_projector' / 'vision_tower' in its name)
        self.frozen_names = set()
        if freeze_projector:
            self.frozen_names |= {n for n in self.lm.names() if "mm_projector" in n}
        if self.freeze_lm and "model.image_newline" in self.lm.offsets:
            self.frozen_names.add("model.image_newline")
        if not [n for n in self.lm.names() if n not in self.frozen_names]:
            raise ValueError("nothing is trainable: mm_tunable_parts must name at least one of mm_vision_tower, mm_mlp_adapter, mm_language_model")
        self.grads = self.lm.like(BF16)
        stores = [self.lm] + ([] if train_vision_tower else [self.vis]) + ([self.base] if self.base is not None else [])
        for k, st in enumerate(stores):
            if init == "portable":
                portable_init_(st, self.l["d"], seed)
            elif init == "fast":
                fast_random_init_(st, self.l["d"], seed + k)
        if self.lora and init in ("portable", "fast"):
            # the projector and the frozen base keep the names (hence values) of the full model; adapters: peft init
            ga = torch.Generator(device=self.device).manual_seed(seed + 7919)      # seeded: two runs of one command start identically
            for n in self.lm.names():
                if n.endswith("lora_B.weight"):
                    self.lm.view(n).zero_()
                elif n.endswith("lora_A.weight") and init == "fast":
                    bound = 1.0 / math.sqrt(self.lm.shapes[n][1])   # kaiming_uniform(a=sqrt(5)) of peft's lora_A
                    self.lm.view(n).copy_((torch.rand(self.lm.shapes[n], device=self.device, generator=ga) * 2 - 1) * bound)
        self.lora_step = 0
        self._patch_w = None
        self._rope = {}
        self._stats = {}
        self.master = self.m = self.vv = None
        self._drop_state8()
        self.opt_step = 0
        self.pg = process_group
        self.world = torch.distributed.get_world_size(process_group) if process_group is not None else 1
        self.bucket_layers = bucket_layers
        from .ddp import FlatGradSync
        # per-layer buckets (~0.4 GB bf16 for the 7B geometry): large transfers suit point-to-point xGMI links
        # force_grad_sync: a one-rank group still issues every bucket's collective (single-GPU rehearsal of the RCCL path)
        self.force_grad_sync = bool(force_grad_sync) and process_group is not None
        self.sync = FlatGradSync(self.grads, process_group, force=self.force_grad_sync) if (self.world > 1 or self.force_grad_sync) else None
        self._select_gemm_launch_shape()
        self.ctx = None
        self.last_preference = None           # pair terms of the last forward(preference=)
        self.last_policy = None               # per-scored-token statistics of the last forward(policy=) / token_logps()
        self.last_distill = None              # per-scored-token divergences of the last forward(distill=)
        self.grad_accum_started = False
        self.loss_scale = 1.0
        import os
        # A/B switch (measurement only): RV_FUSED=0 runs the unfused sequences (GEMM, then rope / swiglu kernels); results are bit-identical
        self.fused = os.environ.get("RV_FUSED", "1") != "0"
        assert padding_side in ("right", "left")
        self.padding_side = padding_side     # config.tokenizer_padding_side (llava_arch.py:520-524)

    def _select_gemm_launch_shape(self):
        """The all-reduce kernels of a data-parallel run share the CUs with backward's GEMMs: one-tile-per-block launches lose part of a
        round to them, a persistent block that cannot start would delay its whole share of the tiles (rv_gemm_select_kernel 40 / 41,
        include/radvlm_hip.h).  The switch is process-wide, so it is set at the top of every forward / backward of THIS engine: a second
        engine in the process (an eval or reference model with or without gradient collectives) cannot leave the wrong shape behind."""
        if self.device.type == "cuda":
            from . import lib
            lib.load().rv_gemm_select_kernel(40 if self.sync is not None else 41)

    # ------------------------------------------------------------------ vocabulary
    def resize_token_embeddings(self, new_vocab):
        """resize_token_embeddings + the mean initialisation of initialize_vision_tokenizer (llava_arch.py:563-575): embed_tokens and
        lm_head grow to `new_vocab` rows, the added rows start as the mean of the existing ones.  Every store that holds one of the
        two tables (the trainable buffer, or the frozen base of LoRA / projector-only runs) is rebuilt with every other tensor copied
        bit for bit; the optimizer state restarts."""
        old_v = self.vocab
        if new_vocab == old_v:
            return
        assert new_vocab > old_v, "the vocabulary only grows"
        import copy
        from collections import OrderedDict
        tables = ("model.embed_tokens.weight", "lm_head.weight")
        phys = _ru(int(new_vocab), 8)        # table rows: a multiple of 8 (GEMM / CE vector width); rows >= new_vocab stay exactly zero
        geo = copy.deepcopy(self.geo)
        geo["lm"]["vocab"] = phys

        def grow(store):
            if not any(t in store.offsets for t in tables):
                return store
            shapes = OrderedDict((n, ((phys, shp[1]) if n in tables else shp)) for n, shp in store.shapes.items())
            new = FlatParams(shapes, self.device)
            for name in store.names():
                src, dst = store.view(name), new.view(name)
                if name in tables:
                    dst[:old_v].copy_(src[:old_v])
                    dst[old_v:new_vocab].copy_(src[:old_v].float().mean(dim=0, keepdim=True).to(BF16).expand(new_vocab - old_v, -1))
                else:
                    dst.copy_(src)
            return new

        tower_shared = self.vis is self.lm
        new_lm = grow(self.lm)
        if self.base is not None:
            self.base = grow(self.base)
        self.vocab = int(new_vocab)
        self.geo, self.l, self.v = geo, geo["lm"], geo["vision"]
        if new_lm is not self.lm:
            self.lm = new_lm
            if tower_shared:
                self.vis = new_lm
            self.grads = new_lm.like(BF16)
            self.master = self.m = self.vv = None
            self._drop_state8()
            self.opt_step = 0
            self.grad_accum_started = False
            if self.sync is not None:
                from .ddp import FlatGradSync
                self.sync = FlatGradSync(self.grads, self.pg, force=self.force_grad_sync)
        self.weights_changed()

    # ------------------------------------------------------------------ weights
    def W(self, name):
        if name in self.lm.offsets:
            return self.lm.view(name)
        return self.base.view(name)

    def G(self, name):
        return self.lm.view(name, self.grads)

    def _layer_views(self, i, flat=None):
        d, F = self.l["d"], self.l["ffn"]
        p = f"model.layers.{i}."
        f = self.lm
        if self.base is not None:
            if flat is not None:
                return {}          # the base weights of a LoRA run have no gradients
            f = self.base
        out = {}
        if self.l.get("qkv_bias"):
            out["bqkv"] = f.fused(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, d + 2 * self.kvd, flat).view(-1)
        if self.nf4 is not None:       # the matrices are views of the one-layer scratch, valid until another layer is asked for
            return dict(out, ln1=f.view(p + "input_layernorm.weight"), ln2=f.view(p + "post_attention_layernorm.weight"), **self._nf4_layer(i))
        return dict(
            out,
            ln1=f.view(p + "input_layernorm.weight", flat),
            qkv=f.fused(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", d + 2 * self.kvd, d, flat),
            o=f.view(p + "self_attn.o_proj.weight", flat),
            ln2=f.view(p + "post_attention_layernorm.weight", flat),
            gu=f.fused(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", 2 * F, d, flat),
            down=f.view(p + "mlp.down_proj.weight", flat),
        )

    def weights_changed(self, tower=True):
        """Call after any in-place edit of the flat parameters (load_state_dict, optimizer step): drops the derived
        copies of tower weights (padded patch / attention projections) when the tower may have changed, and bumps weights_version."""
        self.weights_version += 1
        self.w8 = None           # the int8 copies describe the weights they were made from: a changed engine is a plain bf16 engine again
        self.w4 = None           # the MXFP4 copies likewise
        if tower:
            self._patch_w = None
            self._vis_pad = {}

    def _stat_buffer(self, key, B, H, s_pad):
        """fp32 [B, H, s_pad] softmax-statistics buffers (lse per layer, delta), allocated once (zeroed) and reused every step: the
        kernels overwrite the entries of valid rows only -- no fill kernel per layer.  With ragged data a later batch of the same padded
        shape but shorter samples therefore sees STALE lse / delta in rows >= len (padded layout: the forward and the dQ pass rewrite
        every row below S, so only [S, s_pad) is stale; packed: everything from the sample's length on).  That is harmless by
        construction, not by zeroing, whatever the stale values are (NaN and Inf included): the dK/dV passes reach such rows only in
        their edge tiles, where p AND dS are selected to 0 after lse / delta were used (a select, not a product with 0); the dQ passes
        replace lse by +inf and delta by 0 for rows >= len in their prologue, so p = exp2(-inf) = 0 there
        (tests/test_train_features_gpu.py::test_stale_softmax_statistics_are_masked on the engine,
        tests/test_attention_edges_gpu.py::test_stale_softmax_statistics_never_reach_a_gradient on the kernels)."""
        k = (key, B, H, s_pad)
        buf = self._stats.get(k)
        if buf is None:
            if len(self._stats) > 4 * (self.l["layers"] + self.v["layers"]) + 8:      # shapes change from batch to batch with ragged data: do not hoard
                self._stats.clear()
            buf = self._stats[k] = torch.zeros(B, H, s_pad, dtype=torch.float32, device=self.device)
        return buf

    def _dev(self, a):
        """Host array -> device tensor through pinned memory, asynchronously.  A copy from pageable memory makes the runtime wait for the
        stream first, i.e. the host could never enqueue ahead of the GPU (each of the ~10 index uploads of a step was such a wait: any host
        hiccup then idled the GPU); torch's pinned-memory cache recycles a block only after the copy that used it has finished."""
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        if self.device.type != "cuda" or t.device.type != "cpu":
            return t.to(self.device)
        return (t if t.is_pinned() else t.pin_memory()).to(self.device, non_blocking=True)

    def rope_table(self, S):
        if S not in self._rope:
            self._rope[S] = ops.rope_table(S, self.l["d"] // self.l["heads"], self.theta, self.device)
        return self._rope[S]

    # ------------------------------------------------------------------ vision tower
    def _vision_prepare(self):
        if self._patch_w is None:
            w = self.vis.view(VP + "embeddings.patch_embedding.weight").reshape(self.v["d"], -1)
            pw = torch.zeros(self.v["d"], self.kp, dtype=BF16, device=self.device)
            pw[:, :w.shape[1]] = w
            self._patch_w = pw

    def _vis_attn_weights(self, i):
        """(wqkv [3*H*hp, dv], bqkv [3*H*hp], wo [dv, H*hp]) of tower layer i.  The attention kernels take head_dim 64 or
        128; for any other head_dim (SigLIP-so400m: 72, siglip_encoder.py:185) every head is zero-padded to hp in derived
        copies of the projection weights, so q/k/v come out of the fused GEMM already padded: the padded lanes are exact
        zeros in QK^T and PV and the softmax scale stays head_dim^-0.5."""
        v, f = self.v, self.vis
        dv, H = v["d"], v["heads"]
        hd, hp = dv // H, self.vhd_pad
        p = VP + f"encoder.layers.{i}."
        wqkv = f.fused(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", 3 * dv, dv)
        bqkv = f.fused(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, 3 * dv).view(-1)
        wo = f.view(p + "self_attn.out_proj.weight")
        if hp == hd:
            return wqkv, bqkv, wo
        c = self._vis_pad.get(i)
        if c is None:
            wp = torch.zeros(3, H, hp, dv, dtype=BF16, device=self.device)
            wp[:, :, :hd] = wqkv.view(3, H, hd, dv)
            bp = torch.zeros(3, H, hp, dtype=BF16, device=self.device)
            bp[:, :, :hd] = bqkv.view(3, H, hd)
            op = torch.zeros(dv, H, hp, dtype=BF16, device=self.device)
            op[:, :, :hd] = wo.view(dv, H, hd)
            c = (wp.view(3 * H * hp, dv), bp.view(-1), op.view(dv, H * hp))
            self._vis_pad[i] = c
        return c

    def vision_forward(self, pixels, save=None):
        """pixels bf16 [n,3,H,W] -> the tower's selected hidden state as rows [n*N, dv]:
          CLIP   (clip_encoder.py:68-79): hidden_states[-2], N = P+1 (class token first);
          SigLIP (siglip_encoder.py:568-590): hidden_states[-1] of the encoder WITHOUT its last layer, N = P = 729
        -- both are 'run all layers but the last'.  With `save` (tower tunable) the activations vision_backward needs are kept."""
        v, f = self.v, self.vis
        self._vision_prepare()
        n = pixels.shape[0]
        dv, H = v["d"], v["heads"]
        hd, hp = dv // H, self.vhd_pad
        dvp = H * hp
        N = self.N_vis
        n_pad = _ru(N, 64)
        keep = save is not None
        eps = self.ln_eps
        cols = ops.im2col_patches(pixels, v["patch"], self.kp)
        ln = lambda t, w, b: ops.layernorm_fwd(t, f.view(w), f.view(b), eps=eps, save_stats=keep)
        if self.siglip:
            e = ops.gemm_nt(cols, self._patch_w, bias=f.view(VP + "embeddings.patch_embedding.bias"))
            x = ops.add_pos_rows(e, f.view(VP + "embeddings.position_embedding.weight"), n, self.P)
            st0 = None
        else:
            po = ops.gemm_nt(cols, self._patch_w)
            e = ops.clip_embed(po, f.view(VP + "embeddings.class_embedding"), f.view(VP + "embeddings.position_embedding.weight"),
                               n, self.P, dv)
            r = ln(e, VP + "pre_layrnorm.weight", VP + "pre_layrnorm.bias")
            x, st0 = r if keep else (r, None)
        act_code = ops.ACT_GELU_TANH if self.siglip else ops.ACT_QUICK_GELU
        act_fwd = ops.gelu_tanh_fwd if self.siglip else ops.quick_gelu_fwd
        layers = []
        for i in range(v["layers"] - 1):
            p = VP + f"encoder.layers.{i}."
            r = ln(x, p + "layer_norm1.weight", p + "layer_norm1.bias")
            h, st1 = r if keep else (r, None)
            wqkv, bqkv, wo = self._vis_attn_weights(i)
            qkv = ops.gemm_nt(h, wqkv, bias=bqkv)
            # softmax statistics: one reused buffer for a frozen tower (nobody reads them), one per layer when backward will
            vlse = self._stat_buffer(("vlse", i if keep else -1), n, H, n_pad)
            if hp == 128:     # natural-layout kernel: no V^T copy
                a, lse = ops.attn_fwd(qkv[:, :dvp], qkv[:, dvp:2 * dvp], None, n, N, H, hp, n_pad, causal=False, scale=hd ** -0.5, v=qkv[:, 2 * dvp:], lse=vlse)
            else:
                vT = ops.transpose_heads(qkv[:, 2 * dvp:], n, N, H, hp, n_pad)
                a, lse = ops.attn_fwd(qkv[:, :dvp], qkv[:, dvp:2 * dvp], vT, n, N, H, hp, n_pad, causal=False, scale=hd ** -0.5, lse=vlse)
            x1 = ops.gemm_nt(a, wo, bias=f.view(p + "self_attn.out_proj.bias"), residual=x)
            r = ln(x1, p + "layer_norm2.weight", p + "layer_norm2.bias")
            h2, st2 = r if keep else (r, None)
            if keep:
                z = ops.gemm_nt(h2, f.view(p + "mlp.fc1.weight"), bias=f.view(p + "mlp.fc1.bias"))
                g = act_fwd(z)
            else:
                z = None
                g = ops.gemm_nt(h2, f.view(p + "mlp.fc1.weight"), bias=f.view(p + "mlp.fc1.bias"), act=act_code)
            x2 = ops.gemm_nt(g, f.view(p + "mlp.fc2.weight"), bias=f.view(p + "mlp.fc2.bias"), residual=x1)
            if keep:
                layers.append(dict(x=x, st1=st1, h=h, qkv=qkv, a=a, lse=lse, x1=x1, st2=st2, h2=h2, z=z, g=g))
            x = x2
        if keep:
            save.update(v_cols=cols, v_e=e, v_st0=st0, v_layers=layers, v_n=n)
        return x

    @staticmethod
    def _put(dst, src, acc):
        dst.add_(src) if acc else dst.copy_(src)

    def vision_backward(self, dx, c):
        """Backward of vision_forward: dx = d(selected hidden state) [n*N, dv]; parameter grads -> flat grad views."""
        v, f, G = self.v, self.vis, self.G
        n = c["v_n"]
        dv, H = v["d"], v["heads"]
        hd, hp = dv // H, self.vhd_pad
        dvp = H * hp
        padded = hp != hd
        N = self.N_vis
        n_pad = _ru(N, 64)
        acc = self.grad_accum_started
        W = lambda name: f.view(name)
        act_bwd = ops.gelu_tanh_bwd if self.siglip else ops.quick_gelu_bwd
        for i in reversed(range(v["layers"] - 1)):
            a = c["v_layers"][i]
            p = VP + f"encoder.layers.{i}."
            ops.bias_grad(dx, out=G(p + "mlp.fc2.bias"), accumulate=acc)
            dg = self._linear_bwd(dx, a["g"], W(p + "mlp.fc2.weight"), G(p + "mlp.fc2.weight"))
            dz = act_bwd(dg, a["z"])
            ops.bias_grad(dz, out=G(p + "mlp.fc1.bias"), accumulate=acc)
            dh2 = self._linear_bwd(dz, a["h2"], W(p + "mlp.fc1.weight"), G(p + "mlp.fc1.weight"))
            ops.layernorm_bwd(dh2, a["x1"], W(p + "layer_norm2.weight"), a["st2"], G(p + "layer_norm2.weight"),
                              G(p + "layer_norm2.bias"), dx=dx, dx_add=True, accumulate=acc)
            ops.bias_grad(dx, out=G(p + "self_attn.out_proj.bias"), accumulate=acc)
            wqkv, bqkv, wo = self._vis_attn_weights(i)
            gqkv = f.fused(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", 3 * dv, dv, self.grads)
            gb = f.fused(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, 3 * dv, self.grads).view(-1)
            if padded:   # gradients of the padded copies, valid lanes folded back into the flat views
                gwo = ops.gemm(dx, a["a"], ta=True, tb=True)
                self._put(G(p + "self_attn.out_proj.weight").view(dv, H, hd), gwo.view(dv, H, hp)[:, :, :hd], acc)
                da = ops.gemm(dx, wo, tb=True)
            else:
                da = self._linear_bwd(dx, a["a"], wo, G(p + "self_attn.out_proj.weight"))
            qkv = a["qkv"]
            dqkv = torch.empty_like(qkv)
            ops.attn_bwd(qkv[:, :dvp], qkv[:, dvp:2 * dvp], qkv[:, 2 * dvp:], a["a"], da, a["lse"], n, N, H, hp, n_pad, False,
                         scale=hd ** -0.5, dq=dqkv[:, :dvp], dk=dqkv[:, dvp:2 * dvp], dv=dqkv[:, 2 * dvp:])
            if padded:
                gbp = ops.bias_grad(dqkv)
                self._put(gb.view(3, H, hd), gbp.view(3, H, hp)[:, :, :hd], acc)
                gwp = ops.gemm(dqkv, a["h"], ta=True, tb=True)
                self._put(gqkv.view(3, H, hd, dv), gwp.view(3, H, hp, dv)[:, :, :hd], acc)
                dh = ops.gemm(dqkv, wqkv, tb=True)
            else:
                ops.bias_grad(dqkv, out=gb, accumulate=acc)
                dh = self._linear_bwd(dqkv, a["h"], wqkv, gqkv)
            ops.layernorm_bwd(dh, a["x"], W(p + "layer_norm1.weight"), a["st1"], G(p + "layer_norm1.weight"),
                              G(p + "layer_norm1.bias"), dx=dx, dx_add=True, accumulate=acc)
            c["v_layers"][i] = None
            self._bucket_done(p + "layer_norm1.weight", p + "mlp.fc2.bias")
        if self.siglip:
            de = dx
        else:
            de = ops.layernorm_bwd(dx, c["v_e"], W(VP + "pre_layrnorm.weight"), c["v_st0"], G(VP + "pre_layrnorm.weight"),
                                   G(VP + "pre_layrnorm.bias"), accumulate=acc)
        # embeddings: position table = sum over images, class token = rows t = 0, patch conv = wgrad over im2col rows
        de2 = de.view(n, N * dv)
        ops.bias_grad(de2, out=G(VP + "embeddings.position_embedding.weight").view(-1), accumulate=acc)
        if self.siglip:
            ops.bias_grad(de, out=G(VP + "embeddings.patch_embedding.bias"), accumulate=acc)
            dpo = de
        else:
            ops.bias_grad(de2[:, :dv], out=G(VP + "embeddings.class_embedding"), accumulate=acc)
            drop_cls = (torch.arange(n * self.P, device=self.device, dtype=torch.int32)
                        + torch.arange(n, device=self.device, dtype=torch.int32).repeat_interleave(self.P) + 1)
            dpo = ops.gather_rows(drop_cls, dv, de)
        dwp = ops.gemm(dpo, c["v_cols"], ta=True, tb=True)
        gp = G(VP + "embeddings.patch_embedding.weight").view(dv, -1)
        self._put(gp, dwp[:, :gp.shape[1]], acc)
        # the last encoder layer and post_layernorm do not feed the selected hidden state: their gradients are zero
        last = VP + f"encoder.layers.{v['layers'] - 1}."
        s0, _ = self.lm.span(last + "layer_norm1.weight", last + "layer_norm1.weight")
        _, e1 = self.lm.span(VP + "post_layernorm.bias", VP + "post_layernorm.bias")
        if not acc:
            self.grads[s0:e1].zero_()
        first = VP + ("embeddings.patch_embedding.weight" if self.siglip else "embeddings.class_embedding")
        self._bucket_done(first, VP + ("embeddings.position_embedding.weight" if self.siglip else "pre_layrnorm.bias"))
        self._bucket_done(last + "layer_norm1.weight", VP + "post_layernorm.bias")

    def encode_images(self, pixels, save=None, plan=None):
        """encode_images (llava_arch.py:192-196): tower (patch features, CLS dropped) then mlp2x_gelu projector.
        Returns the feature table [n*P + n_extra + 1, d]: projector rows, then the rows anyres_max creates by bilinear
        down-sampling (llava_arch.py:381-392; a 4-tap weighted gather of projector rows), then image_newline."""
        n = pixels.shape[0]
        rs = (plan or {}).get("resample")
        mp = (plan or {}).get("maxpool")
        n_extra = plan["n_extra_rows"] if (rs or mp) else 0
        d = self.l["d"]
        hid = self.vision_forward(pixels, save=save if (self.train_tower and save is not None) else None)
        if self.has_cls:
            drop_cls = (torch.arange(n * self.P, device=self.device, dtype=torch.int32)
                        + torch.arange(n, device=self.device, dtype=torch.int32).repeat_interleave(self.P) + 1)
            f0 = ops.gather_rows(drop_cls, self.v["d"], hid)
        else:
            f0 = hid
        z1 = ops.gemm_nt(f0, self.W("model.mm_projector.0.weight"), bias=self.W("model.mm_projector.0.bias"))
        a1 = ops.gelu_fwd(z1)
        table = torch.empty(n * self.P + n_extra + 1, d, dtype=BF16, device=self.device)
        ops.gemm_nt(a1, self.W("model.mm_projector.2.weight"), bias=self.W("model.mm_projector.2.bias"), out=table[:n * self.P])
        if rs:
            t = lambda k: self._dev(rs[k])
            ops.weighted_segment_sum_rows(table, t("fwd_off"), t("fwd_pos"), t("fwd_w"), t("fwd_out"), table)
        if mp:
            which = ops.max4_rows_fwd(table, self._dev(mp["idx4"]), self._dev(mp["out"]), table)
            if save is not None:
                save["pool_which"] = which
        if self.with_newline:
            table[n * self.P + n_extra].copy_(self.W("model.image_newline"))
        else:
            table[n * self.P + n_extra].zero_()
        if save is not None:
            save.update(f0=f0, z1=z1, a1=a1)
        return table

    # ------------------------------------------------------------------ forward
    def plan(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """Host-side index planning (numpy); images: list of [3,H,W] or [T,3,H,W] tensors."""
        tiles = [1 if im.ndim == 3 else im.shape[0] for im in images]
        n_proj = sum(tiles) * self.P
        extra = dict(next=n_proj, src=[], w=[])     # rows created by anyres_max down-sampling follow the projector rows
        rows, r0, image_rows = [], 0, []
        for i, t in enumerate(tiles):
            e0 = extra["next"]
            rows.append(merged_feature_rows(r0, t, self.side, self.merge_type, self.aspect,
                                            tuple(image_sizes[i]) if image_sizes is not None else None, self.pinpoints,
                                            self.v["image"], extra=extra))
            image_rows.append((r0, r0 + t * self.P, e0, extra["next"]))
            r0 += t * self.P
        n_extra = extra["next"] - n_proj
        ids = np.asarray(input_ids)
        am = np.asarray(attention_mask).astype(bool) if attention_mask is not None else np.ones_like(ids, dtype=bool)
        lab = np.asarray(labels) if labels is not None else np.full_like(ids, -100)
        plan = build_splice_plan(ids, am, lab, rows, n_proj + n_extra, self.max_len, self.padding_side)
        plan["n_feat_rows"] = n_proj + n_extra
        plan["n_proj_rows"] = n_proj
        plan["n_extra_rows"] = n_extra
        plan["image_rows"] = image_rows      # per image: its projector rows [p0, p1) and anyres_max-created rows [e0, e1) of the feature table
        if extra.get("pool_src"):   # maxpool2x2: created rows = elementwise max of four projector rows
            win = np.concatenate(extra["pool_src"]).astype(np.int32)
            assert (plan["feat_pos"][np.unique(win)] < 0).all()
            plan["maxpool"] = dict(idx4=win.reshape(-1), out=np.concatenate(extra["pool_out"]).astype(np.int32))
        if extra["src"]:
            src = np.concatenate(extra["src"]).reshape(-1)            # [4 * n_resampled] projector rows
            w = np.concatenate(extra["w"]).reshape(-1).astype(np.float32)
            assert (plan["feat_pos"][np.unique(src)] < 0).all()       # a down-sampled grid's sources are never spliced directly
            order = np.argsort(src, kind="stable")
            usrc, starts = np.unique(src[order], return_index=True)
            n_rs = src.shape[0] // 4
            assert n_rs == n_extra or not extra.get("pool_src"), "anyres_max resampling and maxpool2x2 are mutually exclusive merges"
            plan["resample"] = dict(
                fwd_off=np.arange(0, 4 * n_rs + 1, 4, dtype=np.int32), fwd_pos=src.astype(np.int32), fwd_w=w,
                fwd_out=(n_proj + np.arange(n_rs)).astype(np.int32),
                # adjoint: for every source row, the (created row, weight) pairs it feeds
                adj_off=np.concatenate([starts, [src.shape[0]]]).astype(np.int32),
                adj_pos=(n_proj + order // 4).astype(np.int32), adj_w=w[order], adj_out=usrc.astype(np.int32))
        return plan

    # ------------------------------------------------------------------ decoder layer
    def activation_bytes_per_row(self):
        """bf16 bytes one decoder layer keeps per token row for backward: x, h1, q|k|v, attn, x_mid, h2, gate|up, act (+ fp32 statistics)."""
        d, F = self.l["d"], self.l["ffn"]
        n = 2 * (6 * d + 2 * self.kvd + 3 * F) + 4 * (2 + self.l["heads"])
        if getattr(self, "lora", None):     # the seven adapted modules keep their r-wide down-projections
            n += 2 * 7 * self.lora["r"]
        if getattr(self, "hd", 128) != 128:  # head_dim 64 kernels read a V^T copy
            n += 2 * self.kvd
        return n

    def _recompute_layers(self, M):
        """How many decoder layers (the first n) re-run their forward in backward.  False: none -- the activations of all layers stay
        resident (~95 GB for 32 pairs x 704 tokens of the 7B model: what 288 GB of HBM are for); True: all; "auto": as few as the free
        device memory requires (measured on the 7B geometry: one 32k-token sample of the reference recipe, finetune_radio_7b.sh:79, still
        fits whole -- 236 GiB peak; a 50k-token sample recomputes 12 of 32 layers)."""
        L = self.l["layers"]
        if self.recompute is True:
            return L
        if not self.recompute or self.device.type != "cuda":
            return 0
        if self._recompute_forced:           # a step ran out of memory under "auto": the retry (and the same shape later) keeps layer inputs only
            return L
        hit = self._recompute_cache.get(M)
        if hit is not None:
            return hit
        per_layer = M * self.activation_bytes_per_row()
        free, _ = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)     # torch's cached, unused blocks
        # head room: logits (bf16 + dlogits in place) + the lm_head input gradient, one layer's recomputed activations and gradients
        budget = 0.85 * free - (4 * M * self.l["vocab"] + 3 * per_layer)
        keep = int(max(0.0, budget) // max(per_layer + 2 * M * self.l["d"], 1))
        self._recompute_cache[M] = max(0, L - keep)     # one decision per row count: later steps see less free memory only because of this one's caches
        return self._recompute_cache[M]

    def _layer_forward(self, i, x, g, rows=None):
        """One decoder layer (modeling_llama.py:852-911) on token rows x -> (x_out, the activations backward needs).
        rows (LAST layer only; int32 device index, -1 = zero pad row): the rows whose output anything downstream reads -- the labelled rows
        (forward()).  Attention still runs on every row (all rows are keys / values), but o_proj, the residual, the second norm and the
        MLP are evaluated on the gathered rows alone: x_out and the saved x_mid, rstd2, h2, gu, act then have rows.numel() rows."""
        d, F, H = self.l["d"], self.l["ffn"], self.l["heads"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        B, S, s_pad, lens, cu, pos, cs = g["B"], g["S"], g["s_pad"], g["lens"], g["cu"], g["pos"], g["cs"]
        lv = self._layer_views(i)
        h1, rstd1 = ops.rmsnorm_fwd(x, lv["ln1"], self.eps)
        sv = {}
        if self.lora:
            qkv = self._lora_linear(h1, lv["qkv"], i, self._MODS_QKV(d), sv, bias=lv.get("bqkv"))   # frozen q/k/v biases (Qwen2)
            ops.rope_inplace(qkv, cs, S, H + Hkv, hd, 1, 1, positions=pos)   # q heads then k heads: one run of H + Hkv heads
        elif not self.fused:
            qkv = ops.gemm_nt(h1, lv["qkv"], bias=lv.get("bqkv"))
            ops.rope_inplace(qkv, cs, S, H + Hkv, hd, 1, 1, positions=pos)
        else:       # q|k|v projection with the rotary embedding in the GEMM epilogue
            qkv = ops.gemm_rope(h1, lv["qkv"], cs, S, H + Hkv, hd, bias=lv.get("bqkv"), positions=pos)
        if hd == 128:     # natural-layout kernel: K and V tiles are staged as they lie in memory (no V^T copy)
            attn, lse = ops.attn_fwd(qkv[:, :d], qkv[:, d:d + kvd], None, B, S, H, hd, s_pad, causal=True, lens=lens, kv_heads=Hkv, cu=cu,
                                     v=qkv[:, d + kvd:], lse=self._stat_buffer(("lse", i), B, H, s_pad))
        else:
            vT = ops.transpose_heads(qkv[:, d + kvd:], B, S, Hkv, hd, s_pad, cu=cu)
            attn, lse = ops.attn_fwd(qkv[:, :d], qkv[:, d:d + kvd], vT, B, S, H, hd, s_pad, causal=True, lens=lens, kv_heads=Hkv, cu=cu)
        attn_sel = None
        if rows is not None:
            attn_sel = ops.gather_rows(rows, d, attn)
            if self.lora:
                x_mid = self._lora_linear(attn_sel, lv["o"], i, self._MODS_O(d), sv, residual=ops.gather_rows(rows, d, x))
            else:
                x_mid = ops.gemm_nt(attn_sel, lv["o"], residual=ops.gather_rows(rows, d, x))
        elif self.lora:
            x_mid = self._lora_linear(attn, lv["o"], i, self._MODS_O(d), sv, residual=x)
        else:
            x_mid = ops.gemm_nt(attn, lv["o"], residual=x)
        h2, rstd2 = ops.rmsnorm_fwd(x_mid, lv["ln2"], self.eps)
        if self.lora:
            gu = self._lora_linear(h2, lv["gu"], i, self._MODS_GU(F), sv)
            act = ops.swiglu_fwd(gu, F)
        elif not self.fused:
            gu = ops.gemm_nt(h2, lv["gu"])
            act = ops.swiglu_fwd(gu, F)
        else:       # gate|up projection and silu(gate) * up in one launch
            gu, act = ops.gemm_swiglu_fwd(h2, lv["gu"], F)
        if self.lora:
            x_out = self._lora_linear(act, lv["down"], i, self._MODS_DOWN(d), sv, residual=x_mid)
        else:
            x_out = ops.gemm_nt(act, lv["down"], residual=x_mid)
        acts = dict(x=x, rstd1=rstd1, h1=h1, qkv=qkv, attn=attn, lse=lse, x_mid=x_mid, rstd2=rstd2, h2=h2, gu=gu, act=act, lora=sv)
        if attn_sel is not None:
            acts["attn_sel"] = attn_sel
        return x_out, acts

    def _pixels(self, images):
        """The images of a batch (list of [3,H,W] / [T,3,H,W], host or device, float or uint8) -> one bf16 [n,3,H,W] device tensor."""
        dev = self.device
        pix = torch.cat([(im if im.ndim == 4 else im[None]) for im in images], 0)
        if pix.device.type == "cpu" and not pix.is_pinned() and dev.type == "cuda":
            pix = pix.pin_memory()                                                          # pinned: the copy does not stall the stream
        pix = pix.to(dev, non_blocking=True)          # images already on the device (HF Trainer._prepare_inputs moves them) pass through
        if pix.dtype == torch.uint8:
            # device-side normalisation: uint8 HWC tiles from the host (resize / crop / pad only), rescale + (x - mean) / std
            # + channel-first layout + bf16 cast here, in the processors' own fp32 arithmetic
            pix = ops.normalize_tiles_u8(pix.contiguous(), self.v["image"], self.image_mean, self.image_std, mode=1 if self.siglip else 0)
        else:
            pix = pix if pix.dtype == BF16 else ops.to_bf16(pix.float())
        return pix.contiguous()

    def forward(self, input_ids, attention_mask, labels, images, image_sizes=None, want_logits=False, loss_scale=None, policy=None,
                preference=None, _score_only=False, distill=None, _label_logits=False):
        """One training forward. Returns loss (fp32 device tensor [1], never scaled); keeps the context for backward().
        loss_scale multiplies the GRADIENTS only (default: self.loss_scale; a trainer sets 1 / gradient_accumulation_steps, which is
        what HF Trainer.training_step back-propagates, HF:trainer.py training_step `loss / gradient_accumulation_steps`).
        policy: None (the cross entropy) or a policy.PolicyTerms: the GRPO token loss (rv_policy_loss_bf16) takes the cross entropy's
        place on the same logits buffer, in place; everything before it and all of backward() are the same.  The loss returned is then
        sum(weight * loss) over the scored tokens, and self.last_policy holds the per-token statistics (see _policy_loss).
        preference: None or a preference.PreferenceTerms: the batch is P (chosen, rejected) pairs as 2 P sequences and the DPO loss takes
        the cross entropy's place the same way, as three launches on the same logits buffer (see _preference_loss); the loss returned
        is dpo_alpha * mean pair loss + gamma * SFT, and self.last_preference holds the pair terms.
        distill: None or a distill.DistillTerms: knowledge distillation takes the cross entropy's place the same way, one launch of
        rv_distill_loss_bf16 on the logits buffer and the teacher's rows (see _distill_loss); the loss returned is sum(weight * jsd) over
        the scored tokens, and self.last_distill holds the per-token divergences.  It combines with none of the other three.
        _score_only (token_logps): the same pass with the statistics alone -- no dlogits, no activations kept, no context.
        _label_logits (label_logits, with _score_only): no loss at all; self.last_label_logits gets the scored rows of the logits buffer."""
        dev = self.device
        l = self.l
        d, F, H, V, L = l["d"], l["ffn"], l["heads"], l["vocab"], l["layers"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        self._select_gemm_launch_shape()
        plan = self.plan(input_ids, attention_mask, labels, images, image_sizes)
        self.lora_step += 1
        pix = self._pixels(images)
        ctx = dict(plan=plan)
        table = self.encode_images(pix, save=ctx, plan=plan)
        B = int(np.asarray(input_ids).shape[0])   # samples (a sample may hold several images: images are consumed in order)
        S = plan["S"]
        s_pad = _ru(S, 64)
        lens_np = plan["lens"]
        ragged = bool((lens_np != S).any())
        packed = bool(self.packed) if self.packed != "auto" else ragged
        if self.padding_side == "left" and ragged:
            # left padding (llava_arch.py:520-524): the reference discards the spliced position_ids in training (:534-545), so
            # every row keeps positions arange(S) and a short sample starts at position S - len.  That is exactly the packed
            # layout with explicit positions = padded column index: valid tokens only, nothing computed for the pad rows.
            packed = True
            first = S - lens_np
            bad = [b for b in range(len(lens_np)) if 0 < lens_np[b] < S and plan["labels"][b, first[b]] != -100]
            if bad:
                raise ValueError(f"left padding: sample {bad[0]} has a label on its first token; the reference's loss would then read the "
                                 "logits of a padding row (shifted CE), which is not defined here")
        cu = pos = valid_idx = None
        if packed:
            valid = plan["attention_mask"].reshape(-1)
            p2k = np.cumsum(valid) - 1                                        # padded flat row -> packed row
            remap = lambda a: np.where(a >= 0, p2k[np.maximum(a, 0)], -1).astype(np.int32)
            plan = dict(plan, idx=plan["idx"][valid], feat_pos=remap(plan["feat_pos"]), newline_pos=remap(plan["newline_pos"]),
                        tok_pos=remap(plan["tok_pos"]))
            ctx["plan"] = plan
            M = int(valid.sum())
            cu = self._dev(np.concatenate([[0], np.cumsum(lens_np)]).astype(np.int32))
            pos = self._dev((np.arange(B * S, dtype=np.int32) % S)[valid])
            valid_idx = np.nonzero(valid)[0]
            lens = None
        else:
            M = B * S
            lens = self._dev(lens_np)
        idx = self._dev(plan["idx"])
        x = ops.gather_rows(idx, d, self.W("model.embed_tokens.weight"), table)
        cs = self.rope_table(S)
        geom = dict(B=B, S=S, s_pad=s_pad, lens=lens, cu=cu, pos=pos, cs=cs)
        # activation recompute (the reference's --gradient_checkpointing, train/train.py:164,1505-1513): layers [0, n_re) keep only their
        # input and re-run their forward inside backward (bit-identical: the kernels are deterministic, LoRA dropout masks regenerable)
        n_re = 0 if _score_only else self._recompute_layers(M)
        tgt = shifted_labels(plan["labels"])
        if tgt.size and int(tgt.max()) >= self.vocab:     # torch's cross_entropy raises on an out-of-range target too
            raise IndexError(f"label {int(tgt.max())} is out of range for a vocabulary of {self.vocab}")
        count = int((tgt != -100).sum())
        inv = (1.0 / count) if count > 0 else float("nan")
        scored = (tgt != -100).sum(1)                     # per sample: the scored tokens of policy.PolicyTerms
        tgt = tgt.reshape(-1)
        if packed:
            tgt = tgt[valid_idx]
        # The loss reads the logits of the rows that carry a label and of no other row (modeling_llama.py:1326-1337: ignore_index rows
        # contribute neither to the loss nor -- their dlogits being exactly zero -- to any gradient), and nothing after the last decoder
        # layer mixes rows.  So the final norm, the lm_head product, the cross entropy and their backward run on the LABELLED rows only
        # (an instruction sample labels its answer tokens: 64 of 704 rows in the BASELINE workload, 9 % of a 3 x 5.9 TFLOP head).  Same
        # loss, same gradients (the dropped terms are exact zeros); HF's `logits_to_keep` is the same idea.  head_rows = "all" restores
        # the full product (A/B, tests); callers that want logits get the full fp32 product either way.
        head_idx = None
        lab_rows = np.nonzero(tgt != -100)[0]
        if self.head_rows == "labeled" and 0 < lab_rows.size <= 0.75 * M:
            n_sel = _ru(int(lab_rows.size), 64)           # whole 64-row groups: the weight gradient contracts over these rows
            head_idx = np.full(n_sel, -1, dtype=np.int32)
            head_idx[:lab_rows.size] = lab_rows
            t_sel = np.full(n_sel, -100, dtype=tgt.dtype)
            t_sel[:lab_rows.size] = tgt[lab_rows]
            tgt = t_sel
        # The same holds one step earlier: a row of the LAST decoder layer's output feeds its own logits row and nothing else, so that layer's
        # o_proj, second norm and MLP (304 MFLOP per row at 7B widths, x 3 with backward) are dead for the unlabelled rows as well; its
        # attention still runs on every row.  Not taken when the caller wants every row's logits.  (LoRA: the adapters' dropout masks are
        # indexed by the element position in the gathered tensor -- another mask than the all-rows run draws, regenerated identically in
        # backward.)
        last_sel = head_idx is not None and self.last_layer_rows == "labeled" and not want_logits
        layers = []
        for i in range(L):
            x_out, acts = self._layer_forward(i, x, geom, rows=self._dev(head_idx) if (last_sel and i == L - 1) else None)
            if not _score_only:
                layers.append(dict(x=x, lora={}) if i < n_re else acts)
            x = x_out
        ctx["geom"], ctx["n_recomputed"] = geom, n_re
        if head_idx is None or last_sel:
            x_head = x
        else:
            x_head = ops.gather_rows(self._dev(head_idx), d, x)          # pad rows are zero and carry no label
        hN, rstdN = ops.rmsnorm_fwd(x_head, self.W("model.norm.weight"), self.eps)
        logits = ops.gemm_nt(hN, self.W("lm_head.weight"))
        tgt_t = self._dev(tgt)
        logits_out = None
        if want_logits:
            # callers get the reference's fp32 [B, S, V] (llava_llama.py:69-120 -> logits.float()): the lm_head GEMM once more with
            # fp32 output, i.e. the accumulators without the bf16 store the training path's loss reads (eval / tests only)
            hN_all = hN if head_idx is None else ops.rmsnorm_fwd(x, self.W("model.norm.weight"), self.eps)[0]
            lf = ops.gemm_nt(hN_all, self.W("lm_head.weight"), out_dtype=torch.float32)
            if packed:          # padded shape, padding rows zero
                logits_out = torch.zeros(B * S, V, dtype=torch.float32, device=dev)
                logits_out[self._dev(valid_idx)] = lf
            else:
                logits_out = lf
            logits_out = logits_out.view(B, S, V)[..., :self.vocab]
        # CE writes dlogits (scaled by loss_scale/count/world) over the logits buffer
        gscale = (self.loss_scale if loss_scale is None else loss_scale) / self.world
        if distill is not None and (policy is not None or preference is not None or _score_only):
            raise ValueError("distill= does not combine with policy=, preference= or a score-only pass")
        if _label_logits:
            assert _score_only and policy is None and preference is None
            n, _, _ = self._scored_rows(logits.shape[0], lab_rows, head_idx is not None, scored)
            sel = slice(n) if head_idx is not None else self._dev(lab_rows.astype(np.int64))
            self.last_label_logits = dict(logits=logits[sel], scored=np.asarray(scored))
            loss = None
        elif distill is not None:
            loss = self._distill_loss(logits, tgt_t, lab_rows, head_idx is not None, scored, distill, gscale)
        elif preference is not None:
            if policy is not None or _score_only:
                raise ValueError("preference= does not combine with policy= or a score-only pass")
            loss = self._preference_loss(logits, tgt_t, lab_rows, head_idx is not None, scored, preference, gscale)
        elif policy is None and not _score_only:
            loss, _ = self._cross_entropy(logits, tgt_t, self.vocab, inv, gscale)   # V = table rows (pad rows included), CE sees the logical vocabulary
        else:
            loss = self._policy_loss(logits, tgt_t, lab_rows, head_idx is not None, scored, policy, gscale, grad=not _score_only)
        if _score_only:                                  # token_logps(): nothing is kept for a backward pass
            self.ctx = None
            return loss
        ctx.update(B=B, S=S, M=M, s_pad=s_pad, lens=lens, cu=cu, pos=pos, layers=layers, x_last=x_head, rstdN=rstdN, hN=hN, dlogits=logits,
                   table_rows=table.shape[0], count=count, head_idx=head_idx, head_rows=int(lab_rows.size), last_sel=last_sel)
        self.ctx = ctx
        self.last_logits = logits_out
        return loss

    @contextlib.contextmanager
    def _eval_form(self, *also):
        """Eval form: the adapters' input dropout is off inside the block (module.eval() in the reference) and lora_p is put back after
        it, with the attributes named in `also` ("lora_step", "ctx") where the block's forward pass writes them."""
        saved = dict({a: getattr(self, a) for a in also}, lora_p=getattr(self, "lora_p", 0.0))
        self.lora_p = 0.0
        try:
            yield
        finally:
            for name, value in saved.items():
                setattr(self, name, value)

    def forward_embeds(self, inputs_embeds, attention_mask=None, labels=None):
        """The decoder + head on caller-supplied input embeddings -- the call form of LlavaLlamaForCausalLM.forward with `inputs_embeds`
        given (llava_llama.py:69-120: the multimodal splice is skipped and super().forward runs on the embeddings; what generate() and
        eval-loss loops use).  inputs_embeds [B, S, d]; attention_mask [B, S] (None = all valid; right or left padded); labels [B, S] or
        None.  Returns (loss or None, fp32 logits [B, S, vocab]); nothing is kept for a backward pass."""
        dev, l = self.device, self.l
        d, V, L = l["d"], l["vocab"], l["layers"]
        x3 = torch.as_tensor(inputs_embeds)
        B, S = int(x3.shape[0]), int(x3.shape[1])
        assert x3.shape[2] == d, f"inputs_embeds last dimension {x3.shape[2]} != hidden size {d}"
        am = np.ones((B, S), dtype=bool) if attention_mask is None else np.asarray(torch.as_tensor(attention_mask).cpu()).astype(bool)
        lens_np = am.sum(1).astype(np.int32)
        right_padded = all(am[b, :lens_np[b]].all() for b in range(B))
        x = x3.to(dev).reshape(B * S, d)
        x = (x if x.dtype == BF16 else ops.to_bf16(x.float().contiguous())).contiguous()
        s_pad = _ru(S, 64)
        cu = pos = valid_idx = lens = None
        if right_padded:
            M, lens = B * S, self._dev(lens_np)
        else:   # any other mask: valid tokens only, positions = padded column index (HF: position_ids = arange(S) when none are passed)
            valid = am.reshape(-1)
            valid_idx = np.nonzero(valid)[0]
            M = int(valid.sum())
            cu = self._dev(np.concatenate([[0], np.cumsum(lens_np)]).astype(np.int32))
            pos = self._dev((np.arange(B * S, dtype=np.int32) % S)[valid])
            x = x[self._dev(valid_idx.astype(np.int64))].contiguous()
        geom = dict(B=B, S=S, s_pad=s_pad, lens=lens, cu=cu, pos=pos, cs=self.rope_table(S))
        with self._eval_form("lora_step"):
            for i in range(L):
                x, _ = self._layer_forward(i, x, geom)
        hN, _ = ops.rmsnorm_fwd(x, self.W("model.norm.weight"), self.eps)
        lf = ops.gemm_nt(hN, self.W("lm_head.weight"), out_dtype=torch.float32)
        if valid_idx is not None:
            full = torch.zeros(B * S, lf.shape[1], dtype=torch.float32, device=dev)
            full[self._dev(valid_idx.astype(np.int64))] = lf
            lf = full
        logits = lf.view(B, S, -1)[..., :self.vocab]
        loss = None
        if labels is not None:
            lab = np.asarray(torch.as_tensor(labels).cpu()).astype(np.int64)
            tgt = shifted_labels(np.where(am, lab, -100))
            if tgt.size and int(tgt.max()) >= self.vocab:
                raise IndexError(f"label {int(tgt.max())} is out of range for a vocabulary of {self.vocab}")
            count = int((tgt != -100).sum())
            tgt = tgt.reshape(-1)
            if valid_idx is not None:
                tgt = tgt[valid_idx]
            logits_bf = ops.gemm_nt(hN, self.W("lm_head.weight"))     # the loss reads bf16 logits, as the training path does
            loss, _ = self._cross_entropy(logits_bf, self._dev(tgt), self.vocab, (1.0 / count) if count else float("nan"), 0.0)
        self.last_logits = logits
        return loss, logits

    # ------------------------------------------------------------------ generation (KV-cached greedy decode)
    # Rows up to this many per decode GEMM go to rv_gemv_bf16, larger batches to the tiled GEMM.  Same-box A/B of the two at M = 1, 4,
    # 16, 32 on the 7B decode shapes (DESIGN.md "Decode", profiles/decode_ab_gemv.jsonl): the skinny kernel wins at every M on every
    # shape except the 152,064-row Qwen2 lm_head, where it wins at M <= 4 only (0.93x at 16, 0.79x at 32: one K slice, and the tiled
    # GEMM's 256-row tiles amortise the weight stream over the rows better there).
    gemv_max_m = 32
    gemv_max_m_wide = 4          # weights with >= 65,536 rows
    # On a quantised engine (quantize_decoder_) the skinny route reads the int8 copy; False forces the bf16 kernel on the same
    # (dequantised) weights.  The two are bit-identical, so this switch changes time only: it is the A/B arm of tools/decode_bench.py --w8.
    w8_decode = True
    # The same switch for the MXFP4 copy (quantize_decoder_("mxfp4")): the A/B arm of tools/decode_bench.py --w4.
    w4_decode = True

    def _takes_skinny(self, w, rows, skinny=False):
        """Does a decode product of `rows` rows with the weight w take the skinny kernel?  skinny=True: whatever the row count
        (<= ops.GEMV_MAX_M, which the kernel enforces) and the weight's height."""
        max_m = self.gemv_max_m_wide if w.shape[0] >= 65536 else self.gemv_max_m
        return skinny or rows <= min(max_m, ops.GEMV_MAX_M)

    def _decode_linear(self, x, w, bias=None, residual=None, out_dtype=BF16, wq=None, skinny=False):
        """wq: the weight's quantised copy (packed, scales) from _layer_wq, int8 or MXFP4 by its dtype, or None.
        skinny: the skinny kernel whatever the row count (<= ops.GEMV_MAX_M) and the weight's height -- verify_step, whose rows must
        carry the bits of the one-row decode step, which always takes that kernel."""
        if not self._takes_skinny(w, x.shape[0], skinny):
            return ops.gemm_nt(x, w, bias=bias, residual=residual, out_dtype=out_dtype)
        if wq is None:
            return ops.gemv(x, w, bias=bias, residual=residual, out_dtype=out_dtype)
        if wq[0].dtype != torch.uint8:
            return ops.gemv_w8(x, wq[0], wq[1], w.shape[1], bias=bias, residual=residual, out_dtype=out_dtype)
        if self._w4_cell_takes_bf16(w.shape[0], w.shape[1], x.shape[0]):
            return ops.gemv(x, w, bias=bias, residual=residual, out_dtype=out_dtype)
        return ops.gemv_w4(x, wq[0], wq[1], w.shape[1], bias=bias, residual=residual, out_dtype=out_dtype)

    # (N, K) -> the measured row counts at which rv_gemv_w4_bf16 did NOT beat rv_gemv_bf16 on the same weight by more than the bf16 arm's
    # own spread (max - min of its 20 samples); those launches go back to the bf16 kernel, which gives the same bits.  A launch of M rows
    # reads the cell of the next measured M (1, 4, 8, 16, 32) at or above its own.  Record: profiles/decode_ab_gemv.jsonl, mode w4,
    # build "default", field w4_faster_by_more_than_bf16_spread (tests/test_w4_host.py holds this table to that record).  The Qwen2
    # q|k|v and o_proj cells are 1.02x - 1.11x on the medians, inside the spread; the three 7B cells are 1.3x - 1.8x on the medians and
    # fail the bar on one slow bf16 sample each.  Every cell that stays with the 4-bit kernel is 1.23x - 2.28x faster on that record.
    W4_BF16_CELLS = {(12288, 4096): (1,), (4096, 4096): (4, 16), (4608, 3584): (1, 4, 8, 16, 32), (3584, 3584): (1, 4, 8, 16, 32)}

    def _w4_cell_takes_bf16(self, N, K, M):
        cells = self.W4_BF16_CELLS.get((N, K))
        return bool(cells) and next(m for m in (1, 4, 8, 16, 32) if M <= m) in cells

    def _layer_wq(self, i):
        """The quantised copies the decode GEMMs of layer i read: the int8 pairs, the MXFP4 pairs, or none (bf16 on the same weights)."""
        if self.w4 is not None:
            return self.w4[i] if self.w4_decode else {}
        return self.w8[i] if (self.w8 is not None and self.w8_decode) else {}

    @property
    def is_quantized(self):
        return self.w8 is not None or self.w4 is not None

    W8_MATRICES = ("qkv", "o", "gu", "down")

    def quantize_decoder_(self, fmt="int8"):
        """fmt="int8" (the default).  Weight-only int8 for decoding (the reference's load_8bit): every layer's fused q|k|v, o_proj, fused gate|up and down_proj are
        quantised row-wise (s = max|row| / 127, q = clamp(rint(w / s), -127, 127)) and the bf16 weight is OVERWRITTEN with the
        dequantised bf16(float(q) * s), which is the model's weight from then on: prefill, extend, forward and state_dict() read it
        through the unchanged bf16 code, and decode steps read (q, s) through rv_gemv_w8_bf16, which rebuilds the same bits -- one
        function, half the weight bytes per generated token.  lm_head, embeddings, norms, biases, projector and tower stay as they
        are.  The int8 copies are kept beside the bf16 weights (about 1.5x the memory of these matrices).  A one-time act: a second
        call raises (quantising the dequantised weight would round again), and any later write to the weights (load_state_dict,
        optimizer_step, merge_lora_, resize_token_embeddings) drops the int8 copies.  When optimizer state exists, the fp32 master copy
        of the quantised matrices is rewritten from the dequantised weights (as merge_lora_ does), so a later optimizer_step starts from
        them instead of restoring the unquantised values.  Non-finite weights are outside the contract.

        fmt="mxfp4".  The same act with OCP Microscaling FP4 (the 4-bit mode): E2M1 elements, one power-of-two scale per block of 32
        consecutive input features (e = floor(log2 max|block|) - 2, nearest value with ties to the even code, saturating).  The
        quantised weight is exactly a bf16 number and replaces the bf16 weight; the copies go to `w4` ({name: (packed nibbles, scale
        bytes)} per layer, 4.25 bits per weight, about 1.27x the memory of these matrices with the bf16 copy kept) and decode steps
        read them through rv_gemv_w4_bf16, bit-identical to the bf16 kernel on the same weights.  Everything else is as for int8.
        This format is lossy: about 12 % relative Frobenius error per matrix against about 1 % for int8."""
        if fmt not in ("int8", "mxfp4"):
            raise ValueError(f"quantize_decoder_(fmt={fmt!r}): expected 'int8' or 'mxfp4'")
        if self.lora:                        # also with adapter_decoding on: the quantised skinny kernels carry no adapter
            raise NotImplementedError("quantize_decoder_() on a model with LoRA adapters: merge them into the base weights first with "
                                      "model.merge_and_unload()")
        if self.is_quantized:
            raise RuntimeError("quantize_decoder_(): the decoder is already quantised; a second pass would round the weights again")
        quantize = ops.quantize_rows_w8 if fmt == "int8" else ops.quantize_rows_mxfp4
        copies = []
        for i in range(self.l["layers"]):
            lv = self._layer_views(i)
            copies.append({n: quantize(lv[n]) for n in self.W8_MATRICES})
        self.weights_changed(tower=False)
        if fmt == "int8":
            self.w8 = copies
        else:
            self.w4 = copies
        if self.master is not None and self.base is None:
            for i in range(self.l["layers"]):
                for t, _, _ in LORA_TARGETS:
                    off, n = self.lm.offsets[f"model.layers.{i}.{t}.weight"]
                    self.master[off:off + n].copy_(ops.to_f32(self.lm.flat[off:off + n]))

    # ------------------------------------------------------------------ NF4 frozen base (QLoRA)
    def quantize_base_(self, quant_type="nf4", double_quant=False):
        """QLoRA (the reference's --bits 4 --quant_type nf4 with --lora_enable): the seven decoder matrices of every layer of the frozen
        base are quantised to NF4 (rv_nf4_quantize_bf16; 64 weights per block, one fp32 absmax each: 4.5 bits per weight) and the frozen
        store is rebuilt WITHOUT them -- embeddings, norms, q/k/v biases and lm_head stay bf16.  double_quant: the absmax values are
        themselves stored as one byte each, with one fp32 scale per 256 blocks and one fp32 mean per tensor (4.127 bits per weight); the
        dequantised weights then use the rebuilt absmax, so the setting changes the model (tests/nf4_ref.py says exactly how).
        From then on _layer_views(i) dequantises layer i into the one-layer bf16 scratch with one rv_nf4_dequant_bf16 launch and returns
        views of it: forward, recompute and backward run through the unchanged GEMMs.  state_dict() gives the dequantised matrices;
        dequantize_base_() makes the engine a plain LoRA engine on exactly those weights.  A one-time act (a second call raises
        RuntimeError), LoRA engines only (ValueError otherwise).  During the act the bf16 base and the NF4 store are both resident: the
        peak is bf16 + NF4, the saving comes after it.  Generation, scoring and the cached steps are refused on an NF4 base
        (NotImplementedError); the forward-only training-path calls work.  Non-finite weights are outside the contract."""
        from collections import OrderedDict
        from . import nf4 as N
        if quant_type != "nf4":
            raise ValueError(f"quantize_base_(quant_type={quant_type!r}): only 'nf4' is built")
        if not self.lora:
            raise ValueError("quantize_base_() needs a LoRA engine: a 4-bit base is frozen, only adapters on top of it can train")
        if self.nf4 is not None:
            raise RuntimeError("quantize_base_(): the base is already NF4; a second pass would round the weights again")
        plan = N.BasePlan(self.geo, double_quant)
        dev, u8, f32 = self.device, torch.uint8, torch.float32
        st = dict(plan=plan, codes=torch.zeros(plan.code_bytes, dtype=u8, device=dev), absmax=None, absmax_codes=None, scale2=None, offset=None)
        if plan.double_quant:
            st.update(absmax_codes=torch.zeros(plan.nblocks, dtype=u8, device=dev), scale2=torch.zeros(plan.nscale2, dtype=f32, device=dev))
            offsets = np.zeros(len(plan.tensors), np.float32)
            tmp = torch.empty(max(t["nblocks"] for t in plan.tensors.values()), dtype=f32, device=dev)
        else:
            st["absmax"] = torch.zeros(plan.nblocks, dtype=f32, device=dev)
        for name, t in plan.tensors.items():
            w = self.base.view(name).reshape(-1)
            codes = st["codes"][t["code"]:t["code"] + (t["n"] + 1) // 2]
            if not plan.double_quant:
                ops.nf4_quantize(w, codes, st["absmax"][t["block"]:t["block"] + t["nblocks"]])
                continue
            # the second level, once per tensor at load: the mean in its fixed float64 order on the host (nf4.absmax_offset), the
            # subtraction in fp32 there too, the 8-bit codes and scales by the optimizer state's own quantiser
            ops.nf4_quantize(w, codes, tmp[:t["nblocks"]])
            am = tmp[:t["nblocks"]].cpu().numpy()
            offsets[t["slot"]] = off = N.absmax_offset(am)
            ops.adam8_quantize(self._dev((am - off).astype(np.float32)), 0, codes=st["absmax_codes"][t["block"]:t["block"] + t["nblocks"]],
                               absmax=st["scale2"][t["scale2"]:t["scale2"] + t["nscale2"]])
        if plan.double_quant:
            st["offset"] = self._dev(offsets)
        keep = OrderedDict((k, v) for k, v in self.base.shapes.items() if k not in plan.tensors)
        new = FlatParams(keep, dev)
        for k in keep:
            new.view(k).copy_(self.base.view(k))
        self.base = new                        # the bf16 matrices go with the old store
        # One scratch, one stream.  INVARIANT: no caller holds two layers' views at once -- _layer_forward, backward and the recompute
        # inside it take layer i's views, finish every GEMM that reads them, and only then ask for another layer; the launches are
        # ordered on the one stream the engine enqueues on.  `resident` is the layer the scratch holds (an immediately repeated request
        # for it, as by backward after a recomputed forward, launches nothing).
        tabs = [plan.table(plan.names(i)) for i in range(plan.layers)]
        scratch = torch.zeros(plan.scratch_numel, dtype=BF16, device=dev)
        views = {}
        for key, first, last in (("qkv", "self_attn.q_proj", "self_attn.v_proj"), ("o", "self_attn.o_proj", "self_attn.o_proj"),
                                 ("gu", "mlp.gate_proj", "mlp.up_proj"), ("down", "mlp.down_proj", "mlp.down_proj")):
            a, b = plan.tensors[f"model.layers.0.{first}.weight"], plan.tensors[f"model.layers.0.{last}.weight"]
            cols = a["shape"][1]
            views[key] = scratch[a["dst"]:b["dst"] + b["n"]].view(-1, cols)
        st.update(scratch=scratch, views=views, tables=tabs, tables_dev=[self._dev(tab) for tab, _ in tabs], resident=-1)
        self.nf4 = st
        self.weights_changed(tower=False)

    def _nf4_dequant(self, i, dst, table=None):
        """One rv_nf4_dequant_bf16 launch for layer i into the bf16 buffer dst; table: (host table, chunks) with other destinations
        than the scratch offsets."""
        st = self.nf4
        per = st["plan"].per_layer
        tab, nch = st["tables"][i] if table is None else table
        tab_dev = st["tables_dev"][i] if table is None else self._dev(tab)
        if st["plan"].double_quant:
            ops.nf4_dequant(st["codes"], tab_dev, tab, nch, dst, absmax_codes=st["absmax_codes"], scale2=st["scale2"],
                            offset=st["offset"][i * per:(i + 1) * per])
        else:
            ops.nf4_dequant(st["codes"], tab_dev, tab, nch, dst, absmax=st["absmax"])

    def _nf4_layer(self, i):
        """Layer i's four matrices as views of the scratch, dequantised now unless the scratch already holds that layer."""
        st = self.nf4
        if st["resident"] != i:
            st["resident"] = -1
            self._nf4_dequant(i, st["scratch"])
            st["resident"] = i
        return st["views"]

    def dequantize_base_(self):
        """The inverse act of quantize_base_() as far as there is one: the engine becomes a plain LoRA engine whose bf16 base holds
        exactly the dequantised weights (what state_dict() gave), the NF4 store and the scratch are dropped.  RuntimeError without an
        NF4 base."""
        if self.nf4 is None:
            raise RuntimeError("dequantize_base_(): the base is not quantised")
        plan = self.nf4["plan"]
        full = FlatParams(lm_param_shapes(self.geo, False), self.device)
        for k in self.base.names():
            full.view(k).copy_(self.base.view(k))
        for i in range(plan.layers):
            names = plan.names(i)
            self._nf4_dequant(i, full.flat, table=plan.table(names, dst={k: full.offsets[k][0] for k in names}))
        self.base, self.nf4 = full, None
        self.weights_changed(tower=False)

    def base_weight_bytes(self):
        """Bytes of the seven decoder matrices of every layer as this engine stores them: the NF4 store after quantize_base_()
        (nf4.BasePlan.base_weight_bytes; the one-layer scratch is not part of it), 2 bytes per weight otherwise."""
        from . import nf4 as N
        return self.nf4["plan"].base_weight_bytes() if self.nf4 is not None else N.bf16_matrix_bytes(self.geo)

    # Generation on unmerged adapters (model.enable_adapter_decoding()): off, every generation entry point refuses a LoRA engine as it
    # always has; on, prefill() runs the training path's adapted linears in eval form and the cached steps go through
    # _decode_lora_linear.  The adapters are read from self.lm on every call, so an optimizer_step() is seen by the next token.
    adapter_decoding = False
    # True: every adapted linear, on the training path and the decode path alike, behaves as if every lora_B were zero -- the frozen
    # base model, peft's disable_adapter() (model.disable_adapter()).  Forward only: backward() raises.
    adapters_off = False

    def _check_generation(self):
        if self.nf4 is not None:             # the refusal table's row: no decode kernel reads the NF4 store
            from .generation import refuse_combinations
            refuse_combinations({"nf4"}, "generation")
        if self.lora and not self.adapter_decoding:
            raise NotImplementedError("generation with LoRA adapters: merge them into the base weights first with "
                                      "model.merge_and_unload() (the reference merges adapters before evaluation), or decode on the "
                                      "live adapters with model.enable_adapter_decoding() (engine.adapter_decoding)")

    def _decode_lora_linear(self, x, w, i, mods, bias=None, residual=None, wq=None, skinny=False):
        """_decode_linear for a fused projection of layer i whose modules `mods` (name, c0, c1) may carry adapters.  No adapters: that
        call.  Rows that take the skinny route: one rv_lora_down_rows_bf16 launch for the modules' t = (alpha / r) x A_j^T and one
        rv_gemv_lora_bf16 launch, the adapter riding rv_gemv_bf16 (a row's bits do not depend on the row count, as there).  More rows:
        _lora_linear's arithmetic without dropout.  adapters_off: a zero B -- on the skinny route that is rv_gemv_bf16's result bit
        for bit (the kernel's contract), so the two adapter launches are skipped."""
        if not self.lora:
            return self._decode_linear(x, w, bias=bias, residual=residual, wq=wq, skinny=skinny)
        if not self._takes_skinny(w, x.shape[0], skinny):
            return self._lora_linear(x, w, i, mods, {}, residual=residual, bias=bias, p=0.0)
        if self.adapters_off:
            return ops.gemv(x, w, bias=bias, residual=residual)
        pre = f"model.layers.{i}."
        r = self.lora["r"]
        t = ops.lora_down_rows(x, [self.W(f"{pre}{lname}.lora_A.weight") for lname, _, _ in mods], self.lora_scale)
        table = [(c0, c1, j * r, self.W(f"{pre}{lname}.lora_B.weight")) for j, (lname, c0, c1) in enumerate(mods)]
        return ops.gemv_lora(x, w, t, table, bias=bias, residual=residual)

    # An int8-dtype KVCache is stored as (int8, fp32 scale) tensors and read by rv_attn_decode_kv8_bf16; False keeps it as bf16 tensors
    # that hold the dequantised values (written by the same quantise kernels) and reads it with rv_attn_decode_bf16.  The two are
    # bit-identical, so this switch changes time and memory only: it is the A/B arm of tools/decode_bench.py --kv8.
    kv8_decode = True

    @staticmethod
    def _kv_dtype(dtype):
        if dtype in (None, "bf16"):
            return "bf16"
        if dtype == "int8":
            return "int8"
        raise ValueError(f"kv cache dtype must be None, 'bf16' or 'int8', got {dtype!r}")

    def kv_cache_bytes(self, B, L_max, dtype="bf16"):
        """Bytes of a KVCache of B sequences x L_max positions: bf16 K|V rows of every layer (2 * 2*kvd per position and layer), or for
        dtype "int8" their int8 bytes and one fp32 scale per (kv head, K / V) group (2*kvd + 8*Hkv).  What new_kv_cache(B, L_max, dtype)
        .nbytes() reports: with kv8_decode False an int8-dtype cache is stored dequantised and costs the bf16 bytes."""
        per = 2 * self.kvd * 2
        if self._kv_dtype(dtype) == "int8" and self.kv8_decode:
            per = 2 * self.kvd + 8 * self.Hkv
        return self.l["layers"] * int(B) * int(L_max) * per

    def free_device_bytes(self):
        """Device memory a new allocation can take: free HBM plus what torch's caching allocator holds unused."""
        free, _ = torch.cuda.mem_get_info(self.device)
        return int(free + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))

    def _kv_layers(self, B, L_max, dtype):
        """The per-layer tensors of an empty cache: (layers, scales or None)."""
        L, dev = self.l["layers"], self.device
        if dtype == "int8" and self.kv8_decode:
            return ([torch.zeros(B, L_max, 2 * self.kvd, dtype=torch.int8, device=dev) for _ in range(L)],
                    [torch.ones(B, L_max, 2 * self.Hkv, dtype=torch.float32, device=dev) for _ in range(L)])
        return [torch.zeros(B, L_max, 2 * self.kvd, dtype=BF16, device=dev) for _ in range(L)], None

    def new_kv_cache(self, B, L_max, dtype="bf16"):
        """An empty KVCache of B sequences (every length 0) x L_max positions, to be filled by prefill(..., cache=, slots=).  dtype "int8":
        K|V rows are quantised per (position, kv head, K / V) group as they are written (KVCache)."""
        dtype = self._kv_dtype(dtype)
        layers, scales = self._kv_layers(B, L_max, dtype)
        return KVCache(layers, np.zeros(B, np.int64), L_max, dtype=dtype, scales=scales)

    def _kv_write_rows(self, cache_layer, scale_layer, src, rows):
        """An int8-dtype cache's prefill write: quantise the K|V rows src into flat cache rows `rows` (either storage)."""
        if scale_layer is not None:
            ops.kv_quantize_rows(src, rows, self.Hkv, self.hd, cache=(cache_layer, scale_layer))
        else:
            ops.kv_quantize_rows(src, rows, self.Hkv, self.hd, xhat=cache_layer)

    @staticmethod
    def _refuse_int8(cache, what):
        if cache is not None and getattr(cache, "dtype", "bf16") == "int8":
            raise NotImplementedError(f"{what} on an int8 KV cache: only prefill() and the plain decode_step() read it; "
                                      "use a bf16 cache (kv_cache_dtype=None)")

    @staticmethod
    def _refuse_pressed(cache, what):
        if cache is not None and getattr(cache, "pos_off", None) is not None:
            raise NotImplementedError(f"{what} on a cache compressed by prompt_kv_budget: its slots are not its positions, and only "
                                      "prefill() and the plain decode_step() know the offset (KVCache.pos_off)")

    @staticmethod
    def _slot_rows(slots, B, cache, ok=True):
        """slots= of prefill() and extend() as an int64 array: one distinct row of `cache` per prompt (ok: the caller's own count check)."""
        seq = np.asarray(slots, dtype=np.int64).reshape(-1)
        if not ok or seq.shape[0] != B or np.unique(seq).shape[0] != B or (seq < 0).any() or (seq >= cache.B).any():
            raise ValueError(f"slots must be {B} distinct indices into the cache's {cache.B} sequences, got {seq.tolist()}")
        return seq

    def _tokens_dev(self, tokens):       # the token ids of a cached step (int, host or device) as a device int32 tensor
        return tokens.to(self.device, torch.int32) if torch.is_tensor(tokens) else self._dev(np.asarray(tokens, dtype=np.int32))

    def _head_logits(self, x, skinny=False, tapped=None):
        """The tail of a generation entry point: final norm, lm_head in fp32, the vocabulary's columns -> fp32 [rows, vocab].  tapped
        (DoLa: the tapped rows, in tap_layers' order): (those logits, the candidates' fp32 [n, rows, vocab]) through _tap_logits."""
        hN, _ = ops.rmsnorm_fwd(x, self.W("model.norm.weight"), self.eps)
        if tapped is None:
            return self._decode_linear(hN, self.W("lm_head.weight"), out_dtype=torch.float32, skinny=skinny)[:, :self.vocab]
        logits, cand = self._tap_logits(hN, tapped)
        return logits[:, :self.vocab], cand

    def _cached_layer(self, i, x, cs, pos, attend, skinny=False):
        """Decoder layer i of the KV-cached path on the rows x [M, d] -> [M, d]: RMSNorm, fused q|k|v (_decode_lora_linear: quantised
        copies and live adapters ride there), RoPE in place at the rows' positions `pos` from the table cs, attend(i, qkv) -- the
        entry point's own K|V write (qkv[:, d:]) and attention of qkv[:, :d] over the cached keys -- then o_proj + residual, RMSNorm,
        gate|up, SwiGLU, down + residual.  skinny: as in _decode_linear.  Every statement makes a new tensor: x is left as it is."""
        d, F = self.l["d"], self.l["ffn"]
        lv, wq = self._layer_views(i), self._layer_wq(i)
        h1, _ = ops.rmsnorm_fwd(x, lv["ln1"], self.eps)
        qkv = self._decode_lora_linear(h1, lv["qkv"], i, self._MODS_QKV(d), bias=lv.get("bqkv"), wq=wq.get("qkv"), skinny=skinny)
        ops.rope_inplace(qkv, cs, 1, self.l["heads"] + self.Hkv, self.hd, 1, 1, positions=pos)
        x_mid = self._decode_lora_linear(attend(i, qkv), lv["o"], i, self._MODS_O(d), residual=x, wq=wq.get("o"), skinny=skinny)
        h2, _ = ops.rmsnorm_fwd(x_mid, lv["ln2"], self.eps)
        act = ops.swiglu_fwd(self._decode_lora_linear(h2, lv["gu"], i, self._MODS_GU(F), wq=wq.get("gu"), skinny=skinny), F)
        return self._decode_lora_linear(act, lv["down"], i, self._MODS_DOWN(d), residual=x_mid, wq=wq.get("down"), skinny=skinny)

    def prefill(self, input_ids, attention_mask=None, images=None, image_sizes=None, max_new_tokens=0, cache=None, slots=None, kv_dtype=None,
                tap_layers=None, attn_layers=None, attn_mean=False, compress=None):
        """The prompt pass of generation: multimodal splice (plan / encode_images, as in forward) and every decoder layer in the packed
        varlen layout, sequence b at cache rows and positions 0 .. len_b - 1 whatever the padding side.  Each layer's post-RoPE K|V rows go
        into a KVCache of len_b + max_new_tokens slots per sequence; the activations are dropped.  No loss, no saved context (self.ctx and
        the optimizer state are not touched).  images None: text-only prompts, embedded directly.
        cache / slots (generate_batch): sequence b's K|V rows go instead into slot slots[b] of the existing KVCache `cache` (positions
        0 .. len_b - 1; the slot's later positions are left as they are) and cache.lens[slots[b]] = len_b; the arithmetic is the same, so
        the logits and K|V rows are the bits prefill() gives the same group on a cache of cache.L_max positions.  Other slots are untouched.
        kv_dtype ("bf16" / "int8"; None: the passed cache's, else "bf16"): with "int8" each layer's K|V rows are quantised on their way
        into the cache (ops.kv_quantize_rows); the prompt's own attention still runs on the unquantised activations, so the returned
        logits are those of a bf16 cache.
        tap_layers (DoLa, generate(dola_layers=)): a tuple of n distinct layer numbers c in [0, layers); the call then returns a third
        value, fp32 [n, B, vocab]: lm_head of every sequence's last prompt row as it ENTERS decoder layer c (c = 0: the spliced
        embedding row; c = k: the residual stream after layer k), without the final norm, in tap_layers' order (_tap_logits).  Only
        those rows are kept, never whole activations; the cache and the mature logits are bit for bit those of the call without it.
        attn_layers / attn_mean (generate(output_attentions=True)): as in decode_step, for the first generated token -- the call then
        returns (cache, logits, attn), attn a list in attn_layers' order of fp32 [B, H, S] ([B, S] under attn_mean, S the longest
        prompt): the attention probabilities of every sequence's LAST prompt row over its cache positions 0 .. len_b - 1, zeros beyond.
        For each asked layer that row of q is gathered from the layer's own post-RoPE acts["qkv"] (rows cu[1:] - 1) and
        ops.attn_decode_probs runs on those B rows against the cache layer just written, kv_len = len_b; the prompt pass's own
        attention is not touched and only those rows are kept.  The cache and the logits are the bits of the call without it.  Not
        combined with cache= / slots=, kv_dtype "int8" or tap_layers= (NotImplementedError).
        compress (generate(prompt_kv_budget=N, prompt_kv_window=w, prompt_kv_pool=k)): (N, w, k), SnapKV prompt-cache compression.  A
        sequence of P_b <= N prompt rows is cached as ever.  A longer one keeps N positions per layer and kv head: inside the layer loop
        its window rows' attention votes for the prefix keys (ops.kv_votes on the layer's post-RoPE acts["qkv"]), ops.kv_select keeps the
        N - w best max-pooled positions in ascending order plus the w window positions, and ops.kv_gather copies their K|V straight
        from acts["qkv"] into slots 0 .. N - 1 of the cache layer: the full prompt is never cached.  cache.lens[b] is then N and
        cache.pos_off[b] = P_b - N, so decode_step appends at slot lens and rotates at position lens + pos_off.  Without cache= the
        returned cache has max_b min(P_b, N) + max_new_tokens slots and pos_off None when no sequence was compressed; with cache= /
        slots= only those rows' lens and pos_off are set.  The prompt's own attention and the returned logits are not touched.
        self.kvpress_trace (None; a test may set a list) receives (layer, votes, keep) per layer.  Not combined with attn_layers=,
        tap_layers= or an int8 cache (NotImplementedError).
        Returns (cache, fp32 logits [B, vocab] of every sequence's last prompt row), plus the third value above when asked for."""
        self._check_generation()
        dev, l = self.device, self.l
        d, L, kvd = l["d"], l["layers"], self.kvd
        taps = self._check_taps(tap_layers)
        want = self._check_attn_layers(attn_layers)
        if compress is not None:
            cN, cw, ck = (int(v) for v in compress)
            if not (1 <= cw <= ops.KVPRESS_MAX_WINDOW and cN > cw and 1 <= ck <= ops.KVPRESS_MAX_POOL and ck % 2 == 1):
                raise ValueError(f"compress=(N, w, k) needs 1 <= w <= {ops.KVPRESS_MAX_WINDOW}, N > w and an odd k in "
                                 f"[1, {ops.KVPRESS_MAX_POOL}], got {tuple(compress)!r}")
            for name, v in (("attn_layers", want), ("tap_layers", taps)):
                if v is not None:
                    raise NotImplementedError(f"prefill(compress=...) with {name}= (prompt_kv_budget / prompt_kv_window): the compressed "
                                              "prompt pass hands out neither attention rows nor tapped rows")
            if (kv_dtype is not None and self._kv_dtype(kv_dtype) == "int8") or getattr(cache, "dtype", "bf16") == "int8":
                raise NotImplementedError("prefill(compress=...) (prompt_kv_budget / prompt_kv_window) with an int8 KV cache: the gather "
                                          "kernel writes bf16 rows only")
        if want is not None:
            if cache is not None or slots is not None:
                raise NotImplementedError("prefill(attn_layers=...) with cache= / slots=: attention maps are read from a cache of the "
                                          "call's own sequences")
            if kv_dtype is not None and self._kv_dtype(kv_dtype) == "int8":
                raise NotImplementedError("prefill(attn_layers=...) with an int8 KV cache: the probability kernel reads a bf16 cache only")
            if taps is not None:
                raise NotImplementedError("prefill(attn_layers=...) with tap_layers=: attention maps run on the plain prompt pass")
        if cache is not None:
            if kv_dtype is not None and self._kv_dtype(kv_dtype) != cache.dtype:
                raise ValueError(f"kv_dtype {kv_dtype!r} does not match the passed cache's dtype {cache.dtype!r}")
            kv_dtype = cache.dtype
        kv_dtype = self._kv_dtype(kv_dtype)
        from .splice import IMAGE_TOKEN_INDEX
        ids = np.asarray(input_ids)
        B = int(ids.shape[0])
        imgs = [] if images is None else list(images)
        if not imgs and (ids == IMAGE_TOKEN_INDEX).any():
            raise ValueError("the prompt holds an image token but no images were passed")
        plan = self.plan(ids, attention_mask, None, imgs, image_sizes)
        if imgs:
            table = self.encode_images(self._pixels(imgs), plan=plan)
        else:
            table = torch.zeros(1, d, dtype=BF16, device=dev)          # no feature rows: the splice reads token embeddings only
        lens = plan["lens"].astype(np.int64)
        if (lens == 0).any():
            raise ValueError("generation needs at least one prompt token per sequence")
        valid = plan["attention_mask"].reshape(-1)
        S = int(lens.max())
        kept = lens if compress is None else np.minimum(lens, cN)       # cache slots each prompt takes
        pressed = kept < lens
        if cache is None:
            L_max = int(kept.max()) + int(max_new_tokens)
            seq = np.arange(B)
        else:
            seq = self._slot_rows(slots, B, cache)
            L_max = cache.L_max
            if (kept + int(max_new_tokens) > L_max).any():
                raise ValueError(f"the prompts need {int(kept.max()) + int(max_new_tokens)} positions, the cache holds {L_max}")
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        pos = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
        # the rope table of the uncompressed call: a compressed prompt's positions outrun its cache slots
        rope_S = L_max if compress is None else max(L_max, S + int(max_new_tokens))
        geom = dict(B=B, S=S, s_pad=_ru(S, 64), lens=None, cu=self._dev(cu), pos=self._dev(pos), cs=self.rope_table(rope_S))
        x = ops.gather_rows(self._dev(plan["idx"][valid].astype(np.int32)), d, self.W("model.embed_tokens.weight"), table)
        plain = [b for b in range(B) if not pressed[b]]                 # sequences cached whole, by index_copy_ as ever
        rows = None
        if plain:
            rows = self._dev(np.concatenate([seq[b] * L_max + np.arange(lens[b]) for b in plain]).astype(np.int64))   # cache rows
        src = None
        if pressed.any():
            flags_dev, seq_dev = self._dev(pressed.astype(np.int32)), self._dev(seq.astype(np.int32))
            votes = torch.empty(B, self.Hkv, S - cw, dtype=torch.float32, device=dev)
            keep = torch.empty(B, self.Hkv, cN, dtype=torch.int32, device=dev)
            if plain:
                src = self._dev(np.concatenate([cu[b] + np.arange(lens[b]) for b in plain]).astype(np.int64))
        layers = []
        if cache is None and kv_dtype == "int8":
            cache = self.new_kv_cache(B, L_max, kv_dtype)           # seq = 0 .. B - 1: filled like a passed cache's slots
        if taps is not None:
            tap_rows, tapped = self._dev((cu[1:] - 1).astype(np.int32)), {}
        if want is not None:
            last_rows, lens_dev, attn = self._dev((cu[1:] - 1).astype(np.int32)), self._dev(lens.astype(np.int32)), {}
        with self._eval_form():              # live adapters (adapter_decoding): as in forward_embeds; lora_step is only read
            for i in range(L):
                if taps is not None and i in taps:
                    tapped[i] = ops.gather_rows(tap_rows, d, x)
                x, acts = self._layer_forward(i, x, geom)
                if cache is None:
                    kv = torch.zeros(B, L_max, 2 * kvd, dtype=BF16, device=dev)
                    layers.append(kv)
                else:
                    kv = cache.layers[i]
                if kv_dtype == "int8":
                    self._kv_write_rows(kv, cache.scales[i] if cache.scales is not None else None, acts["qkv"][:, d:], rows)
                elif not pressed.any():
                    kv.view(-1, 2 * kvd).index_copy_(0, rows, acts["qkv"][:, d:])
                else:
                    if plain:
                        kv.view(-1, 2 * kvd).index_copy_(0, rows, acts["qkv"][:, d:].index_select(0, src))
                    ops.kv_votes(acts["qkv"], geom["cu"], l["heads"], self.Hkv, self.hd, cw, S, flags=flags_dev, out=votes)
                    ops.kv_select(votes, geom["cu"], cN, cw, ck, flags=flags_dev, out=keep)
                    ops.kv_gather(acts["qkv"][:, d:], geom["cu"], keep, seq_dev, kv, self.Hkv, self.hd, flags=flags_dev)
                    if self.kvpress_trace is not None:
                        self.kvpress_trace.append((i, votes.clone(), keep.clone()))
                if want is not None and i in want:
                    attn[i] = ops.attn_decode_probs(ops.gather_rows(last_rows, d, acts["qkv"]), kv, lens_dev, l["heads"], self.Hkv, self.hd, S,
                                                    per_head=not attn_mean, mean=bool(attn_mean))[1 if attn_mean else 0]
                del acts
        x = ops.gather_rows(self._dev((cu[1:] - 1).astype(np.int32)), d, x)       # every sequence's last prompt row
        out = self._head_logits(x, tapped=taps and [tapped[c] for c in taps])
        if cache is None:
            cache = KVCache(layers, kept, L_max)
            if pressed.any():
                cache.pos_off = (lens - kept).astype(np.int64)
        else:
            cache.lens[seq] = kept
            if compress is not None:
                if cache.pos_off is None:
                    cache.pos_off = np.zeros(cache.B, dtype=np.int64)
                cache.pos_off[seq] = lens - kept
            elif cache.pos_off is not None:
                cache.pos_off[seq] = 0
        if want is not None:
            return cache, out, [attn[c] for c in want]
        return (cache, out) if taps is None else (cache, *out)

    # lm_head of a tapped step: "stacked" puts [mature; candidates] into one skinny launch (skinny=True: a row's bits do not depend on
    # the row count) where that keeps the mature rows' bits, i.e. where the mature rows alone take the skinny kernel today and
    # (1 + n) * B <= ops.GEMV_MAX_M, and is "second" elsewhere; "second" keeps the mature rows' launch as it is and runs the candidates'
    # rows in a second one.  Both give the same bits.  Measured (tools/decode_bench.py --dola, profiles/decode_bench.jsonl mode dola_ab,
    # DESIGN.md 5b "DoLa"; dola_layers="high", B = 1, the only measured batch at which stacking applies): added ms per step over the
    # plain step, second -> stacked: llava15_7b 0.103 -> 0.033, Qwen2-7B 0.400 -> 0.094, each faster by more than the second arm's
    # spread (0.007 / 0.006 ms), so stacking is the default.
    tap_lm_head = "stacked"
    kvpress_trace = None              # prefill(compress=): a list here receives (layer, votes, keep) clones per layer (tests)

    def _check_taps(self, tap_layers):
        if tap_layers is None:
            return None
        taps = tuple(tap_layers)
        L = self.l["layers"]
        if not 1 <= len(taps) <= ops.DOLA_MAX_LAYERS or len(set(taps)) != len(taps) or any(
                isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < L for c in taps):
            raise ValueError(f"tap_layers must be 1 .. {ops.DOLA_MAX_LAYERS} distinct ints in [0, {L}), got {tap_layers!r}")
        return tuple(int(c) for c in taps)

    def _check_attn_layers(self, attn_layers):
        if attn_layers is None:
            return None
        want = tuple(attn_layers)
        L = self.l["layers"]
        if not 1 <= len(want) <= L or len(set(want)) != len(want) or any(
                isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c < L for c in want):
            raise ValueError(f"attn_layers must be 1 .. {L} distinct ints in [0, {L}), got {attn_layers!r}")
        return tuple(int(c) for c in want)

    def _tap_logits(self, hN, hs):
        """(mature fp32 logits [B, ld], candidate fp32 logits [n, B, vocab]) from the normed last rows hN and the n tapped bf16 rows
        hs (each [B, d], no norm): the candidates are _decode_linear(cat(hs), lm_head, out_dtype=fp32) -- row k * B + b is candidate k
        of sequence b -- and the mature rows carry the bits of the call without taps (tap_lm_head)."""
        w = self.W("lm_head.weight")
        B, n = hN.shape[0], len(hs)
        if self.tap_lm_head == "stacked" and self._takes_skinny(w, B) and (1 + n) * B <= ops.GEMV_MAX_M:
            both = self._decode_linear(torch.cat([hN] + list(hs), 0), w, out_dtype=torch.float32, skinny=True)
            return both[:B], both[B:].view(n, B, -1)[:, :, :self.vocab]
        logits = self._decode_linear(hN, w, out_dtype=torch.float32)
        cand = self._decode_linear(torch.cat(list(hs), 0), w, out_dtype=torch.float32)
        return logits, cand.view(n, B, -1)[:, :, :self.vocab]

    def decode_step(self, cache, tokens, beams=None, shared=None, tap_layers=None, attn_layers=None, attn_mean=False):
        """One generated token per sequence: tokens [B] (int, host or device) at position cache.lens[b] -> fp32 logits [B, vocab].
        Every layer is _cached_layer at the token's position, its attention step the cache append and decode attention over the
        sequence's cached keys; then the final norm and the lm_head (_head_logits).
        beams (beam search, generation.beam_generate): .prefix_row / .prefix_len (int32 [B] device) and .tail_src (int32 [B, >=
        .tail_cols] device, or None).  Row r still appends its K|V at position cache.lens[r] of its OWN row, but reads key position j
        from row prefix_row[r] while j < prefix_len[r] and from row tail_src[r, j - prefix_len[r]] after it (rv_attn_decode_beam_bf16,
        bit-identical to the plain kernel on the gathered cache), so beams share their prompt's rows and their ancestors' tokens and
        nothing in the cache moves.  Without it every call is what it was.
        An int8-dtype cache (KVCache.dtype): the K|V row is quantised by the append (ops.kv_append_q8) and attention reads the int8
        rows (ops.attn_decode_kv8), bit-identical to this step on a bf16 cache holding the dequantised values (kv8_decode False runs
        exactly that).  beams= with such a cache raises NotImplementedError.
        shared (generate_batch(share_prefix=True)): a tile table from shared_plan() -- .c0 / .tile, device int32 [B] / [B, 16], uploaded
        when the active set changes, not per step.  Rows of a tile hold equal K|V at their first c0 * chunk positions, and attention
        reads those chunks once per tile (rv_attn_decode_shared_bf16), bit-identical to the plain kernel on the same cache;
        shared_route decides whether it does.  Not combined with beams= or an int8 cache (NotImplementedError).  With shared=None
        every call is what it was.
        tap_layers (DoLa): as in prefill -- a tuple of n distinct layer numbers c in [0, layers); the call then returns (logits, fp32
        [n, B, vocab]): lm_head of the token's row as it enters layer c, no final norm, in tap_layers' order.  The logits and the
        cache are bit for bit those of the call without it; it works with quantised decoders and an int8 cache (lm_head stays bf16,
        the attention branch is not touched) and is not combined with beams= or shared= (NotImplementedError).
        attn_layers (generate(output_attentions=True)): a tuple of distinct layer numbers in [0, layers); the call then returns
        (logits, attn), attn a list in attn_layers' order of fp32 [B, H, L_t] -- or [B, L_t], the mean over the heads, under attn_mean --
        with L_t = max_b(cache.lens[b] + 1) at this step: softmax(q K^T / sqrt(hd)) of the step's query row over the sequence's cache
        positions 0 .. cache.lens[b], zeros beyond.  In those layers ops.attn_decode_probs runs on the same qkv[:, :d], cache layer and
        kv_len, after the K|V append and beside the unchanged ops.attn_decode call, so the logits and the cache are the bits of the
        call without it.  Not combined with beams=, shared=, tap_layers= or an int8 cache (NotImplementedError).
        cache.pos_off (prefill(compress=), generate(prompt_kv_budget=)): when set, the token's K|V still goes to slot cache.lens[b]
        and attention reads kv_len = lens + 1 slots, but its q and k are rotated at position lens[b] + pos_off[b] (the rope table
        covers L_max + max(pos_off)); beams=, shared= and attn_layers= then raise NotImplementedError.  With pos_off None the step
        uploads and launches exactly what it did."""
        self._check_generation()
        off = getattr(cache, "pos_off", None)
        if off is not None:
            for name, v in (("beams", beams), ("shared", shared), ("attn_layers", attn_layers)):
                if v is not None:
                    self._refuse_pressed(cache, f"decode_step({name}=...)")
        taps = self._check_taps(tap_layers)
        want = self._check_attn_layers(attn_layers)
        if want is not None:
            for name, v in (("beams", beams), ("shared", shared), ("tap_layers", tap_layers)):
                if v is not None:
                    raise NotImplementedError(f"decode_step(attn_layers=...) with {name}=: attention maps run on the plain decode step")
            if getattr(cache, "dtype", "bf16") == "int8":
                raise NotImplementedError("decode_step(attn_layers=...) on an int8 KV cache: the probability kernel reads a bf16 cache only")
        if taps is not None and (beams is not None or shared is not None):
            raise NotImplementedError("decode_step(tap_layers=...) with beams= or shared=: DoLa runs on the plain decode step")
        if shared is not None:
            if beams is not None:
                raise NotImplementedError("decode_step(shared=...) with beams=: one row lookup per call")
            self._refuse_int8(cache, "decode_step(shared=...)")
            if shared.c0.numel() != cache.B:
                raise ValueError(f"the tile table has {shared.c0.numel()} rows, the cache {cache.B}")
            if not self._use_shared(shared, cache):
                shared = None
        d, H, L = self.l["d"], self.l["heads"], self.l["layers"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        B = cache.B
        kv8 = getattr(cache, "dtype", "bf16") == "int8"
        if kv8 and beams is not None:
            self._refuse_int8(cache, "decode_step(beams=...)")
        if (cache.lens >= cache.L_max).any():
            raise ValueError(f"the KV cache is full ({cache.L_max} slots per sequence)")
        tok = self._tokens_dev(tokens)
        assert tok.numel() == B
        pos = self._dev(cache.lens.astype(np.int32))
        kv_len = self._dev((cache.lens + 1).astype(np.int32))
        cs = self.rope_table(cache.L_max)
        rpos = pos                             # the RoPE position; a compressed prompt's slots lag its positions by pos_off
        if off is not None:
            rpos = self._dev((cache.lens + off).astype(np.int32))
            cs = self.rope_table(_ru(cache.L_max + int(off.max()), 1024))    # a position's entry does not depend on the table's length
        if want is not None:
            L_t, attn = int(cache.lens.max()) + 1, {}

        def attend(i, qkv):
            if kv8 and cache.scales is not None:
                kvq = (cache.layers[i], cache.scales[i])
                ops.kv_append_q8(qkv[:, d:], pos, Hkv, hd, cache=kvq)
                return ops.attn_decode_kv8(qkv[:, :d], kvq, kv_len, H, Hkv, hd, kvd, chunk=cache.chunk)
            if kv8:         # the reference arm: the dequantised values as bf16, read by the bf16 kernel
                ops.kv_append_q8(qkv[:, d:], pos, Hkv, hd, xhat=cache.layers[i])
                return ops.attn_decode(qkv[:, :d], cache.layers[i], kv_len, H, Hkv, hd, kvd, chunk=cache.chunk)
            if shared is not None:
                ops.kv_append(qkv[:, d:], cache.layers[i], pos)
                return ops.attn_decode_shared(qkv[:, :d], cache.layers[i], kv_len, shared.c0, shared.tile, H, Hkv, hd, kvd, chunk=cache.chunk)
            if beams is None:
                ops.kv_append(qkv[:, d:], cache.layers[i], pos)
                if want is not None and i in want:
                    attn[i] = ops.attn_decode_probs(qkv[:, :d], cache.layers[i], kv_len, H, Hkv, hd, L_t, per_head=not attn_mean,
                                                    mean=bool(attn_mean))[1 if attn_mean else 0]
                return ops.attn_decode(qkv[:, :d], cache.layers[i], kv_len, H, Hkv, hd, kvd, chunk=cache.chunk)
            ops.kv_append(qkv[:, d:], cache.layers[i], pos)
            return ops.attn_decode_beam(qkv[:, :d], cache.layers[i], kv_len, beams.prefix_row, beams.prefix_len, beams.tail_src, H, Hkv,
                                        hd, kvd, tail_cols=beams.tail_cols, chunk=cache.chunk)
        x = ops.gather_rows(tok.contiguous(), d, self.W("model.embed_tokens.weight"))
        tapped = {}
        for i in range(L):
            if taps is not None and i in taps:
                tapped[i] = x                      # _cached_layer makes a new x: the row stays as it is
            x = self._cached_layer(i, x, cs, rpos, attend)
        out = self._head_logits(x, tapped=taps and [tapped[c] for c in taps])
        cache.lens += 1
        return out if want is None else (out, [attn[c] for c in want])

    # decode_step(shared=)'s attention.  rv_attn_decode_shared_bf16 reads a tile's shared chunks once for its 16 / G rows and gives
    # rv_attn_decode_bf16's bits, so the route changes time only.  shared_route: None = the measured table below; "shared" / "plain"
    # force one arm ("plain" ignores the table and runs ops.attn_decode: the reference arm and the benchmark's A/B).  Same-box A/B on
    # the two 7B head shapes at B = 32, rows in groups of 2, 4, 8, 16, 32 holding one prefix of 704 or 7,603 keys (each row 40 keys
    # of its own), cold cache, interleaved, median of 20 (tools/decode_bench.py --shared-shapes, profiles/decode_bench.jsonl mode
    # shared_kernel_ab, DESIGN.md 5b "Shared prompt prefixes"); shared / plain:
    #   one q head per kv head (llava15, 16 rows per tile)   group  2     4     8     16    32
    #                                          704 keys            1.00  0.80  0.75  0.66  0.67     (plain 145 us, spread 2.5 us)
    #                                        7,603 keys            0.87  0.60  0.47  0.41  0.41     (plain 1,146 us, spread 6 - 10 us)
    #   7 q heads per kv head (Qwen2, 2 rows per tile): 1.45 at 704 keys (47 -> 68 us) and 1.21 at 7,603 (318 -> 385 us), every group.
    # The shared arm is taken only where it was faster by more than the plain arm's own spread (p90 - p10): every llava15 cell but
    # (group 2, 704 keys), which is a tie.  Between two measured cells the nearer one in log distance decides: groups 2 | 4 -> 3 rows
    # in the launch's largest tile, keys 704 | 7,603 -> 2,313 shared keys.  Qwen2 loses in every cell (two rows per workgroup do not
    # pay for the staircase's 16-query structure, as in verify_route) and takes the plain kernel; group sizes that were not measured
    # (G = 2 .. 6, 8) take it too until a measurement says otherwise.  Those requests still share the prompt pass.
    shared_route = None

    @property
    def shared_rows_per_tile(self):
        """Rows of one tile of rv_attn_decode_shared_bf16: 16 (row, q head) queries per workgroup over G = heads / kv heads."""
        return ops.SHARED_TILE_COLS // (self.l["heads"] // self.Hkv)

    def shared_plan(self, c0, tile):
        """The device copy of a tile table (generation.shared_tiles), validated first (ops.shared_tiles_upload): decode_step(shared=)."""
        return ops.shared_tiles_upload(c0, tile, self.shared_rows_per_tile, self.device)

    def _use_shared(self, plan, cache):
        if self.shared_route is not None:
            if self.shared_route not in ("shared", "plain"):
                raise ValueError(f"shared_route must be None, 'shared' or 'plain', got {self.shared_route!r}")
            return self.shared_route == "shared"
        if self.l["heads"] != self.Hkv:
            return False
        rows = int((plan.tile_host >= 0).sum(axis=1).max())               # the largest tile
        keys = int(plan.c0_host.max()) * cache.chunk
        return rows >= 3 or keys >= 2313

    # verify_step's attention.  rv_attn_decode_verify_bf16 reads a chunk once for a group of 16 / G rows; the same rows through
    # rv_attn_decode_beam_bf16 (prefix_row 0, prefix_len L_max) give the same bits from R times as many, smaller workgroups.  Same-box
    # A/B on the two 7B head shapes, R = 4, 8, 16, 32 at 704 and 7,603 keys (DESIGN.md 5b "Prompt-lookup decoding",
    # profiles/decode_bench.jsonl mode lookup_kernel_ab): with one q head per kv head (llava15) the new kernel wins at 7,603 keys
    # (0.43 - 0.72x) and at R = 32, and loses at 704 keys with R <= 16 (1.25 - 1.40x: too few workgroups to fill the machine); with
    # 7 q heads per kv head (Qwen2: 2 rows per group) it loses in every cell (1.19 - 1.51x).  The losing cells go to the beam kernel;
    # between two measured cells the nearer one (in log distance) decides: R 16 | 32 -> 23, keys 704 | 7,603 -> 2,313.  Group sizes
    # that were not measured (2 .. 6, 8) sit between the two measured shapes, on the slope of the losing one (fewer rows per group, more
    # serial work per workgroup): they take the beam kernel until a measurement says otherwise.  verify_route: None = this table;
    # "verify" / "beam" force one kernel.
    verify_route = None

    def _verify_use_beam(self, R, keys):
        if self.verify_route is not None:
            return self.verify_route == "beam"
        G = self.l["heads"] // self.Hkv
        return G > 1 or (R < 23 and keys < 2313)

    def verify_step(self, cache, tokens):
        """Prompt-lookup verification on a B = 1 cache: tokens [R] (1 <= R <= 32; the last emitted token, then R - 1 drafted ones) are
        fed at positions cache.lens[0] .. cache.lens[0] + R - 1 -> fp32 logits [R, vocab], row i being bit for bit what decode_step
        returns at that position after tokens[:i] were fed one by one.  _cached_layer on R rows at their positions: one launch writes
        the R K|V rows into the cache row, and row i attends to the keys [0, lens[0] + i + 1) (rv_attn_decode_verify_bf16: the chunk's
        K / V read once for a group of rows; or the beam kernel, verify_route).  Every product takes the skinny kernel (a row's bits
        do not depend on M there), the lm_head included whatever its height.  cache.lens is NOT advanced: the caller adds the number
        of tokens it emits; the K|V rows of rejected drafts stay past lens as stale rows, which every kernel ignores."""
        self._check_generation()
        self._refuse_int8(cache, "verify_step()")
        self._refuse_pressed(cache, "verify_step()")
        d, H, L = self.l["d"], self.l["heads"], self.l["layers"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        if cache.B != 1:
            raise ValueError(f"verify_step() takes a cache of one sequence, this one holds {cache.B}")
        tok = self._tokens_dev(tokens)
        R, n0, L_max = int(tok.numel()), int(cache.lens[0]), cache.L_max
        if not 1 <= R <= min(ops.GEMV_MAX_M, ops.VERIFY_MAX_R):
            raise ValueError(f"verify_step() takes 1 .. {min(ops.GEMV_MAX_M, ops.VERIFY_MAX_R)} tokens, got {R}")
        if n0 + R > L_max:
            raise ValueError(f"the KV cache holds {L_max} positions; {R} tokens from position {n0} do not fit")
        use_beam = self._verify_use_beam(R, n0 + 1)
        # one upload: positions, key counts, the beam route's prefix row and prefix length, kv_len0, then the cache slots as int64
        off = (4 * R + 2) // 2 * 2
        host = np.zeros(off + 2 * R, dtype=np.int32)
        host[:R] = n0 + np.arange(R)
        host[R:2 * R] = n0 + 1 + np.arange(R)
        host[3 * R:4 * R] = L_max
        host[4 * R] = n0 + 1
        host[off:].view(np.int64)[:] = n0 + np.arange(R)
        hd_ = self._dev(host)
        pos, kv_len, zero, plen, kv0 = hd_[:R], hd_[R:2 * R], hd_[2 * R:3 * R], hd_[3 * R:4 * R], hd_[4 * R:4 * R + 1]
        slots = hd_[off:].view(torch.int64)
        cs = self.rope_table(L_max)

        def attend(i, qkv):
            kv = cache.layers[i]
            kv.view(L_max, 2 * kvd).index_copy_(0, slots, qkv[:, d:])
            if use_beam:
                return ops.attn_decode_beam(qkv[:, :d], kv, kv_len, zero, plen, None, H, Hkv, hd, kvd, chunk=cache.chunk)
            return ops.attn_decode_verify(qkv[:, :d], kv, kv0, R, H, Hkv, hd, kvd, chunk=cache.chunk)
        x = ops.gather_rows(tok.contiguous().view(-1), d, self.W("model.embed_tokens.weight"))
        for i in range(L):
            x = self._cached_layer(i, x, cs, pos, attend, skinny=True)
        return self._head_logits(x, skinny=True)

    def extend(self, cache, input_ids, attention_mask=None, images=None, image_sizes=None, reuse=None, max_new_tokens=0, plan=None, slots=None):
        """The prompt pass of a continued generation over a KV cache of an earlier call on the same weights: sequence b's positions
        0 .. reuse[b] - 1 are kept from `cache` (a KVCache; later positions are dropped), its positions reuse[b] .. len_b - 1 (at least one)
        run through every decoder layer as one packed batch of M = sum(len_b - reuse[b]) rows -- _cached_layer at the explicit positions,
        its attention step the K|V rows written into their cache slots and extend attention against the sequence's cached keys
        (rv_attn_extend_bf16) -- then the final norm and the lm_head on each sequence's last row (_head_logits).
        The vision tower runs only when an image feature row (image_newline aside) is among the new rows.  The cache grows (one copy of
        the kept rows) when len_b + max_new_tokens exceeds its slots.  Every reuse[b] == 0 (or no cache): prefill(), bit for bit.
        plan: this prompt's self.plan(...), when the caller has it already.
        slots (generate_batch(share_prefix=True)): sequence b of the prompt batch lives in row slots[b] of `cache`, which may hold more
        rows; the other rows and their lengths are untouched, cache.lens[slots] is set, and a need beyond cache.L_max is a ValueError
        (no growth).  rv_attn_extend_bf16 indexes the cache by sequence number, so it is given all cache.B sequences with no new rows
        for the ones not extended (its workgroups return, its combine skips them) and the packed rows in slot order; a row's
        arithmetic is that of extend() on a cache of these sequences alone with the same L_max.
        Returns (cache, fp32 logits [B, vocab])."""
        self._refuse_int8(cache, "extend()")
        self._refuse_pressed(cache, "extend()")
        if slots is not None and cache is None:
            raise ValueError("extend(slots=) needs the cache the slots index")
        if cache is None or reuse is None or not np.any(reuse):
            if slots is not None:
                return self.prefill(input_ids, attention_mask, images, image_sizes, max_new_tokens=max_new_tokens, cache=cache, slots=slots)
            return self.prefill(input_ids, attention_mask, images, image_sizes, max_new_tokens=max_new_tokens)
        self._check_generation()
        from .generation import grown_length
        d, H, L = self.l["d"], self.l["heads"], self.l["layers"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        ids = np.asarray(input_ids)
        B = int(ids.shape[0])
        imgs = [] if images is None else list(images)
        if plan is None:
            plan = self.plan(ids, attention_mask, None, imgs, image_sizes)
        lens = plan["lens"].astype(np.int64)
        r = np.asarray(reuse, dtype=np.int64).reshape(-1)
        if slots is None:
            seq = np.arange(B)
            if cache.B != B or r.shape[0] != B:
                raise ValueError(f"the cache holds {cache.B} sequences, the prompt {B}")
        else:
            seq = self._slot_rows(slots, B, cache, ok=r.shape[0] == B)
        if (r < 0).any() or (r > cache.lens[seq]).any() or (r >= lens).any():
            raise ValueError("reuse[b] must lie in [0, min(cached length, prompt length - 1)]")
        n = lens - r
        need = int((lens + int(max_new_tokens)).max())
        if slots is None:
            L_new = grown_length(cache.L_max, need)
            if L_new > cache.L_max:
                cache.grow(L_new, int(r.max()))
            cache.lens = r.copy()
        else:
            if need > cache.L_max:
                raise ValueError(f"the prompts need {need} positions, the cache holds {cache.L_max}")
            cache.lens[seq] = r
        CB = cache.B
        order = np.argsort(seq, kind="stable")                # the packed rows go in cache-row order; without slots: 0 .. B - 1
        L_max = cache.L_max
        valid = plan["attention_mask"].reshape(-1)
        flat = plan["idx"][valid]
        cu_full = np.concatenate([[0], np.cumsum(lens)])
        src = np.concatenate([flat[cu_full[b] + r[b]:cu_full[b + 1]] for b in order]).astype(np.int32)
        nl_code = -int(plan["n_feat_rows"]) - 2
        if ((src <= -2) & (src != nl_code)).any():
            if not imgs:
                raise ValueError("the prompt holds an image token but no images were passed")
            table = self.encode_images(self._pixels(imgs), plan=plan)
        else:       # no image feature rows among the new ones (image_newline aside): a one-row table, the tower does not run
            table = (self.W("model.image_newline").reshape(1, d) if self.with_newline else
                     torch.zeros(1, d, dtype=BF16, device=self.device))
            src = np.where(src == nl_code, -2, src).astype(np.int32)
        pos = np.concatenate([np.arange(r[b], lens[b]) for b in order])
        n_all, r_all = np.zeros(CB, dtype=np.int64), np.zeros(CB, dtype=np.int64)
        n_all[seq], r_all[seq] = n, r
        cu_q = np.concatenate([[0], np.cumsum(n_all)]).astype(np.int32)
        rows = self._dev(np.concatenate([seq[b] * L_max + np.arange(r[b], lens[b]) for b in order]).astype(np.int64))
        pos_d, cu_d, r_d = self._dev(pos.astype(np.int32)), self._dev(cu_q), self._dev(r_all.astype(np.int32))
        cs = self.rope_table(L_max)

        def attend(i, qkv):
            kv = cache.layers[i]
            kv.view(CB * L_max, 2 * kvd).index_copy_(0, rows, qkv[:, d:])
            return ops.attn_extend(qkv[:, :d], kv, cu_d, r_d, H, Hkv, hd, kvd, int(n.max()))
        x = ops.gather_rows(self._dev(src), d, self.W("model.embed_tokens.weight"), table)
        for i in range(L):
            x = self._cached_layer(i, x, cs, pos_d, attend)
        last = self._dev((cu_q[seq + 1] - 1).astype(np.int32))              # sequence b's last new row, in the prompt batch's order
        logits = self._head_logits(ops.gather_rows(last, d, x))
        if slots is None:
            cache.lens = lens.copy()
        else:
            cache.lens[seq] = lens
        return cache, logits

    def score_tails(self, prefix, prefix_row, tails, logits, arrays=None):
        """Log-probs of given continuations of prefilled prompts (model.score()).  prefix: a bf16 KVCache filled by prefill(), one row
        per distinct prompt, and `logits` the fp32 last-row logits prefill() returned with it; candidate k continues row prefix_row[k]
        with the tokens tails[k] (n_k >= 1 ids).  Its tokens t_0 .. t_{n-2} run at positions P .. P + n - 2 (P = prefix.lens[row]) as
        one packed batch of M = sum(n_k - 1) rows through _cached_layer at the explicit positions -- its attention step the K|V rows
        written into a tail cache [C, T_max, 2*kvd] per layer and attention over the prompt's keys read in place from `prefix` and
        then the candidate's own (rv_attn_extend_prefix_bf16: no copy of a prompt, however many candidates share it) -- then the
        final norm on every row and the lm_head in row slices
        whose fp32 logits stay under scoring.LOGITS_BYTES_CAP, each slice going straight into rv_token_logprob_rows_f32 with the next
        token as target.  t_0 is scored from row prefix_row[k] of `logits`; a one-token candidate runs no row.  The quantised decoders
        work as in extend() (_decode_linear).  prefix is only read; self.ctx and the optimizer state are not touched.
        arrays: scoring.launch_arrays(prefix_row, prefix.lens[prefix_row], tails), when the caller has it already.
        Returns (fp32 log-probs, int64 argmax ids), device tensors of sum(n_k) entries: candidate k's tokens in order at
        arrays.offsets[k] .. offsets[k + 1]."""
        self._check_generation()
        self._refuse_int8(prefix, "score_tails()")
        self._refuse_pressed(prefix, "score_tails()")
        from . import scoring
        d, H, L = self.l["d"], self.l["heads"], self.l["layers"]
        hd, Hkv, kvd, V = self.hd, self.Hkv, self.kvd, self.vocab
        prow = np.asarray(prefix_row, dtype=np.int64).reshape(-1)
        if prow.shape[0] != len(tails) or (prow < 0).any() or (prow >= prefix.B).any():
            raise ValueError(f"prefix_row must hold one index into the cache's {prefix.B} rows per candidate")
        a = arrays if arrays is not None else scoring.launch_arrays(prow, prefix.lens[prow], tails)
        if a.C != len(tails) or not np.array_equal(a.prefix_row, prow) or not np.array_equal(a.prefix_len, prefix.lens[prow]):
            raise ValueError("arrays does not describe these candidates on this cache")
        if logits.dim() != 2 or logits.shape[0] != prefix.B or logits.dtype != torch.float32:
            raise ValueError(f"logits must be the fp32 [{prefix.B}, vocab] rows prefill() returned with the cache")
        total = int(a.offsets[-1])
        lp = torch.empty(total, dtype=torch.float32, device=self.device)
        am = torch.empty(total, dtype=torch.int64, device=self.device)
        first_lp, first_am = ops.token_logprob_rows(logits, V, self._dev(a.first_targets), src_row=self._dev(a.src_row))
        first_out = self._dev(a.first_out)
        lp.index_copy_(0, first_out, first_lp)
        am.index_copy_(0, first_out, first_am)
        if a.M == 0:
            return lp, am
        C, T_max = a.C, a.T_max
        pos_d, cu_d = self._dev(a.positions), self._dev(a.cu_q)
        prow_d, plen_d, rows = self._dev(a.prefix_row), self._dev(a.prefix_len), self._dev(a.tail_rows)
        cs = self.rope_table(prefix.L_max + T_max)
        table = torch.zeros(1, d, dtype=BF16, device=self.device)      # candidates are text: the splice reads token embeddings only
        x = ops.gather_rows(self._dev(a.tokens), d, self.W("model.embed_tokens.weight"), table)
        tail = [torch.zeros(C, T_max, 2 * kvd, dtype=BF16, device=self.device) for _ in range(L)]

        def attend(i, qkv):
            tail[i].view(C * T_max, 2 * kvd).index_copy_(0, rows, qkv[:, d:])
            return ops.attn_extend_prefix(qkv[:, :d], prefix.layers[i], tail[i], cu_d, prow_d, plen_d, H, Hkv, hd, kvd, a.max_q)
        for i in range(L):
            x = self._cached_layer(i, x, cs, pos_d, attend)
        del tail                             # empties the cell attend reads: the tail cache is freed here
        hN, _ = ops.rmsnorm_fwd(x, self.W("model.norm.weight"), self.eps)
        w_head = self.W("lm_head.weight")
        step = max(1, scoring.LOGITS_BYTES_CAP // (int(w_head.shape[0]) * 4))
        tgt, row_out = self._dev(a.targets), self._dev(a.row_out)
        for m0 in range(0, a.M, step):
            m1 = min(a.M, m0 + step)
            sl = self._decode_linear(hN[m0:m1], w_head, out_dtype=torch.float32)
            s_lp, s_am = ops.token_logprob_rows(sl, V, tgt[m0:m1])
            lp.index_copy_(0, row_out[m0:m1], s_lp)
            am.index_copy_(0, row_out[m0:m1], s_am)
            del sl
        return lp, am

    def _scored_rows(self, rows, lab_rows, gathered, scored):
        """The n scored tokens among forward()'s `rows` head rows (_policy_loss, _preference_loss): rows 0 .. n - 1 when gathered, else
        the rows lab_rows.  Returns (n, per_row, pick): per_row(a) scatters a host array of n entries (or None) to fp64 [rows];
        pick(*ts) takes the scored entries, in scored order, out of device tensors [..., rows] with one upload of the row index."""
        n = int(lab_rows.size)
        assert n == int(scored.sum()), "a scored token on a padding row"

        def per_row(a):
            if a is None:
                return None
            full = np.zeros(rows, dtype=np.float64)          # rows without a label are never read by the kernel
            full[slice(n) if gathered else lab_rows] = a
            return full

        def pick(*ts):
            sel = slice(n) if gathered else self._dev(lab_rows.astype(np.int64))
            return [t[..., sel] for t in ts]
        return n, per_row, pick

    def _policy_loss(self, logits, tgt, lab_rows, gathered, scored, terms, gscale, grad=True):
        """The GRPO token loss in the cross entropy's place: logits (bf16, overwritten by dlogits when grad) and tgt are forward()'s head
        rows; lab_rows the labelled rows among forward()'s token rows, ascending -- the scored order of policy.PolicyTerms, sample by
        sample.  gathered: the head ran on the labelled rows alone (rows 0 .. n - 1 in scored order, then pad rows with label -100);
        else the per-token terms are scattered by lab_rows.  terms None (token_logps): statistics only, every coefficient zero.
        Leaves self.last_policy: logp, loss, kl, clip (0 active / 1 low / 2 high) fp32 [n_scored] and ratio_one bool [n_scored] (no old
        log-probs were given: r = 1 exactly), device tensors in scored order, plus scored = the per-sample counts (host).
        terms.importance_sampling_level == "sequence": the three launches of _policy_loss_sequence instead."""
        if terms is not None and terms.importance_sampling_level == "sequence":
            return self._policy_loss_sequence(logits, tgt, lab_rows, gathered, scored, terms, gscale, grad)
        n, per_row, pick = self._scored_rows(logits.shape[0], lab_rows, gathered, scored)
        if terms is None:
            adv, w, old, ref = np.zeros(n), np.zeros(n), None, None
            eps_low = eps_high = beta = 0.0
        else:
            adv, w, old, ref = terms.per_token(scored)
            eps_low, eps_high, beta = float(terms.epsilon), terms.eps_high, float(terms.beta)
        loss, stats = ops.policy_loss(logits, tgt, self.vocab, per_row(adv), per_row(w), gscale, per_row(old), per_row(ref if beta > 0 else None),
                                      eps_low, eps_high, beta, dlogits="inplace" if grad else None)
        st, = pick(stats)
        self.last_policy = dict(logp=st[0], loss=st[1], kl=st[3], clip=st[4], scored=np.asarray(scored),
                                ratio_one=torch.full((n,), old is None, dtype=torch.bool, device=logits.device))
        return loss

    def _policy_loss_sequence(self, logits, tgt, lab_rows, gathered, scored, terms, gscale, grad=True):
        """_policy_loss with one importance ratio per sample (GSPO), the three launches of _preference_loss on the same head rows:
          (A) rv_policy_loss_bf16 without dlogits: the logp row of every scored token (token_logps()'s bits);
          (B) rv_gspo_seqs_f64: per-sample fp64 sums in the fixed order, the clipped sequence ratio, one coefficient -dL/dlogp and the
              k3 term per scored token, from the lweight / gweight / old / reference rows the token level hands to its kernel;
          (C) (grad) rv_policy_loss_bf16 in place with adv = those device rows, lweight 1, gweight 1, no old or reference log-probs,
              beta 0: r = 1 exactly, so dlogits = (p - onehot) * coef.
        Nothing comes back to the host in between.  Leaves self.last_policy with _policy_loss's keys per scored token -- loss and clip
        are the sample's l and clip code, repeated -- plus coefs (fp32 [n_scored]) and seq_logratio, seq_ratio, seq_clip (fp64 [B]).
        Returns L as fp32 [1]."""
        from . import lib
        rows, dev = logits.shape[0], logits.device
        n, per_row, pick = self._scored_rows(rows, lab_rows, gathered, scored)
        _, w, old, ref = terms.per_token(scored)
        adv_seq, seg_off = terms.per_sequence(scored)
        eps_low, eps_high, beta = float(terms.epsilon), terms.eps_high, float(terms.beta)
        f32 = lambda a: None if a is None else self._dev(a.astype(np.float32))
        w_rows = per_row(w)
        lweight, gweight = f32(w_rows), f32(w_rows * float(gscale))         # ops.policy_loss's two roundings of the weight
        zero = torch.zeros(rows, dtype=torch.float32, device=dev)
        stats = torch.empty(len(ops.POLICY_STATS), rows, dtype=torch.float32, device=dev)
        lib.call("rv_policy_loss_bf16", logits, logits.stride(0), tgt, zero, zero, zero, None, None, 0.0, 0.0, 0.0, stats, None, 0, rows, self.vocab)
        row_idx = None if gathered else self._dev(lab_rows.astype(np.int32))
        coef, kl = torch.zeros(rows, dtype=torch.float32, device=dev), torch.zeros(rows, dtype=torch.float32, device=dev)
        planes, batch = ops.gspo_seqs(stats[0], self._dev(seg_off), row_idx, f32(adv_seq), lweight, gweight, f32(per_row(old)),
                                      f32(per_row(ref if beta > 0 else None)), eps_low, eps_high, beta, coef, kl)
        if grad:
            ones = torch.ones(rows, dtype=torch.float32, device=dev)
            lib.call("rv_policy_loss_bf16", logits, logits.stride(0), tgt, coef, ones, ones, None, None, 0.0, 0.0, 0.0, torch.empty_like(stats),
                     logits, logits.stride(0), rows, self.vocab)
        logp, coefs, kls = pick(stats[0], coef, kl)
        seq_of = self._dev(np.repeat(np.arange(len(adv_seq)), np.asarray(scored, dtype=np.int64)))
        plane = dict(zip(ops.GSPO_PLANES, planes))
        self.last_policy = dict(logp=logp, loss=plane["loss"][seq_of].to(torch.float32), kl=kls, clip=plane["clip"][seq_of].to(torch.float32),
                                scored=np.asarray(scored), ratio_one=torch.full((n,), old is None, dtype=torch.bool, device=dev),
                                coefs=coefs, seq_logratio=plane["logratio"], seq_ratio=plane["ratio"], seq_clip=plane["clip"])
        return batch[:1].to(torch.float32)

    def _distill_loss(self, logits, tgt, lab_rows, gathered, scored, terms, gscale):
        """Knowledge distillation in the cross entropy's place (arguments as _policy_loss): one launch of rv_distill_loss_bf16 on
        forward()'s head rows, in place, against terms.teacher_logits, whose row j belongs to scored token j.  Gathered head: scored
        token j is head row j and the pad rows map to -1; all-rows head: teacher_row maps head row lab_rows[j] to teacher row j and
        every other row to -1.
        Leaves self.last_distill: jsd, kl_teacher, kl_student fp32 [n_scored] on the device in scored order, and scored (host counts).
        Returns sum(weight * jsd) as fp32 [1]."""
        rows = logits.shape[0]
        n, per_row, pick = self._scored_rows(rows, lab_rows, gathered, scored)
        w = terms.per_token(scored, self.vocab)
        teacher = terms.teacher_logits
        if teacher.device != logits.device:
            teacher = teacher.to(logits.device)
        if n and (teacher.stride(1) != 1 or teacher.stride(0) % 8 or teacher.data_ptr() % 16 or teacher.shape[1] < _ru(self.vocab, 8)):
            wide = torch.zeros(n, _ru(teacher.shape[1], 8), dtype=BF16, device=logits.device)      # rows of whole 16-byte vectors
            wide[:, :teacher.shape[1]] = teacher
            teacher = wide
        if n == 0:                           # nothing is scored: no row is paired, the kernel only zeroes dlogits
            teacher = logits
        tmap = np.full(rows, -1, dtype=np.int32)
        tmap[slice(n) if gathered else lab_rows] = np.arange(n, dtype=np.int32)
        tmap = self._dev(tmap)
        loss, stats = ops.distill_loss(logits, teacher, tgt, self.vocab, per_row(w), gscale, terms.beta, terms.temperature, teacher_row=tmap)
        st, = pick(stats)
        self.last_distill = dict(jsd=st[0], kl_teacher=st[2], kl_student=st[3], scored=np.asarray(scored))
        return loss

    def label_logits(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """The bf16 logits rows of the scored tokens, [n_scored, table columns >= ceil8(vocab)] on the device, in scored order (the
        order token_logps() documents): what forward() hands to its loss -- the tiled GEMMs, the same labelled-rows head, the bf16
        store -- in a score-only pass, so a teacher's rows are the bits its own training step would read.  LoRA engines run it in eval
        form.  No context is kept and the training state is not touched.  The per-sample scored counts are left in
        self.last_label_logits["scored"]."""
        with self._eval_form("lora_step", "ctx"):
            self.forward(input_ids, attention_mask, labels, images, image_sizes=image_sizes, _score_only=True, _label_logits=True)
        return self.last_label_logits["logits"]

    def token_logps(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """log p(label) of every scored token (the positions of each spliced row whose shifted target is not -100, sample by sample,
        ascending): fp32 [n_scored] on the device.  It is forward()'s own arithmetic -- the tiled GEMMs, the bf16 logits, the cross
        entropy's lse, the same labelled-rows head -- without a gradient and without a saved context, so old log-probs taken with it
        before an update make the first iteration's ratio exactly 1 (the sampler's fp32 GEMV logits are other bits).  LoRA engines run
        it in eval form (no adapter dropout).  The training state is not touched."""
        with self._eval_form("lora_step", "ctx"):
            self.forward(input_ids, attention_mask, labels, images, image_sizes=image_sizes, _score_only=True)
        return self.last_policy["logp"]

    def _preference_loss(self, logits, tgt, lab_rows, gathered, scored, terms, gscale):
        """The DPO loss in the cross entropy's place, three launches on forward()'s head rows (arguments as _policy_loss):
          (A) rv_policy_loss_bf16 without dlogits: the logp row of every scored token (token_logps()'s bits);
          (B) rv_dpo_pairs_f64: per-sequence fp64 sums in a fixed order, the pair terms, one coefficient A = -dL/dlogp per scored token;
          (C) rv_policy_loss_bf16 in place with adv = those device rows, lweight 1, gweight fp32(gscale), no old or reference log-probs,
              beta 0: r = 1 exactly, so dlogits = (p - onehot) * gweight * A.
        Nothing comes back to the host in between.  Leaves self.last_preference: planes (fp64 [7, P], ops.DPO_PLANES order), batch
        (fp64 [3]: L, dpo_alpha * mean pair loss, SFT loss), coefs and logp (fp32 [n_scored], scored order) on the device, scored (host counts)
        and P.  Returns L as fp32 [1]."""
        from . import lib
        rows, dev = logits.shape[0], logits.device
        _, _, pick = self._scored_rows(rows, lab_rows, gathered, scored)
        P, seg_off, rho, a_P, g_N = terms.per_pair(scored)
        zero = torch.zeros(rows, dtype=torch.float32, device=dev)
        stats = torch.empty(len(ops.POLICY_STATS), rows, dtype=torch.float32, device=dev)
        lib.call("rv_policy_loss_bf16", logits, logits.stride(0), tgt, zero, zero, zero, None, None, 0.0, 0.0, 0.0, stats, None, 0, rows, self.vocab)
        row_idx = None if gathered else self._dev(lab_rows.astype(np.int32))
        coef = torch.zeros(rows, dtype=torch.float32, device=dev)
        planes, batch = ops.dpo_pairs(stats[0], self._dev(seg_off), row_idx, None if rho is None else self._dev(rho), terms.loss_type,
                                      terms.beta, terms.label_smoothing, a_P, g_N, coef)
        ones = torch.ones(rows, dtype=torch.float32, device=dev)
        gweight = torch.full((rows,), float(np.float32(gscale)), dtype=torch.float32, device=dev)
        stats_c = torch.empty_like(stats)
        lib.call("rv_policy_loss_bf16", logits, logits.stride(0), tgt, coef, ones, gweight, None, None, 0.0, 0.0, 0.0, stats_c, logits,
                 logits.stride(0), rows, self.vocab)
        coefs, logp = pick(coef, stats[0])
        self.last_preference = dict(planes=planes, batch=batch, coefs=coefs, logp=logp, scored=np.asarray(scored), P=P)
        return batch[:1].to(torch.float32)

    def sequence_logps(self, input_ids, attention_mask, labels, images, image_sizes=None):
        """The summed log-prob of every sample's scored tokens: token_logps() followed by rv_seq_logp_sums_f64 -- fp64 [B] on the
        device, the bits the pair kernel forms for the same batch -- and the per-sample scored counts (host int64 [B])."""
        lp = self.token_logps(input_ids, attention_mask, labels, images, image_sizes=image_sizes)
        counts = np.asarray(self.last_policy["scored"], dtype=np.int64)
        if lp.numel() == 0:
            return torch.zeros(counts.size, dtype=torch.float64, device=self.device), counts
        from .preference import pair_offsets
        return ops.seq_logp_sums(lp.contiguous(), self._dev(pair_offsets(counts))), counts

    def _cross_entropy(self, logits, tgt, V, inv, gscale):
        from . import lib
        rows = logits.shape[0]
        loss_rows = torch.empty(rows, dtype=torch.float32, device=logits.device)
        lib.call("rv_cross_entropy", logits, logits.stride(0), tgt, loss_rows, logits, logits.stride(0), rows, V, inv * gscale)
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        lib.call("rv_sum_f32", loss_rows, rows, inv, loss)
        return loss, loss_rows

    # ------------------------------------------------------------------ backward
    def _linear_bwd(self, dy, x, w, gw, need_dx=True, dx_out=None):
        """Backward of y = x W^T:  dW[N,K] = dY^T X  (both operands read contraction-major, in place) into the flat
        grad view (skipped when gw is None: frozen weight), and dX[M,K] = dY W (W read contraction-major) -- no
        transposed copies of weights or activations."""
        acc = self.grad_accum_started
        if gw is not None:
            ops.gemm(dy, x, ta=True, tb=True, out=gw, residual=gw if acc else None)
        if need_dx:
            return ops.gemm(dy, w, tb=True, out=dx_out)
        return None

    # ------------------------------------------------------------------ LoRA (peft LoraLayer semantics, train.py:1515-1532)
    def _lora_seed(self, i, lname):
        k = [t for t, _, _ in LORA_TARGETS].index(lname)
        return (self.lora_step * 1000003 + i * 131 + k) & 0x7FFFFFFFFFFFFFFF

    def _MODS_QKV(self, d):
        kvd = self.kvd      # == d without grouped-query attention
        return (("self_attn.q_proj", 0, d), ("self_attn.k_proj", d, d + kvd), ("self_attn.v_proj", d + kvd, d + 2 * kvd))

    def _MODS_O(self, d):
        return (("self_attn.o_proj", 0, d),)

    def _MODS_GU(self, F):
        return (("mlp.gate_proj", 0, F), ("mlp.up_proj", F, 2 * F))

    def _MODS_DOWN(self, d):
        return (("mlp.down_proj", 0, d),)

    def _lora_ws(self):
        if getattr(self, "_ws", None) is None:
            self._ws = torch.empty(32 << 20, dtype=torch.float32, device=self.device)   # split-K scratch (128 MiB)
        return self._ws

    def _zero_B(self, B):
        """adapters_off: a zero matrix of lora_B's shape, so that the launch is the zero-B call itself."""
        z = getattr(self, "_zero_b", None)
        if z is None or z.numel() < B.numel():
            z = self._zero_b = torch.zeros(B.numel(), dtype=BF16, device=self.device)
        return z[:B.numel()].view(B.shape)

    def _lora_linear(self, x, w, i, mods, saved, residual=None, bias=None, p=None):
        """y[:, c0:c1] = x W[c0:c1]^T + t B^T (+ residual) with t = (alpha/r) dropout(x) A^T: ONE launch per adapted module,
        the adapter rides the main GEMM as a second operand pair (K + r), no second pass over y.
        p: the dropout rate when it is not self.lora_p (the decode path passes 0)."""
        p = self.lora_p if p is None else p
        y = torch.empty(x.shape[0], w.shape[0], dtype=BF16, device=self.device)
        for lname, c0, c1 in mods:
            pre = f"model.layers.{i}.{lname}."
            A, B = self.W(pre + "lora_A.weight"), self.W(pre + "lora_B.weight")
            if self.adapters_off:
                B = self._zero_B(B)
            # t = (alpha / r) * dropout(x) A^T: one pass over x, the mask applied to the operand fragments (rv_lora_down_bf16)
            t = ops.lora_down(x, A, self.lora_scale, p, self._lora_seed(i, lname))
            ops.gemm(x, w[c0:c1], out=y[:, c0:c1], bias=None if bias is None else bias[c0:c1],
                     residual=None if residual is None else residual[:, c0:c1], a2=t, b2=B)
            saved[lname] = t
        return y

    def _lora_linear_bwd(self, dy, x, w, i, mods, saved):
        """dx = sum_j dy_j W_j + (adapter path); dA, dB into the flat grad views (split-K: r-wide outputs, token-long K)."""
        acc = self.grad_accum_started
        ws = self._lora_ws()
        dx = None
        if self.lora_p > 0 and len(mods) > 1:
            # base path of a fused projection (q|k|v, gate|up): ONE input-gradient GEMM over the stacked frozen weight, dx = dy W, instead of
            # one per module accumulated through the residual (two fewer passes over dx, one long K loop); the adapters add into it below
            dx = ops.gemm(dy[:, mods[0][1]:mods[-1][2]], w[mods[0][1]:mods[-1][2]], tb=True)
        base_done = dx is not None
        for lname, c0, c1 in mods:
            pre = f"model.layers.{i}.{lname}."
            A, B = self.W(pre + "lora_A.weight"), self.W(pre + "lora_B.weight")
            gA, gB = self.G(pre + "lora_A.weight"), self.G(pre + "lora_B.weight")
            dyj = dy[:, c0:c1]
            t = saved[lname]                                        # already scaled by alpha/r
            # d(dropout(x) A^T) = (alpha / r) dy B: an r-wide product over a token-long stream -- the skinny one-pass kernel (B^T is 64 rows)
            dts = ops.lora_down(dyj, ops.transpose(B), self.lora_scale, 0.0, 0) if B.shape[1] <= 64 else ops.gemm(dyj, B, tb=True, alpha=self.lora_scale)
            ops.gemm(dyj, t, ta=True, tb=True, out=gB, residual=gB if acc else None, workspace=ws)
            first = dx is None
            if first:
                dx = torch.empty(x.shape[0], w.shape[1], dtype=BF16, device=self.device)
            if self.lora_p > 0:
                seed = self._lora_seed(i, lname)
                ops.lora_a_grad(dts, x, gA, self.lora_p, seed, acc, ws)     # gA (+)= dts^T dropout(x): the mask is re-created in registers
                if not base_done:
                    ops.gemm(dyj, w[c0:c1], tb=True, out=dx, residual=None if first else dx)
                ops.gemm_dropout_add(dts, A, dx, self.lora_p, seed)   # dx += dropout'(dts A): the mask is applied in the GEMM epilogue
            else:
                ops.gemm(dts, x, ta=True, tb=True, out=gA, residual=gA if acc else None, workspace=ws)
                ops.gemm(dyj, w[c0:c1], tb=True, out=dx, residual=None if first else dx, a2=dts, b2=A)
        return dx

    def _lm_linear_bwd(self, dy, x, w, gw, i, mods, saved):
        if self.lora:
            return self._lora_linear_bwd(dy, x, w, i, mods, saved)
        return self._linear_bwd(dy, x, w, gw)

    def backward(self):
        """Backward of the last forward(); gradients land in self.grads (bf16, flat)."""
        c = self.ctx
        assert c is not None, "forward() first"
        if self.adapters_off:
            raise RuntimeError("backward() with the adapters switched off (model.disable_adapter()): that forward is for evaluation")
        self._select_gemm_launch_shape()
        l = self.l
        d, F, H, V, L = l["d"], l["ffn"], l["heads"], l["vocab"], l["layers"]
        hd, Hkv, kvd = self.hd, self.Hkv, self.kvd
        B, S, M, s_pad, lens, cu, pos = c["B"], c["S"], c["M"], c["s_pad"], c["lens"], c["cu"], c["pos"]
        acc = self.grad_accum_started
        cs = self.rope_table(S)
        # head
        frozen_lm = self.base is not None          # LoRA or projector-only: the decoder weights receive no gradients
        dhN = self._linear_bwd(c["dlogits"], c["hN"], self.W("lm_head.weight"), None if frozen_lm else self.G("lm_head.weight"))
        dx, _ = ops.rmsnorm_bwd(dhN, c["x_last"], self.W("model.norm.weight"), c["rstdN"],
                                dw=None if frozen_lm else self.G("model.norm.weight"), dw_accumulate=acc)
        back = None
        if c["head_idx"] is not None:       # the head ran on the labelled rows: every other row of the last layer's output has zero gradient
            back = np.full(M, -1, dtype=np.int32)
            back[c["head_idx"][:c["head_rows"]]] = np.arange(c["head_rows"], dtype=np.int32)
            back = self._dev(back)
            if not c["last_sel"]:
                dx = ops.gather_rows(back, d, dx)
        if not frozen_lm:
            self._bucket_done("lm_head.weight", "lm_head.weight")
            self._bucket_done("model.norm.weight", "model.norm.weight")
        for i in reversed(range(L)):
            a = c["layers"][i]
            if "h1" not in a:      # activation recompute: this layer kept only its input
                _, a = self._layer_forward(i, a["x"], c["geom"], rows=self._dev(c["head_idx"]) if (c["last_sel"] and i == L - 1) else None)
            lv, gv = self._layer_views(i), self._layer_views(i, self.grads)
            sv = a["lora"]
            if self.lora or not self.fused:
                dact = self._lm_linear_bwd(dx, a["act"], lv["down"], gv.get("down"), i, self._MODS_DOWN(d), sv)
                dgu = ops.swiglu_bwd(dact, a["gu"], F)
            else:       # down_proj: weight gradient, then the input gradient with the SwiGLU backward in its epilogue (d(act) never stored)
                self._linear_bwd(dx, a["act"], lv["down"], gv.get("down"), need_dx=False)
                dgu = ops.gemm_swiglu_bwd(dx, lv["down"], a["gu"], F)
            dh2 = self._lm_linear_bwd(dgu, a["h2"], lv["gu"], gv.get("gu"), i, self._MODS_GU(F), sv)
            ops.rmsnorm_bwd(dh2, a["x_mid"], lv["ln2"], a["rstd2"], dx=dx, dx_add=True, dw=gv.get("ln2"), dw_accumulate=acc)
            dattn = self._lm_linear_bwd(dx, a.get("attn_sel", a["attn"]), lv["o"], gv.get("o"), i, self._MODS_O(d), sv)
            if "attn_sel" in a:       # last layer on the labelled rows: back to all token rows (zero elsewhere) for the attention backward
                dattn, dx = ops.gather_rows(back, d, dattn), ops.gather_rows(back, d, dx)
            qkv = a["qkv"]
            dqkv = torch.empty_like(qkv)
            # the rotary embedding's adjoint runs in the dQ / dK epilogues: dqkv = gradient of the un-rotated q|k|v projection
            ops.attn_bwd(qkv[:, :d], qkv[:, d:d + kvd], qkv[:, d + kvd:], a["attn"], dattn, a["lse"], B, S, H, hd, s_pad, True,
                         lens=lens, dq=dqkv[:, :d], dk=dqkv[:, d:d + kvd], dv=dqkv[:, d + kvd:], kv_heads=Hkv, cu=cu,
                         rope=(cs, pos) if self.fused else None, delta=self._stat_buffer("delta", B, H, s_pad))
            if not self.fused:
                ops.rope_inplace(dqkv, cs, S, H + Hkv, hd, 1, -1, positions=pos)
            if "bqkv" in gv:
                ops.bias_grad(dqkv, out=gv["bqkv"], accumulate=acc)
            dh1 = self._lm_linear_bwd(dqkv, a["h1"], lv["qkv"], gv.get("qkv"), i, self._MODS_QKV(d), sv)
            ops.rmsnorm_bwd(dh1, a["x"], lv["ln1"], a["rstd1"], dx=dx, dx_add=True, dw=gv.get("ln1"), dw_accumulate=acc)
            c["layers"][i] = None  # free this layer's activations
            p = f"model.layers.{i}."
            if self.freeze_lm:
                pass                        # nothing trainable inside the layer
            elif frozen_lm:
                self._bucket_done(p + "self_attn.q_proj.lora_A.weight", p + "mlp.down_proj.lora_B.weight")
            else:
                self._bucket_done(p + "input_layernorm.weight", p + "mlp.down_proj.weight")
        # dx = gradient of inputs_embeds [M, d]
        plan = c["plan"]
        dev = self.device
        # projector: rows of dx at the positions where projector outputs were spliced in (unused rows -> zero)
        n_rows = plan["n_feat_rows"]
        fpos = self._dev(plan["feat_pos"])
        dfeat = ops.gather_rows(fpos, d, dx)
        rs = plan.get("resample")
        mp = plan.get("maxpool")
        if mp:   # adjoint of the 2x2 max pooling: each pooled row's gradient goes to the winning source element
            ops.max4_rows_bwd(dfeat, self._dev(mp["idx4"]), self._dev(mp["out"]), c["pool_which"], dfeat)
            dfeat = dfeat[:plan["n_proj_rows"]]
        if rs:   # adjoint of the bilinear down-sampling: gradients of the created rows flow to their 4 source rows
            t = lambda k: self._dev(rs[k])
            ops.weighted_segment_sum_rows(dfeat, t("adj_off"), t("adj_pos"), t("adj_w"), t("adj_out"), dfeat)
            dfeat = dfeat[:plan["n_proj_rows"]]
        g = self.G
        ops.bias_grad(dfeat, out=g("model.mm_projector.2.bias"), accumulate=acc)
        da1 = self._linear_bwd(dfeat, c["a1"], self.W("model.mm_projector.2.weight"), g("model.mm_projector.2.weight"))
        dz1 = ops.gelu_bwd(da1, c["z1"])
        ops.bias_grad(dz1, out=g("model.mm_projector.0.bias"), accumulate=acc)
        df0 = self._linear_bwd(dz1, c["f0"], self.W("model.mm_projector.0.weight"), g("model.mm_projector.0.weight"),
                               need_dx=self.train_tower)
        if self.with_newline:
            gn = g("model.image_newline").view(1, d)
            if not acc:
                gn.zero_()
            npos = plan["newline_pos"]
            if npos.size:
                tmp = torch.zeros(1, d, dtype=BF16, device=dev)
                ops.segment_sum_rows(dx, self._dev(np.array([0, npos.size], dtype=np.int32)),
                                     self._dev(npos), torch.zeros(1, dtype=torch.int32, device=dev), tmp)
                gn.add_(tmp) if acc else gn.copy_(tmp)
        # embedding rows: segment sums by token id (no atomics)
        train_embed = "model.embed_tokens.weight" in self.lm.offsets     # full fine-tune, or the pretraining stage with extra tokens
        ge = g("model.embed_tokens.weight") if train_embed else None
        if not train_embed:
            pass
        elif acc:
            tmp = torch.zeros_like(ge)
            ops.segment_sum_rows(dx, self._dev(plan["tok_off"]), self._dev(plan["tok_pos"]),
                                 self._dev(plan["tok_ids"]), tmp)
            ge.add_(tmp)
        else:
            ge.zero_()
            ops.segment_sum_rows(dx, self._dev(plan["tok_off"]), self._dev(plan["tok_pos"]),
                                 self._dev(plan["tok_ids"]), ge)
        last = "model.image_newline" if self.with_newline else "model.mm_projector.2.bias"
        self._bucket_done("model.embed_tokens.weight" if train_embed else "model.mm_projector.0.weight", last)
        if self.train_tower:
            if self.has_cls:
                n_img = c["v_n"]
                put = torch.full((n_img, self.N_vis), -1, dtype=torch.int32, device=dev)
                put[:, 1:] = torch.arange(n_img * self.P, device=dev, dtype=torch.int32).view(n_img, self.P)
                dhid = ops.gather_rows(put.view(-1), self.v["d"], df0)   # CLS rows receive zero
            else:
                dhid = df0
            self.vision_backward(dhid, c)
        self.ctx = None
        self.grad_accum_started = True

    # ------------------------------------------------------------------ data-parallel gradient sync
    def _bucket_done(self, first, last):
        """Gradients of tensors first..last are final: start their all-reduce on the comm stream (RCCL), in place."""
        if self.sync is None or not self.sync_this_backward:
            return
        s, e = self.lm.span(first, last)
        self.sync.bucket_done(s, e)

    sync_this_backward = True

    def finish_grad_sync(self):
        if self.sync is not None:
            self.sync.finish()

    def zero_grad(self):
        self.grad_accum_started = False

    def _replica_buffers(self):
        bufs = [("parameters", self.lm.flat)]
        if self.vis is not self.lm:
            bufs.append(("vision_tower", self.vis.flat))
        if self.base is not None:
            bufs.append(("frozen_language_model", self.base.flat))
        if self.nf4 is not None:
            bufs += [("nf4_" + k, self.nf4[k]) for k in ("codes", "absmax", "absmax_codes", "scale2", "offset") if self.nf4.get(k) is not None]
        bufs += [("fp32_master", self.master), ("exp_avg", self.m), ("exp_avg_sq", self.vv)]
        if self.state_bits == 8 and self.master is not None:
            bufs += [("exp_avg_codes", self.m8), ("exp_avg_sq_codes", self.v8), ("exp_avg_absmax", self.am8), ("exp_avg_sq_absmax", self.av8)]
        return [(n, t) for n, t in bufs if t is None or t.numel()]

    def broadcast_parameters(self):
        """Rank 0's parameters (and optimizer state, once it exists) become every rank's: the broadcast DistributedDataParallel performs
        when it wraps the model (HF Trainer / accelerate in the reference).  No-op for one rank."""
        if self.world > 1:
            from .ddp import broadcast_from_rank0
            broadcast_from_rank0(self._replica_buffers(), self.pg)
            self.weights_changed(tower=True)

    def check_replicas(self, where=""):
        """Raise unless every rank holds bit-identical parameters, frozen stores and optimizer state (all-reduced checksums)."""
        if self.world > 1:
            from .ddp import assert_replicas_equal
            assert_replicas_equal(self._replica_buffers(), self.pg, where)

    def barrier(self):
        if self.world > 1:
            torch.distributed.barrier(group=self.pg)

    # ------------------------------------------------------------------ optimizer
    state_bits = 32                          # width of the AdamW moments: 32 (fp32, the default) or 8 (optim8.py, csrc/adam8.hip)

    def _drop_state8(self):
        self.plan8 = None                    # optim8.StatePlan of self.lm while the moments are 8-bit
        self.m8 = self.v8 = self.am8 = self.av8 = None
        self._runs8 = {}

    def init_optimizer(self, state_bits=None):
        """Allocate the optimizer state on first use: the fp32 master copy and the two moments, fp32 (state_bits 32, the default) or
        8-bit block-quantised (state_bits 8: uint8 codes m8 / v8 and per-block absmax am8 / av8 for the tensors optim8.takes_8bit
        names; self.m / self.vv then hold the fp32 moments of the remaining tensors only, in the plan's compact layout).  state_bits
        None keeps the width in use.  With a state of the other width present the moments are converted in place
        (rv_adam8_quantize_f32 / rv_adam8_dequantize_f32 per tensor); the master copy is fp32 either way."""
        bits = self.state_bits if state_bits is None else int(state_bits)
        if bits not in (8, 32):
            raise ValueError(f"init_optimizer(state_bits={state_bits!r}): 8 or 32")
        if self.master is not None and bits == self.state_bits:
            return
        F = torch.float32
        old_m, old_v, old_plan = self.m, self.vv, self.plan8
        old8 = (self.m8, self.v8, self.am8, self.av8)
        had = self.master is not None
        if not had:
            self.master = ops.to_f32(self.lm.flat)
        if bits == 32:
            self.m, self.vv = self.lm.like(F), self.lm.like(F)
            if had:                                                     # 8 -> 32
                for name, t in old_plan.tensors.items():
                    off, n = t["off"], t["n"]
                    if t["bits"] == 8:
                        b, nb = t["block"], (n + 255) // 256
                        ops.adam8_dequantize(old8[0][b * 256:b * 256 + n], old8[2][b:b + nb], n, 0, self.m[off:off + n])
                        ops.adam8_dequantize(old8[1][b * 256:b * 256 + n], old8[3][b:b + nb], n, 1, self.vv[off:off + n])
                    else:
                        self.m[off:off + n].copy_(old_m[t["pos"]:t["pos"] + n])
                        self.vv[off:off + n].copy_(old_v[t["pos"]:t["pos"] + n])
            self._drop_state8()
            self.state_bits = 32
            return
        from .optim8 import StatePlan
        plan = StatePlan(self.lm.offsets, self.lm.shapes)
        dev = self.device
        self.m8 = torch.full((plan.ncodes,), 127, dtype=torch.uint8, device=dev)          # 127 / 0: the codes of 0 in the two tables
        self.v8 = torch.zeros(plan.ncodes, dtype=torch.uint8, device=dev)
        self.am8, self.av8 = torch.zeros(plan.nblocks, dtype=F, device=dev), torch.zeros(plan.nblocks, dtype=F, device=dev)
        self.m, self.vv = torch.zeros(plan.n32, dtype=F, device=dev), torch.zeros(plan.n32, dtype=F, device=dev)
        if had:                                                         # 32 -> 8
            for name, t in plan.tensors.items():
                off, n = t["off"], t["n"]
                if t["bits"] == 8:
                    b, nb = t["block"], (n + 255) // 256
                    ops.adam8_quantize(old_m[off:off + n], 0, self.m8[b * 256:b * 256 + n], self.am8[b:b + nb])
                    ops.adam8_quantize(old_v[off:off + n], 1, self.v8[b * 256:b * 256 + n], self.av8[b:b + nb])
                else:
                    self.m[t["pos"]:t["pos"] + n].copy_(old_m[off:off + n])
                    self.vv[t["pos"]:t["pos"] + n].copy_(old_v[off:off + n])
        self.state_bits, self.plan8, self._runs8 = 8, plan, {}

    def optimizer_state_bytes(self):
        """Bytes allocated for AdamW's two moments (codes and absmax arrays included; the fp32 master copy, 4 B per parameter at
        either width, is not counted).  0 before the state exists."""
        if self.master is None:
            return 0
        bufs = [self.m, self.vv] + ([self.m8, self.v8, self.am8, self.av8] if self.state_bits == 8 else [])
        return sum(t.numel() * t.element_size() for t in bufs)

    def optimizer_state_dict(self):
        """(tensors, meta) of a checkpoint's optimizer.safetensors.  fp32 state: master, exp_avg, exp_avg_sq and meta None (the
        layout every earlier checkpoint has).  8-bit state: master, the code and absmax arrays of the 8-bit tensors, the compact fp32
        moments of the rest, and meta {"bits": 8, "block": 256, "codebook": sha of csrc/adam8_codebook.h's tables}."""
        if self.state_bits == 32:
            return {"master": self.master, "exp_avg": self.m, "exp_avg_sq": self.vv}, None
        from .optim8 import BLOCK, codebook_sha
        return ({"master": self.master, "exp_avg_codes": self.m8, "exp_avg_sq_codes": self.v8, "exp_avg_absmax": self.am8,
                 "exp_avg_sq_absmax": self.av8, "exp_avg_fp32": self.m, "exp_avg_sq_fp32": self.vv},
                {"bits": 8, "block": BLOCK, "codebook": codebook_sha()})

    def load_optimizer_state_dict(self, st, meta=None, say=None):
        """Load what optimizer_state_dict() gave, into a state of self.state_bits: the same width is a plain copy; a state of the other
        width is loaded as it is and then converted by init_optimizer (quantised / dequantised on the device), which `say` is told."""
        from .optim8 import BLOCK, codebook_sha
        want = self.state_bits
        have = 8 if "exp_avg_codes" in st else 32
        if have == 8:
            meta = meta or {}
            if meta.get("codebook") != codebook_sha() or meta.get("block") != BLOCK:
                raise ValueError(f"8-bit optimizer state of another format (block {meta.get('block')}, codebook {meta.get('codebook')}): "
                                 f"this build has block {BLOCK}, codebook {codebook_sha()}")
        self.master = self.m = self.vv = None
        self._drop_state8()
        self.init_optimizer(state_bits=have)
        keys = {"master": self.master, "exp_avg": self.m, "exp_avg_sq": self.vv} if have == 32 else self.optimizer_state_dict()[0]
        for k, dst in keys.items():
            if tuple(st[k].shape) != tuple(dst.shape):
                raise ValueError(f"optimizer state '{k}': shape {tuple(st[k].shape)}, this model needs {tuple(dst.shape)}")
            dst.copy_(st[k])
        if have != want:
            if say is not None:
                say(f"optimizer state: the checkpoint holds {have}-bit AdamW moments, this run keeps {want}-bit ones: "
                    + ("quantising" if want == 8 else "dequantising") + " on load")
            self.init_optimizer(state_bits=want)

    def moment_views(self, name):
        """The stored moments of one trainable tensor: {"exp_avg", "exp_avg_sq"} fp32 views [n] at 32 bits; at 8 bits the same two keys for
        a tensor that keeps fp32 moments, else {"exp_avg_codes", "exp_avg_sq_codes" (uint8 [n]), "exp_avg_absmax", "exp_avg_sq_absmax"
        (fp32 [ceil(n / 256)])}.  Views: writing them writes the state."""
        off, n = self.lm.offsets[name]
        if self.state_bits == 32:
            return {"exp_avg": self.m[off:off + n], "exp_avg_sq": self.vv[off:off + n]}
        t = self.plan8.tensors[name]
        if t["bits"] == 32:
            return {"exp_avg": self.m[t["pos"]:t["pos"] + n], "exp_avg_sq": self.vv[t["pos"]:t["pos"] + n]}
        b, nb = t["block"], (n + 255) // 256
        return {"exp_avg_codes": self.m8[b * 256:b * 256 + n], "exp_avg_sq_codes": self.v8[b * 256:b * 256 + n],
                "exp_avg_absmax": self.am8[b:b + nb], "exp_avg_sq_absmax": self.av8[b:b + nb]}

    def _adamw8_runs(self, s, e):
        """The 8-bit and 32-bit runs of the parameter-group slice [s, e), with the device block tables of the 8-bit ones (built once)."""
        if (s, e) not in self._runs8:
            runs = []
            for run in self.plan8.runs(s, e):
                if run[0] == 8:
                    first, last = self.plan8.tensors[run[1][0]], self.plan8.tensors[run[1][-1]]
                    tab, nb = self.plan8.block_table(run[1], origin=first["off"])
                    runs.append((8, first["off"], last["off"] + last["n"], first["block"], nb, torch.from_numpy(tab).to(self.device)))
                else:
                    runs.append(run)
            self._runs8[(s, e)] = runs
        return self._runs8[(s, e)]

    def param_groups(self, lr, weight_decay=0.0, mm_projector_lr=None, no_decay_1d=True, mm_vision_tower_lr=None):
        """Contiguous (start, end, lr, wd) slices following LLaVATrainer.create_optimizer (llava_trainer.py:369-418):
        no weight decay for norm weights and biases; optional separate LR for the projector."""
        groups = []
        fresh = True             # a frozen tensor in between: the next group must not be merged across its slice
        frozen = getattr(self, "frozen_names", ())
        for name in self.lm.names():
            if name in frozen:
                fresh = True
                continue
            off, n = self.lm.offsets[name]
            shp = self.lm.shapes[name]
            nodecay = no_decay_1d and (len(shp) == 1 and ("norm" in name or name.endswith("bias")))
            glr = mm_projector_lr if (mm_projector_lr is not None and "mm_projector" in name) else lr
            if mm_vision_tower_lr is not None and "vision_tower" in name:
                glr = mm_vision_tower_lr
            gwd = 0.0 if nodecay else weight_decay
            if groups and not fresh and groups[-1][2] == glr and groups[-1][3] == gwd and groups[-1][1] <= off:
                groups[-1][1] = off + n  # merge (alignment gaps hold zeros and stay zero)
            else:
                groups.append([off, off + n, glr, gwd])
            fresh = False
        return [tuple(g) for g in groups]

    def optimizer_step(self, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, mm_projector_lr=None,
                       mm_vision_tower_lr=None):
        """AdamW over the flat buffers (fp32 master + moments), optional global-norm clipping without host sync."""
        self.init_optimizer()
        self.finish_grad_sync()
        self.opt_step += 1
        coef = None
        self.last_grad_norm = None
        for name in self.frozen_names:          # frozen tensors of the buffer take no part in the gradient norm
            self.G(name).zero_()
        if max_grad_norm is not None and max_grad_norm > 0:
            nc = ops.grad_norm_clip_coef(self.grads, max_grad_norm)
            self.last_grad_norm = nc[0:1]
            coef = nc[1:2]
        for s, e, glr, gwd in self.param_groups(lr, weight_decay, mm_projector_lr, mm_vision_tower_lr=mm_vision_tower_lr):
            if self.state_bits == 32:
                ops.adamw(self.lm.flat[s:e], self.master[s:e], self.grads[s:e], self.m[s:e], self.vv[s:e], glr, betas[0], betas[1],
                          eps, gwd, self.opt_step, gscale=coef)
                continue
            for run in self._adamw8_runs(s, e):             # one rv_adamw8 launch per 8-bit run, one rv_adamw per fp32 run
                if run[0] == 8:
                    _, a, b, blk, nb, tab = run
                    ops.adamw8(self.lm.flat[a:b], self.master[a:b], self.grads[a:b], self.m8[blk * 256:(blk + nb) * 256],
                               self.v8[blk * 256:(blk + nb) * 256], self.am8[blk:blk + nb], self.av8[blk:blk + nb], tab, nb, glr,
                               betas[0], betas[1], eps, gwd, self.opt_step, gscale=coef)
                else:
                    _, a, b, pos = run
                    ops.adamw(self.lm.flat[a:b], self.master[a:b], self.grads[a:b], self.m[pos:pos + b - a], self.vv[pos:pos + b - a],
                              glr, betas[0], betas[1], eps, gwd, self.opt_step, gscale=coef)
        self.weights_changed(tower=self.train_tower)
        self.zero_grad()

    # ------------------------------------------------------------------ state dict (reference names)
    def state_dict(self):
        """Every tensor under its reference name: trainable buffer, frozen tower and -- for LoRA / projector-only runs -- the frozen
        language-model store (adapters keep their .lora_A/.lora_B names; lora_state_dict() gives peft's layout)."""
        out = {}
        stores = [self.lm] + ([] if self.vis is self.lm else [self.vis]) + ([self.base] if self.base is not None else [])
        for fp in stores:
            for n in fp.names():
                if n in out:
                    continue        # the projector lives in the trainable buffer; the base store's copy of it is unused
                out[n] = fp.view(n)[:self.vocab] if n in ("model.embed_tokens.weight", "lm_head.weight") else fp.view(n)
        if self.nf4 is not None:            # an NF4 base: the dequantised bf16 matrices, which is what the model computes with
            plan = self.nf4["plan"]
            for i in range(plan.layers):
                buf = torch.zeros(plan.scratch_numel, dtype=BF16, device=self.device)
                self._nf4_dequant(i, buf)
                for n in plan.names(i):
                    t = plan.tensors[n]
                    out[n] = buf[t["dst"]:t["dst"] + t["n"]].view(t["shape"])
        return out

    def lora_state_dict(self):
        """Adapter tensors under peft's key layout (base_model.model.<module>.lora_{A,B}.default.weight) + the
        non-LoRA trainables (the reference saves them as non_lora_trainables.bin, train/train.py:1708-1717)."""
        assert self.lora
        adapters, others = {}, {}
        for n in self.lm.names():
            if ".lora_" in n:
                adapters["base_model.model." + n.replace(".weight", ".default.weight")] = self.lm.view(n)
            else:
                others[n] = self.lm.view(n)
        return adapters, others

    # ------------------------------------------------------------------ LoRA merge (peft merge_and_unload)
    def merge_lora_(self, adapters, scale):
        """W <- bf16(W + scale * B A) in place (rv_lora_merge_bf16) for every entry of `adapters`: {"model.layers.{i}.{module}": (A [r, in],
        B [out, r])}, module one of the seven adapted decoder linears.  W is wherever the weight lives -- the trainable buffer or the frozen
        base store, a row slice of the fused q|k|v / gate|up storage.  Every entry is checked before the first one is merged (KeyError on
        an unknown module or a shape that does not match its weight).  Biases, norms, embeddings, lm_head, the projector and the tower are
        not touched."""
        targets = {t for t, _, _ in LORA_TARGETS}
        work = []
        for name, (A, B) in adapters.items():
            parts = name.split(".", 3)
            wname = name + ".weight"
            if len(parts) != 4 or parts[:2] != ["model", "layers"] or parts[3] not in targets or not (
                    wname in self.lm.offsets or (self.base is not None and wname in self.base.offsets)):
                raise KeyError(f"{name}: not an adapted decoder linear of this model")
            w = self.W(wname)
            if A.dim() != 2 or B.dim() != 2 or A.shape[0] != B.shape[1] or A.shape[1] != w.shape[1] or B.shape[0] != w.shape[0]:
                raise KeyError(f"{name}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not match the weight {tuple(w.shape)}")
            work.append((wname, w, A.to(self.device, BF16).contiguous(), B.to(self.device, BF16).contiguous()))
        for wname, w, A, B in work:
            ops.lora_merge(w, A, B, scale)
        self.weights_changed()
        if self.master is not None:
            for wname, w, _, _ in work:
                if wname in self.lm.offsets:
                    off, n = self.lm.offsets[wname]
                    self.master[off:off + n].copy_(ops.to_f32(w.reshape(-1)))

    def merge_lora(self):
        """Merge this engine's own adapters into the frozen base (scale alpha / r), then become the projector-only layout
        (freeze_lm=True): frozen language model in self.base, projector and image_newline in the trainable buffer.  The adapters,
        their gradients and their AdamW state are dropped; the projector keeps its optimizer state.  A later training step follows
        the projector-only semantics (tune_mm_mlp_adapter): the projector trains, image_newline and the decoder are frozen."""
        if not self.lora:
            raise ValueError("merge_lora(): this engine has no LoRA adapters")
        if self.nf4 is not None:            # the merged weight is bf16(deq(W) + s B A); it is not requantised
            self.dequantize_base_()
        from collections import OrderedDict
        pairs = {}
        for i in range(self.l["layers"]):
            for t, _, _ in LORA_TARGETS:
                pre = f"model.layers.{i}.{t}"
                pairs[pre] = (self.lm.view(pre + ".lora_A.weight"), self.lm.view(pre + ".lora_B.weight"))
        self.merge_lora_(pairs, self.lora_scale)
        old = self.lm
        keep = [n for n in old.names() if ".lora_" not in n]
        new = FlatParams(OrderedDict((n, old.shapes[n]) for n in keep), self.device)
        for n in keep:
            new.view(n).copy_(old.view(n))
        if self.master is not None and self.state_bits == 32:
            state = []
            for buf in (self.master, self.m, self.vv):
                nb = new.like(torch.float32)
                for n in keep:
                    new.view(n, nb).copy_(old.view(n, buf))
                state.append(nb)
            self.master, self.m, self.vv = state
        saved8 = None
        if self.master is not None and self.state_bits == 8:            # per-tensor blocks: a plain copy per name into the new plan
            saved8 = {n: {k: v.clone() for k, v in self.moment_views(n).items()} for n in keep}
            nb = new.like(torch.float32)
            for n in keep:
                new.view(n, nb).copy_(old.view(n, self.master))
            saved8["master"] = nb
        self.lm = new
        if saved8 is not None:
            self.master = self.m = self.vv = None
            self._drop_state8()
            self.init_optimizer(state_bits=8)
            self.master = saved8.pop("master")
            for n, views in saved8.items():
                for k, v in self.moment_views(n).items():
                    v.copy_(views[k])
        self.grads = new.like(BF16)
        self.grad_accum_started = False
        self.ctx = None
        self._ws = None
        if self.sync is not None:
            from .ddp import FlatGradSync
            self.sync = FlatGradSync(self.grads, self.pg, force=self.force_grad_sync)
        self.lora = None
        self.freeze_lm = True
        self.frozen_names = {n for n in self.frozen_names if n in new.offsets}
        if "model.image_newline" in new.offsets:
            self.frozen_names.add("model.image_newline")
        self.weights_changed()

    def load_state_dict(self, sd, strict=False):
        from .params import load_named
        if self.nf4 is not None:
            from .config import canonical_name
            hit = [k for k in sd if canonical_name(k) in self.nf4["plan"].tensors]
            if hit:
                raise RuntimeError(f"load_state_dict(): {hit[0]} (and {len(hit) - 1} more) are decoder matrices of an NF4 base, which holds "
                                   "codes, not bf16 weights; load before quantize_base_(), or call dequantize_base_() first")
        missing, rest = load_named(self.lm, sd)
        for fp in ([] if self.vis is self.lm else [self.vis]) + ([self.base] if self.base is not None else []):
            m, rest2 = load_named(fp, {k: v for k, v in sd.items() if k in rest})
            if fp is self.base:     # the base store also has projector slots (unused): not "missing"
                m = [k for k in m if k not in self.lm.offsets]
            missing, rest = missing + m, rest2
        self.weights_changed()
        if self.master is not None:
            self.master.copy_(ops.to_f32(self.lm.flat))
        if strict and (missing or rest):
            raise KeyError(f"missing={missing[:4]} unexpected={rest[:4]}")
        return missing, rest


class KVCache:
    """Keys and values of one generate() call: per decoder layer a bf16 [B, L_max, 2 * kvd] tensor holding each position's post-RoPE
    K | V row as it sits in the q|k|v product (sequence b at rows 0 .. lens[b] - 1), and the host-side lengths.  Freed with the object.
    dtype "int8": every (position, kv head, K / V) group of hd values is stored as s = max|x| / 127 (1 for a zero group) and
    q = clamp(rint(x / s), -127, 127): layers[i] is int8 [B, L_max, 2 * kvd] with the bf16 cache's columns and scales[i] is fp32
    [B, L_max, 2 * Hkv] (column g: K head g; column Hkv + g: V head g); the value read back is bf16(float(q) * s).  With
    LlavaEngine.kv8_decode False the same values are kept dequantised instead: layers[i] bf16, scales None.
    pos_off (None, or int64 [B]; prefill(compress=)): sequence b's slot s < lens[b] need not hold position s -- a compressed prompt
    keeps lens[b] = N of its P positions per layer and kv head -- and the next token sits at position lens[b] + pos_off[b]."""
    chunk = 128           # keys per decode-attention workgroup: fixed, so a sequence's result never depends on the batch around it

    def __init__(self, layers, lens, L_max, dtype="bf16", scales=None):
        self.layers = layers
        self.scales = scales
        self.dtype = dtype
        self.lens = np.asarray(lens, dtype=np.int64).copy()
        self.L_max = int(L_max)
        self.pos_off = None

    @property
    def B(self):
        return int(self.lens.shape[0])

    def grow(self, L_new, keep):
        """Reallocate every layer to L_new slots per sequence, copying the first `keep` rows of each sequence (what is still valid)."""
        assert L_new >= self.L_max and 0 <= keep <= self.L_max
        for group in (self.layers, self.scales or []):
            for i, t in enumerate(group):
                nt = torch.zeros(t.shape[0], L_new, t.shape[2], dtype=t.dtype, device=t.device)
                nt[:, :keep].copy_(t[:, :keep])
                group[i] = nt
        self.L_max = int(L_new)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in list(self.layers) + list(self.scales or []))

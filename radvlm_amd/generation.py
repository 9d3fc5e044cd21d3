"""Greedy generation over the engine's KV-cached decode (LlavaLlamaForCausalLM.generate).

HF semantics followed (HF: = transformers as pinned by the reference): GenerationMixin.generate -> _sample with do_sample=False
(HF:generation/utils.py), for a decoder-only model called with inputs_embeds, which is how the reference's generate() calls it after
the multimodal splice (llava_llama.py generate()).  The returned sequences then hold the NEW tokens only.  Every row is generated as
if it were alone (left-padded HF generation: the row's own positions 0 .. len - 1).  The bookkeeping below is host code without a
device, so it is tested on its own (tests/test_generate_host.py).
"""
from types import SimpleNamespace

import numpy as np
import torch

_IGNORED_WHEN_GREEDY = ("temperature", "top_p", "top_k", "typical_p")     # sampling knobs HF ignores (with a warning) when do_sample=False
_ACCEPTED = ("max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "attention_mask", "stopping_criteria", "use_cache", "do_sample",
             "num_beams", "streamer", "output_scores", "return_dict_in_generate", "num_return_sequences", "position_ids", "inputs_embeds") + _IGNORED_WHEN_GREEDY


class GenerateDecoderOnlyOutput(SimpleNamespace):
    """HF's return_dict_in_generate output: .sequences [B, T_new], .scores (one fp32 [B, vocab] tensor per step) or None."""

    def __getitem__(self, k):
        return getattr(self, k)


def parse_generate_kwargs(kwargs, lora=False, config_eos=None, config_pad=None):
    """Validate generate() keyword arguments; returns a namespace with the normalised settings.  Raises NotImplementedError for what this
    build does not do (sampling, beam search, streamers, caller-supplied inputs_embeds, LoRA engines) and TypeError for unknown names."""
    unknown = sorted(k for k in kwargs if k not in _ACCEPTED)
    if unknown:
        raise TypeError(f"generate() got unexpected keyword arguments {unknown}")
    if kwargs.get("inputs_embeds") is not None:
        raise NotImplementedError("`inputs_embeds` is not supported")      # the reference's generate() raises the same
    if kwargs.get("do_sample"):
        raise NotImplementedError("do_sample=True: only greedy decoding is implemented")
    if (kwargs.get("num_beams") or 1) > 1:
        raise NotImplementedError("num_beams > 1: beam search is not implemented")
    if (kwargs.get("num_return_sequences") or 1) > 1:
        raise NotImplementedError("num_return_sequences > 1 needs sampling or beam search")
    if kwargs.get("streamer") is not None:
        raise NotImplementedError("streamer: token streaming is not implemented")
    if lora:
        raise NotImplementedError("generation with LoRA adapters: merge them into the base weights first with "
                                  "model.merge_and_unload() (the reference merges adapters before evaluation)")
    eos = kwargs.get("eos_token_id", config_eos)
    eos = [] if eos is None else ([int(eos)] if isinstance(eos, (int, np.integer)) else [int(e) for e in eos])
    pad = kwargs.get("pad_token_id", config_pad)
    if pad is None:
        pad = eos[0] if eos else 0
    mnt, ml = kwargs.get("max_new_tokens"), kwargs.get("max_length")
    if mnt is not None and int(mnt) < 0:
        raise ValueError("max_new_tokens must be >= 0")
    crit = kwargs.get("stopping_criteria") or []
    crit = list(crit) if isinstance(crit, (list, tuple)) or hasattr(crit, "__iter__") else [crit]
    for c in crit:
        if not callable(c):
            raise TypeError(f"stopping criterion {c!r} is not callable")
    return SimpleNamespace(eos=eos, pad=int(pad), max_new_tokens=None if mnt is None else int(mnt), max_length=None if ml is None else int(ml),
                           stopping_criteria=crit, output_scores=bool(kwargs.get("output_scores", False)),
                           return_dict=bool(kwargs.get("return_dict_in_generate", False)), attention_mask=kwargs.get("attention_mask"))


def new_token_budget(cfg, prompt_len):
    """Number of tokens to generate at most.  max_new_tokens wins; else HF's max_length, which for inputs_embeds generation counts the
    prompt embeddings as well (HF: _prepare_generated_length subtracts inputs_embeds.shape[1]); else HF's default max_length of 20."""
    if cfg.max_new_tokens is not None:
        return cfg.max_new_tokens
    if cfg.max_length is not None:
        return max(0, cfg.max_length - int(prompt_len))
    return 20


class GreedyState:
    """Finished-row bookkeeping of HF's greedy loop: a finished row emits pad_token_id; a row finishes on an EOS token or when a stopping
    criterion says so (criteria get the new tokens so far [B, t] and the step's scores, and return a bool or a bool tensor [B])."""

    def __init__(self, B, cfg):
        self.cfg = cfg
        self.unfinished = np.ones(B, dtype=bool)
        self.tokens = []

    def step(self, next_tokens, scores=None, device=None):
        """next_tokens: argmax ids [B] (int array / tensor).  Returns the emitted tokens [B] (numpy int64)."""
        nt = np.asarray(next_tokens.cpu() if torch.is_tensor(next_tokens) else next_tokens, dtype=np.int64).reshape(-1)
        if self.cfg.eos:
            nt = np.where(self.unfinished, nt, self.cfg.pad)
        self.tokens.append(nt)
        done = np.zeros_like(self.unfinished)
        if self.cfg.eos:
            done |= np.isin(nt, self.cfg.eos)
        if self.cfg.stopping_criteria:
            ids = torch.as_tensor(self.sequences(), device=device)
            for c in self.cfg.stopping_criteria:
                r = c(ids, scores)
                r = r.detach().cpu().numpy() if torch.is_tensor(r) else np.asarray(r)
                done |= np.broadcast_to(r.astype(bool).reshape(-1) if r.ndim else r.astype(bool), done.shape)
        self.unfinished &= ~done
        return nt

    @property
    def all_done(self):
        return not self.unfinished.any()

    def sequences(self):
        B = self.unfinished.shape[0]
        return np.stack(self.tokens, 1) if self.tokens else np.zeros((B, 0), dtype=np.int64)


def greedy_generate(engine, input_ids, attention_mask, images, image_sizes, cfg):
    """prefill once, then decode_step per token until every row has finished or the budget is spent."""
    from . import ops
    ids = np.asarray(input_ids.cpu() if torch.is_tensor(input_ids) else input_ids)
    if ids.ndim == 1:
        ids = ids[None]
    am = cfg.attention_mask
    am = None if am is None else np.asarray(am.cpu() if torch.is_tensor(am) else am)
    B = ids.shape[0]
    st = GreedyState(B, cfg)
    scores = []
    dev = engine.device
    # prompt length in HF's sense: the spliced inputs_embeds width (the longest spliced prompt of the batch)
    plan_len = None
    if cfg.max_new_tokens is None and cfg.max_length is not None:
        plan_len = int(engine.plan(ids, am, None, list(images) if images is not None else [], image_sizes)["S"])
    T = new_token_budget(cfg, plan_len or 0)
    if T > 0:
        cache, logits = engine.prefill(ids, am, images, image_sizes, max_new_tokens=T)
        for t in range(T):
            nxt = ops.argmax_rows(logits, engine.vocab)
            if cfg.output_scores:
                scores.append(logits.clone())
            tok = st.step(nxt, logits, device=dev)
            if st.all_done or t == T - 1:
                break
            logits = engine.decode_step(cache, torch.from_numpy(tok))
        del cache
    seq = torch.from_numpy(st.sequences()).to(dev)
    if cfg.return_dict:
        return GenerateDecoderOnlyOutput(sequences=seq, scores=tuple(scores) if cfg.output_scores else None)
    return seq

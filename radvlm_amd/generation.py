"""Greedy and seeded-sampling generation over the engine's KV-cached decode (LlavaLlamaForCausalLM.generate).

HF semantics followed (HF: = transformers as pinned by the reference): GenerationMixin.generate -> _sample with do_sample=False
(HF:generation/utils.py), for a decoder-only model called with inputs_embeds, which is how the reference's generate() calls it after
the multimodal splice (llava_llama.py generate()).  The returned sequences then hold the NEW tokens only.  Every row is generated as
if it were alone (left-padded HF generation: the row's own positions 0 .. len - 1).  HF's greedy logits processors run on each step's fp32 scores
(HF:generation/logits_process.py); with inputs_embeds HF's input_ids start empty, so they see the generated tokens only, never the
prompt.  The bookkeeping below is host code without a device, so it is tested on its own (tests/test_generate_host.py,
tests/test_logits_process_host.py).

Sampling (do_sample=True together with seed=): after the processors HF runs the warpers temperature -> top-k -> top-p -> min-p, takes the
softmax and draws one token (HF: _sample with do_sample=True).  Here the draw is counter-based: row or request i at its own step t uses
u(seed_i, t) (sample_uniform below), so a result is reproducible by construction and does not depend on batching or scheduling.  It is NOT
torch's global generator stream, which is why a bare do_sample=True keeps raising.
"""
from types import SimpleNamespace

import numpy as np
import torch

# sampling knobs HF ignores (with a warning) when do_sample=False
_IGNORED_WHEN_GREEDY = ("temperature", "top_p", "top_k", "typical_p", "min_p", "epsilon_cutoff", "eta_cutoff")
# HF's greedy logits processors (HF: generation/logits_process.py, wired by GenerationMixin._get_logits_processor)
_PROCESSORS = ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "suppress_tokens",
               "begin_suppress_tokens")
_ACCEPTED = ("max_new_tokens", "max_length", "eos_token_id", "pad_token_id", "attention_mask", "stopping_criteria", "use_cache", "do_sample",
             "num_beams", "streamer", "output_scores", "output_logits", "return_dict_in_generate", "num_return_sequences", "position_ids",
             "inputs_embeds", "past_key_values", "seed", "kv_cache_dtype") + _PROCESSORS + _IGNORED_WHEN_GREEDY
# prompt-lookup decoding (HF's names): generate() alone takes them, generate_batch() and generate_beams() reject them as unknown
_LOOKUP = ("prompt_lookup_num_tokens", "max_matching_ngram_size")
# assisted generation (HF's names): a draft model proposes, the model verifies; generate() alone takes them, as the lookup names
_ASSIST = ("assistant_model", "num_assistant_tokens")
ASSIST_DEFAULT_TOKENS = 5     # HF's num_assistant_tokens default, kept constant (no "heuristic" schedule)
# classifier-free guidance (HF's names; negative_images / negative_image_sizes are ours: HF's negative prompt cannot carry an image)
_GUIDANCE = ("guidance_scale", "negative_prompt_ids", "negative_prompt_attention_mask", "negative_images", "negative_image_sizes")
# DoLa, decoding by contrasting layers (HF's name); _parse_dola / resolve_dola_layers
_DOLA = ("dola_layers",)
DOLA_MAX_LAYERS = 16          # candidate layers per call (rv_dola_contrast_rows_f32)
# constrained decoding (ours: HF's prefix_allowed_tokens_fn is a Python callback per row and step); constraints.TokenConstraint
_CONSTRAINT = ("constraint",)
# decode attention maps (output_attentions is HF's name; attention_layers / attention_reduce are ours): generate() alone takes them,
# generate_batch() and generate_beams() reject them as unknown; _parse_attentions / resolve_attention_layers
_ATTENTIONS = ("output_attentions", "attention_layers", "attention_reduce")
# prompt cache compression (ours: SnapKV, Li et al. 2024): generate() and generate_batch() take them, generate_beams() and score() reject
# them as unknown; parse_prompt_kv
_KVPRESS = ("prompt_kv_budget", "prompt_kv_window", "prompt_kv_pool")
KVPRESS_MAX_WINDOW = 64       # observation window rows (rv_kv_votes_f32)
KVPRESS_MAX_POOL = 63         # pooling width (rv_kv_select_i32)
LOOKUP_MAX_TOKENS = 31        # k drafted tokens are verified as k + 1 rows, and the skinny GEMM takes ops.GEMV_MAX_M = 32


class GenerateDecoderOnlyOutput(SimpleNamespace):
    """HF's return_dict_in_generate output: .sequences [B, T_new]; .scores (output_scores: the processed fp32 [B, vocab] scores of each
    step) and .logits (output_logits: the raw ones), each a tuple or None.  output_attentions: .attentions, a tuple over the generated
    steps of a tuple over .attention_layers (the resolved layer numbers) of fp32 [B, H, 1, L_t] ([B, 1, 1, L_t] under "mean_heads")."""

    def __getitem__(self, k):
        return getattr(self, k)


def parse_generate_kwargs(kwargs, lora=False, config_eos=None, config_pad=None, lookup=False, attentions=False):
    """Validate generate() keyword arguments; returns a namespace with the normalised settings.  Every argument is checked on its own
    first: TypeError for unknown names, ValueError for a bad value, NotImplementedError for what this build does not do at all
    (do_sample=True without seed=, beam search, streamers, caller-supplied inputs_embeds, LoRA engines).  Then the combinations:
    NotImplementedError for the first row of REFUSALS whose two features are both on (refuse_combinations).
    .sampling: None for greedy, else the warper settings and the seed as given (sampling_seeds() resolves it per row).
    lookup: also take prompt_lookup_num_tokens / max_matching_ngram_size (.lookup: None, or .k and .max_ngram; .drafter: None,
    greedy_generate then builds a PromptLookupDrafter; a test or a benchmark may set another object with propose(seq)).
    lookup also takes assistant_model / num_assistant_tokens (.assistant: None, or .model and .k; greedy_generate then checks the model
    against the engine and builds an assist.ModelDrafter).
    attentions: also take output_attentions / attention_layers / attention_reduce (.attentions: None, or .layers and .reduce).
    .kv_cache_dtype: "bf16" or "int8"; .guidance (_parse_guidance), .dola (_parse_dola), .constraint (_parse_constraint) and .kvpress
    ((N, w, k), parse_prompt_kv): None when off; the resolve_* functions finish them once the call knows the engine and the rows."""
    unknown = sorted(k for k in kwargs if k not in _ACCEPTED and k not in _GUIDANCE and k not in _DOLA and k not in _CONSTRAINT
                     and k not in _KVPRESS and not (lookup and k in _LOOKUP + _ASSIST) and not (attentions and k in _ATTENTIONS))
    if unknown:
        raise TypeError(f"generate() got unexpected keyword arguments {unknown}")
    guidance = _parse_guidance(kwargs)
    dola = _parse_dola(kwargs)
    constraint = _parse_constraint(kwargs)
    att = _parse_attentions(kwargs)
    press = parse_prompt_kv(kwargs)
    if kwargs.get("inputs_embeds") is not None:
        raise NotImplementedError("`inputs_embeds` is not supported")      # the reference's generate() raises the same
    if kwargs.get("do_sample") and kwargs.get("seed") is None:
        raise NotImplementedError("do_sample=True without seed=: drawing from torch's global RNG is not implemented; pass seed= (an int, "
                                  "or one int per row) for counter-based, reproducible sampling")
    if (kwargs.get("num_beams") or 1) > 1:
        raise NotImplementedError("num_beams > 1: beam search is not implemented here; call model.generate_beams(...)")
    if (kwargs.get("num_return_sequences") or 1) > 1:
        raise NotImplementedError("num_return_sequences > 1 needs sampling or beam search")
    if kwargs.get("streamer") is not None:
        raise NotImplementedError("streamer: token streaming is not implemented")
    pkv = kwargs.get("past_key_values")
    if pkv is not None:
        if not isinstance(pkv, GenerationCache):
            raise TypeError(f"past_key_values must be a radvlm_amd.generation.GenerationCache (create an empty one with GenerationCache() "
                            f"and pass it to every call of the conversation), not {type(pkv).__name__}")
        if kwargs.get("use_cache") is False:
            raise ValueError("use_cache=False contradicts past_key_values: pass one or the other")
    if lora:
        raise NotImplementedError("generation with LoRA adapters: merge them into the base weights first with "
                                  "model.merge_and_unload() (the reference merges adapters before evaluation), or decode on the "
                                  "live adapters with model.enable_adapter_decoding()")
    kv_dtype = parse_kv_cache_dtype(kwargs.get("kv_cache_dtype"))
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
    cfg = SimpleNamespace(eos=eos, pad=int(pad), max_new_tokens=None if mnt is None else int(mnt), max_length=None if ml is None else int(ml),
                          stopping_criteria=crit, output_scores=bool(kwargs.get("output_scores", False)),
                          output_logits=bool(kwargs.get("output_logits", False)),
                          return_dict=bool(kwargs.get("return_dict_in_generate", False)), attention_mask=kwargs.get("attention_mask"),
                          past_key_values=pkv, sampling=_parse_sampling(kwargs), lookup=_parse_lookup(kwargs), drafter=None,
                          assistant=_parse_assistant(kwargs),
                          kv_cache_dtype=kv_dtype, guidance=guidance, dola=dola, constraint=constraint, attentions=att, kvpress=press,
                          **_parse_processors(kwargs, eos))
    refuse_combinations(features_of(cfg), "generate()")
    return cfg


# Combinations that are not implemented.  FEATURES: a feature's name in features_of() -> how a message names it.  REFUSALS: (feature,
# feature, why); the message is "<feature> with <feature>: <why>".  The first row whose two features are both on is the one reported, so
# the order is part of the behaviour.  A new feature adds its rows here and nowhere else.
FEATURES = dict(kvpress="prompt_kv_budget / prompt_kv_window", attentions="output_attentions", constraint="constraint", guidance="guidance_scale",
                dola="dola_layers", past_key_values="past_key_values", lookup="prompt_lookup_num_tokens", int8="kv_cache_dtype='int8'",
                share_prefix="share_prefix=True", sampling="do_sample=True", lora="LoRA adapters", assistant="assistant_model",
                nf4="an NF4 base (quantize_base_())")
REFUSALS = (
    ("kvpress", "past_key_values", "the extend pass reads a cache whose slots are its positions"),
    ("kvpress", "lookup", "the verify step reads a cache whose slots are its positions"),
    ("kvpress", "guidance", "compressing the two branches of a guided call is not implemented"),
    ("kvpress", "dola", "the compressed prompt pass hands out no tapped rows"),
    ("kvpress", "attentions", "a map over a compact cache's slots has no position axis"),
    ("kvpress", "int8", "the gather kernel writes bf16 rows only"),
    ("attentions", "int8", "the probability kernel reads a bf16 cache only"),
    ("attentions", "past_key_values", "the extend pass hands out no attention rows"),
    ("attentions", "lookup", "the verify step hands out no attention rows"),
    ("attentions", "guidance", "maps of the two branches of a guided step are not implemented"),
    ("attentions", "dola", "the tapped decode step hands out no attention rows"),
    ("constraint", "lookup", "every drafted row of a verify step would need its own automaton state, which is not implemented"),
    ("constraint", "guidance", "masking the two branches of a guided step is not implemented"),
    ("constraint", "dola", "masking the contrasted scores is not implemented"),
    ("guidance", "past_key_values", "a guided call fills one cache with both branches and keeps none of it across calls"),
    ("guidance", "lookup", "verifying drafts on two branches is not implemented"),
    ("dola", "guidance", "contrasting layers on top of the guided scores is not implemented"),
    ("dola", "past_key_values", "the extend pass hands out no intermediate hidden states"),
    ("dola", "lookup", "the verify step hands out no intermediate hidden states"),
    ("int8", "past_key_values", "a GenerationCache is extended by the extend-attention kernel, which reads a bf16 cache only"),
    ("int8", "lookup", "the verify-attention kernel reads a bf16 cache only"),
    ("lookup", "sampling", "speculative sampling is not implemented"),
    ("share_prefix", "int8", "the extend-attention and shared decode kernels read a bf16 cache only"),
    ("share_prefix", "guidance", "sharing across the two branches of a guided call is not implemented"),
    ("share_prefix", "dola", "the extend pass and the shared decode step hand out no intermediate hidden states"),
    ("kvpress", "share_prefix", "a follower's copy and the extend pass read a cache whose slots are its positions"),
    ("attentions", "lora", "attention maps on the live adapters are not implemented; merge them first with model.merge_and_unload()"),
    ("assistant", "lookup", "a call takes one drafter: the draft model or the n-gram lookup"),
    ("kvpress", "assistant", "the verify step reads a cache whose slots are its positions"),
    ("attentions", "assistant", "the verify step hands out no attention rows"),
    ("constraint", "assistant", "every drafted row of a verify step would need its own automaton state, which is not implemented"),
    ("guidance", "assistant", "verifying drafts on two branches is not implemented"),
    ("dola", "assistant", "the verify step hands out no intermediate hidden states"),
    ("int8", "assistant", "the verify-attention kernel reads a bf16 cache only"),
    ("assistant", "past_key_values", "the draft model's cache is not kept across calls"),
    # a row whose second feature is None refuses its first feature on its own: "<feature>: <why>"
    ("nf4", None, "generation, scoring and the cached decode steps read bf16 (or int8 / MXFP4 decode) weights and there is no NF4 decode "
                  "kernel; call model.dequantize_base_() to keep training on the dequantised bf16 base, or model.merge_and_unload()"),
)


def features_of(cfg, lora=False):
    """The FEATURES that a cfg has on, parsed or built by hand (a missing attribute is off).  lora: the engine decodes on live
    adapters."""
    get = lambda name: getattr(cfg, name, None)
    # a drafter set by hand counts as the lookup; the draft model's drafter is the assistant's, and sampling composes with it
    lookup = get("lookup") if get("drafter") is None or get("assistant") is not None else True
    on = dict(assistant=get("assistant"), kvpress=get("kvpress"), attentions=get("attentions"), constraint=get("constraint"), guidance=get("guidance"), dola=get("dola"),
              past_key_values=get("past_key_values"), sampling=get("sampling"), lookup=lookup,
              int8=get("kv_cache_dtype") == "int8" or None, share_prefix=get("share_prefix") or None, lora=lora or None)
    return {name for name, v in on.items() if v is not None}


def refuse_combinations(features_on, where):
    """NotImplementedError for the first row of REFUSALS whose two features are both in features_on.  where: the caller, named when
    features_on holds a name that is no feature."""
    if not set(features_on) <= set(FEATURES):
        raise ValueError(f"{where}: unknown features {sorted(set(features_on) - set(FEATURES))}")
    for a, b, why in REFUSALS:
        if a in features_on and b is None:
            raise NotImplementedError(f"{FEATURES[a]}: {why}")
        if a in features_on and b in features_on:
            raise NotImplementedError(f"{FEATURES[a]} with {FEATURES[b]}: {why}")


def _parse_attentions(kwargs):
    """The attention-map keywords as far as they can be checked without the model's depth; None when output_attentions is off.
    output_attentions: a bool (None: off), and True needs return_dict_in_generate=True; attention_layers: None (all layers) or a list
    or tuple of ints, negative ones counting from the last layer as in HF's hidden_states (-1: the last); attention_reduce: None or
    "mean_heads".  ValueError for anything else, and for attention_layers / attention_reduce while output_attentions is off."""
    on = kwargs.get("output_attentions")
    if on is not None and not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"`output_attentions` has to be True or False, but is {on!r}")
    layers, reduce = kwargs.get("attention_layers"), kwargs.get("attention_reduce")
    if not on:
        given = [k for k, v in (("attention_layers", layers), ("attention_reduce", reduce)) if v is not None]
        if given:
            raise ValueError(f"{given} given without output_attentions=True")
        return None
    if not kwargs.get("return_dict_in_generate"):
        raise ValueError("output_attentions=True needs return_dict_in_generate=True: the maps are returned as .attentions")
    if reduce is not None and not (isinstance(reduce, str) and reduce == "mean_heads"):
        raise ValueError(f"`attention_reduce` has to be None or 'mean_heads', but is {reduce!r}")
    if layers is not None:
        if not isinstance(layers, (list, tuple)):
            raise ValueError(f"`attention_layers` has to be None or a list of layer numbers, but is {layers!r}")
        if any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) for c in layers):
            raise ValueError(f"`attention_layers` has to hold ints, but is {layers!r}")
        if not layers:
            raise ValueError("`attention_layers` is an empty list: pass None for every layer")
        layers = tuple(int(c) for c in layers)
    return SimpleNamespace(layers=layers, reduce=reduce)


def resolve_attention_layers(spec, L):
    """The layer numbers of an output_attentions call on a decoder of L layers, in the given order: None is every layer; a negative
    entry c means L + c.  ValueError for a value outside [-L, L) and for a layer named twice after that normalisation."""
    L = int(L)
    if spec is None:
        return tuple(range(L))
    if any(not -L <= c < L for c in spec):
        raise ValueError(f"attention_layers={list(spec)}: every entry has to lie in [-{L}, {L})")
    layers = tuple(c + L if c < 0 else c for c in spec)
    if len(set(layers)) != len(layers):
        raise ValueError(f"attention_layers={list(spec)} names a layer twice: {list(layers)}")
    return layers


def _parse_constraint(kwargs):
    """The constraint keyword as far as it can be checked without the row count and the vocabulary: None (off), a TokenConstraint, or
    a list of TokenConstraint and None entries (a tuple becomes a list).  ValueError for anything else."""
    from .constraints import TokenConstraint
    v = kwargs.get("constraint")
    if v is None or isinstance(v, TokenConstraint):
        return v
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"`constraint` has to be a TokenConstraint or a list with one (or None) per row, not {type(v).__name__}")
    for i, c in enumerate(v):
        if c is not None and not isinstance(c, TokenConstraint):
            raise ValueError(f"`constraint[{i}]` has to be a TokenConstraint or None, not {type(c).__name__}")
    return list(v)


class ConstraintMirror:
    """The host's copy of the automaton states a constrained call keeps on the device, one per row (generate) or per cache slot
    (generate_batch), advanced with the tokens the loop reads back anyway: it finds a dead end at the step where it happens, without
    another copy from the device.  A dead end: the processors or warpers banned everything the state allows -- min_new_tokens against
    a state that allows only EOS, say -- so the row is all -inf and its token means nothing."""

    def __init__(self, table, n):
        self.table = table
        self.state = np.full(n, -1, dtype=np.int64)

    def take(self, idx, tokens, minus_inf, who, steps):
        """Entries idx (int array) emitted `tokens` at their steps `steps`.  minus_inf(k): is the score of tokens[k] -inf?  Asked only
        for a live entry that emitted token 0, which is what the argmax of an all -inf row gives; a negative token is the sampler's mark
        for such a row.  RuntimeError naming who(k) and the step at the first dead end."""
        idx, tokens = np.asarray(idx, dtype=np.int64), np.asarray(tokens, dtype=np.int64)
        s = self.state[idx]
        nxt = self.table.advance(s, tokens)
        for k in np.flatnonzero((s >= 0) & ((nxt == -2) | (tokens == 0))):
            if nxt[k] == -2 or minus_inf(int(k)):
                ids = self.table.allowed(int(s[k]))
                raise RuntimeError(f"constraint: {who(int(k))} reached a dead end at step {int(np.broadcast_to(steps, idx.shape)[k])}: "
                                   f"its automaton state allows only the ids {ids[:8].tolist()}{' ...' if ids.size > 8 else ''}, and "
                                   f"the logits processors or warpers banned all of them (or left no finite score)")
        self.state[idx] = nxt


def _parse_dola(kwargs):
    """The dola_layers keyword, validated as far as it can be without the model's depth: None (off), "low", "high", or a tuple of
    distinct non-negative ints (a list or tuple, in the given order).  ValueError for any other string or type, an empty list, a bool,
    a non-int, a negative value, a duplicate, and more than DOLA_MAX_LAYERS values."""
    v = kwargs.get("dola_layers")
    if v is None:
        return None
    if isinstance(v, str):
        if v not in ("low", "high"):
            raise ValueError(f"`dola_layers` has to be 'low', 'high' or a list of layer numbers, but is {v!r}")
        return v
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"`dola_layers` has to be 'low', 'high' or a list of layer numbers, but is {v!r}")
    if any(isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) for c in v):
        raise ValueError(f"`dola_layers` has to hold ints, but is {v!r}")
    layers = tuple(int(c) for c in v)
    if not layers:
        raise ValueError("`dola_layers` is an empty list: there is no layer to contrast with")
    if min(layers) < 0:
        raise ValueError(f"`dola_layers` holds a negative layer number: {list(layers)}")
    if len(set(layers)) != len(layers):
        raise ValueError(f"`dola_layers` holds a layer twice: {list(layers)}")
    if len(layers) > DOLA_MAX_LAYERS:
        raise ValueError(f"`dola_layers` holds {len(layers)} layers; at most {DOLA_MAX_LAYERS} candidates are contrasted")
    return layers


def resolve_dola_layers(spec, L, tied=False):
    """The candidate layer numbers of a DoLa call on a decoder of L layers (HF: _dola_decoding), in contrast order: "low" is
    range(start, L // 2, 2) for L <= 40, else range(start, 20, 2); "high" is range(L // 2, L, 2) for L <= 40, else range(L - 20, L,
    2); a tuple is taken as given.  start = 0 for untied output embeddings (every geometry here); tied: HF's 2 if L > 2, 1 if L == 2,
    else 0.  Layer c is the hidden state that enters decoder layer c (0: the embeddings).  ValueError for an empty result, a value
    outside [0, L) -- HF drops those silently -- and more than DOLA_MAX_LAYERS candidates."""
    L = int(L)
    start = (2 if L > 2 else (1 if L == 2 else 0)) if tied else 0
    if spec == "low":
        layers = tuple(range(start, L // 2, 2)) if L <= 40 else tuple(range(start, 20, 2))
    elif spec == "high":
        layers = tuple(range(L // 2, L, 2)) if L <= 40 else tuple(range(L - 20, L, 2))
    else:
        layers = _parse_dola(dict(dola_layers=spec))
        if layers is None or isinstance(layers, str):
            raise ValueError(f"`dola_layers` has to be 'low', 'high' or a list of layer numbers, but is {spec!r}")
    if not layers:
        raise ValueError(f"dola_layers={spec!r} names no layer of a {L}-layer decoder")
    if any(not 0 <= c < L for c in layers):
        raise ValueError(f"dola_layers={list(layers)}: every candidate has to lie in [0, {L}) (0: the embeddings, k: after layer k)")
    if len(layers) > DOLA_MAX_LAYERS:
        raise ValueError(f"dola_layers={spec!r} gives {len(layers)} layers; at most {DOLA_MAX_LAYERS} candidates are contrasted")
    return layers


def _parse_guidance(kwargs):
    """Classifier-free guidance settings; None when it is off.  guidance_scale: None or 1 is off (HF adds no processor then, and the call
    is today's call); any other finite real -- 0, negatives and values below 1 included, as in HF -- turns it on.  ValueError for a bool,
    a non-number, a value that is not finite as fp32 (the kernel's scale), and for any negative_* argument while guidance is off.  The
    negative prompt is kept as given; resolve_negative_prompts() checks it against the prompt."""
    g = kwargs.get("guidance_scale")
    if g is not None:
        ok = not isinstance(g, bool) and isinstance(g, (int, float, np.floating, np.integer))
        if ok:
            with np.errstate(all="ignore"):
                ok = bool(np.isfinite(np.float32(min(max(g, -1e39), 1e39))))
        if not ok:
            raise ValueError(f"`guidance_scale` has to be a finite number, but is {g!r}")
    neg = {k: kwargs.get(k) for k in _GUIDANCE[1:]}
    if g is None or g == 1:
        given = sorted(k for k, v in neg.items() if v is not None)
        if given:
            raise ValueError(f"{given} given without a guidance_scale other than 1: a negative prompt has no effect without guidance")
        return None
    return SimpleNamespace(scale=float(g), negative_prompt_ids=neg["negative_prompt_ids"],
                           negative_prompt_attention_mask=neg["negative_prompt_attention_mask"], negative_images=neg["negative_images"],
                           negative_image_sizes=neg["negative_image_sizes"])


def _check_negative_images(what, ids, images):
    """The image rule of a negative prompt: images are required when it holds placeholders and refused when it holds none."""
    from .splice import IMAGE_TOKEN_INDEX
    k = int((np.asarray(ids) == IMAGE_TOKEN_INDEX).sum())
    n = len(images)
    if k and not n:
        raise ValueError(f"{what}: the negative prompt holds {k} image tokens but no negative_images were passed")
    if n and not k:
        raise ValueError(f"{what}: negative_images were passed but the negative prompt holds no image token")
    if k != n:
        raise ValueError(f"{what}: the negative prompt holds {k} image tokens but {n} negative_images were passed")


def resolve_negative_prompts(guidance, ids, am):
    """The unconditional rows of a guided generate() call: (ids int64 [B, Ln], mask bool [B, Ln], images list, image_sizes or None).
    Without negative_prompt_ids each row's negative prompt is its last real prompt token (HF: input_ids[:, -1:] on the first pass).
    ValueError for a row count other than B, a mask of another shape, a row that is empty after masking, and images that do not match
    the placeholders (_check_negative_images)."""
    ids = np.asarray(ids)
    B = ids.shape[0]
    nid, nam = guidance.negative_prompt_ids, guidance.negative_prompt_attention_mask
    to_np = lambda v: np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)
    if nid is None:
        if nam is not None:
            raise ValueError("negative_prompt_attention_mask given without negative_prompt_ids")
        if am is None:
            nid = ids[:, -1:]
        else:
            m = np.asarray(am).reshape(B, -1).astype(bool)
            if not m.any(1).all():
                raise ValueError("the default negative prompt is each row's last prompt token, but a row has none")
            last = m.shape[1] - 1 - np.argmax(m[:, ::-1], axis=1)
            nid = ids[np.arange(B), last][:, None]
        nid = np.ascontiguousarray(nid, dtype=np.int64)
        nam = np.ones(nid.shape, dtype=bool)
    else:
        nid = to_np(nid)
        if nid.ndim == 1:
            nid = nid[None]
        if nid.ndim != 2 or not np.issubdtype(nid.dtype, np.integer):
            raise ValueError(f"`negative_prompt_ids` has to hold token ids [B, Ln], got shape {nid.shape}, dtype {nid.dtype}")
        if nid.shape[0] != B:
            raise ValueError(f"`negative_prompt_ids` holds {nid.shape[0]} rows for {B} prompt rows")
        nid = nid.astype(np.int64)
        if nam is None:
            nam = np.ones(nid.shape, dtype=bool)
        else:
            nam = to_np(nam)
            if nam.ndim == 1:
                nam = nam[None]
            if nam.shape != nid.shape:
                raise ValueError(f"`negative_prompt_attention_mask` has shape {nam.shape}, `negative_prompt_ids` {nid.shape}")
            nam = nam.astype(bool)
        if nid.shape[1] == 0 or not nam.any(1).all():
            raise ValueError("every row of the negative prompt needs at least one token after masking")
    imgs = guidance.negative_images
    imgs = [] if imgs is None else ([im for im in imgs] if torch.is_tensor(imgs) else list(imgs))
    sizes = guidance.negative_image_sizes
    if sizes is not None and not imgs:
        raise ValueError("negative_image_sizes given without negative_images")
    _check_negative_images("generate()", nid[nam], imgs)
    return nid, nam, imgs, sizes


def parse_prompt_kv(kwargs):
    """prompt_kv_budget / prompt_kv_window / prompt_kv_pool -> None (no budget: the cache holds every prompt position) or (N, w, k):
    N prompt positions kept per sequence, layer and kv head, the last w (default 32, 1 .. KVPRESS_MAX_WINDOW) among them, votes
    max-pooled over k (default 7, odd, 1 .. KVPRESS_MAX_POOL) positions.  ValueError for a bool, a non-int, N <= w, an even or
    out-of-range k, and for a window or pool given without a budget."""
    N, w, k = (kwargs.get(name) for name in _KVPRESS)
    if N is None:
        given = [name for name, v in zip(_KVPRESS[1:], (w, k)) if v is not None]
        if given:
            raise ValueError(f"{given} given without prompt_kv_budget")
        return None
    w, k = 32 if w is None else w, 7 if k is None else k
    for name, v in zip(_KVPRESS, (N, w, k)):
        if not _is_int(v):
            raise ValueError(f"`{name}` has to be an int, but is {v!r}")
    if not 1 <= w <= KVPRESS_MAX_WINDOW:
        raise ValueError(f"`prompt_kv_window` has to lie in [1, {KVPRESS_MAX_WINDOW}], but is {w!r}")
    if not 1 <= k <= KVPRESS_MAX_POOL or k % 2 == 0:
        raise ValueError(f"`prompt_kv_pool` has to be odd and lie in [1, {KVPRESS_MAX_POOL}], but is {k!r}")
    if N <= w:
        raise ValueError(f"`prompt_kv_budget` ({N!r}) has to exceed `prompt_kv_window` ({w!r}): the window is always kept")
    return int(N), int(w), int(k)


def parse_kv_cache_dtype(v):
    """kv_cache_dtype: None or "bf16" (the bf16 cache, returned as "bf16") or "int8" (K|V rows quantised per position, kv head and K / V
    as they enter the cache: LlavaEngine / KVCache); ValueError for anything else."""
    if v is None or v == "bf16":
        return "bf16"
    if v == "int8":
        return "int8"
    raise ValueError(f"`kv_cache_dtype` has to be None, 'bf16' or 'int8', but is {v!r}")


def _parse_lookup(kwargs):
    """prompt_lookup_num_tokens (an int in 1 .. 31) and max_matching_ngram_size (an int >= 1, HF's default 2); None when unset."""
    k = kwargs.get("prompt_lookup_num_tokens")
    if k is None:
        return None
    if not _is_int(k) or not 1 <= k <= LOOKUP_MAX_TOKENS:
        raise ValueError(f"`prompt_lookup_num_tokens` has to be an integer in [1, {LOOKUP_MAX_TOKENS}], but is {k!r}")
    ng = kwargs.get("max_matching_ngram_size")
    ng = 2 if ng is None else ng
    if not _is_int(ng) or ng < 1:
        raise ValueError(f"`max_matching_ngram_size` has to be a strictly positive integer, but is {ng!r}")
    return SimpleNamespace(k=int(k), max_ngram=int(ng))


def _parse_assistant(kwargs):
    """assistant_model (a model of this project's classes: it has an .engine) and num_assistant_tokens (an int in 1 .. 31, default
    ASSIST_DEFAULT_TOKENS, constant over the call); None when no assistant is given.  ValueError for a bad k, for k without a model
    and for an object without an engine."""
    m, k = kwargs.get("assistant_model"), kwargs.get("num_assistant_tokens")
    if m is None:
        if k is not None:
            raise ValueError("`num_assistant_tokens` given without `assistant_model`")
        return None
    if getattr(m, "engine", None) is None:
        raise ValueError(f"`assistant_model` has to be a model of this package (LlavaLlamaForCausalLM or LlavaQwenForCausalLM), not "
                         f"{type(m).__name__}")
    k = ASSIST_DEFAULT_TOKENS if k is None else k
    if not _is_int(k) or not 1 <= k <= LOOKUP_MAX_TOKENS:
        raise ValueError(f"`num_assistant_tokens` has to be an integer in [1, {LOOKUP_MAX_TOKENS}], but is {k!r}")
    return SimpleNamespace(model=m, k=int(k))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


SEED_LIMIT = 1 << 63          # seeds are uint64 on the device; below 2^63 they also fit the int64 tensor that carries them


def _parse_sampling(kwargs):
    """The sampling settings (do_sample=True with seed=), validated as HF's warper constructors do; None for greedy decoding.  Defaults
    are HF's GenerationConfig: temperature 1.0, top_k 50, top_p 1.0, min_p None; top_k None or 0 is off; min_tokens_to_keep is 1."""
    seed = kwargs.get("seed")
    if not kwargs.get("do_sample"):
        if seed is not None:
            raise ValueError("seed= is given but do_sample is not True: a seed only has a meaning for sampling")
        return None
    for k in ("typical_p", "epsilon_cutoff", "eta_cutoff"):
        v = kwargs.get(k)
        if v is not None and v != (1.0 if k == "typical_p" else 0.0):
            raise NotImplementedError(f"{k}: typical / epsilon / eta sampling is not implemented")
    T = kwargs.get("temperature")
    T = 1.0 if T is None else T
    # the kernel takes it as fp32: a value that rounds to 0 or inf there is as bad as 0 or inf
    T32 = None
    if not isinstance(T, bool) and isinstance(T, (int, float, np.floating, np.integer)):
        with np.errstate(all="ignore"):
            T32 = np.float32(min(max(T, -1), 1e39))                      # an int beyond the floats is inf like any other
    if T32 is None or not T32 > 0 or not np.isfinite(T32):
        raise ValueError(f"`temperature` (={T!r}) has to be a strictly positive float")
    k = kwargs.get("top_k", 50)
    k = 0 if k is None else k
    if not _is_int(k) or k < 0:
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {k!r}")
    vals = {}
    for name, default in (("top_p", 1.0), ("min_p", 0.0)):
        v = kwargs.get(name)
        v = default if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 0 <= v <= 1.0:
            raise ValueError(f"`{name}` has to be a float in the [0, 1] interval, but is {v!r}")
        vals[name] = float(v)
    if _is_int(seed):
        seeds = int(seed)
    else:
        if isinstance(seed, (str, bytes)) or not hasattr(seed, "__iter__"):
            raise ValueError(f"`seed` has to be an int or a list with one int per row, but is {seed!r}")
        seeds = list(seed.tolist() if hasattr(seed, "tolist") else seed)
        if any(not _is_int(v) for v in seeds):
            raise ValueError(f"`seed` has to be an int or a list with one int per row, but is {seed!r}")
        seeds = [int(v) for v in seeds]
    if any(not 0 <= v < SEED_LIMIT for v in ([seeds] if isinstance(seeds, int) else seeds)):
        raise ValueError(f"every seed has to be in [0, 2^63), but `seed` is {seed!r}")
    return SimpleNamespace(temperature=float(T), top_k=int(k), top_p=vals["top_p"], min_p=vals["min_p"], seed=seeds)


def sampling_seeds(sampling, n):
    """The seed of each of n rows (generate) or requests (generate_batch): an int s gives row i the seed s + i, a list gives its entries.
    ValueError for a list of another length."""
    s = sampling.seed
    if isinstance(s, int):
        seeds = [s + i for i in range(n)]
    else:
        if len(s) != n:
            raise ValueError(f"`seed` holds {len(s)} seeds for {n} rows")
        seeds = list(s)
    if any(not 0 <= v < SEED_LIMIT for v in seeds):
        raise ValueError("every row's seed has to be in [0, 2^63)")
    return seeds


def sample_uniform(seed, t, tag=0):
    """The uniform of row seed `seed` at its step t (the tokens it has generated so far), in (0, 1):
    ((portable_rng._stream(seed, tag, t + 1)[t] >> 40) + 0.5) * 2^-24, an odd multiple of 2^-25 (exact in float64; rv_sample_rows_f32
    restates it on the device and keeps it as an integer).  tag: the stream -- 0 the sampler's and speculative sampling's resample /
    bonus draw, 1 its accept tests, 2 the draft model's own draws (rv_sample_uniform24_tagged)."""
    from .portable_rng import _splitmix64
    with np.errstate(over="ignore"):
        base = _splitmix64(np.array([(int(seed) * 1000003 + int(tag)) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))
        v = _splitmix64(np.array([int(t)], dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + base)[0]
    return (float(int(v) >> 40) + 0.5) * 2.0 ** -24


def _check_sampled(tok, rows=None):
    """rv_sample_rows_f32 marks a row it cannot sample with -1 (as torch.multinomial raises in HF)."""
    bad = [int(r) for r in (range(len(tok)) if rows is None else rows) if tok[r] < 0]
    if bad:
        raise ValueError(f"sampling: the scores of rows {bad} hold a NaN or +inf, or no finite entry (probability tensor contains "
                         f"either `inf`, `nan` or element < 0)")


def _token_list(name, v):
    if v is None:
        return None
    try:
        ids = list(v)
    except TypeError:
        raise ValueError(f"`{name}` has to be a list of token ids, but is {v!r}") from None
    if any(not _is_int(i) for i in ids):
        raise ValueError(f"`{name}` has to be a list of token ids, but is {v!r}")
    return [int(i) for i in ids]


def _parse_processors(kwargs, eos):
    """The greedy logits-processor settings, validated as HF's processor constructors do (ValueError for a bad value).  Off: None, a
    repetition_penalty of 1.0, a no_repeat_ngram_size of 0."""
    p = kwargs.get("repetition_penalty")
    if p is not None and p != 1.0:
        if not isinstance(p, float) or not p > 0:
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {p!r}")
    p = None if p is None or p == 1.0 else float(p)
    ng = kwargs.get("no_repeat_ngram_size")
    if ng is not None and (not _is_int(ng) or ng < 0):
        raise ValueError(f"`no_repeat_ngram_size` has to be a non-negative integer, but is {ng!r}")
    bw = kwargs.get("bad_words_ids")
    if bw is not None:
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw!r}")
        if any(not isinstance(w, list) for w in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw!r}")
        if any(len(w) == 0 or any(not _is_int(i) or i < 0 for i in w) for w in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of non-negative integers, but is {bw!r}")
        # HF: NoBadWordsLogitsProcessor drops the sequences [eos]; the rest become the keys of a dict (duplicates merge)
        bw = list(dict.fromkeys(tuple(int(i) for i in w) for w in bw if not any(list(w) == [e] for e in eos)))
        if not bw:
            raise ValueError("`bad_words_ids` holds only EOS sequences: nothing is left to ban")
    vals = {}
    for k in ("min_length", "min_new_tokens"):
        v = kwargs.get(k)
        if v is not None and (not _is_int(v) or v < 0):
            raise ValueError(f"`{k}` has to be a non-negative integer, but is {v!r}")
        vals[k] = None if v is None else int(v)
    return dict(repetition_penalty=p, no_repeat_ngram_size=int(ng or 0), bad_words_ids=bw, min_length=vals["min_length"],
                min_new_tokens=vals["min_new_tokens"], suppress_tokens=_token_list("suppress_tokens", kwargs.get("suppress_tokens")),
                begin_suppress_tokens=_token_list("begin_suppress_tokens", kwargs.get("begin_suppress_tokens")))


def min_new_length(cfg, prompt_len):
    """Tokens before which EOS is banned.  HF for inputs_embeds generation: min_new_tokens wins; else min_length counts the prompt
    embeddings (min_length <- max(min_length - inputs_embeds.shape[1], 0)).  0 without an EOS id (HF then adds neither processor)."""
    if not cfg.eos:
        return 0
    if cfg.min_new_tokens is not None:
        return cfg.min_new_tokens
    return max((cfg.min_length or 0) - int(prompt_len), 0)


def min_needs_prompt_len(cfg):
    return bool(cfg.eos) and cfg.min_new_tokens is None and bool(cfg.min_length)


class LogitsProcessors:
    """The active processors of one generate() call on a vocabulary of `vocab` ids.  `active` is False when none of them can change a
    score; greedy_generate then keeps the plain argmax.  The ids banned on every row of step t (suppress_tokens, begin_suppress_tokens
    at t == 0, EOS while t < min_new, one-token bad words) are composed here; they change only at t == 0 and at t == min_new."""

    def __init__(self, cfg, vocab, prompt_len=0):
        self.vocab = int(vocab)
        self.penalty = cfg.repetition_penalty if cfg.repetition_penalty is not None else 1.0
        self.ngram = cfg.no_repeat_ngram_size
        bw = cfg.bad_words_ids or []
        bad_ids = sorted({i for w in bw for i in w if i >= self.vocab})
        if bad_ids:
            raise ValueError(f"The model vocabulary size is {self.vocab}, but the following tokens were being biased: {bad_ids}")
        inv = lambda ids: [i for i in (ids or []) if 0 <= i < self.vocab]           # HF: torch.isin over arange(vocab)
        self.suppress = inv(cfg.suppress_tokens)
        self.begin = inv(cfg.begin_suppress_tokens)
        self.eos = inv(cfg.eos)
        self.one = [w[0] for w in bw if len(w) == 1]
        self.multi = [w for w in bw if len(w) > 1]
        self.min_new = min_new_length(cfg, prompt_len)
        self.active = (self.penalty != 1.0 or self.ngram > 0 or bool(bw) or bool(self.suppress) or bool(self.begin) or
                       (self.min_new > 0 and bool(self.eos)))
        self._dev = {}

    def static_ban(self, t):
        """Sorted distinct ids banned on every row at step t (t = tokens generated so far)."""
        ids = set(self.suppress) | set(self.one)
        if t == 0:
            ids |= set(self.begin)
        if t < self.min_new:
            ids |= set(self.eos)
        return sorted(ids)

    def bad_csr(self):
        """(tokens, offsets) of the multi-token bad words, int32 numpy."""
        off = np.cumsum([0] + [len(w) for w in self.multi]).astype(np.int32)
        tok = np.array([i for w in self.multi for i in w], dtype=np.int32)
        return tok, off

    def device_args(self, t, device):
        """(ban, bad_tok, bad_off) device int32 tensors for step t (None where empty); uploaded once per distinct list."""
        key = (t == 0, t < self.min_new)
        if key not in self._dev:
            ban = self.static_ban(t)
            if "bad" not in self._dev:
                tok, off = self.bad_csr()
                self._dev["bad"] = ((torch.from_numpy(tok).to(device), torch.from_numpy(off).to(device)) if self.multi else (None, None))
            self._dev[key] = torch.tensor(ban, dtype=torch.int32, device=device) if ban else None
        return (self._dev[key],) + self._dev["bad"]

    def rows_device_args(self, device):
        """(ban_always, ban_begin, ban_eos, bad_tok, bad_off) device int32 tensors of the per-row kernel (None where empty), which
        composes a row's bans from the row's own step; uploaded by every call."""
        i32 = lambda ids: torch.tensor(ids, dtype=torch.int32, device=device) if ids else None
        bans = (i32(sorted(set(self.suppress) | set(self.one))), i32(sorted(set(self.begin))), i32(sorted(set(self.eos))))
        tok, off = self.bad_csr()
        return bans + ((torch.from_numpy(tok).to(device), torch.from_numpy(off).to(device)) if self.multi else (None, None))


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


# ------------------------------------------------------------------------------------------------ reuse of a conversation's KV cache
NEWLINE_RECORD = -1           # record of an image_newline row (the same learned vector whatever the image)
_LOCAL_BITS = 24              # image row records: -(2 + (image uid << 24) + row index within the image's merged rows)


def position_records(plan, image_uids):
    """What every spliced position of a plan holds, one int64 array per sequence (its valid positions 0 .. len_b - 1, whatever the padding
    side): a token id (>= 0); NEWLINE_RECORD; or an image feature row, -(2 + (uid << 24) + k) with uid = image_uids[i] of the image the row
    comes from (equal uids: bit-identical pixels and image_size) and k its row in that image's feature rows (projector rows, then the
    rows anyres_max creates), which the splice plan fixes (plan["idx"], plan["image_rows"]).  Equal records at positions 0 .. p on the same
    weights give the same K|V at p."""
    B = plan["attention_mask"].shape[0]
    idx = plan["idx"].reshape(B, -1).astype(np.int64)
    am = plan["attention_mask"].astype(bool)
    nfr = int(plan["n_feat_rows"])
    code = np.zeros(nfr + 1, dtype=np.int64)
    code[nfr] = NEWLINE_RECORD
    for i, (p0, p1, e0, e1) in enumerate(plan.get("image_rows", [])):
        base = 2 + (int(image_uids[i]) << _LOCAL_BITS)
        code[p0:p1] = -(base + np.arange(p1 - p0))
        code[e0:e1] = -(base + (p1 - p0) + np.arange(e1 - e0))
    out = []
    for b in range(B):
        v = idx[b][am[b]]
        out.append(np.where(v >= 0, v, code[np.clip(-v - 2, 0, nfr)]))
    return out


def reuse_lengths(cached, new):
    """Positions of each sequence whose cached K|V a continued call keeps: the longest common prefix of the cached records and the new
    ones, capped at len_b - 1 (the last prompt position is always recomputed: its logits start the decoding).  int64 [B]."""
    r = np.zeros(len(new), dtype=np.int64)
    for b, (c, n) in enumerate(zip(cached, new)):
        k = min(len(c), len(n))
        neq = np.nonzero(np.asarray(c[:k]) != np.asarray(n[:k]))[0]
        r[b] = min(int(neq[0]) if neq.size else k, max(len(n) - 1, 0))
    return r


def grown_length(L_max, need):
    """Slots per sequence of a cache that must hold `need` positions: L_max when they fit, else need rounded up to 256."""
    return int(L_max) if need <= L_max else (int(need) + 255) // 256 * 256


def _same_pixels(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a = a.detach().contiguous().view(torch.uint8).reshape(-1)
    b = b.detach().to(a.device).contiguous().view(torch.uint8).reshape(-1)
    return bool(torch.equal(a, b))


class GenerationCache:
    """A conversation's KV cache across generate() calls, HF's `past_key_values` idiom: create an empty one (GenerationCache(), as HF's
    DynamicCache()), pass it to each call with the FULL prompt and images, and every call reuses the positions it already holds -- the
    longest common prefix of what each cached position holds (a token id, or an image feature row identified by the image's bits, its
    image_size and the row's index) and the new spliced prompt, at most len_b - 1 -- and recomputes only the rest (LlavaEngine.extend).
    It holds the engine's KVCache (bf16 [B, L_max, 2 * kvd] per layer, sequence b at positions 0 .. n_b - 1), the per-position records,
    the images they refer to and the engine and weights version they were computed with: a cache of older weights (an optimizer step,
    load_state_dict, a LoRA merge, a vocabulary resize, a checkpoint load since) is emptied and the call runs as a fresh one."""

    def __init__(self):
        self.kv = None
        self.records = None
        self.images = []              # (uid, pixels, image_size) of the images the records refer to
        self.engine = None
        self.weights_version = None
        self._next_uid = 0

    @property
    def batch_size(self):
        return None if self.kv is None else self.kv.B

    def get_seq_length(self, layer_idx=0):
        """Positions held by the longest cached sequence (0 when empty)."""
        return 0 if self.kv is None else int(self.kv.lens.max())

    def crop(self, max_length):
        """Keep at most max_length positions per sequence (a negative value drops that many from the longest, as HF's crop)."""
        if self.kv is None:
            return
        if max_length < 0:
            max_length = self.get_seq_length() - abs(max_length)
        n = max(int(max_length), 0)
        self.kv.lens = np.minimum(self.kv.lens, n)
        self.records = [r[:n] for r in self.records]

    def reset(self):
        self.kv, self.records, self.images = None, None, []

    def _bind(self, engine, B):
        """Checks before a call: ValueError for another engine or another batch size; a stale cache is emptied."""
        if self.engine is not None and self.engine is not engine:
            raise ValueError("this GenerationCache was filled by another model: use one cache per model")
        if self.kv is not None and self.kv.B != B:
            raise ValueError(f"the GenerationCache holds {self.kv.B} sequences, the prompt has {B}")
        if self.kv is not None and self.weights_version != engine.weights_version:
            self.reset()
        self.engine = engine

    def _image_uids(self, images, image_sizes):
        """uid of each image of a call: the uid of a cached image with the same bits and image_size, else a new one."""
        uids = []
        for i, im in enumerate(images or []):
            size = None if image_sizes is None else tuple(int(v) for v in image_sizes[i])
            hit = next((u for u, px, sz in self.images if sz == size and _same_pixels(px, im)), None)
            if hit is None:
                hit = self._next_uid
                self._next_uid += 1
            uids.append(hit)
        return uids

    def _store(self, kv, records, images, image_sizes, uids, engine):
        self.kv, self.records = kv, records
        held = {u: px for u, px, _ in self.images}            # an image already held is not copied again
        self.images = [(u, held[u] if u in held else im.detach().clone(), None if image_sizes is None else tuple(int(v) for v in image_sizes[i]))
                       for i, (u, im) in enumerate(zip(uids, images or []))]
        self.engine, self.weights_version = engine, engine.weights_version


# ------------------------------------------------------------------------------------------------ prompt-lookup decoding
class PromptLookupDrafter:
    """HF's PromptLookupCandidateGenerator.get_candidates (called with logits_processor=None) on the host: the draft is the continuation
    of an earlier occurrence of the sequence's last n-gram.  n runs from min(max_ngram, len - 1) down to 1; the first (leftmost)
    occurrence with a non-empty continuation wins; the continuation is at most k tokens, ends where the sequence ends and is cut before
    its first EOS id (a match cut to nothing ends the search, as in HF).  It is also cut before the first id outside [0, vocab), which
    is how an image placeholder (a negative id, left in place so that the text after it can still match) never becomes a draft."""

    def __init__(self, k, max_ngram=2, eos=(), vocab=None):
        if not _is_int(k) or k < 1 or not _is_int(max_ngram) or max_ngram < 1:
            raise ValueError("Invalid max_matching_ngram_size or num_output_tokens")
        self.k, self.max_ngram, self.vocab = int(k), int(max_ngram), None if vocab is None else int(vocab)
        self.eos = np.asarray(sorted(int(e) for e in (eos if eos is not None else [])), dtype=np.int64)

    def propose(self, seq):
        """seq: the prompt ids as passed (masked positions removed) followed by the emitted tokens.  Returns the draft, int64 [0 .. k]."""
        seq = np.asarray(seq, dtype=np.int64).reshape(-1)
        n = seq.shape[0]
        for ng in range(min(self.max_ngram, n - 1), 0, -1):
            win = np.lib.stride_tricks.sliding_window_view(seq, ng)
            idx = np.flatnonzero((win[:n - ng] == seq[n - ng:]).all(1))          # windows with at least one token after them
            if idx.size == 0:
                continue
            start = int(idx[0]) + ng
            out = seq[start:min(start + self.k, n)]
            if self.eos.size:
                hit = np.flatnonzero(np.isin(out, self.eos))
                if hit.size:
                    out = out[:int(hit[0])]
            return clamp_draft(out, self.k, self.vocab)
        return np.zeros(0, dtype=np.int64)


def clamp_draft(draft, limit, vocab=None):
    """The draft cut to `limit` tokens and before its first id outside [0, vocab) (negative ids when vocab is None): what the accept
    loop applies to any drafter's proposal, so that no token past the budget, no position past the cache's L_max and no id without an
    embedding row is ever fed."""
    d = np.asarray(draft, dtype=np.int64).reshape(-1)[:max(int(limit), 0)]
    bad = np.flatnonzero(d < 0) if vocab is None else np.flatnonzero((d < 0) | (d >= vocab))
    return d[:int(bad[0])].copy() if bad.size else d.copy()


def _lookup_loop(engine, cache, logits, prompt_ids, st, lp, cfg, T, scores, raw, seed=None):
    """The accept loop of prompt-lookup decoding on one sequence, from the prompt pass's logits to the end of generation.  Each round
    holds fp32 logits [R, vocab]: row 0 from feeding the last emitted token, row i from feeding draft i - 1 after it, so row i is the
    plain loop's step t + i provided the drafts before it were right.  The R token choices run in one launch (rv_argmax_rows_f32, or
    rv_logits_process_argmax_rows_f32 with row i at step t + i reading the history `emitted + drafts[:i]`, its begin / EOS bans composed
    per row) and come to the host in one copy; drafts are accepted while draft[i] == choice[i], and the round emits them and the
    choice after them through GreedyState.step, one token at a time with that token's own score row, stopping at the first EOS, at the
    budget or where a criterion says so.  The next round feeds the last emitted token and a new draft: verify_step, or decode_step when
    the draft is empty.  cache.lens advances by the tokens emitted, so it always counts the prompt and every emitted token but the
    last; the K|V rows of rejected drafts stay past it.  Returns dict(steps=, drafted=, accepted=): engine steps after the prompt pass,
    draft tokens fed and draft tokens that matched.
    cfg.sampling (a draft model only; seed: the row's seed): the rows and the loop are the same, the round differs only in how the R
    processed rows become "accepted count, next token".  The seeded sampler warps the R rows in place (row i at step t + i; its own
    draws are not used), ops.spec_accept_rows tests draft i against the drafter's warped row i (cfg.drafter.q_rows) and draws the token
    after the accepted ones, and (accepted, token) come to the host in one copy.  scores then holds the target's warped rows."""
    from . import ops
    dev, V, sm = engine.device, engine.vocab, cfg.sampling
    stats = dict(steps=0, drafted=0, accepted=0)
    seq = [int(v) for v in prompt_ids]
    hist = None
    if lp.active:
        hist = torch.zeros(1, T, dtype=torch.int32, device=dev)
        bans = lp.rows_device_args(dev)
    if sm is not None:
        seed1 = torch.tensor([seed], dtype=torch.int64, device=dev)
        seedR = seed1.expand(ops.SPEC_MAX_R).contiguous()
        sws, aws = ops.sample_rows_workspace(ops.SPEC_MAX_R, dev), ops.spec_accept_workspace(1, ops.SPEC_MAX_R, dev)
    draft = np.zeros(0, dtype=np.int64)
    t, fed = 0, False                      # fed: the round's rows come from a step that wrote K|V rows (every round but the first)
    while True:
        R = 1 + draft.shape[0]
        if cfg.output_logits:
            raw_rows = logits.clone()
        if lp.active:
            # one upload: slot, step and EOS minimum of every row, then the drafts
            info = engine._dev(np.stack([np.zeros(R), t + np.arange(R), np.full(R, lp.min_new), np.append(draft, 0)]).astype(np.int32))
            if R > 1:                      # the drafts go behind the emitted tokens: row i reads hist[0, :t + i]
                hist[0, t:t + R - 1] = info[3, :R - 1]
            nxt = ops.logits_process_argmax_rows(logits, V, hist, info[0], info[1], info[2], lp.penalty, lp.ngram, *bans)
            if sm is None:
                hist[0, t:t + R] = nxt     # the choices: the drafts while they are accepted, then the token after them
        elif sm is None:
            nxt = ops.argmax_rows(logits, V)
        if sm is not None:
            # one upload: the rows' steps, then the drafts
            si = engine._dev(np.concatenate([t + np.arange(R), draft]).astype(np.int32))
            # the sampler is run for its warp only (write_scores): its R draws are deliberately unused, the tokens come from the
            # accept kernel below
            ops.sample_rows(logits, V, seedR[:R], si[:R], sm.temperature, sm.top_k, sm.top_p, sm.min_p, write_scores=True, ws=sws)
            n_acc, tok, _ = ops.spec_accept_rows(logits, cfg.drafter.q_rows[:R - 1] if R > 1 else None, si[R:], seed1, si[:1], V, ws=aws)
            if lp.active:                  # the token after the accepted drafts goes behind them
                hist[0].scatter_(0, n_acc.long() + t, tok.int())
            a, token = (int(v) for v in torch.stack([n_acc.long(), tok]).cpu().reshape(-1))
            _check_sampled([token])
            choice = np.append(draft[:a], token)
        if cfg.output_scores:
            score_rows = logits.clone()
        if sm is None:
            choice = np.asarray(nxt.cpu() if torch.is_tensor(nxt) else nxt, dtype=np.int64).reshape(-1)
            a = 0
            while a < R - 1 and draft[a] == choice[a]:
                a += 1
        stats["drafted"] += R - 1
        stats["accepted"] += a
        n_emit = 0
        for i in range(a + 1):
            if cfg.output_logits:
                raw.append(raw_rows[i:i + 1])
            if cfg.output_scores:
                scores.append(score_rows[i:i + 1])
            st.step(choice[i:i + 1], logits[i:i + 1], device=dev)
            seq.append(int(choice[i]))
            n_emit += 1
            t += 1
            if st.all_done or t == T:
                break
        if fed:
            cache.lens += n_emit
        if st.all_done or t == T:
            return stats
        room = min(T - t - 1, cache.L_max - int(cache.lens[0]) - 1)
        draft = clamp_draft(cfg.drafter.propose(np.asarray(seq, dtype=np.int64)), room, V) if room > 0 else np.zeros(0, dtype=np.int64)
        if draft.shape[0]:
            logits = engine.verify_step(cache, np.concatenate([[seq[-1]], draft]))
        else:
            logits = engine.decode_step(cache, np.asarray([seq[-1]]))
            cache.lens -= 1                # decode_step counts the token it was fed; this loop counts it once the round has emitted
        stats["steps"] += 1
        fed = True


def _uniform_choice(engine, cfg, lp, B, T, seeds, keep_history):
    """The token choice of a call whose rows are all at the same step, set up once per call: the processors and their argmax
    (ops.logits_process_argmax over `hist`, the tokens generated so far with the pads of finished rows, HF's input_ids of inputs_embeds
    generation: no prompt), the plain argmax, or the processors and then the seeded sampler (row b with seeds[b] at step t; the warped
    scores are written back only when output_scores or a stopping criterion reads them).  Returns (choose, hist): choose(logits, t)
    processes logits in place and returns the ids, a device tensor from an argmax and a host array from the sampler (-1: a row it could
    not sample); the caller writes each step's emitted tokens into hist (None when no processor is active)."""
    from . import ops
    dev, V, sm = engine.device, engine.vocab, cfg.sampling
    if sm is not None:
        seed = torch.tensor(seeds, dtype=torch.int64, device=dev)
        steps = torch.arange(T, dtype=torch.int32, device=dev)[:, None].expand(T, B).contiguous()     # row t: every row at step t
        write = cfg.output_scores or bool(cfg.stopping_criteria)
    hist = torch.zeros(B, T, dtype=torch.int32, device=dev) if lp.active and keep_history else None
    ws = ops.sample_rows_workspace(B, dev) if sm is not None else None      # the sampler's scratch, once per call

    def choose(logits, t):
        if lp.active:                     # in place: logits become HF's processed scores
            nxt = ops.logits_process_argmax(logits, V, hist, t, lp.penalty, lp.ngram, *lp.device_args(t, dev))
        elif sm is None:
            nxt = ops.argmax_rows(logits, V)
        if sm is not None:                # in place when someone reads them: the processed scores become HF's warped scores
            nxt = ops.sample_rows(logits, V, seed, steps[t], sm.temperature, sm.top_k, sm.top_p, sm.min_p, write_scores=write, ws=ws)
            nxt = nxt.cpu().numpy()
        return nxt
    return choose, hist


def greedy_generate(engine, input_ids, attention_mask, images, image_sizes, cfg):
    """One prompt pass, then decode_step per token until every row has finished or the budget is spent: the prompt pass, one loop and
    one output builder.  The prompt pass is a prefill; with cfg.past_key_values (a GenerationCache) it reuses what the cache holds
    (LlavaEngine.extend; an empty cache: prefill as without one) and the cache keeps the prompt and every generated token but the
    last; with cfg.guidance it is two prefills into one KVCache of 2 * B rows (below).  Each step of the loop: output_logits clones the
    raw rows; guidance, DoLa or the constraint transform them in place; _uniform_choice picks the tokens (the processors, then the
    argmax or the seeded sampler of cfg.sampling); output_scores and the stopping criteria get the rows as the choice left them;
    GreedyState.step books the tokens and they are fed to decode_step.  The keywords of prefill and decode_step are built once, and a
    keyword is passed only when its feature is on.  cfg.kv_cache_dtype "int8": the cache holds int8 K|V rows with one fp32 scale per
    (position, kv head, K / V) group; the first token comes from the unquantised prompt pass, every later one reads the quantised rows.
    cfg.guidance (classifier-free guidance): rows 0 .. B - 1 of the cache are prefilled with the prompts and rows B .. 2B - 1 with
    the negative prompts (resolve_negative_prompts), L_max = the longer spliced length + the budget.  Every decode step runs all
    2 * B rows and feeds the emitted token (the pad of a finished row) to both halves, which is what HF's processor does with
    input_ids[:, -1:].  ops.cfg_guide_rows turns (conditional, unconditional) into the guided rows in place (CFG is HF's first
    processor); output_logits holds the raw conditional rows.  min_length / max_length count the conditional prompt.
    cfg.dola (DoLa): the spec is resolved against the engine's depth once; prefill and every decode_step are asked for the candidate
    layers' logits (tap_layers=) and ops.dola_contrast_rows turns each step's raw rows into the contrasted rows in place.  The dict
    output then carries dola_premature_layers, int64 [B, steps]: the layer each row chose, -1 at steps after the row has finished.
    cfg.constraint (constrained decoding): the rows' automata become one table and one int32 state per row on the device
    (constraints.resolve_constraints), every call starting at the start states.  ops.constrain_rows advances every live state by the
    token the row emitted last (the device copy of the tokens that decode_step is fed) and writes -inf on what the new state does
    not allow, so output_scores, the stopping criteria and the sampler see the masked rows.  A row that took an EOS edge is free and
    no longer touched; a row finished by a stopping criterion is fed pads, which may kill its state, and its rows mean nothing
    then as before.  ConstraintMirror follows the states on the host and raises RuntimeError at the step of a dead end."""
    from . import ops
    ids = np.asarray(input_ids.cpu() if torch.is_tensor(input_ids) else input_ids)
    if ids.ndim == 1:
        ids = ids[None]
    am = cfg.attention_mask
    am = None if am is None else np.asarray(am.cpu() if torch.is_tensor(am) else am)
    B, dev, V = ids.shape[0], engine.device, engine.vocab
    gc, gd, att = cfg.past_key_values, getattr(cfg, "guidance", None), getattr(cfg, "attentions", None)
    refuse_combinations(features_of(cfg, lora=att is not None and engine.lora), "generate()")          # protects a cfg built by hand
    if gc is not None:
        gc._bind(engine, B)
    assist = getattr(cfg, "assistant", None)
    lookup = getattr(cfg, "lookup", None) is not None or getattr(cfg, "drafter", None) is not None or assist is not None
    if lookup and B != 1:
        raise ValueError(f"{'prompt_lookup_num_tokens' if assist is None else 'assistant_model'} takes one prompt row (HF's assisted "
                         f"generation is batch-size-1 too), got {B}")
    if assist is not None and cfg.drafter is None:
        from .assist import check_assistant
        check_assistant(engine, assist.model.engine)
    lookup_stats = dict(steps=0, drafted=0, accepted=0)
    st = GreedyState(B, cfg)
    scores, raw, picks, attns = [], [], [], []
    step_kw = {}                          # the keywords of decode_step, and of prefill with prompt_kw: only those of a feature that is on
    dola = getattr(cfg, "dola", None)
    if dola is not None:
        dola = resolve_dola_layers(dola, engine.l["layers"])
        step_kw["tap_layers"] = dola
    ctab = None
    if getattr(cfg, "constraint", None) is not None:
        from .constraints import resolve_constraints
        ctab, cstart = resolve_constraints(cfg.constraint, B, V)
    if att is not None:
        att_layers = resolve_attention_layers(att.layers, engine.l["layers"])
        step_kw.update(attn_layers=att_layers, attn_mean=att.reduce == "mean_heads")
    kvd = getattr(cfg, "kv_cache_dtype", "bf16")
    kv_args = () if kvd == "bf16" else (kvd,)                 # the default dtype keeps the two-argument calls
    prompt_kw = dict(step_kw)
    if kvd != "bf16":
        prompt_kw["kv_dtype"] = kvd
    if getattr(cfg, "kvpress", None) is not None:
        prompt_kw["compress"] = cfg.kvpress
    imgs = list(images) if images is not None else []
    # prompt length in HF's sense: the spliced inputs_embeds width (the longest spliced prompt of the batch)
    plan_len = 0
    if gd is not None:
        nids, nam, nimgs, nsizes = resolve_negative_prompts(gd, ids, am)
        plan, nplan = engine.plan(ids, am, None, imgs, image_sizes), engine.plan(nids, nam, None, nimgs, nsizes)
        plan_len = int(plan["S"])
    elif (cfg.max_new_tokens is None and cfg.max_length is not None) or min_needs_prompt_len(cfg):
        plan_len = int(engine.plan(ids, am, None, imgs, image_sizes)["S"])
    T = new_token_budget(cfg, plan_len)
    lp = LogitsProcessors(cfg, V, plan_len)
    sm = cfg.sampling
    seeds = None if sm is None else sampling_seeds(sm, B)
    if T > 0:
        # ---------------------------------------------------------------------------------------- the prompt pass
        if gd is not None:
            L_max = max(int(plan["lens"].max()), int(nplan["lens"].max())) + T
            need, free = engine.kv_cache_bytes(2 * B, L_max, *kv_args), engine.free_device_bytes()
            if free is not None and need > free:
                raise ValueError(f"guided generate(): the KV cache of 2 x {B} rows x {L_max} positions needs {need} bytes, but only {free} "
                                 f"bytes of device memory are free: lower the batch or the token budget")
            cache = engine.new_kv_cache(2 * B, L_max, *kv_args)
            _, logits = engine.prefill(ids, am, images, image_sizes, cache=cache, slots=np.arange(B))
            _, uncond = engine.prefill(nids, nam, nimgs or None, nsizes, cache=cache, slots=B + np.arange(B))
            choose, hist = _uniform_choice(engine, cfg, lp, B, T, seeds, True)
            gws = ops.cfg_guide_workspace(B, dev)
        else:
            choose, hist = _uniform_choice(engine, cfg, lp, B, T, seeds, not lookup)       # the accept loop keeps its own history
            if gc is None:
                cache, logits, *extra = engine.prefill(ids, am, images, image_sizes, max_new_tokens=T, **prompt_kw)
            else:
                plan = engine.plan(ids, am, None, imgs, image_sizes)
                uids = gc._image_uids(imgs, image_sizes)
                recs = position_records(plan, uids)
                reuse = np.zeros(B, dtype=np.int64) if gc.kv is None else reuse_lengths(gc.records, recs)
                kv, gc.kv, gc.records = gc.kv, None, None         # an unused cache is freed before prefill allocates the new one
                if not reuse.any():
                    kv = None
                cache, logits = engine.extend(kv, ids, am, images, image_sizes, reuse=reuse, max_new_tokens=T, plan=plan)
                del kv
            if dola is not None:
                dws = ops.dola_workspace(B, len(dola), dev)
        if lookup:                        # the accept loop runs the whole generation
            prompt_ids = ids[0] if am is None else ids[0][np.asarray(am).reshape(B, -1)[0].astype(bool)]
            if cfg.drafter is None and assist is not None:
                from .assist import ModelDrafter
                cfg.drafter = ModelDrafter(assist.model.engine, assist.k, cfg, T, len(prompt_ids), plan_len, None if sm is None else seeds[0])
                cfg.drafter.start(ids, am, images, image_sizes)
            elif cfg.drafter is None:
                cfg.drafter = PromptLookupDrafter(cfg.lookup.k, cfg.lookup.max_ngram, cfg.eos, V)
            lookup_stats = _lookup_loop(engine, cache, logits, prompt_ids, st, lp, cfg, T, scores, raw, None if sm is None else seeds[0])
        if ctab is not None:              # every call starts at the start states, a continued conversation too
            ctabs, cstate, ctok = ctab.device_tables(dev), engine._dev(cstart), None
            mirror = ConstraintMirror(ctab, B)
            mirror.state[:] = cstart
        # ---------------------------------------------------------------------------------------- the loop
        for t in range(0 if lookup else T):
            if cfg.output_logits:
                raw.append(logits.clone())
            if att is not None:           # the maps of the step that gave these logits: HF's [B, H, 1, L_t]
                attns.append(tuple(a[:, None, None, :] if a.dim() == 2 else a[:, :, None, :] for a in extra[0]))
            # the transforms, in place: the raw rows become the guided rows, the contrasted rows, the rows the automaton allows
            if gd is not None:
                ops.cfg_guide_rows(logits, uncond, V, gd.scale, ws=gws)
            if dola is not None:
                picks.append((ops.dola_contrast_rows(logits, extra[0], V, ws=dws)[1], st.unfinished.copy()))
            if ctab is not None:          # each live row's state takes the row's last token first
                ops.constrain_rows(logits, V, cstate, ctabs, tok=ctok)
            nxt = choose(logits, t)
            if sm is not None:
                if ctab is not None:      # the sampler's -1 on a constrained row is a dead end, named as one
                    bad = np.flatnonzero(st.unfinished & (nxt < 0))
                    mirror.take(bad, nxt[bad], None, lambda k: f"row {bad[k]}", t)
                _check_sampled(nxt, np.flatnonzero(st.unfinished))
            if cfg.output_scores:
                scores.append(logits.clone())
            was = st.unfinished.copy() if ctab is not None else None
            tok = st.step(nxt, logits, device=dev)
            if hist is not None:
                hist[:, t] = torch.from_numpy(tok.astype(np.int32)).to(dev)
            if ctab is not None:
                was = np.flatnonzero(was)
                mirror.take(was, tok[was], lambda k: lp.active and bool(torch.isneginf(logits[was[k], 0])), lambda k: f"row {was[k]}", t)
            if st.all_done or t == T - 1:
                break
            if ctab is not None:          # one upload serves the next step's advance and the decode step
                feed = ctok = engine._dev(tok)
            else:                         # a guided step feeds the token to both halves
                feed = torch.from_numpy(tok if gd is None else np.concatenate([tok, tok]))
            out = engine.decode_step(cache, feed, **step_kw)
            logits, *extra = out if step_kw else (out,)
            if gd is not None:
                logits, uncond = logits[:B], logits[B:]
        if gc is not None:          # the prompt and the tokens fed to decode_step (every emitted one but the last; pads of finished rows)
            fed = st.sequences()[:, :int(cache.lens[0] - plan["lens"][0])]
            gc._store(cache, [np.concatenate([recs[b], fed[b]]) for b in range(B)], imgs, image_sizes, uids, engine)
        del cache
    # -------------------------------------------------------------------------------------------- the output
    seq = torch.from_numpy(st.sequences()).to(dev)
    if not cfg.return_dict:
        return seq
    out = GenerateDecoderOnlyOutput(sequences=seq, scores=tuple(scores) if cfg.output_scores else None,
                                    logits=tuple(raw) if cfg.output_logits else None, past_key_values=gc)
    if assist is not None:
        out.assist_stats = lookup_stats
    elif lookup:
        out.lookup_stats = lookup_stats
    if att is not None:
        out.attentions, out.attention_layers = tuple(attns), att_layers
    if dola is not None:
        lay = np.full((B, len(picks)), -1, dtype=np.int64)
        if picks:
            ch = torch.stack([c for c, _ in picks], 1).cpu().numpy()           # one copy: [B, steps] indices into `dola`
            live = np.stack([u for _, u in picks], 1)
            lay[live] = np.asarray(dola, dtype=np.int64)[ch[live]]
        out.dola_premature_layers = torch.from_numpy(lay).to(dev)
    return out


# ------------------------------------------------------------------------------------------------ continuous batching: generate_batch
# Admission threshold in free slots.  Picked from the sweep over 1, 4, 8 and 16 (profiles/decode_bench.jsonl, mode
# generate_batch_sweep; DESIGN.md §5b "Batched generation"): 4 had the shortest wall time for both 7B models on the mixed-budget split.
ADMIT_FREE_SLOTS = 4
_NO_PER_REQUEST = ("attention_mask", "past_key_values", "position_ids", "output_scores", "output_logits", "return_dict_in_generate")


class GenerationOutput(SimpleNamespace):
    """One request's result, with HF 5.x continuous batching's field names: request_id ("req_<i>"), prompt_ids (list[int], as given),
    generated_tokens (list[int]: up to and including the EOS token, or the token after which a stopping criterion returned True; no
    padding), logprobs (list[float], one per generated token with return_logprobs, else empty), error (None), status."""

    def is_finished(self):
        return self.status == "finished"


def parse_batch_kwargs(kwargs, n, lora=False, config_eos=None, config_pad=None):
    """generate_batch() keywords: generate()'s greedy and sampling settings (seed: an int, or a list of n ints), validated by parse_generate_kwargs and applied per request;
    max_new_tokens may also be a list of n budgets (cfg.budgets).  TypeError for arguments without a per-request meaning.
    share_prefix (cfg.share_prefix, default False): a bool, ValueError otherwise; its rows of REFUSALS are checked here.  constraint
    (cfg.constraint): one TokenConstraint for every request or a list of n entries, None for an unconstrained request; ValueError
    for another length."""
    given = sorted(k for k in _NO_PER_REQUEST if kwargs.get(k) is not None and kwargs.get(k) is not False)
    if given:
        raise TypeError(f"generate_batch() got arguments without a per-request meaning: {given}")
    if kwargs.get("negative_prompt_attention_mask") is not None:
        raise TypeError("generate_batch() takes unpadded negative prompts (negative_prompt_ids: a list of 1-D id sequences); "
                        "negative_prompt_attention_mask has no per-request meaning")
    kw = {k: v for k, v in kwargs.items() if k not in _NO_PER_REQUEST}
    share = kw.pop("share_prefix", False)                     # generate_batch() alone takes it: generate() / generate_beams() reject the name
    if not isinstance(share, (bool, np.bool_)):
        raise ValueError(f"share_prefix must be True or False, got {share!r}")
    budgets = None
    mnt = kw.get("max_new_tokens")
    if mnt is not None and not _is_int(mnt):
        if not isinstance(mnt, (list, tuple)):
            raise TypeError(f"max_new_tokens must be an int or a list of {n} ints, not {type(mnt).__name__}")
        if len(mnt) != n:
            raise ValueError(f"max_new_tokens holds {len(mnt)} budgets for {n} requests")
        if any(not _is_int(b) or b < 0 for b in mnt):
            raise ValueError(f"every max_new_tokens budget must be an int >= 0, got {list(mnt)}")
        budgets = [int(b) for b in mnt]
        del kw["max_new_tokens"]
    cfg = parse_generate_kwargs(kw, lora=lora, config_eos=config_eos, config_pad=config_pad)
    cfg.budgets = budgets
    cfg.share_prefix = bool(share)
    refuse_combinations(features_of(cfg), "generate_batch()")
    if cfg.guidance is not None:
        for k in ("negative_prompt_ids", "negative_images", "negative_image_sizes"):
            _per_request(k, getattr(cfg.guidance, k), n)      # a list of another length: ValueError here, before anything runs
    if cfg.sampling is not None:
        sampling_seeds(cfg.sampling, n)                       # a list of another length: ValueError here, before anything runs
    if isinstance(cfg.constraint, list) and len(cfg.constraint) != n:
        raise ValueError(f"`constraint` holds {len(cfg.constraint)} entries for {n} requests")
    return cfg


def _per_request(name, v, n):
    if v is None:
        return [None] * n
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"`{name}` must be None or a list of {n} entries, one per request")
    if len(v) != n:
        raise ValueError(f"`{name}` has {len(v)} entries for {n} requests")
    return list(v)


def _size_list(v):
    if v is None:
        return None
    v = v.tolist() if torch.is_tensor(v) else list(v)
    if v and _is_int(v[0]):
        return [tuple(int(x) for x in v)]                     # one (h, w)
    return [tuple(int(x) for x in s) for s in v]


def batch_requests(inputs, images=None, image_sizes=None, guidance=None):
    """The requests of generate_batch(), normalised: ids (int64 numpy, as given), images (the request's tensors in image-token order)
    and sizes (one (h, w) per image, or None).  ValueError for a list of the wrong length or images that do not match the image tokens.
    guidance (cfg.guidance of a guided call): every request also gets neg_ids (its entry of negative_prompt_ids, a non-empty 1-D id
    sequence; without one, the request's last prompt token, HF's rule), neg_images and neg_sizes (its entries of negative_images /
    negative_image_sizes: required when neg_ids holds image tokens, refused when it holds none)."""
    from .splice import IMAGE_TOKEN_INDEX
    inputs = list(inputs)
    n = len(inputs)
    ims, szs = _per_request("images", images, n), _per_request("image_sizes", image_sizes, n)
    reqs = []
    for i, p in enumerate(inputs):
        ids = np.asarray(p.detach().cpu() if torch.is_tensor(p) else p)
        if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"request {i}: a prompt is a non-empty 1-D sequence of token ids, got shape {ids.shape}, dtype {ids.dtype}")
        im = [] if ims[i] is None else ([ims[i]] if torch.is_tensor(ims[i]) else list(ims[i]))
        sz = _size_list(szs[i])
        k = int((ids == IMAGE_TOKEN_INDEX).sum())
        if k and not im:
            raise ValueError(f"request {i}: the prompt holds an image token but no images were passed")
        if k != len(im):
            raise ValueError(f"request {i}: the prompt holds {k} image tokens but {len(im)} images were passed")
        if sz is not None and len(sz) != len(im):
            raise ValueError(f"request {i}: {len(sz)} image sizes for {len(im)} images")
        reqs.append(SimpleNamespace(index=i, ids=ids.astype(np.int64), images=im, sizes=sz))
    with_img = [r for r in reqs if r.images]
    if any(r.sizes is None for r in with_img) and any(r.sizes is not None for r in with_img):
        raise ValueError("image_sizes: give the sizes of every request's images or of none")
    if guidance is not None:
        nids = _per_request("negative_prompt_ids", guidance.negative_prompt_ids, n)
        nims = _per_request("negative_images", guidance.negative_images, n)
        nszs = _per_request("negative_image_sizes", guidance.negative_image_sizes, n)
        for i, r in enumerate(reqs):
            if nids[i] is None:
                neg = r.ids[-1:]
            else:
                neg = np.asarray(nids[i].detach().cpu() if torch.is_tensor(nids[i]) else nids[i])
                if neg.ndim != 1 or neg.size == 0 or not np.issubdtype(neg.dtype, np.integer):
                    raise ValueError(f"request {i}: a negative prompt is a non-empty 1-D sequence of token ids, got shape {neg.shape}, "
                                     f"dtype {neg.dtype}")
            im = [] if nims[i] is None else ([nims[i]] if torch.is_tensor(nims[i]) else list(nims[i]))
            sz = _size_list(nszs[i])
            _check_negative_images(f"request {i}", neg, im)
            if sz is not None and len(sz) != len(im):
                raise ValueError(f"request {i}: {len(sz)} negative image sizes for {len(im)} negative images")
            r.neg_ids, r.neg_images, r.neg_sizes = neg.astype(np.int64), im, sz
        with_img = [r for r in reqs if r.neg_images]
        if any(r.neg_sizes is None for r in with_img) and any(r.neg_sizes is not None for r in with_img):
            raise ValueError("negative_image_sizes: give the sizes of every request's negative images or of none")
    return reqs


# ------------------------------------------------------------------------------------------------ shared prompt prefixes
SHARE_MIN_PREFIX = 128        # = KVCache.chunk: below one decode chunk neither the prompt pass nor the decode kernel gains anything
SHARED_TILE_COLS = 16         # columns of the tile table (rv_attn_decode_shared_bf16 reads 16 // G of them)


def common_prefix(a, b):
    """Length of the longest common prefix of two record arrays."""
    k = min(len(a), len(b))
    neq = np.nonzero(np.asarray(a[:k]) != np.asarray(b[:k]))[0]
    return int(neq[0]) if neq.size else k


def best_source(records, sources):
    """The source of a request among `sources`, (slot, records) pairs: P = the longest common prefix of records, capped at
    len(records) - 1 (the last prompt position is always computed: its logits start the decoding) and, being a common prefix, at the
    source's prompt length; the longest P wins, ties go to the lowest slot.  Returns (slot, P), or (-1, 0) when P < SHARE_MIN_PREFIX
    for every source: the request is then a leader."""
    best, bp = -1, 0
    for slot, rec in sorted(sources, key=lambda e: e[0]):
        p = min(common_prefix(records, rec), len(records) - 1)
        if p > bp:
            best, bp = int(slot), p
    return (best, bp) if bp >= SHARE_MIN_PREFIX else (-1, 0)


def shared_tiles(active_slots, lineage, P, rows_per_tile, chunk, S):
    """The tile table of rv_attn_decode_shared_bf16 for S cache rows.  lineage[s]: the lineage of slot s (any int >= 0: the slots copied,
    directly or transitively, from one leader prompt, and that leader), -1 for an ungrouped slot; P[s]: the positions slot s holds in
    common with its lineage (a leader: the largest P a follower took from it).  The active slots of a lineage, sorted by slot, are cut
    into tiles of rows_per_tile rows; a tile's shared chunk count is min(P over its rows) // chunk.  Returns (c0 int32 [S]: 0 for
    ungrouped rows, idle rows, tiles of one row and tiles with no whole shared chunk; tile int32 [S, 16]: row s lists its tile's slots
    when it is the tile's first row, padded with -1, else tile[s, 0] == -1)."""
    c0 = np.zeros(S, dtype=np.int32)
    tile = np.full((S, SHARED_TILE_COLS), -1, dtype=np.int32)
    assert 1 <= rows_per_tile <= SHARED_TILE_COLS and chunk > 0
    groups = {}
    for s in sorted(int(v) for v in active_slots):
        if lineage[s] >= 0:
            groups.setdefault(int(lineage[s]), []).append(s)
    for rows in groups.values():
        for k in range(0, len(rows), rows_per_tile):
            t = rows[k:k + rows_per_tile]
            c = min(int(P[s]) for s in t) // chunk
            if len(t) < 2 or c <= 0:
                continue
            c0[t] = c
            tile[t[0], :len(t)] = t
    return c0, tile


def check_shared_tiles(c0, tile, rows_per_tile):
    """ValueError unless (c0 [S], tile [S, 16]) is a table shared_tiles could have built: every tile entry in [-1, S); a listed tile
    names its own row first (the leader), then distinct rows, at most rows_per_tile of them, -1 only as padding; c0 >= 0, equal within a
    tile; a row with c0 > 0 belongs to exactly one listed tile and a row with c0 == 0 to none."""
    c0, tile = np.asarray(c0), np.asarray(tile)
    S = c0.shape[0]
    if c0.ndim != 1 or tile.shape != (S, SHARED_TILE_COLS):
        raise ValueError(f"shared tiles: c0 must be [S] and tile [S, {SHARED_TILE_COLS}], got {c0.shape} and {tile.shape}")
    if not 1 <= rows_per_tile <= SHARED_TILE_COLS:
        raise ValueError(f"shared tiles: rows_per_tile must lie in [1, {SHARED_TILE_COLS}], got {rows_per_tile}")
    if (tile < -1).any() or (tile >= S).any():
        raise ValueError(f"shared tiles: an entry lies outside [-1, {S})")
    if (c0 < 0).any():
        raise ValueError("shared tiles: a negative shared chunk count")
    member = np.zeros(S, dtype=np.int64)
    for s in range(S):
        if tile[s, 0] == -1:
            if (tile[s] != -1).any():
                raise ValueError(f"shared tiles: row {s} lists rows after a -1")
            continue
        if tile[s, 0] != s:
            raise ValueError(f"shared tiles: row {s} lists a tile that starts with row {int(tile[s, 0])}: the leader comes first")
        n = int((tile[s] >= 0).sum())
        rows = tile[s, :n]
        if (rows < 0).any() or n > rows_per_tile or np.unique(rows).shape[0] != n:
            raise ValueError(f"shared tiles: row {s}'s tile must be at most {rows_per_tile} distinct rows with -1 only as padding")
        if c0[s] <= 0 or (c0[rows] != c0[s]).any():
            raise ValueError(f"shared tiles: the rows of row {s}'s tile must have one shared chunk count > 0, got {c0[rows].tolist()}")
        member[rows] += 1
    if (member > 1).any() or ((c0 > 0) != (member == 1)).any():
        raise ValueError("shared tiles: a row with c0 > 0 must belong to exactly one listed tile and a row with c0 == 0 to none")


class DevicePicker:
    """Token choice of one generate_batch() step on the device, for rows at different steps: rv_argmax_rows_f32 when no processor is
    active and no logprobs are asked for, else rv_logits_process_argmax_rows_f32 (row r at its own step t[r] with its own EOS minimum).
    The emitted tokens go into the device history, int32 [slots, max budget], at (slot, t); a slot's history restarts at t = 0 with
    each request admitted into it.  With cfg.sampling the token of row r is drawn by rv_sample_rows_f32 with the seed of the slot's
    request at t[r], after the processors when one is active; the logprob is then log q of the drawn token, and the warped scores are
    written back only when a stopping criterion will read them."""

    def __init__(self, engine, cfg, slots, max_budget, logprobs, any_min_new):
        lp = LogitsProcessors(cfg, engine.vocab)
        self.engine, self.vocab, self.logprobs = engine, engine.vocab, bool(logprobs)
        self.sampling, self.write_scores = cfg.sampling, bool(cfg.stopping_criteria)
        self.penalty, self.ngram = lp.penalty, lp.ngram
        self.active = (lp.penalty != 1.0 or lp.ngram > 0 or bool(cfg.bad_words_ids) or bool(lp.suppress) or bool(lp.begin) or
                       (any_min_new and bool(lp.eos)))
        self.bans = lp.rows_device_args(engine.device)
        self.hist = torch.zeros(slots, max(int(max_budget), 1), dtype=torch.int32, device=engine.device) if self.active else None
        self.ws, self.ws_rows = None, 0                       # the sampler's scratch, kept across steps

    def __call__(self, logits, slot, t, min_new, seed=None):
        """logits: fp32 [rows, vocab] (processed in place); slot / t / min_new: numpy ints [rows]; seed: the rows' request seeds when
        sampling.  Returns (tokens, logprobs or None)."""
        from . import ops
        if self.sampling is not None:
            return self._sample(logits, slot, t, min_new, seed)
        if not (self.active or self.logprobs):
            return ops.argmax_rows(logits, self.vocab).cpu().numpy(), None
        cols = 1 if self.hist is None else self.hist.shape[1]
        info = self.engine._dev(np.stack([slot, t, min_new, slot * cols + t]).astype(np.int32))
        lpo = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device) if self.logprobs else None
        tok = ops.logits_process_argmax_rows(logits, self.vocab, self.hist, info[0], info[1], info[2], self.penalty, self.ngram, *self.bans,
                                             logprob=lpo)
        if self.hist is not None:
            self.hist.view(-1).index_copy_(0, info[3].long(), tok.to(torch.int32))
        return tok.cpu().numpy(), None if lpo is None else lpo.cpu().numpy()

    def _sample(self, logits, slot, t, min_new, seed):
        from . import ops
        sm, rows = self.sampling, logits.shape[0]
        cols = 1 if self.hist is None else self.hist.shape[1]
        host = np.empty(6 * rows, dtype=np.int32)             # one upload: slot, t, min_new, history index (int32), then the int64 seeds
        host[:4 * rows] = np.stack([slot, t, min_new, slot * cols + t]).astype(np.int32).reshape(-1)
        host[4 * rows:].view(np.int64)[:] = np.asarray(seed, dtype=np.int64)
        d = self.engine._dev(host)
        info, seeds = d[:4 * rows].view(4, rows), d[4 * rows:].view(torch.int64)
        if self.active:
            ops.logits_process_argmax_rows(logits, self.vocab, self.hist, info[0], info[1], info[2], self.penalty, self.ngram, *self.bans)
        if self.ws is None or self.ws_rows < rows:            # grows to the largest step (all slots) and stays
            self.ws, self.ws_rows = ops.sample_rows_workspace(rows, logits.device), rows
        lpo = torch.empty(rows, dtype=torch.float32, device=logits.device) if self.logprobs else None
        tok = ops.sample_rows(logits, self.vocab, seeds, info[1], sm.temperature, sm.top_k, sm.top_p, sm.min_p,
                              write_scores=self.write_scores, logprob=lpo, ws=self.ws)
        if self.hist is not None:
            self.hist.view(-1).index_copy_(0, info[3].long(), tok.clamp(min=0).to(torch.int32))
        return tok.cpu().numpy(), None if lpo is None else lpo.cpu().numpy()


class BatchScheduler:
    """Continuous batching of greedy or sampled requests over one KVCache of `slots` sequences (generate_batch).  Host code: it reaches the engine
    through plan, kv_cache_bytes, free_device_bytes, new_kv_cache, prefill(..., cache=, slots=) and decode_step, and chooses tokens
    through `picker` (default DevicePicker), so a fake engine and picker can drive it on the CPU.

    Every request is planned once (spliced length, budget, EOS minimum).  Waiting requests enter free slots in input order; those admitted
    together are prefilled together (one prefill, their images encoded together).  A group is admitted when `admit_free` slots are free,
    when nothing is decoding, or when every waiting request fits.  Each decode step runs all slots: an idle slot is fed token 0 at
    position 0 (its length is 0 before and after the step) and its logits are ignored.  A request finishes on an EOS token, its budget or a
    stopping criterion (called as generate() calls it at B = 1: the request's tokens [1, t] and its processed scores [1, vocab]), and
    frees its slot.  With cfg.sampling request i carries its own seed (sampling_seeds: an int s gives s + i) and the picker is called with
    seed=, the seeds of the rows' requests (0 for an idle slot), next to each row's step t: what a request draws depends on neither the
    slot nor the schedule.  cfg.kv_cache_dtype "int8": the memory check and the cache are sized for the int8 cache (the dtype is passed to
    kv_cache_bytes and new_kv_cache; the default dtype keeps their two-argument calls).
    cfg.guidance (classifier-free guidance; the requests then carry neg_ids / neg_images / neg_sizes, batch_requests): the cache has
    2 * slots rows, slot s holding the request's prompt and row slots + s its negative prompt; the memory check counts both halves and
    L_max covers the longer of the two prompts plus the budget; an admitted group is two prefills (the negative group ordered by the
    same image-first rule); a decode step runs all 2 * slots rows, feeding a request's token to both of its rows (an idle slot's two
    rows: token 0 at length 0); `guide(cond, uncond)` -- default ops.cfg_guide_rows with the call's scale -- then turns the first
    `slots` rows into the guided scores in place and the picker runs on them as it does without guidance.  A finished request frees
    both rows.  Without cfg.guidance nothing here changes.  `events` records the schedule: ("admit", requests, slots), ("decode", active slots), ("finish", request, slot, t).
    cfg.share_prefix (shared prompt prefixes; the engine is then also reached through extend(..., slots=, reuse=), shared_rows_per_tile,
    shared_plan and decode_step(shared=)): every request's position_records are computed once, image uids by content with one table per
    call.  Each request of an admitted group, in input order, takes as source the active slot or earlier leader of the same admission
    with the longest common prefix P (best_source); with P >= SHARE_MIN_PREFIX it is a follower, else a leader.  Leaders are prefilled
    as ever; then every follower's positions 0 .. P - 1 are copied into its own slot (one copy per layer) and one extend computes all
    the followers' suffixes; _step runs once per phase and ("share", request, slot, source slot, P) follows the "admit" entry.  A
    row is self-contained, so a group outlives its leader and no cache bytes are saved.  The decode step's tile table (shared_tiles
    over the active slots' lineages) is rebuilt when an admission or a finish changes the active set and uploaded when it differs;
    while no tile shares a chunk decode_step is called without shared=.  Without cfg.share_prefix nothing here changes.
    cfg.dola (DoLa): the spec is resolved against the engine's depth once per call; admissions and decode steps ask the engine for the
    candidate layers' logits (tap_layers=) and `contrast(logits, candidates)` -- default ops.dola_contrast_rows -- turns the rows into
    the contrasted rows in place where `guide` runs in a guided call, before the picker.  Every row chooses its own layer, so an idle
    slot's garbage row touches no other row.  Not combined with guidance or share_prefix.  Without cfg.dola nothing here changes.
    cfg.constraint (constrained decoding): the requests' automata become one table (constraints.resolve_constraints, checked against
    the vocabulary before anything runs) and the device keeps one int32 state per cache slot.  _step runs `constrain(logits, slots,
    starts, fed)` -- default: ops.constrain_rows -- before the picker.  After an admission (fed None) it first writes the admitted
    requests' start states into their slots and masks the group's rows through slot=; in a decode step (fed: the device copy of the
    tokens decode_step was given, one upload for both) row s is slot s, each live state takes its token's edge and the row is
    masked.  An idle slot keeps whatever state its last request left, advanced by the 0 an idle slot is fed; its row is ignored as
    ever and the next admission overwrites the state.  ConstraintMirror follows the states per slot on the host and raises
    RuntimeError naming the request and its step at a dead end.  Without cfg.constraint nothing here changes.
    cfg.kvpress (prompt cache compression, (N, w, k)): L_max and the memory check count min(spliced, N) + budget positions per request,
    and engine.prefill is given compress=(N, w, k) -- only then, so an engine without the argument serves every other call.  The
    engine keeps each slot's position offset in the cache (KVCache.pos_off); nothing else here changes.  Not combined with
    share_prefix, guidance, dola or an int8 cache."""

    def __init__(self, engine, reqs, cfg, max_batch_size=32, return_logprobs=False, admit_free=None, picker=None, guide=None,
                 constrain=None):
        if not _is_int(max_batch_size) or max_batch_size < 1:
            raise ValueError(f"max_batch_size must be an int >= 1, got {max_batch_size!r}")
        refuse_combinations(features_of(cfg), "generate_batch()")        # protects a cfg built by hand
        self.engine, self.reqs, self.cfg = engine, reqs, cfg
        self.logprobs = bool(return_logprobs)
        n = len(reqs)
        plans = [engine.plan(r.ids[None], None, None, r.images, r.sizes) for r in reqs]
        self.spliced = [int(pl["lens"][0]) for pl in plans]
        self.share = bool(getattr(cfg, "share_prefix", False))
        if self.share:
            held = []                                         # one uid table per call: (pixels, image_size) of every distinct image
            self.records = [position_records(pl, self._image_uids(held, r))[0] for pl, r in zip(plans, reqs)]
        del plans
        self.budget = [cfg.budgets[i] if cfg.budgets is not None else new_token_budget(cfg, self.spliced[i]) for i in range(n)]
        self.min_new = [min_new_length(cfg, self.spliced[i]) for i in range(n)]
        self.seeds = None if getattr(cfg, "sampling", None) is None else sampling_seeds(cfg.sampling, n)
        self.runs = [i for i in range(n) if self.budget[i] > 0]
        self.slots = min(int(max_batch_size), len(self.runs))
        self.L_max = max([self.spliced[i] + self.budget[i] for i in self.runs], default=0)
        self.press = getattr(cfg, "kvpress", None)
        if self.press is not None:            # a request then takes min(spliced, N) slots: the cache and the memory check shrink with it
            self.L_max = max([min(self.spliced[i], self.press[0]) + self.budget[i] for i in self.runs], default=0)
        self.guidance, self.guide = getattr(cfg, "guidance", None), guide
        self.dola, self.contrast = getattr(cfg, "dola", None), None
        if self.dola is not None:
            self.dola = resolve_dola_layers(self.dola, engine.l["layers"])
        # the keywords of decode_step, and of prefill with compress=: only those of a feature that is on
        self.step_kw = {} if self.dola is None else dict(tap_layers=self.dola)
        self.prefill_kw = dict(self.step_kw) if self.press is None else dict(self.step_kw, compress=self.press)
        self.ctab, self.constrain = None, constrain
        if getattr(cfg, "constraint", None) is not None:
            from .constraints import resolve_constraints
            self.ctab, self.cstart = resolve_constraints(cfg.constraint, n, engine.vocab, what="request")
        if self.guidance is not None:
            self.neg_spliced = [int(engine.plan(r.neg_ids[None], None, None, r.neg_images, r.neg_sizes)["lens"][0]) for r in reqs]
            self.L_max = max([max(self.spliced[i], self.neg_spliced[i]) + self.budget[i] for i in self.runs], default=0)
        self.max_budget = max([self.budget[i] for i in self.runs], default=0)
        self.admit_free = max(1, min(ADMIT_FREE_SLOTS if admit_free is None else int(admit_free), self.slots))
        self.picker = picker
        self.events = []
        self.tokens = [[] for _ in range(n)]
        self.logps = [[] for _ in range(n)]

    @staticmethod
    def _image_uids(held, r):
        """uid of each image of request r by content, as GenerationCache._image_uids: the same bits and image_size, the same uid."""
        uids = []
        for i, im in enumerate(r.images):
            size = None if r.sizes is None else tuple(int(v) for v in r.sizes[i])
            hit = next((u for u, (px, sz) in enumerate(held) if sz == size and (px is im or _same_pixels(px, im))), None)
            if hit is None:
                hit = len(held)
                held.append((im, size))
            uids.append(hit)
        return uids

    def run(self):
        """Generate every request; returns {"req_<i>": GenerationOutput} in input order."""
        if self.runs:
            self._run()
        return {f"req_{i}": GenerationOutput(request_id=f"req_{i}", prompt_ids=[int(v) for v in r.ids], generated_tokens=list(self.tokens[i]),
                                             logprobs=list(self.logps[i]), error=None, status="finished")
                for i, r in enumerate(self.reqs)}

    def _run(self):
        eng, S = self.engine, self.slots
        kvd = getattr(self.cfg, "kv_cache_dtype", "bf16")
        kv_args = () if kvd == "bf16" else (kvd,)             # the default dtype keeps the two-argument calls
        rows = 2 * S if self.guidance is not None else S      # guidance: row S + s is slot s's unconditional sequence
        need = eng.kv_cache_bytes(rows, self.L_max, *kv_args)
        free = eng.free_device_bytes()
        if free is not None and need > free:
            raise ValueError(f"generate_batch: the KV cache of {rows} rows x {self.L_max} positions needs {need} bytes, but only {free} bytes "
                             f"of device memory are free: lower max_batch_size or the token budgets")
        if self.picker is None:
            self.picker = DevicePicker(eng, self.cfg, S, self.max_budget, self.logprobs, any(self.min_new[i] > 0 for i in self.runs))
        self.cache = eng.new_kv_cache(rows, self.L_max, *kv_args)
        if self.guidance is not None and self.guide is None:
            from . import ops
            gws, g, V = ops.cfg_guide_workspace(S, eng.device), self.guidance.scale, eng.vocab
            self.guide = lambda c, u: ops.cfg_guide_rows(c, u, V, g, ws=gws)
        if self.dola is not None:
            from . import ops
            dws, V = ops.dola_workspace(S, len(self.dola), eng.device), eng.vocab
            self.contrast = lambda f, c: ops.dola_contrast_rows(f, c, V, ws=dws)
        # what turns a step's rows into the rows the picker sees, in place: (conditional, unconditional) or (last layer, candidates)
        self.transform = self.guide if self.guidance is not None else self.contrast
        if self.ctab is not None:
            self.mirror = ConstraintMirror(self.ctab, S)
            if self.constrain is None:
                self.constrain = self._device_constrain()
        self.owner = np.full(S, -1, dtype=np.int64)           # request in each slot, -1: idle
        self.t = np.zeros(S, dtype=np.int64)                  # tokens the slot's request has generated
        self.mn = np.zeros(S, dtype=np.int64)                 # its EOS minimum
        self.pending = np.zeros(S, dtype=np.int64)            # its last token, fed to the next decode step
        self.free = list(range(S))
        if self.share:
            self.slot_rec = [None] * S                        # prompt records of the slot's request, None: idle
            self.lineage = np.full(S, -1, dtype=np.int64)     # the request whose prompt the slot's shared positions come from, -1: none
            self.P = np.zeros(S, dtype=np.int64)              # positions the slot holds in common with its lineage
            self.plan, self.plan_key, self.retile = None, None, False
        waiting = list(self.runs)
        while waiting or (self.owner >= 0).any():
            while waiting and (len(self.free) >= self.admit_free or not (self.owner >= 0).any() or len(waiting) <= len(self.free)):
                k = min(len(self.free), len(waiting))
                group, waiting = waiting[:k], waiting[k:]
                gslots, self.free = self.free[:k], self.free[k:]
                self._admit(group, gslots)
            if (self.owner >= 0).any():
                self._decode()
        del self.cache

    @staticmethod
    def _pack(requests, negative=False):
        """The padded prompt batch of `requests` (negative: of their negative prompts), image requests first: in a batch the splice
        gives a text-only prompt a (dummy) image slot, which must not shift later images.  Returns (order, ids, am, imgs, sizes): row b
        holds requests[order[b]]; imgs is the flat image list in row order and sizes their sizes, None when no request gives any."""
        part = (lambda r: (r.neg_ids, r.neg_images, r.neg_sizes)) if negative else (lambda r: (r.ids, r.images, r.sizes))
        order = sorted(range(len(requests)), key=lambda j: not part(requests[j])[1])
        rows = [part(requests[j]) for j in order]
        ids = np.zeros((len(rows), max(p.size for p, _, _ in rows)), dtype=np.int64)
        am = np.zeros(ids.shape, dtype=bool)
        for b, (p, _, _) in enumerate(rows):
            ids[b, :p.size], am[b, :p.size] = p, True
        imgs = [im for _, ims, _ in rows for im in ims]
        sizes = [s for _, _, sz in rows for s in (sz or [])] if any(sz is not None for _, _, sz in rows) else None
        return order, ids, am, imgs, sizes

    def _admit(self, group, gslots):
        """An admission, in up to two phases: the leaders (without share_prefix: everyone) through one prefill -- a guided call
        prefills their negative prompts into rows slots + s after it -- then every follower's shared positions are copied into its
        slot (one copy per layer) and one extend computes all the followers' suffixes.  _step runs once per phase."""
        eng = self.engine
        self.events.append(("admit", tuple(group), tuple(gslots)))
        for q, s in zip(group, gslots):
            self.owner[s], self.t[s], self.mn[s] = q, 0, self.min_new[q]
        followers = self._match(group, gslots) if self.share else {}
        for phase in (False, True):
            members = [j for j in range(len(group)) if (j in followers) == phase]
            if not members:
                continue
            order, ids, am, imgs, sizes = self._pack([self.reqs[group[j]] for j in members])
            rows = [members[j] for j in order]
            rs = [gslots[j] for j in rows]
            if not phase:
                _, logits, *other = eng.prefill(ids, am, imgs or None, sizes, cache=self.cache, slots=rs, **self.prefill_kw)
                if self.guidance is not None:
                    other = [self._prefill_negative([self.reqs[group[j]] for j in rows], rs)]
            else:
                reuse = np.array([followers[j][1] for j in rows], dtype=np.int64)
                for j in members:                             # input order: a source is an older slot or a leader of phase 1
                    src, p = followers[j]
                    for layer in self.cache.layers:
                        layer[gslots[j], :p] = layer[src, :p]
                    self.cache.lens[gslots[j]] = p            # the slot holds these positions now: what extend(reuse=) checks
                _, logits = eng.extend(self.cache, ids, am, imgs or None, sizes, reuse=reuse, slots=rs)
            if self.transform is not None:
                self.transform(logits, other[0])
            self._step(logits, rs)

    def _match(self, group, gslots):
        """Sources of an admitted group (share_prefix): for each request in input order, the best source (best_source) among the active
        slots' prompts -- the group's own slots were free, so they are none of those -- and the earlier leaders of this admission.
        Books records, lineage and P per slot and the "share" events; returns {index in group: (source slot, P)} of the followers."""
        taken = set(int(s) for s in gslots)
        sources = [(s, self.slot_rec[s]) for s in range(self.slots) if self.owner[s] >= 0 and s not in taken]
        followers = {}
        for j, (q, s) in enumerate(zip(group, gslots)):
            rec = self.records[q]
            src, p = best_source(rec, sources)
            self.slot_rec[s] = rec
            if src < 0:
                self.lineage[s], self.P[s] = -1, 0
                sources.append((int(s), rec))                 # a leader of this admission: prefilled before any follower is copied
                continue
            followers[j] = (src, p)
            if self.lineage[src] < 0:                         # the source becomes a lineage's leader
                self.lineage[src] = self.owner[src]
            if self.lineage[src] == self.owner[src]:          # a leader's own P: the largest P a follower took from it
                self.P[src] = max(self.P[src], p)
            # copied from a follower, the row holds the lineage's prompt only as far as that follower does
            self.lineage[s], self.P[s] = self.lineage[src], min(p, int(self.P[src]))
            self.events.append(("share", int(q), int(s), int(src), int(p)))
        self.retile = True
        return followers

    def _shared_plan(self):
        """The decode step's tile table, rebuilt when an admission or a finish changed the active set and uploaded when it differs
        from the last one; None while no tile shares a chunk."""
        if self.retile:
            self.retile = False
            c0, tile = shared_tiles(np.flatnonzero(self.owner >= 0), self.lineage, self.P, self.engine.shared_rows_per_tile,
                                    type(self.cache).chunk, self.slots)
            key = (c0.tobytes(), tile.tobytes())
            if key != self.plan_key:
                self.plan_key = key
                self.plan = self.engine.shared_plan(c0, tile) if c0.any() else None
        return self.plan

    def _prefill_negative(self, rq, rs):
        """Prefill the negative prompts of the admitted requests rq (slots rs) into rows slots + s; returns their logits in rq's order."""
        order, ids, am, imgs, sizes = self._pack(rq, negative=True)
        _, un = self.engine.prefill(ids, am, imgs or None, sizes, cache=self.cache, slots=[self.slots + rs[j] for j in order])
        back = np.argsort(np.asarray(order))                                    # row j of the group is row back[j] of `un`
        if not np.array_equal(back, np.arange(len(order))):
            un = un[torch.as_tensor(back, device=un.device)]
        return un

    def _decode(self):
        """One decode step over every cache row: the slots, and under guidance the rows slots + s after them, fed the same tokens."""
        idle, S = self.owner < 0, self.slots
        self.events.append(("decode", tuple(int(s) for s in np.flatnonzero(~idle))))
        idle_rows = idle if self.guidance is None else np.concatenate([idle, idle])
        self.cache.lens[idle_rows] = 0
        kw = self.step_kw
        plan = self._shared_plan() if self.share else None
        if plan is not None:
            kw = dict(kw, shared=plan)
        feed, fed = np.where(idle, 0, self.pending), None
        if self.ctab is not None:         # one upload: the decode step's tokens are the ones the automaton states take
            feed = fed = self.engine._dev(feed.astype(np.int64))
        if self.guidance is not None:
            feed = np.concatenate([feed, feed])
        out = self.engine.decode_step(self.cache, feed, **kw)
        self.cache.lens[idle_rows] = 0
        logits, *other = out if self.step_kw else (out,)
        if self.guidance is not None:
            logits, other = logits[:S], [logits[S:]]
        if self.transform is not None:
            self.transform(logits, other[0])
        self._step(logits, list(range(S)), fed)

    def _device_constrain(self):
        """The default `constrain`: the call's table and one int32 state per slot on the device, ops.constrain_rows."""
        from . import ops
        eng, V = self.engine, self.engine.vocab
        tabs = self.ctab.device_tables(eng.device)
        state = torch.full((self.slots,), -1, dtype=torch.int32, device=eng.device)

        def constrain(logits, slots, starts, fed):
            if fed is None:               # an admission: the start states go into the slots, then the rows are masked through slot=
                info = eng._dev(np.stack([slots, starts]).astype(np.int32))
                state.index_copy_(0, info[0].long(), info[1])
                ops.constrain_rows(logits, V, state, tabs, slot=info[0])
            else:                         # a decode step: row s is slot s
                ops.constrain_rows(logits, V, state, tabs, tok=fed)
        return constrain

    def _step(self, logits, row_slots, fed=None):
        """Choose the tokens of logits' rows (row r belongs to slot row_slots[r]) and book them per request.  fed (constrained
        decoding): the device tokens of the decode step that made these rows; None after an admission."""
        cfg = self.cfg
        sl = np.asarray(row_slots, dtype=np.int64)
        if self.ctab is not None:
            starts = self.cstart[self.owner[sl]] if fed is None else None
            self.constrain(logits, sl, starts, fed)
            if fed is None:
                self.mirror.state[sl] = starts
        if self.seeds is None:
            tok, lps = self.picker(logits, sl, self.t[sl], self.mn[sl])
        else:
            seed = np.array([self.seeds[q] if q >= 0 else 0 for q in self.owner[sl]], dtype=np.int64)
            tok, lps = self.picker(logits, sl, self.t[sl], self.mn[sl], seed=seed)
        if self.ctab is not None:         # before the booking below frees slots: a dead end names its request and step
            act = np.flatnonzero(self.owner[sl] >= 0)
            self.mirror.take(sl[act], np.asarray(tok)[act],
                             lambda k: getattr(self.picker, "active", True) and float(logits[act[k], 0]) == float("-inf"),
                             lambda k: f"request {int(self.owner[sl[act[k]]])}", self.t[sl[act]])
        for r, s in enumerate(row_slots):
            q = int(self.owner[s])
            if q < 0:
                continue
            tk = int(tok[r])
            if tk < 0:
                _check_sampled(tok, [r])
            self.tokens[q].append(tk)
            if self.logprobs:
                self.logps[q].append(float(lps[r]))
            n = len(self.tokens[q])
            done = tk in cfg.eos or n >= self.budget[q]
            if cfg.stopping_criteria:
                ids = torch.tensor([self.tokens[q]], dtype=torch.int64, device=self.engine.device)
                for c in cfg.stopping_criteria:
                    res = c(ids, logits[r:r + 1])
                    res = res.detach().cpu().numpy() if torch.is_tensor(res) else np.asarray(res)
                    done = done or bool(res.astype(bool).any())
            if done:
                self.events.append(("finish", q, int(s), n))
                self.owner[s], self.t[s], self.mn[s] = -1, 0, 0
                self.free = sorted(self.free + [int(s)])
                if self.share:                                # the row keeps its bits until the slot is refilled, but it is no source
                    self.slot_rec[s], self.lineage[s], self.P[s], self.retile = None, -1, 0, True
            else:
                self.pending[s], self.t[s] = tk, n


def generate_batch(engine, inputs, images, image_sizes, cfg, max_batch_size=32, return_logprobs=False):
    """Continuous batching over many prompts (LlavaLlamaForCausalLM.generate_batch); cfg from parse_batch_kwargs.  Each request's
    generated tokens are what generate() returns for it alone (B = 1, the same settings), up to rounding."""
    return BatchScheduler(engine, batch_requests(inputs, images, image_sizes, getattr(cfg, "guidance", None)), cfg, max_batch_size,
                          return_logprobs).run()


# ------------------------------------------------------------------------------------------------ beam search: generate_beams
# HF semantics followed: GenerationMixin._beam_search of transformers 5.x (HF: generation/utils.py) for a decoder-only model called with
# inputs_embeds: input_ids start empty, decoder_prompt_len = 0, lengths count generated tokens only, the sequences hold the new tokens
# only.  BeamState restates its bookkeeping step for step in numpy fp32.  One place is stricter than HF: torch.topk leaves the order
# among equal values open; every top-K here is total (value descending, then the lower flat index beam * vocab + token, or the lower
# candidate slot).  The division by length ** length_penalty is an fp32 division by the fp32-rounded power (torch's CPU result).
BEAM_MAX = 16                 # num_beams limit (rv_beam_topk_f32)
BEAM_TOPK_MAX = 64            # candidates kept per prompt and step, K = max(2, 1 + n_eos) * num_beams
_BEAM_ONLY = ("length_penalty", "early_stopping")
_NEG = np.float32(-1.0e9)


class GenerateBeamDecoderOnlyOutput(SimpleNamespace):
    """HF's return_dict_in_generate output of beam search: .sequences [B * num_return_sequences, T_out]; .sequences_scores (None unless
    output_scores); .scores (output_scores: per step the processed log-probs [B * num_beams, vocab]); .logits (output_logits: the raw
    ones); .beam_indices [B * num_return_sequences, T_out] (-1 past a hypothesis' end); .past_key_values (the engine's beam KVCache)."""

    def __getitem__(self, k):
        return getattr(self, k)


def beams_to_keep(num_beams, n_eos):
    return max(2, 1 + int(n_eos)) * int(num_beams)


def parse_beam_kwargs(kwargs, lora=False, config_eos=None, config_pad=None):
    """Validate generate_beams() keyword arguments: generate()'s, plus length_penalty (float, default 1.0), early_stopping (False, True
    or "never") and num_return_sequences <= num_beams.  ValueError for num_beams outside [1, 16] or K = max(2, 1 + n_eos) * num_beams
    above 64; NotImplementedError for do_sample=True (beam sampling), past_key_values, streamer, inputs_embeds, LoRA engines and
    kv_cache_dtype="int8" (None and "bf16" are accepted and change nothing), for dola_layers, and for classifier-free guidance
    (guidance_scale or any negative_* argument given);
    TypeError for unknown names.  The sampling knobs HF ignores when greedy stay ignored."""
    unknown = sorted(k for k in kwargs if k not in _ACCEPTED and k not in _BEAM_ONLY and k not in _GUIDANCE and k not in _DOLA)
    if unknown:
        raise TypeError(f"generate_beams() got unexpected keyword arguments {unknown}")
    if kwargs.get("dola_layers") is not None:
        raise NotImplementedError("dola_layers with beams: contrasting layers per beam is not implemented; generate() and generate_batch() "
                                  "take it")
    given = sorted(k for k in _GUIDANCE if kwargs.get(k) is not None)
    if given:
        raise NotImplementedError(f"classifier-free guidance with beams is not implemented (guidance_scale and its negative prompt: "
                                  f"got {given}); generate() and generate_batch() take them")
    if kwargs.get("do_sample"):
        raise NotImplementedError("do_sample=True with beams: beam sampling is not implemented")
    if kwargs.get("past_key_values") is not None:
        raise NotImplementedError("past_key_values: a GenerationCache across generate_beams() calls is not implemented")
    if parse_kv_cache_dtype(kwargs.get("kv_cache_dtype")) == "int8":
        raise NotImplementedError("kv_cache_dtype='int8' with beams: the beam-attention kernel reads a bf16 cache only")
    nb = kwargs.get("num_beams")
    nb = 1 if nb is None else nb
    if not _is_int(nb) or not 1 <= nb <= BEAM_MAX:
        raise ValueError(f"`num_beams` has to be an integer in [1, {BEAM_MAX}], but is {nb!r}")
    nrs = kwargs.get("num_return_sequences")
    nrs = 1 if nrs is None else nrs
    if not _is_int(nrs) or nrs < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {nrs!r}")
    if nrs > nb:
        raise ValueError(f"`num_return_sequences` (={nrs}) has to be smaller or equal to `num_beams` (={nb})")
    pen = kwargs.get("length_penalty")
    pen = 1.0 if pen is None else pen
    if isinstance(pen, bool) or not isinstance(pen, (int, float, np.floating, np.integer)) or not np.isfinite(pen):
        raise ValueError(f"`length_penalty` has to be a finite float, but is {pen!r}")
    es = kwargs.get("early_stopping")
    es = False if es is None else es
    if not (es is True or es is False or es == "never"):
        raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {es!r}")
    kw = {k: v for k, v in kwargs.items() if k not in _BEAM_ONLY and k not in ("num_beams", "num_return_sequences")}
    cfg = parse_generate_kwargs(kw, lora=lora, config_eos=config_eos, config_pad=config_pad)
    K = beams_to_keep(nb, len(cfg.eos))
    if K > BEAM_TOPK_MAX:
        raise ValueError(f"num_beams={nb} with {len(cfg.eos)} EOS ids keeps max(2, 1 + n_eos) * num_beams = {K} candidates per step; the limit is "
                         f"{BEAM_TOPK_MAX}")
    # HF: output_fill_value = pad_token_id or eos_token_id[0] if eos_token_id is not None else -1 (generate() has set a missing
    # pad_token_id to the first EOS id by then).  Read as Python reads it: without an EOS id the fill is -1 whatever the pad.
    pad = kwargs.get("pad_token_id", config_pad)
    cfg.fill = (int(pad) if pad else cfg.eos[0]) if cfg.eos else -1
    cfg.num_beams, cfg.num_return_sequences, cfg.length_penalty, cfg.early_stopping, cfg.K = int(nb), int(nrs), float(pen), es, K
    return cfg


def _topk_desc(v, k):
    """Indices of the k best entries of each row of v [B, N]: value descending, then the lower index (a stable sort of -v)."""
    return np.argsort(-v, axis=1, kind="stable")[:, :k]


def _take(a, idx):
    """HF's _gather_beams: a [B, N, ...] at idx [B, k] along dim 1."""
    return np.take_along_axis(a, idx.reshape(idx.shape + (1,) * (a.ndim - 2)), axis=1)


def advance_tail_src(tail_src, parent_rows, i):
    """The ancestry table after the beam step that chose the running beams of generated position i: row r continues row parent_rows[r]
    (cache rows, b * num_beams + beam), so it inherits that row's first i entries, and its own position i lives in row r itself.
    tail_src: int32 [rows, T]; returns a new array, the input is not modified."""
    rows = tail_src.shape[0]
    new = tail_src[np.asarray(parent_rows, dtype=np.int64).reshape(rows)].copy()
    new[:, i] = np.arange(rows, dtype=tail_src.dtype)
    return new


class BeamState:
    """The bookkeeping of HF's _beam_search for B prompts x num_beams beams over a vocabulary of `vocab` ids and at most max_new
    generated tokens (HF's max_length under inputs_embeds generation).  numpy, fp32, no device.  It receives each step's K = max(2, 1 +
    n_eos) * num_beams best candidates per prompt (it does not compute them): step() returns the parent beam and the token of every
    next running beam; `done` is HF's `this_peer_finished`; finalize() the returned hypotheses.
    running_*: the live beams (sequences [B, nb, max_new] filled with `fill`, scores starting at [0, -1e9, ...], beam indices filled
    with -1); sequences / beam_scores / beam_indices / is_sent_finished: the finished set; unsat: the early-stop heuristic flag."""

    def __init__(self, B, num_beams, vocab, max_new, eos=(), length_penalty=1.0, early_stopping=False, fill=-1):
        self.B, self.nb, self.vocab, self.T = int(B), int(num_beams), int(vocab), int(max_new)
        self.eos = [int(e) for e in eos]
        self.K = beams_to_keep(self.nb, len(self.eos))
        self.length_penalty, self.early_stopping = length_penalty, early_stopping
        B, nb, T = self.B, self.nb, self.T
        self.running_sequences = np.full((B, nb, T), int(fill), dtype=np.int64)
        self.sequences = self.running_sequences.copy()
        self.running_scores = np.zeros((B, nb), dtype=np.float32)
        self.running_scores[:, 1:] = _NEG
        self.beam_scores = np.full((B, nb), _NEG, dtype=np.float32)
        self.is_sent_finished = np.zeros((B, nb), dtype=bool)
        self.unsat = np.ones((B, 1), dtype=bool)
        self.hits = np.zeros((B, nb), dtype=bool)
        self.running_beam_indices = np.full((B, nb, T), -1, dtype=np.int32)
        self.beam_indices = self.running_beam_indices.copy()
        self.cur = 0
        self.done = self.T == 0

    def candidates(self, topk_flat_idx):
        """The K candidate sequences of a step, flattened as HF hands them to the stopping criteria: int64 [B * K, cur + 1]."""
        flat = np.asarray(topk_flat_idx, dtype=np.int64).reshape(self.B, self.K)
        seq = _take(self.running_sequences, flat // self.vocab)[:, :, :self.cur + 1].copy()
        seq[:, :, self.cur] = flat % self.vocab
        return seq.reshape(self.B * self.K, self.cur + 1)

    def step(self, topk_vals, topk_flat_idx, hits_user_criteria=None):
        """topk_vals fp32 [B, K] / topk_flat_idx [B, K] (beam * vocab + token): the step's K best accumulated log-probs per prompt, best
        first; hits_user_criteria: None or bool [B, K] (or [B * K]), the OR of the user's stopping criteria on candidates().
        Returns (parent [B, nb], token [B, nb]) of the next running beams."""
        assert not self.done
        B, nb, K, cur = self.B, self.nb, self.K, self.cur
        vals = np.asarray(topk_vals, dtype=np.float32).reshape(B, K)
        flat = np.asarray(topk_flat_idx, dtype=np.int64).reshape(B, K)
        beam, tok = flat // self.vocab, flat % self.vocab
        # _get_top_k_continuations
        topk_seq = _take(self.running_sequences, beam)
        topk_seq[:, :, cur] = tok
        topk_idx = _take(self.running_beam_indices, beam)
        topk_idx[:, :, cur] = (beam + np.arange(B)[:, None] * nb).astype(np.int32)
        # stopping criteria on the candidates: the length budget, an EOS id, the user's
        hits = np.full((B, K), cur + 1 >= self.T, dtype=bool)
        if self.eos:
            hits |= np.isin(tok, self.eos)
        if hits_user_criteria is not None:
            hits |= np.asarray(hits_user_criteria, dtype=bool).reshape(B, K)
        # _get_running_beams_for_next_iteration
        run_vals = vals + hits.astype(np.float32) * _NEG
        nxt = _topk_desc(run_vals, nb)
        self.running_sequences = _take(topk_seq, nxt)
        self.running_scores = _take(run_vals, nxt)
        self.running_beam_indices = _take(topk_idx, nxt)
        # _update_finished_beams
        just = hits & (np.arange(K) < nb)[None, :]
        fin = vals / np.float32(float(cur + 1) ** self.length_penalty)
        full = self.is_sent_finished.all(axis=-1, keepdims=True) & (self.early_stopping is True)
        fin = fin + full.astype(np.float32) * _NEG
        fin = fin + (~self.unsat).astype(np.float32) * _NEG
        fin = fin + (~just).astype(np.float32) * _NEG
        m_scores = np.concatenate([self.beam_scores, fin], axis=1)
        best = _topk_desc(m_scores, nb)
        self.sequences = _take(np.concatenate([self.sequences, topk_seq], axis=1), best)
        self.beam_scores = _take(m_scores, best)
        self.beam_indices = _take(np.concatenate([self.beam_indices, topk_idx], axis=1), best)
        self.is_sent_finished = _take(np.concatenate([self.is_sent_finished, just], axis=1), best)
        self.hits = hits
        self.cur = cur = cur + 1
        # _check_early_stop_heuristic
        if self.early_stopping == "never" and self.length_penalty > 0.0:
            best_len = self.T
        else:
            best_len = cur
        best_run = self.running_scores[:, :1] / np.float32(float(best_len) ** self.length_penalty)
        worst = np.where(self.is_sent_finished, self.beam_scores.min(axis=1, keepdims=True), _NEG)
        self.unsat = self.unsat & (best_run > worst).any(axis=-1, keepdims=True)
        # _beam_search_has_unfinished_sequences
        unfinished = self.unsat.any() and not (self.is_sent_finished.all() and self.early_stopping is True) and not hits.all()
        self.done = not unfinished
        return _take(beam, nxt), _take(tok, nxt)

    def finalize(self, num_return_sequences=1):
        """(sequences int64 [B * nrs, T_out], scores fp32 [B * nrs], beam_indices int32 [B * nrs, T_out]), cropped as HF crops them."""
        n = int(num_return_sequences)
        seq = self.sequences[:, :n].reshape(self.B * n, self.T)
        sc = self.beam_scores[:, :n].reshape(self.B * n)
        bi = self.beam_indices[:, :n].reshape(self.B * n, self.T)
        T_out = int((bi != -1).sum(axis=1).max()) if bi.size else 0
        return seq[:, :T_out].copy(), sc.copy(), bi[:, :T_out].copy()


def beam_generate(engine, input_ids, attention_mask, images, image_sizes, cfg):
    """Beam search over the engine (LlavaLlamaForCausalLM.generate_beams); cfg from parse_beam_kwargs.  The prompts are prefilled once,
    prompt b into cache row b * num_beams of a KVCache of B * num_beams rows; every beam then appends its K|V to its own row and decode
    attention follows the beam's ancestry (engine.decode_step(beams=)), so no cache position is ever copied.  Per step, on the device:
    log-softmax of the raw scores, the logits processors (history: the running beams' tokens), the running score added inside the
    top-K; one device-to-host copy of the B * K values and indices feeds BeamState on the host."""
    from . import ops
    ids = np.asarray(input_ids.cpu() if torch.is_tensor(input_ids) else input_ids)
    if ids.ndim == 1:
        ids = ids[None]
    am = cfg.attention_mask
    am = None if am is None else np.asarray(am.cpu() if torch.is_tensor(am) else am)
    engine._check_generation()
    B, nb, K, V, dev = ids.shape[0], cfg.num_beams, cfg.K, engine.vocab, engine.device
    rows = B * nb
    imgs = list(images) if images is not None else []
    plan = engine.plan(ids, am, None, imgs, image_sizes)
    lens = plan["lens"].astype(np.int64)
    T = new_token_budget(cfg, int(plan["S"]))
    lp = LogitsProcessors(cfg, V, int(plan["S"]))
    st = BeamState(B, nb, V, T, cfg.eos, cfg.length_penalty, cfg.early_stopping, cfg.fill)
    scores, raw, cache = [], [], None
    if T > 0:
        if K > nb * V:
            raise ValueError(f"generate_beams: {K} candidates per step do not exist on {nb} beams over a vocabulary of {V} ids")
        if rows > 65535:
            raise ValueError(f"generate_beams: {B} prompts x {nb} beams = {rows} cache rows; a decode step takes at most 65535")
        L_max = int(lens.max()) + T
        need, free = engine.kv_cache_bytes(rows, L_max), engine.free_device_bytes()
        if free is not None and need > free:
            raise ValueError(f"generate_beams: the KV cache of {B} prompts x {nb} beams x {L_max} positions needs {need} bytes, but only "
                             f"{free} bytes of device memory are free: lower num_beams, the batch or the token budget")
        cache = engine.new_kv_cache(rows, L_max)
        roots = np.arange(B) * nb
        _, logits = engine.prefill(ids, am, images, image_sizes, max_new_tokens=T, cache=cache, slots=roots)
        cache.lens[:] = np.repeat(lens, nb)
        logits = logits.repeat_interleave(nb, dim=0)              # step 0 is not special: every beam carries the prefill scores
        geo = SimpleNamespace(prefix_row=engine._dev(np.repeat(roots, nb).astype(np.int32)),
                              prefix_len=engine._dev(np.repeat(lens, nb).astype(np.int32)), tail_src=None, tail_cols=0)
        tail = np.zeros((rows, T), dtype=np.int32)
        ws = ops.beam_topk_workspace(B, nb, V, K, dev)
        hist = None
        keep_scores = cfg.output_scores and cfg.return_dict
        for t in range(T):
            if cfg.output_logits:
                raw.append(logits.clone())
            ops.log_softmax_rows(logits, V)
            if lp.active:                 # in place on the log-probs; all rows share t, the argmax it returns is not used
                ops.logits_process_argmax(logits, V, hist, t, lp.penalty, lp.ngram, *lp.device_args(t, dev))
            if cfg.output_scores:
                scores.append(logits.clone())
            top = ops.beam_topk(logits, V, nb, engine._dev(st.running_scores.reshape(-1)), K, ws=ws).cpu()     # the step's one sync
            vals, flat = top[0].view(torch.float32).numpy(), top[1].numpy()
            hit = None
            if cfg.stopping_criteria:
                cand = torch.from_numpy(st.candidates(flat)).to(dev)
                hit = np.zeros(B * K, dtype=bool)
                for c in cfg.stopping_criteria:
                    r = c(cand, tuple(scores) if keep_scores else None)
                    r = r.detach().cpu().numpy() if torch.is_tensor(r) else np.asarray(r)
                    hit |= np.broadcast_to(r.astype(bool).reshape(-1) if r.ndim else r.astype(bool), hit.shape)
            parent, tok = st.step(vals, flat, hit)
            if st.done:
                break
            tail = advance_tail_src(tail, (roots[:, None] + parent).reshape(-1), t)
            geo.tail_src, geo.tail_cols = engine._dev(tail), t + 1
            if lp.active:                 # the running beams' tokens, re-gathered by parent inside BeamState
                hist = engine._dev(st.running_sequences.reshape(rows, T).astype(np.int32))
            logits = engine.decode_step(cache, tok.reshape(-1), beams=geo)
    seq, sc, bi = st.finalize(cfg.num_return_sequences)
    seq = torch.from_numpy(seq).to(dev)
    if cfg.return_dict:
        return GenerateBeamDecoderOnlyOutput(sequences=seq, sequences_scores=torch.from_numpy(sc).to(dev) if cfg.output_scores else None,
                                             scores=tuple(scores) if cfg.output_scores else None,
                                             logits=tuple(raw) if cfg.output_logits else None, beam_indices=torch.from_numpy(bi).to(dev),
                                             past_key_values=cache)
    return seq

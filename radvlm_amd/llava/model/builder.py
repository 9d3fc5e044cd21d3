"""``load_pretrained_model`` (reference finetuning/llava/model/builder.py): a model directory -> (tokenizer, model, image_processor,
context_len) for evaluation.  The directory is one written by ``save_pretrained`` (config.json in HF's keys + model.safetensors, tower
included) or any local HF-format LLaVA checkpoint that ``resolve_model_sources`` accepts; nothing is downloaded.  With ``model_base``
(builder.py:58-140) it is the output of a LoRA run (adapter_config.json: base weights + non_lora_trainables.bin + the adapters merged
in) or of a projector-only run (mm_projector.bin over the base weights); the branch follows the files present."""
import os
from types import SimpleNamespace

_TOKENIZER_FILES = ("tokenizer.json", "tokenizer.model", "tokenizer_config.json", "vocab.json")


def _build_model(config_dir, weights_dir, device):
    """A plain (no adapters) model with the geometry and mm_* / image_* settings of config_dir's config.json and the weights of
    weights_dir (the tower from the checkpoint itself or from the directory config_dir names)."""
    from ...checkpoint_io import load_pretrained, read_config
    from ..train.train import resolve_model_sources
    from .llava_llama import LlavaConfig, LlavaLlamaForCausalLM
    from .llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    args = SimpleNamespace(model_name_or_path=config_dir, vision_tower=None, geometry=None)
    geometry, _, tower_dir, is_qwen, true_vocab = resolve_model_sources(args)
    cfg_json = read_config(config_dir)
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if is_qwen else (LlavaConfig, LlavaLlamaForCausalLM)
    kw = {k: cfg_json[k] for k in ("mm_patch_merge_type", "image_aspect_ratio", "image_grid_pinpoints", "tokenizer_model_max_length",
                                   "tokenizer_padding_side", "eos_token_id", "pad_token_id") if cfg_json.get(k) is not None}
    cfg = Config(geometry=geometry, rms_norm_eps=geometry["lm"].get("rms_eps", 1e-5), rope_theta=geometry["lm"].get("rope_theta", 10000.0), **kw)
    cfg._name_or_path = config_dir
    model = Model(cfg, device=device, init="fast")
    if true_vocab != geometry["lm"]["vocab"]:
        model.engine.resize_token_embeddings(true_vocab)
    load_pretrained(model.engine, lm_path=weights_dir, tower_path=tower_dir)
    return model


def _load_into(model, sd, what):
    missing, unexpected = model.engine.load_state_dict(sd)
    if unexpected:
        raise KeyError(f"{what}: tensors the model does not have: {unexpected[:4]}")


def load_pretrained_model(model_path, model_base=None, model_name=None, load_8bit=False, device="cuda", quantization=None, **ignored):
    """Returns (tokenizer or None, model, image_processor or None, context_len).
      * adapter_config.json in model_path (LoRA run): the model is built from model_base (or the adapter config's
        base_model_name_or_path when that is a local directory), non_lora_trainables.bin is loaded over it and the adapters are merged
        into the weights on the device (W += scale * B A);
      * model_base given and no adapters (projector-only run): model_base's weights, then mm_projector.bin from model_path;
      * otherwise model_path is a full checkpoint.
    load_8bit=True (builder.py:27-31): after loading (and merging adapters, if any) the decoder's matrices are quantised to row-wise
    int8 for decoding, model.quantize_decoder_(); lm_head stays bf16 as in the reference.  quantization="int8" is the same thing;
    quantization="mxfp4" is the 4-bit mode, model.quantize_decoder_("mxfp4") (lossy: about 12 % relative error per matrix).  Any other
    string, or load_8bit=True together with "mxfp4", is a ValueError.  load_4bit is accepted and ignored.
    Geometry and mm_* / image_* settings come from model_path's config.json in every case.  The tokenizer comes from
    transformers.AutoTokenizer only when its files are in model_base or model_path."""
    from ... import lora_io
    if quantization not in (None, "int8", "mxfp4"):
        raise ValueError(f"quantization={quantization!r}: expected None, 'int8' or 'mxfp4'")
    if load_8bit and quantization == "mxfp4":
        raise ValueError("load_8bit=True and quantization='mxfp4' name two different formats: pass one of them")
    if load_8bit:
        quantization = "int8"
    if os.path.exists(os.path.join(model_path, "adapter_config.json")):
        acfg = lora_io.read_adapter_config(model_path)
        if model_base is None:
            if not (acfg.base and os.path.isdir(acfg.base)):
                raise ValueError(f"{model_path} holds LoRA adapters: pass model_base=<local directory of the base model> (the adapter "
                                 f"config names {acfg.base!r}, which is not a local directory; nothing is downloaded)")
            model_base = acfg.base
        model = _build_model(model_path, model_base, device)
        non_lora = lora_io.read_non_lora_trainables(model_path)
        if non_lora:
            _load_into(model, non_lora, "non_lora_trainables.bin")
        pairs = lora_io.adapter_pairs(lora_io.read_adapter_weights(model_path), acfg)
        dev = model.engine.device
        model.engine.merge_lora_({k: (A.to(dev), B.to(dev)) for k, (A, B) in pairs.items()}, acfg.scale)
    elif model_base is not None:
        if not os.path.exists(os.path.join(model_path, "mm_projector.bin")):
            raise FileNotFoundError(f"model_base given but {model_path} holds neither adapter_config.json nor mm_projector.bin")
        model = _build_model(model_path, model_base, device)
        _load_into(model, lora_io.read_projector(model_path), "mm_projector.bin")
    else:
        model = _build_model(model_path, model_path, device)
    if quantization is not None:
        model.quantize_decoder_(quantization)
    model.eval()
    tokenizer = None
    tok_dir = next((p for p in (model_base, model_path) if p and any(os.path.exists(os.path.join(p, f)) for f in _TOKENIZER_FILES)), None)
    if tok_dir is not None:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(tok_dir, use_fast=False, local_files_only=True)
    image_processor = None
    tower = model.get_vision_tower()
    if hasattr(tower, "image_processor"):
        image_processor = tower.image_processor
    from ...checkpoint_io import read_config
    cfg_json = read_config(model_path)
    context_len = int(cfg_json.get("tokenizer_model_max_length") or cfg_json.get("max_sequence_length") or 2048)
    return tokenizer, model, image_processor, context_len

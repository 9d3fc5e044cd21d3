"""``load_pretrained_model`` (reference finetuning/llava/model/builder.py): a model directory -> (tokenizer, model, image_processor,
context_len) for evaluation.  Here the directory is one written by ``save_pretrained`` (config.json in HF's keys + model.safetensors,
tower included) or any local HF-format LLaVA checkpoint that ``resolve_model_sources`` accepts; nothing is downloaded."""
import os
from types import SimpleNamespace

_TOKENIZER_FILES = ("tokenizer.json", "tokenizer.model", "tokenizer_config.json", "vocab.json")


def load_pretrained_model(model_path, model_base=None, model_name=None, device="cuda", **ignored):
    """Returns (tokenizer or None, model, image_processor or None, context_len).  model_base (LoRA merge) is not supported: merge the
    adapters before saving.  The tokenizer comes from transformers.AutoTokenizer only when its files are in the directory."""
    if model_base is not None:
        raise NotImplementedError("model_base (LoRA adapters over a base model): merge the adapters and save the full model first")
    from ...checkpoint_io import load_pretrained, read_config
    from ..train.train import resolve_model_sources
    from .llava_llama import LlavaConfig, LlavaLlamaForCausalLM
    from .llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    args = SimpleNamespace(model_name_or_path=model_path, vision_tower=None, geometry=None)
    geometry, lm_dir, tower_dir, is_qwen, true_vocab = resolve_model_sources(args)
    cfg_json = read_config(model_path)
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if is_qwen else (LlavaConfig, LlavaLlamaForCausalLM)
    kw = {k: cfg_json[k] for k in ("mm_patch_merge_type", "image_aspect_ratio", "image_grid_pinpoints", "tokenizer_model_max_length",
                                   "tokenizer_padding_side", "eos_token_id", "pad_token_id") if cfg_json.get(k) is not None}
    cfg = Config(geometry=geometry, rms_norm_eps=geometry["lm"].get("rms_eps", 1e-5), rope_theta=geometry["lm"].get("rope_theta", 10000.0), **kw)
    cfg._name_or_path = model_path
    model = Model(cfg, device=device, init="fast")
    if true_vocab != geometry["lm"]["vocab"]:
        model.engine.resize_token_embeddings(true_vocab)
    load_pretrained(model.engine, lm_path=lm_dir, tower_path=tower_dir)
    model.eval()
    tokenizer = None
    if any(os.path.exists(os.path.join(model_path, f)) for f in _TOKENIZER_FILES):
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(model_path, use_fast=False, local_files_only=True)
    image_processor = None
    tower = model.get_vision_tower()
    if hasattr(tower, "image_processor"):
        image_processor = tower.image_processor
    context_len = int(cfg_json.get("tokenizer_model_max_length") or cfg_json.get("max_sequence_length") or 2048)
    return tokenizer, model, image_processor, context_len

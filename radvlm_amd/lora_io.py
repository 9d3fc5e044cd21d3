"""Reading the files of a LoRA run for the merge (host code, no device).

A LoRA run saves what peft's save_pretrained leaves plus the reference's extra file (train/train.py:1708-1717): adapter_config.json,
adapter_model.bin (or adapter_model.safetensors) with keys base_model.model.<module>.lora_{A,B}[.default].weight, and
non_lora_trainables.bin (projector, image_newline) under base_model.model.* names.  load_pretrained_model(model_path, model_base=...)
reads them here, then merges W += scale * B A on the device (LlavaEngine.merge_lora_); the key handling follows the reference's
model/builder.py:58-140.  Options that change what a merge means (DoRA, trained biases, per-layer ranks, ...) are refused, not ignored.
"""
import math
import os
import re
from types import SimpleNamespace

import torch

# peft target_modules names -> the module path inside a decoder layer (the seven linears find_all_linear_names adapts, train.py:242-255)
TARGET_MODULES = {"q_proj": "self_attn.q_proj", "k_proj": "self_attn.k_proj", "v_proj": "self_attn.v_proj", "o_proj": "self_attn.o_proj",
                  "gate_proj": "mlp.gate_proj", "up_proj": "mlp.up_proj", "down_proj": "mlp.down_proj"}
MAX_RANK = 256                       # rv_lora_merge_bf16

_ADAPTER_KEY = re.compile(r"^base_model\.model\.(model\.layers\.\d+\.(?:self_attn|mlp)\.[a-z_]+)\.lora_([AB])(?:\.[A-Za-z0-9_]+)?\.weight$")


def parse_adapter_config(cfg):
    """adapter_config.json (dict) -> namespace(r, alpha, scale, targets, base).  scale = lora_alpha / r, or lora_alpha / sqrt(r) with
    use_rslora (peft LoraLayer.update_layer); targets = the adapted module paths ("self_attn.q_proj", ...)."""
    if cfg.get("peft_type", "LORA") != "LORA":
        raise NotImplementedError(f"peft_type {cfg.get('peft_type')!r}: only LoRA adapters can be merged")
    refused = [("use_dora", bool(cfg.get("use_dora"))), ("bias", cfg.get("bias", "none") not in (None, "none")),
               ("fan_in_fan_out", bool(cfg.get("fan_in_fan_out"))), ("rank_pattern", bool(cfg.get("rank_pattern"))),
               ("alpha_pattern", bool(cfg.get("alpha_pattern"))), ("layers_to_transform", cfg.get("layers_to_transform") is not None),
               ("modules_to_save", bool(cfg.get("modules_to_save")))]
    bad = [k for k, hit in refused if hit]
    if bad:
        raise NotImplementedError(f"adapter_config.json sets {bad[0]}={cfg.get(bad[0])!r}: merging such adapters is not implemented")
    r = int(cfg["r"])
    if not 1 <= r <= MAX_RANK:
        raise NotImplementedError(f"LoRA rank r={r}: the merge supports 1 <= r <= {MAX_RANK}")
    alpha = float(cfg.get("lora_alpha", 8))
    tm = cfg.get("target_modules")
    if tm == "all-linear":           # peft: every linear except the output layer
        names = list(TARGET_MODULES)
    elif isinstance(tm, (list, tuple)) and tm:
        names = [t.rsplit(".", 1)[-1] for t in tm]
    else:
        raise NotImplementedError(f"target_modules={tm!r}: give a list of module names")
    unknown = [n for n in names if n not in TARGET_MODULES]
    if unknown:
        raise NotImplementedError(f"target_modules {unknown}: only the decoder linears {sorted(TARGET_MODULES)} can be merged")
    scale = alpha / math.sqrt(r) if cfg.get("use_rslora") else alpha / r
    targets = tuple(TARGET_MODULES[n] for n in TARGET_MODULES if n in names)
    return SimpleNamespace(r=r, alpha=alpha, scale=scale, targets=targets, base=cfg.get("base_model_name_or_path"))


def read_adapter_config(path):
    import json
    with open(os.path.join(path, "adapter_config.json")) as f:
        return parse_adapter_config(json.load(f))


def adapter_pairs(sd, acfg):
    """peft adapter state dict -> {"model.layers.{i}.{module}": (A [r, in], B [out, r])}.  Raises KeyError for a key that is not a LoRA
    A / B weight of a targeted decoder linear, a module with only one of the two, or a rank other than the config's r."""
    halves = {}
    for k, t in sd.items():
        m = _ADAPTER_KEY.match(k)
        if m is None or m.group(1).split(".", 3)[3] not in acfg.targets:
            raise KeyError(f"adapter key {k!r} is not a lora_A / lora_B weight of a targeted decoder linear {acfg.targets}")
        halves.setdefault(m.group(1), {})[m.group(2)] = t
    out = {}
    for mod, ab in sorted(halves.items()):
        if set(ab) != {"A", "B"}:
            raise KeyError(f"{mod}: lora_A and lora_B must both be present")
        A, B = ab["A"], ab["B"]
        if A.dim() != 2 or B.dim() != 2 or A.shape[0] != acfg.r or B.shape[1] != acfg.r:
            raise KeyError(f"{mod}: lora_A {tuple(A.shape)} / lora_B {tuple(B.shape)} do not have rank r={acfg.r}")
        out[mod] = (A, B)
    if not out:
        raise KeyError("the adapter file holds no LoRA weights")
    return out


def read_adapter_weights(path):
    """The tensors of adapter_model.safetensors or adapter_model.bin (loaders that execute nothing from the file)."""
    st, bn = os.path.join(path, "adapter_model.safetensors"), os.path.join(path, "adapter_model.bin")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st)
    if os.path.exists(bn):
        return torch.load(bn, map_location="cpu", weights_only=True)
    raise FileNotFoundError(f"{path}: adapter_config.json without adapter_model.safetensors / adapter_model.bin")


def normalize_non_lora_keys(sd):
    """builder.py:104-106: strip 'base_model.', then 'model.' when keys start with 'model.model.'."""
    sd = {(k[len("base_model."):] if k.startswith("base_model.") else k): v for k, v in sd.items()}
    if any(k.startswith("model.model.") for k in sd):
        sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    return sd


def read_non_lora_trainables(path):
    f = os.path.join(path, "non_lora_trainables.bin")
    if not os.path.exists(f):
        return {}
    return normalize_non_lora_keys(torch.load(f, map_location="cpu", weights_only=True))


def read_projector(path):
    """mm_projector.bin of a projector-only run (train.py saves full state-dict names; a 'model.' prefix is added where absent)."""
    sd = torch.load(os.path.join(path, "mm_projector.bin"), map_location="cpu", weights_only=True)
    return {(k if k.startswith("model.") else "model." + k): v for k, v in sd.items()}

"""Host tests of the LoRA merge plumbing: the C-ABI declaration, adapter_config.json parsing, key normalisation of the adapter files and
the branch choice of load_pretrained_model (model construction stubbed: no device)."""
import json
import math
import os

import pytest
import torch

from radvlm_amd import lora_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL7 = ["q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"]


def _cfg(**kw):
    c = {"peft_type": "LORA", "r": 8, "lora_alpha": 16, "bias": "none", "target_modules": list(ALL7), "fan_in_fan_out": False,
         "layers_to_transform": None, "modules_to_save": None, "base_model_name_or_path": None}
    c.update(kw)
    return c


def test_merge_entry_point_declared_and_bound():
    from radvlm_amd import lib
    with open(os.path.join(ROOT, "include", "radvlm_hip.h")) as f:
        assert "int rv_lora_merge_bf16(void* W, int64_t ldw, const void* B, int64_t ldb, const void* A, int64_t lda" in f.read()
    assert len(lib.SIGNATURES["rv_lora_merge_bf16"][1]) == 11


def test_adapter_config_scale_and_targets():
    a = lora_io.parse_adapter_config(_cfg(r=64, lora_alpha=16))
    assert a.r == 64 and a.scale == 16 / 64 and len(a.targets) == 7
    b = lora_io.parse_adapter_config(_cfg(r=64, lora_alpha=16, use_rslora=True))
    assert b.scale == pytest.approx(16 / math.sqrt(64))
    c = lora_io.parse_adapter_config(_cfg(target_modules=["v_proj", "q_proj"]))
    assert c.targets == ("self_attn.q_proj", "self_attn.v_proj")
    assert lora_io.parse_adapter_config(_cfg(target_modules="all-linear")).targets == a.targets
    assert lora_io.parse_adapter_config(_cfg(target_modules=["model.layers.0.mlp.down_proj"])).targets == ("mlp.down_proj",)


@pytest.mark.parametrize("bad", [dict(use_dora=True), dict(bias="all"), dict(bias="lora_only"), dict(fan_in_fan_out=True),
                                 dict(rank_pattern={"q_proj": 4}), dict(alpha_pattern={"q_proj": 4}), dict(layers_to_transform=[0]),
                                 dict(modules_to_save=["lm_head"]), dict(target_modules=["lm_head"]), dict(target_modules=".*proj"),
                                 dict(r=512), dict(peft_type="IA3")])
def test_adapter_config_refused_options(bad):
    with pytest.raises(NotImplementedError):
        lora_io.parse_adapter_config(_cfg(**bad))


def _adapters(layers, mods, r=8, d=16, default=False):
    sd = {}
    for i in range(layers):
        for m in mods:
            sub = "mlp" if "proj" in m and m in ("gate_proj", "up_proj", "down_proj") else "self_attn"
            mid = ".default" if default else ""
            sd[f"base_model.model.model.layers.{i}.{sub}.{m}.lora_A{mid}.weight"] = torch.full((r, d), float(i + 1))
            sd[f"base_model.model.model.layers.{i}.{sub}.{m}.lora_B{mid}.weight"] = torch.full((d, r), -float(i + 1))
    return sd


@pytest.mark.parametrize("default", [False, True])
def test_adapter_keys_normalised(default):
    acfg = lora_io.parse_adapter_config(_cfg(target_modules=["q_proj", "v_proj"]))
    pairs = lora_io.adapter_pairs(_adapters(2, ["q_proj", "v_proj"], default=default), acfg)
    assert sorted(pairs) == ["model.layers.0.self_attn.q_proj", "model.layers.0.self_attn.v_proj", "model.layers.1.self_attn.q_proj",
                             "model.layers.1.self_attn.v_proj"]
    A, B = pairs["model.layers.1.self_attn.v_proj"]
    assert A.shape == (8, 16) and B.shape == (16, 8) and float(A[0, 0]) == 2.0 and float(B[0, 0]) == -2.0
    with pytest.raises(KeyError):      # an adapter of a module outside target_modules
        lora_io.adapter_pairs(_adapters(1, ["q_proj", "k_proj"]), acfg)
    half = _adapters(1, ["q_proj"])
    del half["base_model.model.model.layers.0.self_attn.q_proj.lora_B.weight"]
    with pytest.raises(KeyError):      # lora_A without lora_B
        lora_io.adapter_pairs(half, acfg)
    with pytest.raises(KeyError):      # rank other than r
        lora_io.adapter_pairs(_adapters(1, ["q_proj"], r=4), acfg)
    with pytest.raises(KeyError):
        lora_io.adapter_pairs({"base_model.model.model.embed_tokens.lora_embedding_A.weight": torch.zeros(8, 4)}, acfg)


def test_adapter_files_bin_and_safetensors(tmp_path):
    from safetensors.torch import save_file
    sd = _adapters(1, ALL7)
    torch.save(sd, tmp_path / "adapter_model.bin")
    got = lora_io.read_adapter_weights(str(tmp_path))
    assert set(got) == set(sd)
    st = tmp_path / "st"
    st.mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(st / "adapter_model.safetensors"))
    assert set(lora_io.read_adapter_weights(str(st))) == set(sd)
    with pytest.raises(FileNotFoundError):
        lora_io.read_adapter_weights(str(tmp_path / "nowhere"))


def test_non_lora_trainables_keys(tmp_path):
    t = torch.ones(3)
    assert set(lora_io.normalize_non_lora_keys({"base_model.model.model.mm_projector.0.bias": t, "base_model.model.model.image_newline": t})) \
        == {"model.mm_projector.0.bias", "model.image_newline"}
    assert set(lora_io.normalize_non_lora_keys({"base_model.model.mm_projector.0.bias": t})) == {"model.mm_projector.0.bias"}
    torch.save({"base_model.model.model.mm_projector.2.weight": torch.zeros(2, 2)}, tmp_path / "non_lora_trainables.bin")
    assert set(lora_io.read_non_lora_trainables(str(tmp_path))) == {"model.mm_projector.2.weight"}
    assert lora_io.read_non_lora_trainables(str(tmp_path / "x")) == {}
    torch.save({"mm_projector.0.weight": torch.zeros(2, 2), "model.mm_projector.0.bias": torch.zeros(2)}, tmp_path / "mm_projector.bin")
    assert set(lora_io.read_projector(str(tmp_path))) == {"model.mm_projector.0.weight", "model.mm_projector.0.bias"}


class _StubEngine:
    device = torch.device("cpu")

    def __init__(self, log):
        self.log = log

    def load_state_dict(self, sd, strict=False):
        self.log.append(("load", sorted(sd)))
        return [], []

    def merge_lora_(self, adapters, scale):
        self.log.append(("merge", sorted(adapters), scale))


class _StubModel:
    def __init__(self, log):
        self.engine = _StubEngine(log)

    def eval(self):
        return self

    def get_vision_tower(self):
        return object()


@pytest.fixture
def stub_build(monkeypatch):
    from radvlm_amd.llava.model import builder
    log = []

    def build(config_dir, weights_dir, device):
        log.append(("build", config_dir, weights_dir))
        return _StubModel(log)

    monkeypatch.setattr(builder, "_build_model", build)
    return builder, log


def _write(d, files):
    d.mkdir(parents=True, exist_ok=True)
    (d / "config.json").write_text(json.dumps({"tokenizer_model_max_length": 512}))
    for name, obj in files.items():
        if name.endswith(".json"):
            (d / name).write_text(json.dumps(obj))
        else:
            torch.save(obj, d / name)


def test_branch_lora(stub_build, tmp_path):
    builder, log = stub_build
    run, base = tmp_path / "run", tmp_path / "base"
    base.mkdir()
    _write(run, {"adapter_config.json": _cfg(target_modules=["q_proj", "v_proj"], r=8, lora_alpha=32), "adapter_model.bin": _adapters(1, ["q_proj", "v_proj"]),
                 "non_lora_trainables.bin": {"base_model.model.model.mm_projector.0.bias": torch.zeros(4)}})
    tok, model, proc, ctx = builder.load_pretrained_model(str(run), model_base=str(base), device="cpu")
    assert ctx == 512 and tok is None
    assert log == [("build", str(run), str(base)), ("load", ["model.mm_projector.0.bias"]),
                   ("merge", ["model.layers.0.self_attn.q_proj", "model.layers.0.self_attn.v_proj"], 4.0)]


def test_branch_lora_base_from_adapter_config(stub_build, tmp_path):
    builder, log = stub_build
    base = tmp_path / "base"
    base.mkdir()
    run = tmp_path / "run"
    _write(run, {"adapter_config.json": _cfg(base_model_name_or_path=str(base)), "adapter_model.bin": _adapters(1, ALL7)})
    builder.load_pretrained_model(str(run), device="cpu")
    assert log[0] == ("build", str(run), str(base)) and log[-1][0] == "merge" and len(log[-1][1]) == 7


@pytest.mark.parametrize("named", [None, "lmsys/vicuna-7b-v1.5"])
def test_branch_lora_without_base_raises(stub_build, tmp_path, named):
    builder, log = stub_build
    run = tmp_path / "run"
    _write(run, {"adapter_config.json": _cfg(base_model_name_or_path=named), "adapter_model.bin": _adapters(1, ALL7)})
    with pytest.raises(ValueError, match="model_base"):
        builder.load_pretrained_model(str(run), device="cpu")
    assert log == []


def test_branch_projector_only(stub_build, tmp_path):
    builder, log = stub_build
    run, base = tmp_path / "run", tmp_path / "base"
    base.mkdir()
    _write(run, {"mm_projector.bin": {"model.mm_projector.0.weight": torch.zeros(2, 2), "model.mm_projector.0.bias": torch.zeros(2)}})
    builder.load_pretrained_model(str(run), model_base=str(base), device="cpu")
    assert log == [("build", str(run), str(base)), ("load", ["model.mm_projector.0.bias", "model.mm_projector.0.weight"])]
    empty = tmp_path / "empty"
    _write(empty, {})
    with pytest.raises(FileNotFoundError):
        builder.load_pretrained_model(str(empty), model_base=str(base), device="cpu")


def test_branch_full_checkpoint(stub_build, tmp_path):
    builder, log = stub_build
    full = tmp_path / "full"
    _write(full, {})
    builder.load_pretrained_model(str(full), device="cpu")
    assert log == [("build", str(full), str(full))]


def test_engine_merge_checks_names_and_shapes():
    """merge_lora_ validates every entry before any launch (a CPU engine: the checks run on the host)."""
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.engine import LlavaEngine
    eng = LlavaEngine(GEOMETRIES["toy_qwen"], device="cpu", init=None)
    d, kvd = 256, 128
    with pytest.raises(KeyError):        # k_proj is kvd x d under grouped-query attention
        eng.merge_lora_({"model.layers.0.self_attn.k_proj": (torch.zeros(8, d), torch.zeros(d, 8))}, 1.0)
    with pytest.raises(KeyError):
        eng.merge_lora_({"model.layers.0.self_attn.q_proj": (torch.zeros(8, d), torch.zeros(d, 4))}, 1.0)
    with pytest.raises(KeyError):
        eng.merge_lora_({"lm_head": (torch.zeros(8, d), torch.zeros(1000, 8))}, 1.0)
    with pytest.raises(KeyError):
        eng.merge_lora_({"model.layers.9.self_attn.q_proj": (torch.zeros(8, d), torch.zeros(d, 8))}, 1.0)
    with pytest.raises(AssertionError):  # shapes fine: the op refuses host tensors (no CPU fall-back)
        eng.merge_lora_({"model.layers.0.self_attn.k_proj": (torch.zeros(8, d), torch.zeros(kvd, 8))}, 1.0)
    with pytest.raises(ValueError):
        eng.merge_lora()

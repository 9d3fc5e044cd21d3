"""Host tests of the int8 KV cache (no GPU): the numpy restatement (tests/kv8_ref.py) meets the per-group error bound, the keyword
kv_cache_dtype is accepted, validated or refused by the three parsers, BatchScheduler sizes its memory check and its cache with the
dtype, and the byte formula of kv_cache_bytes."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kv8_ref
import w8_ref
from radvlm_amd import lib, portable_rng
from radvlm_amd.config import GEOMETRIES
from radvlm_amd.engine import KVCache, LlavaEngine
from radvlm_amd.generation import (BatchScheduler, GenerationCache, batch_requests, parse_batch_kwargs, parse_beam_kwargs,
                                   parse_generate_kwargs)
from test_generate_batch_host import FakeEngine, HostPicker, _prompts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 128), (1, 128), (2, 64), (1, 64), (4, 128), (32, 128)]      # (Hkv, hd): the kernel tests' shapes, Qwen2-7B's and the 7B's


def _kv_rows(Hkv, hd, std, seed, M=6):
    """Gaussian bf16 K|V rows (bit patterns); group (row 1, K head 0) is zeros, group (row 2, V head Hkv - 1) has a 40 sigma outlier."""
    x = portable_rng.normal(seed, portable_rng.name_tag(f"kv8_host_{Hkv}_{hd}_{std}"), (M, 2 * Hkv * hd), std)
    x[1, :hd] = 0.0
    x[2, (2 * Hkv - 1) * hd + hd // 3] = 40.0 * std
    return w8_ref.f32_to_bf16_bits(x)


@pytest.mark.parametrize("Hkv,hd", SHAPES)
@pytest.mark.parametrize("std", [1e-3, 0.5, 30.0])
def test_dequantised_group_within_derived_bound(Hkv, hd, std):
    """|x^ - x| <= s / 2 + 2^-8 |x| elementwise, with s the scale of x's own group (tests/test_w8_host.py derives it for a row; a group
    is a row of hd entries): rint leaves at most half a step of s, and the one rounding to bf16 adds half an ulp -- 2^-9 relative -- of a
    value of magnitude at most |x| + s / 2, which 2^-8 |x| covers together with the s / 2 part of that magnitude and the fp32 roundings
    of the division and the product."""
    bits = _kv_rows(Hkv, hd, std, 3)
    q, s, xhat = kv8_ref.quantize_kv_rows(bits, Hkv, hd)
    assert q.dtype == np.int8 and q.shape == bits.shape and s.shape == (bits.shape[0], 2 * Hkv) and xhat.shape == bits.shape
    assert int(np.abs(q.astype(np.int32)).max()) <= 127
    x = w8_ref.bf16_bits_to_f32(bits).astype(np.float64)
    err = np.abs(w8_ref.bf16_bits_to_f32(xhat).astype(np.float64) - x)
    bound = np.repeat(s.astype(np.float64), hd, axis=1) / 2 + 2.0 ** -8 * np.abs(x)
    assert int((err > bound).sum()) == 0, float((err - bound).max())
    # every group's scale is its own maximum / 127, in the public column order
    amax = np.abs(w8_ref.bf16_bits_to_f32(bits)).reshape(bits.shape[0], 2 * Hkv, hd).max(axis=2)
    want = np.where(amax > 0, amax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("Hkv,hd", SHAPES)
def test_zero_group_has_unit_scale(Hkv, hd):
    bits = _kv_rows(Hkv, hd, 0.5, 4)
    q, s, xhat = kv8_ref.quantize_kv_rows(bits, Hkv, hd)
    assert s[1, 0] == np.float32(1.0) and not q[1, :hd].any() and not xhat[1, :hd].any()
    assert (s[0] != np.float32(1.0)).all() and q[1, hd:].any()


def test_restatement_is_w8_ref_per_group():
    Hkv, hd = 2, 64
    bits = _kv_rows(Hkv, hd, 0.5, 5)
    q, s, xhat = kv8_ref.quantize_kv_rows(bits, Hkv, hd)
    for m in (0, 2):
        for g in range(2 * Hkv):
            qq, ss, xx = w8_ref.quantize_rows(bits[m:m + 1, g * hd:(g + 1) * hd])
            assert np.array_equal(q[m, g * hd:(g + 1) * hd], qq[0]) and s[m, g] == ss[0] and np.array_equal(xhat[m, g * hd:(g + 1) * hd], xx[0])


# ------------------------------------------------------------------------------------------------ keyword
def test_generate_parser_takes_kv_cache_dtype():
    assert parse_generate_kwargs({}).kv_cache_dtype == "bf16"
    assert parse_generate_kwargs(dict(kv_cache_dtype=None)).kv_cache_dtype == "bf16"
    assert parse_generate_kwargs(dict(kv_cache_dtype="bf16")).kv_cache_dtype == "bf16"
    assert parse_generate_kwargs(dict(kv_cache_dtype="int8"), lookup=True).kv_cache_dtype == "int8"
    cfg = parse_generate_kwargs(dict(kv_cache_dtype="int8", do_sample=True, seed=3, top_k=5, repetition_penalty=1.2, output_scores=True,
                                     output_logits=True, return_dict_in_generate=True))
    assert cfg.kv_cache_dtype == "int8" and cfg.sampling is not None and cfg.output_logits
    for bad in ("fp8", "int4", 8, True, "INT8"):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            parse_generate_kwargs(dict(kv_cache_dtype=bad))
    with pytest.raises(NotImplementedError, match="past_key_values"):
        parse_generate_kwargs(dict(kv_cache_dtype="int8", past_key_values=GenerationCache()))
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        parse_generate_kwargs(dict(kv_cache_dtype="int8", prompt_lookup_num_tokens=3), lookup=True)
    # the bf16 spellings keep composing with both
    assert parse_generate_kwargs(dict(kv_cache_dtype="bf16", past_key_values=GenerationCache())).past_key_values is not None
    assert parse_generate_kwargs(dict(kv_cache_dtype=None, prompt_lookup_num_tokens=3), lookup=True).lookup.k == 3


def test_batch_parser_takes_kv_cache_dtype():
    assert parse_batch_kwargs({}, 3).kv_cache_dtype == "bf16"
    assert parse_batch_kwargs(dict(kv_cache_dtype="bf16"), 3).kv_cache_dtype == "bf16"
    cfg = parse_batch_kwargs(dict(kv_cache_dtype="int8", max_new_tokens=[1, 2, 3], do_sample=True, seed=[1, 2, 3]), 3)
    assert cfg.kv_cache_dtype == "int8" and cfg.budgets == [1, 2, 3]
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        parse_batch_kwargs(dict(kv_cache_dtype="fp8"), 3)


def test_beam_parser_refuses_int8_and_ignores_bf16():
    for v in (None, "bf16"):
        cfg = parse_beam_kwargs(dict(num_beams=3, kv_cache_dtype=v))
        assert cfg.num_beams == 3 and cfg.kv_cache_dtype == "bf16"
    with pytest.raises(NotImplementedError, match="beam"):
        parse_beam_kwargs(dict(num_beams=3, kv_cache_dtype="int8"))
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        parse_beam_kwargs(dict(num_beams=3, kv_cache_dtype="fp8"))


# ------------------------------------------------------------------------------------------------ scheduler
class DtypeEngine(FakeEngine):
    """The fake engine with the real engine's dtype-taking signatures: an int8 cache costs 5 bytes per position where bf16 costs 8."""

    def __init__(self, free=None):
        super().__init__(free)
        self.bytes_calls, self.cache_calls = [], []

    def kv_cache_bytes(self, B, L, dtype="bf16"):
        self.bytes_calls.append((B, L, dtype))
        return B * L * (5 if dtype == "int8" else 8)

    def new_kv_cache(self, B, L, dtype="bf16"):
        self.cache_calls.append((B, L, dtype))
        return KVCache([np.full((B, L), -7, dtype=np.int64)], np.zeros(B, np.int64), L, dtype=dtype)


def _schedule(eng, n=5, slots=2, **kw):
    ps, ims = _prompts(n, 1)
    cfg = parse_batch_kwargs(dict(kw, max_new_tokens=4, eos_token_id=None), n)
    sch = BatchScheduler(eng, batch_requests(ps, ims), cfg, slots, picker=HostPicker(cfg))
    return sch, sch.run()


def test_scheduler_passes_the_dtype_to_both_calls():
    eng = DtypeEngine()
    sch, out = _schedule(eng, kv_cache_dtype="int8")
    assert eng.bytes_calls == [(2, sch.L_max, "int8")] and eng.cache_calls == [(2, sch.L_max, "int8")]
    assert all(len(o.generated_tokens) == 4 for o in out.values())
    base = FakeEngine()                                                     # two-argument signatures: the default dtype still runs on it
    _, want = _schedule(base)
    _, same = _schedule(FakeEngine(), kv_cache_dtype="bf16")
    assert {k: v.generated_tokens for k, v in want.items()} == {k: v.generated_tokens for k, v in same.items()}
    assert {k: v.generated_tokens for k, v in want.items()} == {k: v.generated_tokens for k, v in out.items()}


def test_scheduler_memory_check_uses_the_int8_bytes():
    probe = DtypeEngine()
    sch, _ = _schedule(probe, kv_cache_dtype="int8")
    n8, n16 = 2 * sch.L_max * 5, 2 * sch.L_max * 8
    _schedule(DtypeEngine(free=n8), kv_cache_dtype="int8")                  # fits exactly
    with pytest.raises(ValueError, match=f"needs {n8} bytes"):
        _schedule(DtypeEngine(free=n8 - 1), kv_cache_dtype="int8")
    with pytest.raises(ValueError, match=f"needs {n16} bytes"):            # the same memory does not hold the bf16 cache
        _schedule(DtypeEngine(free=n8))


# ------------------------------------------------------------------------------------------------ bytes
@pytest.mark.parametrize("gname", ["toy", "toy_qwen", "llava15_7b", "llava_ov_qwen2_7b"])
def test_kv_cache_bytes_formula(gname):
    l = GEOMETRIES[gname]["lm"]
    hd = l["d"] // l["heads"]
    Hkv = l.get("kv_heads", l["heads"])
    kvd = Hkv * hd
    stub = SimpleNamespace(l=l, kvd=kvd, Hkv=Hkv, hd=hd, kv8_decode=True, _kv_dtype=LlavaEngine._kv_dtype)
    B, L_max = 3, 37
    assert LlavaEngine.kv_cache_bytes(stub, B, L_max) == l["layers"] * B * L_max * 4 * kvd
    assert LlavaEngine.kv_cache_bytes(stub, B, L_max, "bf16") == l["layers"] * B * L_max * 4 * kvd
    assert LlavaEngine.kv_cache_bytes(stub, B, L_max, "int8") == l["layers"] * B * L_max * (2 * kvd + 8 * Hkv)
    stub.kv8_decode = False                                                 # the reference arm stores the dequantised bf16 values
    assert LlavaEngine.kv_cache_bytes(stub, B, L_max, "int8") == l["layers"] * B * L_max * 4 * kvd
    with pytest.raises(ValueError):
        LlavaEngine.kv_cache_bytes(stub, B, L_max, "fp8")
    if gname == "llava15_7b":
        assert 2 * kvd + 8 * Hkv == 8448 and 4 * kvd == 16384
    if gname == "llava_ov_qwen2_7b":
        assert 2 * kvd + 8 * Hkv == 1056 and 4 * kvd == 2048


def test_kvcache_counts_and_grows_both_tensors():
    layers = [torch.zeros(2, 5, 16, dtype=torch.int8) for _ in range(3)]
    scales = [torch.ones(2, 5, 4, dtype=torch.float32) for _ in range(3)]
    scales[1][1, 2, 3] = 7.0
    layers[1][1, 2, 9] = -5
    c = KVCache(layers, np.array([3, 1]), 5, dtype="int8", scales=scales)
    assert c.dtype == "int8" and c.nbytes() == 3 * 2 * 5 * (16 + 4 * 4)
    c.grow(9, 3)
    assert c.L_max == 9 and c.nbytes() == 3 * 2 * 9 * (16 + 4 * 4)
    assert c.layers[1].shape == (2, 9, 16) and c.scales[1].shape == (2, 9, 4)
    assert c.scales[1][1, 2, 3] == 7.0 and c.layers[1][1, 2, 9] == -5
    plain = KVCache([torch.zeros(2, 5, 16, dtype=torch.bfloat16)], np.zeros(2), 5)
    assert plain.dtype == "bf16" and plain.scales is None and plain.nbytes() == 2 * 5 * 16 * 2


# ------------------------------------------------------------------------------------------------ plumbing
def test_entry_points_declared_and_bound():
    assert {"rv_kv_quantize_rows_bf16", "rv_kv_append_q8_bf16", "rv_attn_decode_kv8_bf16"} <= set(lib.SIGNATURES)
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "kvq" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build


def test_public_surface():
    import inspect
    from radvlm_amd import ops
    from radvlm_amd.llava.model.llava_llama import LlavaLlamaForCausalLM
    assert LlavaEngine.kv8_decode is True
    assert inspect.signature(LlavaEngine.new_kv_cache).parameters["dtype"].default == "bf16"
    assert inspect.signature(LlavaEngine.kv_cache_bytes).parameters["dtype"].default == "bf16"
    assert inspect.signature(LlavaEngine.prefill).parameters["kv_dtype"].default is None
    assert callable(ops.kv_quantize_rows) and callable(ops.kv_append_q8) and callable(ops.attn_decode_kv8)
    assert list(inspect.signature(ops.attn_decode_kv8).parameters) == list(inspect.signature(ops.attn_decode).parameters)
    for fn in (LlavaLlamaForCausalLM.generate, LlavaLlamaForCausalLM.generate_batch, LlavaLlamaForCausalLM.generate_beams):
        assert "kv_cache_dtype" in fn.__doc__

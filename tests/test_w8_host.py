"""Host tests of the int8 decoder weights (no GPU): the numpy restatement of the quantised weight (tests/w8_ref.py) meets the derived
error bound, and the argument plumbing of load_8bit / quantize_decoder_ / the two entry points is in place."""
import inspect
import os

import numpy as np
import pytest

import w8_ref
from radvlm_amd import lib, portable_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(K, std, seed):
    """Gaussian bf16 rows of K entries (bit patterns): 6 plain rows, one with a planted 40 sigma outlier, one of zeros."""
    w = portable_rng.normal(seed, portable_rng.name_tag(f"w8_host_{K}_{std}"), (8, K), std)
    w[6, K // 3] = 40.0 * std
    w[7] = 0.0
    return w8_ref.f32_to_bf16_bits(w)


CASES = [(K, std) for K in (448, 4096, 11008) for std in (1e-3, 0.02, 1.0)]


@pytest.mark.parametrize("K,std", CASES)
def test_q_range_and_row_maximum(K, std):
    bits = _rows(K, std, 1)
    q, s, _ = w8_ref.quantize_rows(bits)
    w = w8_ref.bf16_bits_to_f32(bits)
    assert q.dtype == np.int8 and int(np.abs(q.astype(np.int32)).max()) <= 127
    for r in range(7):
        j = int(np.abs(w[r]).argmax())
        assert int(q[r, j]) == (127 if w[r, j] > 0 else -127), (r, j)
        assert s[r] == np.float32(np.abs(w[r]).max()) / np.float32(127.0)


@pytest.mark.parametrize("K,std", CASES)
def test_zero_row_has_unit_scale(K, std):
    q, s, what = w8_ref.quantize_rows(_rows(K, std, 2))
    assert s[7] == np.float32(1.0) and not q[7].any() and not what[7].any()


@pytest.mark.parametrize("K,std", CASES)
def test_dequantised_weight_within_derived_bound(K, std):
    """|W^ - w| <= s / 2 + 2^-8 |w| elementwise: half a quantisation step, plus bf16's half-ulp on a value of magnitude at most
    |w| + s / 2 (a half-ulp is 2^-9 relative, so 2^-8 |w| also covers the s / 2 part of that magnitude and the fp32 roundings)."""
    bits = _rows(K, std, 3)
    _, s, what = w8_ref.quantize_rows(bits)
    w = w8_ref.bf16_bits_to_f32(bits).astype(np.float64)
    err = np.abs(w8_ref.bf16_bits_to_f32(what).astype(np.float64) - w)
    bound = s.astype(np.float64)[:, None] / 2 + 2.0 ** -8 * np.abs(w)
    assert int((err > bound).sum()) == 0, float((err - bound).max())


def test_ties_round_to_even():
    """A row whose maximum is 127 * 2^e has s = 2^e exactly, and (n + 1/2) 2^e is a bf16 number for small n: q is the even neighbour."""
    e = -6
    vals = np.array([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5], np.float32) * np.float32(2.0 ** e)
    q, s, what = w8_ref.quantize_rows(w8_ref.f32_to_bf16_bits(vals)[None])
    assert s[0] == np.float32(2.0 ** e)
    assert q[0].tolist() == [127, 0, 2, 2, 0, -2, -2, 4]
    assert np.array_equal(w8_ref.bf16_bits_to_f32(what[0]), q[0].astype(np.float32) * s[0])


def test_bf16_rounding_restatement_matches_torch():
    import torch
    x = portable_rng.normal(5, 77, (4096,), 3.0)
    x[:4] = [0.0, 1.00390625, 1.01171875, -1.00390625]           # exact ties: 1 + 2^-8 (down to even), 1 + 3 * 2^-8 (up to even)
    got = w8_ref.f32_to_bf16_bits(x)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("K", [8, 32, 40, 64, 96, 448, 4096, 11008])
def test_packed_layout_round_trip(K):
    from radvlm_amd import ops
    q = portable_rng.integers(7, K, (3, K), -127, 128).astype(np.int8)
    p = w8_ref.pack_rows(q)
    assert p.shape == (3, w8_ref.packed_row_bytes(K)) and p.shape[1] % 64 == 0 and p.shape[1] >= K
    assert ops.w8_row_bytes(K) == w8_ref.packed_row_bytes(K)
    assert np.array_equal(w8_ref.unpack_rows(p, K), q)
    # lane group g's 16 bytes of pair 0: its 8 weights of step 0, then of step 1
    if K >= 64:
        assert np.array_equal(p[:, 16:24], q[:, 8:16]) and np.array_equal(p[:, 24:32], q[:, 40:48])


def test_entry_points_declared_and_bound():
    assert {"rv_quantize_rows_w8_bf16", "rv_gemv_w8_bf16", "rv_w8_row_bytes"} <= set(lib.SIGNATURES)
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "gemv" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if os.path.exists(so):
        l = lib.load()
        for K in (8, 32, 40, 4096, 11008, 18944):
            assert int(l.rv_w8_row_bytes(K)) == w8_ref.packed_row_bytes(K)


def test_public_surface():
    from radvlm_amd import ops
    from radvlm_amd.engine import LlavaEngine
    from radvlm_amd.llava.model.builder import load_pretrained_model
    from radvlm_amd.llava.model.llava_llama import LlavaLlamaForCausalLM
    from radvlm_amd.llava.model.llava_qwen import LlavaQwenForCausalLM
    sig = inspect.signature(load_pretrained_model)
    assert sig.parameters["load_8bit"].default is False
    assert callable(ops.quantize_rows_w8) and callable(ops.gemv_w8)
    assert list(inspect.signature(ops.gemv_w8).parameters)[:4] == ["x", "packed", "scale", "K"]
    assert list(inspect.signature(ops.gemv_w8).parameters)[4:] == list(inspect.signature(ops.gemv).parameters)[2:]
    assert callable(LlavaEngine.quantize_decoder_) and LlavaEngine.w8_decode is True
    for cls in (LlavaLlamaForCausalLM, LlavaQwenForCausalLM):
        assert callable(cls.quantize_decoder_) and isinstance(cls.is_quantized, property)

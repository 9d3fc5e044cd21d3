"""Host tests of the MXFP4 decoder weights (no GPU): the numpy restatement of the quantised weight (tests/w4_ref.py) gives bf16
numbers, is idempotent, meets the elementwise bound and the measured Frobenius error, its packed layout round-trips, and the argument
plumbing of quantization="mxfp4" / quantize_decoder_(fmt) / the entry points is in place."""
import inspect
import os

import numpy as np
import pytest

import w4_ref
from radvlm_amd import lib, portable_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(K, std, seed):
    """Gaussian bf16 rows of K entries (bit patterns): 6 plain rows, one with a planted 40 sigma outlier, one of zeros."""
    w = portable_rng.normal(seed, portable_rng.name_tag(f"w4_host_{K}_{std}"), (8, K), std)
    w[6, K // 3] = 40.0 * std
    w[7] = 0.0
    return w4_ref.f32_to_bf16_bits(w)


CASES = [(K, std) for K in (40, 416, 4096) for std in (1e-3, 0.02, 1.0)]


@pytest.mark.parametrize("K,std", CASES)
def test_quantised_weight_is_a_bf16_number_and_idempotent(K, std):
    bits = _rows(K, std, 1)
    nib, sb, what = w4_ref.quantize_rows(bits)
    assert nib.dtype == np.uint8 and int(nib.max()) <= 15 and not (nib == 8).any()           # never "-0"
    # W^ by floating-point arithmetic on (code, e) is the same bf16 number: rounding it to bf16 changes nothing
    val = w4_ref.dequantize(nib, sb)
    assert np.array_equal(w4_ref.f32_to_bf16_bits(val), what) and np.array_equal(w4_ref.bf16_bits_to_f32(what), val)
    n2, s2, w2 = w4_ref.quantize_rows(what)
    assert np.array_equal(w2, what) and np.array_equal(n2, nib) and np.array_equal(s2, sb)   # a block's maximum keeps its binade
    assert sb[7].tolist() == [127] * sb.shape[1] and not nib[7].any() and not what[7].any()   # the zero row


@pytest.mark.parametrize("K,std", CASES)
def test_scale_is_the_block_maximum_exponent_minus_two(K, std):
    bits = _rows(K, std, 2)
    nib, sb, _ = w4_ref.quantize_rows(bits)
    w = np.abs(w4_ref.bf16_bits_to_f32(bits))
    for r in range(7):
        for j in range(sb.shape[1]):
            blk = w[r, 32 * j:32 * j + 32]                                                     # the last block may be short
            e = int(np.floor(np.log2(float(blk.max())))) - 2
            assert int(sb[r, j]) == e + 127, (r, j)
            top = int(nib[r, 32 * j + int(blk.argmax())] & 7)
            assert top in (6, 7), (r, j, top)                                                  # the maximum lands in [4, 8) 2^e


@pytest.mark.parametrize("K,std", CASES)
def test_elementwise_bound(K, std):
    """|W^ - w| <= 2^e below saturation (the widest gap between neighbouring values, 4 to 6, is 2, so nearest is within 1), and
    <= 2 * 2^e at saturation (a < 8 meets 6)."""
    bits = _rows(K, std, 3)
    nib, sb, what = w4_ref.quantize_rows(bits)
    w = w4_ref.bf16_bits_to_f32(bits).astype(np.float64)
    err = np.abs(w4_ref.bf16_bits_to_f32(what).astype(np.float64) - w)
    ulp = np.ldexp(1.0, np.repeat(sb.astype(np.int32) - 127, 32, axis=1)[:, :K])
    sat = np.abs(w) > 6 * ulp
    assert int((err[~sat] > ulp[~sat]).sum()) == 0 and int((err[sat] > 2 * ulp[sat]).sum()) == 0
    assert ((nib & 7)[sat] == 7).all()


def test_nearest_value_with_ties_to_the_even_code():
    """Brute force over a = bf16(j / 64) in (0, 7.5]: the code is a nearest value; where two are equally near, the even code."""
    j = np.arange(1, 481, dtype=np.float32)
    vals = np.concatenate([[np.float32(7.5)], j / np.float32(64.0)])[None]                    # block maximum 7.5: e = 0
    for lo in range(0, 480, 31):                                                               # blocks of 32 with the maximum first
        blk = np.concatenate([vals[:, :1], vals[:, 1 + lo:32 + lo]], axis=1)
        bits = w4_ref.f32_to_bf16_bits(blk)                                                    # j / 64 is rounded to bf16 at 2 and above
        nib, sb, _ = w4_ref.quantize_rows(bits)
        assert sb[0, 0] == 127
        for a, c in zip(w4_ref.bf16_bits_to_f32(bits[0]).tolist(), (nib[0] & 7).tolist()):
            d = np.abs(w4_ref.VALUES.astype(np.float64) - a)
            near = np.flatnonzero(d == d.min())
            assert c in near and (len(near) == 1 or c % 2 == 0), (a, c)
    tie = np.array([4, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5], np.float32) * np.float32(2.0 ** -9)
    nib, sb, what = w4_ref.quantize_rows(w4_ref.f32_to_bf16_bits(tie[None]))
    assert sb[0, 0] == 127 - 9
    assert nib[0].tolist() == [6, 0, 2, 2, 4, 4, 6, 6, 0, 8 | 2, 8 | 2, 8 | 4, 8 | 4, 8 | 6, 8 | 6]
    assert what[0, 8] == 0 and what[0, 1] == 0                                                  # -0.25 -> +0.0


# Relative Frobenius error of W^ on Gaussian rows (64 rows, K = 4096, this file's generator): measured 0.1135 (std 0.02) and 0.1151
# (std 1) on plain rows, 0.1179 and 0.1588 with a 40 sigma outlier per row (40 lands on the 4|6 tie of its block at std 1 and loses 8);
# int8 gives 0.010 to 0.013 on the same rows.  Gated at 1.25x the measured value, as the full-size gates are.
FROB = {(0.02, False): 0.1135, (1.0, False): 0.1151, (0.02, True): 0.1179, (1.0, True): 0.1588}


@pytest.mark.parametrize("std,outlier", sorted(FROB))
def test_relative_frobenius_error_on_gaussian_rows(std, outlier):
    w = portable_rng.normal(1, 5, (64, 4096), std)
    if outlier:
        w[:, 4096 // 3] = 40 * std
    bits = w4_ref.f32_to_bf16_bits(w)
    _, _, what = w4_ref.quantize_rows(bits)
    w0 = w4_ref.bf16_bits_to_f32(bits).astype(np.float64)
    rel = float(np.linalg.norm(w4_ref.bf16_bits_to_f32(what).astype(np.float64) - w0) / np.linalg.norm(w0))
    print(f"std {std} outlier {outlier}: relative Frobenius error {rel:.4f}")
    assert rel <= 1.25 * FROB[(std, outlier)]
    assert rel > 0.05                                                                          # a lossy format: nobody should read it as int8-like


@pytest.mark.parametrize("K", [8, 40, 416, 4096])
def test_packed_layout_round_trip(K):
    from radvlm_amd import ops
    nib = portable_rng.integers(7, K, (3, K), 0, 16).astype(np.uint8)
    sb = portable_rng.integers(8, K, (3, w4_ref.steps(K)), 5, 250).astype(np.uint8)
    p, s = w4_ref.pack_rows(nib, sb)
    assert p.shape == (3, w4_ref.packed_row_bytes(K)) and p.shape[1] % 64 == 0 and 2 * p.shape[1] >= K
    assert s.shape == (3, w4_ref.scale_row_bytes(K)) and s.shape[1] % 4 == 0 and (s[:, w4_ref.steps(K):] == 127).all()
    assert ops.w4_row_bytes(K) == w4_ref.packed_row_bytes(K) and ops.w4_scale_row_bytes(K) == w4_ref.scale_row_bytes(K)
    a, b = w4_ref.unpack_rows(p, s, K)
    assert np.array_equal(a, nib) and np.array_equal(b, sb)
    # lane group 1's first dword of quad 0: weights k = 8 .. 15 of step 0, weight i in bits 4 i .. 4 i + 3
    if K >= 16:
        dword = p[:, 16:20].astype(np.uint32) @ (np.uint32(1) << (8 * np.arange(4, dtype=np.uint32)))
        assert all(np.array_equal((dword >> np.uint32(4 * i)) & 15, nib[:, 8 + i]) for i in range(8))
    if K >= 40:                                                                                 # lane group 0's dword of step 1
        assert np.array_equal(p[:, 4] & 15, nib[:, 32]) and np.array_equal(p[:, 4] >> 4, nib[:, 33])


def test_entry_points_declared_and_bound():
    assert {"rv_quantize_rows_mxfp4_bf16", "rv_gemv_w4_bf16", "rv_w4_row_bytes", "rv_w4_scale_row_bytes"} <= set(lib.SIGNATURES)
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "gemv" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if os.path.exists(so):
        l = lib.load()
        for K in (8, 32, 40, 416, 4096, 11008, 18944):
            assert int(l.rv_w4_row_bytes(K)) == w4_ref.packed_row_bytes(K)
            assert int(l.rv_w4_scale_row_bytes(K)) == w4_ref.scale_row_bytes(K)


def test_public_surface():
    from radvlm_amd import ops
    from radvlm_amd.engine import LlavaEngine
    from radvlm_amd.llava.model.builder import load_pretrained_model
    from radvlm_amd.llava.model.llava_llama import LlavaLlamaForCausalLM
    from radvlm_amd.llava.model.llava_qwen import LlavaQwenForCausalLM
    sig = inspect.signature(load_pretrained_model)
    assert sig.parameters["quantization"].default is None and sig.parameters["load_8bit"].default is False
    assert callable(ops.quantize_rows_mxfp4) and callable(ops.gemv_w4)
    assert list(inspect.signature(ops.gemv_w4).parameters)[:4] == ["x", "packed", "scales", "K"]
    assert list(inspect.signature(ops.gemv_w4).parameters)[4:] == list(inspect.signature(ops.gemv).parameters)[2:]
    assert inspect.signature(LlavaEngine.quantize_decoder_).parameters["fmt"].default == "int8"
    assert LlavaEngine.w4_decode is True and LlavaEngine.w8_decode is True
    for cls in (LlavaLlamaForCausalLM, LlavaQwenForCausalLM):
        assert inspect.signature(cls.quantize_decoder_).parameters["fmt"].default == "int8"


def test_router_table_is_the_record():
    """LlavaEngine.W4_BF16_CELLS holds exactly the (shape, M) cells of the committed per-shape record (default build) in which the 4-bit
    kernel did not beat the bf16 kernel by more than that arm's spread, and no cell left with the 4-bit kernel is slower on it."""
    import json
    from radvlm_amd.engine import LlavaEngine
    recs = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "decode_ab_gemv.jsonl"))]
    recs = [r for r in recs if r.get("mode") == "w4" and r.get("build") == "default"]
    assert len(recs) == 8 * 5 and {r["M"] for r in recs} == {1, 4, 8, 16, 32}
    want = {}
    for r in recs:
        assert r["w4_faster_by_more_than_bf16_spread"] == (r["bf16_us"] - r["w4_us"] > r["bf16_max_us"] - r["bf16_min_us"])
        if not r["w4_faster_by_more_than_bf16_spread"]:
            want.setdefault((r["N"], r["K"]), []).append(r["M"])
        else:
            assert r["w4_us"] < r["bf16_us"], r
    assert {k: tuple(sorted(v)) for k, v in want.items()} == LlavaEngine.W4_BF16_CELLS
    eng = LlavaEngine.__new__(LlavaEngine)                                                      # the lookup alone: no device, no weights
    assert eng._w4_cell_takes_bf16(4608, 3584, 3) and eng._w4_cell_takes_bf16(12288, 4096, 1)
    assert not eng._w4_cell_takes_bf16(12288, 4096, 2) and not eng._w4_cell_takes_bf16(22016, 4096, 32)
    assert eng._w4_cell_takes_bf16(4096, 4096, 9) and not eng._w4_cell_takes_bf16(4096, 4096, 8) and not eng._w4_cell_takes_bf16(640, 128, 1)


def test_loader_refuses_unknown_and_contradictory_formats(tmp_path):
    """The format is checked before anything is read: no checkpoint and no GPU needed."""
    from radvlm_amd.llava.model.builder import load_pretrained_model
    with pytest.raises(ValueError, match="quantization"):
        load_pretrained_model(str(tmp_path), quantization="nf4")
    with pytest.raises(ValueError, match="load_8bit"):
        load_pretrained_model(str(tmp_path), load_8bit=True, quantization="mxfp4")

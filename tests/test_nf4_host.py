"""CPU checks of the NF4 frozen base's definition: the committed table against tests/nf4_ref.py, the midpoint rule at the midpoints'
neighbours, the round trip of dequantised weights, packing at odd lengths, the fixed-order mean of double quantisation, the byte
accounting and alignment of radvlm_amd/nf4.py's BasePlan, and the reading of --bits / --quant_type / --lora_enable."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam8_ref
import nf4_ref as R
from radvlm_amd import nf4 as N
from radvlm_amd.config import GEOMETRIES

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ tables
def test_header_table_is_the_reference_table():
    t = N.read_table()
    assert t.dtype == np.float32 and t.shape == (16,)
    assert np.array_equal(t.view(np.uint32), R.TABLE.view(np.uint32))
    assert np.all(np.diff(t) > 0) and t[7] == 0 and t[0] == -1 and t[15] == 1
    assert np.array_equal(N.midpoints(t).view(np.uint32), R.MID.view(np.uint32)) and np.all(np.diff(R.MID) > 0)


def test_codebook_sha_is_of_both_tables():
    import hashlib
    from radvlm_amd import optim8
    want = hashlib.sha256(N.read_table().astype("<f4").tobytes() + optim8.read_codebook()[0].astype("<f4").tobytes()).hexdigest()
    assert N.codebook_sha() == want
    rec = N.base_quant_record(True)
    assert rec == {"type": "nf4", "block": 64, "double_quant": True, "codebook": want}


def test_the_kernels_are_built_declared_and_under_the_scratch_gate():
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "nf4" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    from radvlm_amd import lib
    for name, nargs in (("rv_nf4_quantize_bf16", 5), ("rv_nf4_dequant_bf16", 10)):
        assert len(lib.SIGNATURES[name][1]) == nargs, name
    src = open(os.path.join(ROOT, "radvlm_amd", "csrc", "nf4.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")


# ------------------------------------------------------------------------------------------------ the midpoint rule
def test_midpoint_rule_at_the_neighbours_of_every_midpoint():
    """A value exactly at a midpoint takes the LOWER code (strictly below), one ulp above it the upper one."""
    below, above = np.nextafter(R.MID, F32(-np.inf)), np.nextafter(R.MID, F32(np.inf))
    for i in range(15):
        x = np.array([1.0, below[i], R.MID[i], above[i]], F32)          # absmax 1: a = x
        codes, absmax = R.codes_of(x)
        assert absmax[0] == 1 and codes.tolist() == [15, i, i, i + 1]


def test_midpoint_rule_is_not_nearest_in_float64():
    """Where the exact float64 midpoint is not an fp32 number, an fp32 neighbour of the rounded midpoint lies on the other side of
    the exact one: "nearest level in float64" gives another code there, and the rule here is the midpoint rule."""
    t64 = R.TABLE.astype(np.float64)
    exact = (t64[:-1] + t64[1:]) / 2
    inexact = np.flatnonzero(R.MID.astype(np.float64) != exact)
    assert inexact.size > 0
    differs = 0
    for i in inexact:
        m = R.MID[i]
        # the fp32 midpoint itself: the rule gives code i; nearest-in-float64 gives i + 1 when the rounded midpoint is above the exact one
        nearest = int(np.argmin(np.abs(t64 - np.float64(m))))
        rule = int(R.codes_of(np.array([1.0, m], F32))[0][1])
        assert rule == i
        differs += nearest != rule
    assert differs > 0


# ------------------------------------------------------------------------------------------------ round trip, packing
@pytest.mark.parametrize("name", list(R.host_inputs()))
def test_quantising_the_dequantised_weights_gives_the_same_store(name):
    """Without double quantisation: the block maximum is bf16-exact (level +-1 times absmax), every other dequantised value sits within
    2^-9 relative of a level times absmax, far from any midpoint (the closest pair of levels is 0.0796 apart)."""
    x = R.host_inputs()[name]
    packed, absmax = R.quantize(x)
    deq = R.bf16_to_f32(R.dequantize(packed, absmax, x.size))
    packed2, absmax2 = R.quantize(deq)
    assert np.array_equal(absmax.view(np.uint32), absmax2.view(np.uint32))
    assert np.array_equal(packed, packed2)
    assert np.array_equal(R.dequantize(packed2, absmax2, x.size), R.bf16_bits(deq))


@pytest.mark.parametrize("n", R.LENGTHS)
def test_lengths_pack_and_unpack(n):
    x = R.host_inputs()[f"n{n}"]
    codes, absmax = R.codes_of(x)
    packed = R.pack(codes)
    assert packed.size == (n + 1) // 2 and absmax.size == (n + 63) // 64
    assert np.array_equal(R.unpack(packed, n), codes)
    assert int(packed[0] >> 4) == int(codes[0])                            # element 0 in the high nibble
    if n & 1:
        assert packed[-1] & 15 == 0 and int(packed[-1] >> 4) == int(codes[-1])
    else:
        assert int(packed[-1] & 15) == int(codes[-1])


def test_special_blocks():
    z = R.host_inputs()["zero_and_single"]
    codes, absmax = R.codes_of(z)
    assert absmax[1] == 0 and np.all(codes[64:128] == 7)                   # the all-zero block divides by 1 and takes the level 0
    assert absmax[2] == F32(0.375) and codes[128 + 17] == 0 and np.all(np.delete(codes[128:192], 17) == 7)
    e = R.host_inputs()["max_at_ends"]
    codes, absmax = R.codes_of(e)
    assert absmax.tolist() == [0.5, 0.25, 2.0, 2.0]
    assert (codes[0], codes[63], codes[64], codes[127], codes[191], codes[192]) == (15, 0, 0, 15, 15, 0)
    deq = R.bf16_to_f32(R.dequantize(R.pack(codes), absmax, e.size))
    assert deq[0] == 0.5 and deq[63] == -0.5 and deq[191] == 2.0 and deq[192] == -2.0


# ------------------------------------------------------------------------------------------------ double quantisation
def test_offset_is_the_left_to_right_float64_mean():
    r = np.random.RandomState(3)
    am = np.abs(r.randn(70001)).astype(F32) * F32(0.07)
    ref = R.absmax_offset(am)
    assert N.absmax_offset(am).view(np.uint32) == ref.view(np.uint32)
    s = np.float64(0)
    for v in am:
        s = s + np.float64(v)
    assert ref == F32(s / am.size)


def test_double_quantisation_is_the_signed_8bit_scheme_on_absmax_minus_offset():
    x = R.host_inputs()[f"n{64 * 256 + 63}"]
    _, absmax = R.quantize(x)
    assert absmax.size == 257                                              # a short last second-level block of one entry
    codes2, scale2, off = R.double_quantize(absmax)
    want_c, want_s = adam8_ref.quantize((absmax - off).astype(F32), adam8_ref.SIGNED)
    assert np.array_equal(codes2, want_c) and np.array_equal(scale2, want_s) and scale2.size == 2
    eff = R.effective_absmax(codes2, scale2, off)
    q8 = adam8_ref.codebook(adam8_ref.SIGNED)
    assert eff[256] == F32(F32(q8[codes2[256]] * scale2[1]) + off)
    assert np.all(np.abs(eff - absmax) <= 0.05 * absmax.max()) and not np.array_equal(eff, absmax)


# ------------------------------------------------------------------------------------------------ the plan
def _check_plan(geo, dq):
    plan = N.BasePlan(geo, dq)
    l = geo["lm"]
    d, F = l["d"], l["ffn"]
    kvd = d // l["heads"] * l.get("kv_heads", l["heads"])
    per_layer = d * d * 2 + 2 * kvd * d + 3 * F * d
    assert plan.weights == l["layers"] * per_layer and len(plan.tensors) == 7 * l["layers"]
    assert list(plan.tensors) == N.matrix_names(geo)
    code_end = blk_end = s2_end = 0
    for name, t in plan.tensors.items():
        assert t["code"] % 16 == 0 and t["code"] >= code_end                 # 16-byte alignment of every tensor's codes ...
        assert (t["block"] * (1 if dq else 4)) % 16 == 0 and t["block"] >= blk_end      # ... and of its absmax entries (bytes or fp32)
        assert t["nblocks"] == -(-t["n"] // 64) and t["n"] == int(np.prod(t["shape"]))
        code_end, blk_end = t["code"] + (t["n"] + 1) // 2, t["block"] + t["nblocks"]
        if dq:
            assert (t["scale2"] * 4) % 16 == 0 and t["scale2"] >= s2_end and t["nscale2"] == -(-t["nblocks"] // 256)
            s2_end = t["scale2"] + t["nscale2"]
        assert t["dst"] % 8 == 0 and t["dst"] + t["n"] <= plan.scratch_numel
    assert plan.code_bytes == code_end and plan.nblocks == blk_end and plan.nscale2 == s2_end
    p = "model.layers.1."
    T = plan.tensors
    q, k, v = (T[p + f"self_attn.{m}_proj.weight"] for m in "qkv")
    assert k["dst"] == q["dst"] + q["n"] and v["dst"] == k["dst"] + k["n"]     # the fused q|k|v view is contiguous
    g, u = T[p + "mlp.gate_proj.weight"], T[p + "mlp.up_proj.weight"]
    assert u["dst"] == g["dst"] + g["n"]
    assert T["model.layers.0.mlp.down_proj.weight"]["dst"] == T[p + "mlp.down_proj.weight"]["dst"]      # one scratch for every layer
    spans = sorted((t["dst"], t["dst"] + t["n"]) for t in T.values() if t["layer"] == 0)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for i in range(l["layers"]):
        tab, nch = plan.table(plan.names(i))
        assert tab.shape == (6, 7) and tab.dtype == np.int64 and nch == sum(-(-T[n]["n"] // N.CHUNK) for n in plan.names(i))
        assert tab[0, 0] == 0 and np.array_equal(tab[0, 1:], np.cumsum(-(-tab[3] // N.CHUNK))[:-1])
    return plan


@pytest.mark.parametrize("dq", [False, True])
def test_plan_bytes_at_7b(dq):
    geo = GEOMETRIES["llava15_7b"]
    plan = _check_plan(geo, dq)
    w = plan.weights
    assert w == 32 * (4 * 4096 * 4096 + 3 * 4096 * 11008)
    if not dq:
        assert plan.base_weight_bytes() * 8 == w * 4.5 * 1                 # exactly 4.5 bits per matrix weight
    else:
        assert plan.base_weight_bytes() == w // 2 + w // 64 + 4 * (w // 16384) + 4 * 7 * 32       # 4 + 8/64 + 32/16384 bits, + 4 B per tensor
    assert N.base_weight_bytes(geo, "nf4", dq) == plan.base_weight_bytes() and N.base_weight_bytes(geo) == 2 * w
    assert plan.scratch_bytes() == 2 * (4 * 4096 * 4096 + 3 * 4096 * 11008)
    with pytest.raises(ValueError):
        N.base_weight_bytes(geo, "fp4")


@pytest.mark.parametrize("name", ["toy", "toy_qwen", "llava15_13b"])
@pytest.mark.parametrize("dq", [False, True])
def test_plans_are_consistent_with_their_shapes(name, dq):
    from radvlm_amd.params import lm_param_shapes
    geo = GEOMETRIES[name]
    plan = _check_plan(geo, dq)
    shapes = lm_param_shapes(geo)
    for n, t in plan.tensors.items():
        assert tuple(shapes[n]) == tuple(t["shape"])
    assert plan.base_weight_bytes() < 0.3 * N.bf16_matrix_bytes(geo)


# ------------------------------------------------------------------------------------------------ --bits / --quant_type / --lora_enable
def test_trainer_arguments_select_the_act():
    from radvlm_amd.llava.train.train import TrainingArguments
    f = TrainingArguments.__dataclass_fields__
    assert (f["bits"].default, f["quant_type"].default, f["double_quant"].default) == (16, "nf4", True)
    said = []
    assert N.base_quant_choice(4, "nf4", True, said.append) == "nf4" and not said
    assert N.base_quant_choice(16, "nf4", True, said.append) is None and N.base_quant_choice(16, "nf4", False, said.append) is None
    assert not said                                                         # --bits 16 is untouched and silent
    for args, word in (((8, "nf4", True), "--bits 8"), ((4, "fp4", True), "fp4"), ((4, "nf4", False), "without --lora_enable")):
        said.clear()
        assert N.base_quant_choice(*args, said.append) is None
        assert len(said) == 1 and word in said[0] and "bf16 base" in said[0]
    assert N.base_quant_choice(8, "nf4", True) is None                      # no callable: nothing to tell


def test_the_refusal_table_has_the_nf4_row():
    from radvlm_amd.generation import FEATURES, REFUSALS, refuse_combinations
    rows = [r for r in REFUSALS if r[0] == "nf4"]
    assert len(rows) == 1 and rows[0][1] is None and "nf4" in FEATURES
    with pytest.raises(NotImplementedError, match=r"dequantize_base_\(\).*merge_and_unload\(\)"):
        refuse_combinations({"nf4"}, "generation")
    refuse_combinations({"sampling"}, "generate()")


def test_train_header_no_longer_says_ignored():
    head = open(os.path.join(ROOT, "radvlm_amd", "llava", "train", "train.py")).read().split('"""')[1]
    assert "bits/quantisation) are accepted and ignored" not in head and "QLoRA" in head

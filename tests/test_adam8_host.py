"""CPU checks of the 8-bit AdamW state's definition: the committed codebook against its formula, tests/adam8_ref.py's quantiser at the
midpoints and block edges, the tensor rule and block table of radvlm_amd/optim8.py, the convergence of the restated optimizer against
fp32 Adam on a heterogeneous noisy quadratic (and what the guard is for), and the reading of --optim."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam8_ref as R
from radvlm_amd import optim8

F32 = np.float32


probe_block, host_inputs = R.probe_block, R.host_inputs


# ------------------------------------------------------------------------------------------------ header table
@pytest.mark.parametrize("kind", [R.SIGNED, R.UNSIGNED])
def test_header_table_is_the_formula(kind):
    q = optim8.read_codebook()[kind]
    assert q.dtype == np.float32 and q.shape == (256,)
    assert np.array_equal(q.view(np.uint32), R.codebook(kind).view(np.uint32))
    assert np.all(np.diff(q) > 0) and np.all(np.diff(R.midpoints(q)) > 0)
    assert q[-1] == 1.0
    if kind == R.SIGNED:
        assert (q < 0).sum() == 127 and (q > 0).sum() == 128 and q[127] == 0
        assert q[0] == F32(-0.99296874) and q[128] == F32(5.5e-7) and q[126] == F32(-5.5e-7)
        assert np.array_equal(-q[:127][::-1], q[128:255])    # symmetric below 1.0
    else:
        assert q[0] == 0 and (q > 0).sum() == 255 and q[1] == F32(3.25e-7)


def test_codebook_sha_is_of_the_tables():
    import hashlib
    s, u = optim8.read_codebook()
    assert optim8.codebook_sha() == hashlib.sha256(s.astype("<f4").tobytes() + u.astype("<f4").tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ reference quantiser
@pytest.mark.parametrize("kind", [R.SIGNED, R.UNSIGNED])
@pytest.mark.parametrize("scale", [1.0, 3.0, 2.0 ** -40])
def test_midpoint_rule_at_the_midpoints(kind, scale):
    x = probe_block(kind, scale)
    codes, absmax = R.quantize(x, kind)
    assert np.all(absmax == F32(scale))
    mid = R.midpoints(R.codebook(kind)).astype(np.float64)
    a = (x / F32(scale)).astype(F32).astype(np.float64)      # the rule is stated on the fp32 quotient
    want = (mid[None, :] < a[:, None]).sum(1)
    if kind == R.UNSIGNED:
        want = np.where((x > 0) & (want == 0), 1, want)
    assert np.array_equal(codes, want)
    if scale == 1.0:                                         # at a midpoint exactly: the lower code; one ulp above: the upper
        m32 = R.midpoints(R.codebook(kind))
        c_at, _ = R.quantize(np.concatenate([[F32(1)], m32]), kind)
        c_up, _ = R.quantize(np.concatenate([[F32(1)], np.nextafter(m32, F32(np.inf))]), kind)
        lo = np.arange(255)
        if kind == R.UNSIGNED:
            lo = np.maximum(lo, 1)
        assert np.array_equal(c_at[1:], lo) and np.array_equal(c_up[1:], np.arange(1, 256))


def test_zero_block_negative_max_guard_and_short_block():
    for kind, zero_code in ((R.SIGNED, 127), (R.UNSIGNED, 0)):
        codes, absmax = R.quantize(np.zeros(300, F32), kind)
        assert np.all(codes == zero_code) and np.all(absmax == 0) and absmax.size == 2
        assert np.all(R.dequantize(codes, absmax, kind) == 0)
    y = host_inputs(R.SIGNED)["negative_max"]
    codes, absmax = R.quantize(y, R.SIGNED)
    assert absmax[0] == 2.0 and codes[17] == 0 and R.dequantize(codes, absmax, R.SIGNED)[17] == F32(-0.99296874) * F32(2)
    z = host_inputs(R.UNSIGNED)["guard"]
    codes, absmax = R.quantize(z, R.UNSIGNED)
    assert absmax[0] == 7.0 and codes[5] == 255 and codes[9] == 1 and codes[11] == 0
    assert R.quantize(z, R.UNSIGNED, guard=False)[0][9] == 0
    assert R.dequantize(codes, absmax, R.UNSIGNED)[9] > 0
    x = host_inputs(R.SIGNED)["n257"]
    codes, absmax = R.quantize(x, R.SIGNED)
    assert codes.size == 257 and absmax.size == 2 and absmax[1] == abs(x[256]) and codes[256] == (255 if x[256] > 0 else 0)


@pytest.mark.parametrize("kind", [R.SIGNED, R.UNSIGNED])
def test_elementwise_error_bound(kind):
    """|x^ - x| <= (half the local code gap) * absmax, the gap being that of the two codes around x / absmax (plus the roundings of the
    quotient, the midpoint and the product: 3 ulp of the larger code, counted in float64)."""
    r = np.random.RandomState(3)
    x = (r.randn(4096) * np.exp(3 * r.randn(4096))).astype(F32)
    if kind == R.UNSIGNED:
        x = x * x
    codes, absmax = R.quantize(x, kind)
    xh = R.dequantize(codes, absmax, kind).astype(np.float64)
    q = R.codebook(kind).astype(np.float64)
    s = np.repeat(absmax, 256)[:x.size].astype(np.float64)
    a = x.astype(np.float64) / s
    hi = np.clip(np.searchsorted(q, a, side="left"), 1, 255)
    gap = q[hi] - q[hi - 1]
    guarded = (kind == R.UNSIGNED) & (codes == 1) & (a < q[1])
    bound = np.where(guarded, q[1], gap / 2) * s + 3 * 2.0 ** -23 * s
    assert np.all(np.abs(xh - x) <= bound)


# ------------------------------------------------------------------------------------------------ tensor rule and block table
def _layout(shapes):
    import torch
    from radvlm_amd.params import FlatParams
    return FlatParams(shapes, torch.device("meta"))           # offsets only: no storage


def _check_plan(shapes):
    fp = _layout(shapes)
    plan = optim8.StatePlan(fp.offsets, fp.shapes)
    nb = 0
    for name, t in plan.tensors.items():
        shp = shapes[name]
        want8 = len(shp) >= 2 and int(np.prod(shp)) >= 4096 and not name.endswith(("embed_tokens.weight", "position_embedding.weight"))
        assert t["bits"] == (8 if want8 else 32), name
        if want8:
            assert t["block"] == nb                          # consecutive blocks, a fresh one at every tensor start: none straddles
            nb += -(-t["n"] // 256)
    assert plan.nblocks == nb and plan.ncodes == nb * 256
    # the compact fp32 layout: no overlap, and the same offsets modulo 64 as in the flat buffer (alignment of rv_adamw's vectors)
    spans = sorted((t["pos"], t["pos"] + t["n"]) for t in plan.tensors.values() if t["bits"] == 32)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= plan.n32)
    assert all((t["pos"] - t["off"]) % 64 == 0 for t in plan.tensors.values() if t["bits"] == 32)
    # runs over the whole buffer cover every tensor once, in order
    seen = []
    for run in plan.runs(0, fp.numel):
        if run[0] == 8:
            tab, n = plan.block_table(run[1], origin=0)
            assert n == sum(-(-plan.tensors[k]["n"] // 256) for k in run[1]) and tab.shape == (3, len(run[1]))
            seen += run[1]
        else:
            _, s, e, pos = run
            inside = [k for k, t in plan.tensors.items() if s <= t["off"] and t["off"] + t["n"] <= e]
            assert all(plan.tensors[k]["bits"] == 32 and plan.tensors[k]["pos"] == pos + plan.tensors[k]["off"] - s for k in inside)
            seen += inside
    assert seen == list(plan.tensors)
    return plan


def test_tensor_rule_and_block_table_on_the_toy_and_7b_lists():
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.params import lm_param_shapes, lora_trainable_shapes, vision_param_shapes
    for geo_name in ("toy", "llava15_7b"):
        geo = GEOMETRIES[geo_name]
        full = _check_plan(lm_param_shapes(geo, with_newline=True))
        assert full.tensors["model.embed_tokens.weight"]["bits"] == 32
        assert full.tensors["model.norm.weight"]["bits"] == 32 and full.tensors["model.mm_projector.0.bias"]["bits"] == 32
        assert full.tensors["model.image_newline"]["bits"] == 32
        tower = _check_plan(vision_param_shapes(geo))
        assert all(t["bits"] == 32 for k, t in tower.tensors.items() if "position_embedding" in k or len(vision_param_shapes(geo)[k]) == 1)
    geo = GEOMETRIES["llava15_7b"]
    full = optim8.StatePlan(*(lambda fp: (fp.offsets, fp.shapes))(_layout(lm_param_shapes(geo))))
    for k in ("lm_head.weight", "model.mm_projector.0.weight", "model.mm_projector.2.weight", "model.layers.31.mlp.down_proj.weight"):
        assert full.tensors[k]["bits"] == 8
    lora = _check_plan(lora_trainable_shapes(geo, 128))
    assert all(t["bits"] == 8 for k, t in lora.tensors.items() if ".lora_" in k)
    # 8 B + 32 B per 256 moments against 8 B per moment pair: the 7B full fine-tune's moments shrink below 0.3x
    bytes8 = 2 * full.ncodes + 8 * full.nblocks + 8 * full.n32
    assert bytes8 < 0.3 * 8 * sum(t["n"] for t in full.tensors.values())


def test_a_block_never_straddles_a_tensor_with_odd_sizes():
    shapes = OrderedDict([("a.weight", (300, 20)), ("b.weight", (5,)), ("c.weight", (4099, 1)), ("d.q_proj.weight", (64, 65)),
                          ("d.k_proj.weight", (64, 65)), ("e.embed_tokens.weight", (100, 64)), ("f.weight", (64, 64))])
    plan = _check_plan(shapes)
    assert [plan.tensors[k]["block"] for k in plan.names(8)] == [0, 24, 41, 58, 75]


# ------------------------------------------------------------------------------------------------ convergence
@pytest.mark.parametrize("sigma", [0.5, 1.5, 2.5])
def test_convergence_stays_with_fp32_adam(sigma):
    """Gate (set with the format): at every one of the 300 steps the 8-bit run's loss is <= 1.25 x fp32 Adam's on the same draws.
    Measured here: worst ratio 1.038 / 1.007 / 1.010, final ratio 1.006 / 0.772 / 0.882 for sigma 0.5 / 1.5 / 2.5."""
    ref, got = R.noisy_quadratic(sigma, 32), R.noisy_quadratic(sigma, 8)
    ratio = got / ref
    print(f"sigma {sigma}: worst ratio {ratio.max():.4f}, final {ratio[-1]:.4f}")
    assert np.all(np.isfinite(got)) and ratio.max() <= 1.25


def test_without_the_guard_the_same_run_blows_up():
    """What the guard is for: exp_avg_sq of a low-curvature coordinate dequantises to 0 and the step divides by eps (measured: 3964x)."""
    ratio = R.noisy_quadratic(1.5, 8, guard=False) / R.noisy_quadratic(1.5, 32)
    print(f"no guard: worst ratio {ratio.max():.1f}")
    assert ratio.max() > 100


def test_the_kernels_are_built_declared_and_under_the_scratch_gate():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = open(os.path.join(root, "radvlm_amd", "csrc", "build.sh")).read()
    assert "adam8" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    from radvlm_amd import lib
    for name, nargs in (("rv_adam8_quantize_f32", 6), ("rv_adam8_dequantize_f32", 6), ("rv_adamw8", 19)):
        assert len(lib.SIGNATURES[name][1]) == nargs, name
    ops_src = open(os.path.join(root, "radvlm_amd", "csrc", "ops.hip")).read()
    assert '#include "adamw_update.h"' in ops_src and "void adamw_update(" not in ops_src       # one definition, in the shared header


# ------------------------------------------------------------------------------------------------ --optim
def test_optim_parsing():
    said = []
    assert optim8.optim_state_bits("adamw_bnb_8bit", said.append) == 8 and optim8.optim_state_bits("adamw_8bit", said.append) == 8
    for name in ("adamw_torch", "adamw_hf", "adamw_torch_fused"):
        assert optim8.optim_state_bits(name, said.append) == 32
    assert not said
    assert optim8.optim_state_bits("adafactor", said.append) == 32 and len(said) == 1 and "adafactor" in said[0]
    from radvlm_amd.llava.train.train import TrainingArguments
    assert TrainingArguments.__dataclass_fields__["optim"].default == "adamw_torch"

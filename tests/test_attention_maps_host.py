"""CPU checks of the attention-map feature: which generate() entry point takes output_attentions / attention_layers / attention_reduce
and what each refuses, the layer resolution, and radvlm_amd.attention_maps on splice plans built from the committed goldens' inputs."""
import json
import os
import re

import numpy as np
import pytest

from radvlm_amd.attention_maps import image_attention_map, image_token_positions, step_image_maps
from radvlm_amd.config import GEOMETRIES
from radvlm_amd.generation import (GenerationCache, parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs,
                                   resolve_attention_layers)
from radvlm_amd.splice import NEWLINE, build_splice_plan, merged_feature_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON = dict(output_attentions=True, return_dict_in_generate=True)


def _parse(**kw):
    return parse_generate_kwargs(kw, attentions=True, lookup=True)


# ------------------------------------------------------------------------------------------------ keywords
def test_generate_accepts_the_three_keywords():
    assert _parse().attentions is None and _parse(output_attentions=False).attentions is None
    a = _parse(**ON).attentions
    assert a.layers is None and a.reduce is None
    a = _parse(**ON, attention_layers=[-1, 0, np.int64(2)], attention_reduce="mean_heads").attentions
    assert a.layers == (-1, 0, 2) and a.reduce == "mean_heads"
    assert resolve_attention_layers(None, 4) == (0, 1, 2, 3)
    assert resolve_attention_layers((-1, 0, 2), 4) == (3, 0, 2) and resolve_attention_layers((-4,), 4) == (0,)
    # composes with the processors, sampling, a constraint-free call, stopping criteria
    c = _parse(**ON, do_sample=True, seed=3, repetition_penalty=1.2, stopping_criteria=[lambda *a: False], output_scores=True)
    assert c.attentions is not None and c.sampling is not None


@pytest.mark.parametrize("kw", [
    dict(output_attentions=1, return_dict_in_generate=True), dict(output_attentions="yes", return_dict_in_generate=True),
    dict(output_attentions=True), dict(output_attentions=True, return_dict_in_generate=False),
    dict(attention_layers=[0]), dict(attention_reduce="mean_heads"), dict(output_attentions=False, attention_layers=[0]),
    dict(**ON, attention_reduce="mean"), dict(**ON, attention_reduce=True), dict(**ON, attention_layers=[True]),
    dict(**ON, attention_layers=[0.0]), dict(**ON, attention_layers=0), dict(**ON, attention_layers="all"), dict(**ON, attention_layers=[]),
])
def test_generate_value_errors(kw):
    with pytest.raises(ValueError):
        _parse(**kw)


def test_layer_resolution_errors():
    for spec in ((4,), (-5,), (0, 0), (3, -1), (1, -3)):
        with pytest.raises(ValueError):
            resolve_attention_layers(spec, 4)


@pytest.mark.parametrize("kw,name", [
    (dict(kv_cache_dtype="int8"), "kv_cache_dtype='int8'"), (dict(past_key_values=GenerationCache()), "past_key_values"),
    (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"), (dict(guidance_scale=1.5), "guidance_scale"),
    (dict(dola_layers="low"), "dola_layers")])
def test_generate_refuses_named_combinations(kw, name):
    with pytest.raises(NotImplementedError, match=re.escape(f"output_attentions with {name}")):
        _parse(**ON, **kw)
    assert _parse(**kw).attentions is None                    # the combination's other half alone is what it was
    with pytest.raises(NotImplementedError, match="LoRA"):
        parse_generate_kwargs(dict(ON), lora=True, attentions=True)


@pytest.mark.parametrize("name,value", [("output_attentions", True), ("attention_layers", [0]), ("attention_reduce", "mean_heads")])
def test_other_entry_points_reject_the_names(name, value):
    with pytest.raises(TypeError, match=name):
        parse_generate_kwargs({name: value})
    with pytest.raises(TypeError, match=name):
        parse_batch_kwargs({name: value}, 2)
    with pytest.raises(TypeError, match=name):
        parse_beam_kwargs({name: value, "num_beams": 2})


def test_symbols_declared_bound_and_built():
    from radvlm_amd import lib, ops
    hdr = open(os.path.join(ROOT, "include", "radvlm_hip.h")).read()
    assert len(lib.SIGNATURES["rv_attn_decode_probs_f32"][1]) == 20
    assert "int64_t rv_attn_decode_probs_ws_bytes(int B, int H, int L_out);" in hdr
    assert "modeling_llama.py:352-382" in hdr.split("int rv_attn_decode_probs_f32(")[0][-2500:]
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "attn_probs" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    assert callable(ops.attn_decode_probs)


# ------------------------------------------------------------------------------------------------ positions
def _plan(golden_dir, name, padding_side="right", sizes=None):
    """LlavaEngine.plan()'s bookkeeping from a golden's inputs, without an engine: (plan, tiles per image, side, merged rows).
    sizes: other original image sizes than the golden's (same tile grids), so that unpad has something to crop."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    meta = json.load(open(os.path.join(golden_dir, name + "_gradnorms.json")))
    v = GEOMETRIES[meta["geometry"]]["vision"]
    side = v["image"] // v["patch"]
    P = side * side
    n_img = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    tiles = [1 if g[f"image{i}"].ndim == 3 else g[f"image{i}"].shape[0] for i in range(n_img)]
    n_proj = sum(tiles) * P
    extra = dict(next=n_proj, src=[], w=[])
    rows, r0, image_rows = [], 0, []
    for i, t in enumerate(tiles):
        e0 = extra["next"]
        rows.append(merged_feature_rows(r0, t, side, meta["merge_type"], meta["aspect"], tuple(sizes[i]) if sizes else tuple(g["image_sizes"][i].tolist()),
                                        meta["pinpoints"], v["image"], extra=extra))
        image_rows.append((r0, r0 + t * P, e0, extra["next"]))
        r0 += t * P
    plan = build_splice_plan(g["input_ids"], g["attention_mask"].astype(bool), g["labels"], rows, extra["next"], padding_side=padding_side)
    plan["n_feat_rows"], plan["image_rows"] = extra["next"], image_rows
    return plan, tiles, side, rows


def _expected(plan, rows, image_rows):
    """Per image, straight from the merged row lists: the cache position of every feature row of sequence b = image i (the goldens
    hold one image per sequence, in order), counting the sequence's valid positions."""
    B, S = plan["attention_mask"].shape
    idx = plan["idx"].reshape(B, S)
    out = []
    for i, (p0, p1, e0, e1) in enumerate(image_rows):
        valid = idx[i][plan["attention_mask"][i]]
        where = {}
        if not (valid <= -2).any():                                 # a text-only sample: its dummy image lands nowhere
            out.append((np.full(p1 - p0, -1), np.full(e1 - e0, -1)))
            continue
        first = int(np.flatnonzero(valid <= -2)[0])                 # the image's rows are one consecutive run
        for k, r in enumerate(rows[i]):
            if r != NEWLINE and first + k < valid.size:
                where[int(r)] = first + k
        out.append((np.array([where.get(r, -1) for r in range(p0, p1)]), np.array([where.get(r, -1) for r in range(e0, e1)])))
    return out


def test_flat_positions_are_consecutive_and_row_major(golden_dir):
    plan, tiles, side, rows = _plan(golden_dir, "toy_e2e")
    got = image_token_positions(plan)
    assert len(got) == 3 and [im["seq"] for im in got] == [0, 1, -1]        # the third sample is text only: its dummy image lands nowhere
    assert (got[2]["pos"] == -1).all() and got[2]["pos"].size == side * side
    assert int(got[0]["pos"][0]) == 5 and int(got[1]["pos"][0]) == 3         # where the prompts hold their image placeholder
    for im in got[:2]:
        assert im["extra_pos"].size == 0 and im["pos"].size == side * side and (im["pos"] >= 0).all()
        assert np.array_equal(np.diff(im["pos"]), np.ones(side * side - 1, dtype=np.int64))
    for im, (pos, _) in zip(got, _expected(plan, rows, plan["image_rows"])):
        assert np.array_equal(im["pos"], pos)


# the unpad golden's own sizes fill their tile grids exactly; these two (same grids: 2 x 2 and 3 x 1) leave padding that unpad crops
UNPAD_SIZES = {"toy_anyres_e2e": [(112, 90), (150, 30)], "toy_qwen_anyres_max_e2e": None}


@pytest.mark.parametrize("name", ["toy_anyres_e2e", "toy_qwen_anyres_max_e2e"])
def test_unpad_and_anyres_max_positions(golden_dir, name):
    plan, tiles, side, rows = _plan(golden_dir, name, sizes=UNPAD_SIZES[name])
    got = image_token_positions(plan)
    exp = _expected(plan, rows, plan["image_rows"])
    B, S = plan["attention_mask"].shape
    newline_cache_pos = set()
    rank = np.cumsum(plan["attention_mask"], 1) - 1
    for f in plan["newline_pos"]:
        newline_cache_pos.add((int(f) // S, int(rank[int(f) // S, int(f) % S])))
    assert newline_cache_pos, "these merges splice image_newline rows"
    dropped = created = 0
    for i, (im, (pos, epos)) in enumerate(zip(got, exp)):
        assert im["seq"] == i and np.array_equal(im["pos"], pos) and np.array_equal(im["extra_pos"], epos)
        assert im["pos"].size == tiles[i] * side * side
        landed = np.concatenate([im["pos"][im["pos"] >= 0], im["extra_pos"][im["extra_pos"] >= 0]])
        assert np.unique(landed).size == landed.size and (landed < plan["lens"][i]).all()
        assert not {(i, int(p)) for p in landed} & newline_cache_pos                     # newlines belong to no image
        assert (im["pos"][:side * side] >= 0).all()                                      # the base tile is always spliced whole
        dropped += int((im["pos"] < 0).sum())
        created += im["extra_pos"].size
    assert dropped > 0                                                                   # unpad crops (or anyres_max replaces) rows
    if "anyres_max" in name:
        assert created == 38 * 38 and got[0]["extra_pos"].size == 38 * 38 and got[1]["extra_pos"].size == 0
        assert (got[0]["extra_pos"] >= 0).all() and (got[0]["pos"][side * side:] < 0).all()   # the resampled grid replaces its sources
    else:
        assert created == 0 and [int((im["pos"] < 0).sum()) for im in got] == [16, 24]      # 16 + 48 of 80 rows and 16 + 24 of 64 survive


@pytest.mark.parametrize("name", ["toy_e2e", "toy_qwen_anyres_max_e2e"])
def test_left_padding_gives_the_same_positions(golden_dir, name):
    right, left = _plan(golden_dir, name, "right")[0], _plan(golden_dir, name, "left")[0]
    assert len(set(right["lens"].tolist())) > 1 and not np.array_equal(right["idx"], left["idx"])
    for a, b in zip(image_token_positions(right), image_token_positions(left)):
        assert a["seq"] == b["seq"] and np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["extra_pos"], b["extra_pos"])


def test_round_trip_and_step_maps(golden_dir):
    plan, tiles, side, _ = _plan(golden_dir, "toy_anyres_e2e")
    im = image_token_positions(plan)[0]
    n = int(plan["lens"][0])
    want = np.arange(1, im["pos"].size + 1, dtype=np.float32)
    row = np.zeros(n + 3, dtype=np.float32)
    ok = im["pos"] >= 0
    row[im["pos"][ok]] = want[ok]
    m = image_attention_map(row, im["pos"], tiles[0], side)
    assert m.dtype == np.float32 and m.shape == (tiles[0], side, side)
    assert np.array_equal(m.reshape(-1)[ok], want[ok]) and not m.reshape(-1)[~ok].any()
    assert not image_attention_map(row[:1], im["pos"], tiles[0], side).any() or im["pos"].min() <= 0     # past the row's end: 0
    with pytest.raises(ValueError):
        image_attention_map(row, im["pos"][:-1], tiles[0], side)
    # step_image_maps: per-head rows averaged on the host = the mean form
    from types import SimpleNamespace
    rng = np.random.default_rng(0)
    B, H = plan["attention_mask"].shape[0], 4
    steps = [rng.random((B, H, 1, n + t)).astype(np.float32) for t in range(3)]
    per_head = SimpleNamespace(attentions=tuple((np.zeros_like(a), a) for a in steps))
    mean = SimpleNamespace(attentions=tuple((np.zeros_like(a[:, :1]), a.astype(np.float64).mean(1, keepdims=True)) for a in steps))
    a, b = step_image_maps(per_head, plan, side=side), step_image_maps(mean, plan, side=side)
    assert a.shape == (3, tiles[0], side, side) and a.dtype == np.float32 and np.array_equal(a, b)
    assert np.array_equal(a[1], image_attention_map(steps[1][0].astype(np.float64).mean(0)[0], im["pos"], tiles[0], side))
    assert not step_image_maps(per_head, plan, layer=0, side=side).any()
    with pytest.raises(ValueError):
        step_image_maps(per_head, plan)                              # five tiles are no square: side= is needed

"""GPU tests of generate_batch(share_prefix=True) through the engine and the model API: extend(..., slots=) against extend on a compact
cache, decode_step(shared=plan) against the plain step, generate_batch with sharing on against the reference arm
(shared_route="plain", exact) and against sharing off (the rule of tests/test_generate_batch_gpu.py), the number of tower runs and
prefills, sampling, prompts with nothing in common, and one full-width decoder layer of each 7B head shape.

The toy model's image is 16 positions, so its requests carry a common 300-token text after the image token (where a LLaVA
conversation has its text): requests about one image then share two whole decode chunks and requests about different images share
nothing, as with toy_qwen's 729-position image.  A second toy set has the text in front of everything: there every request follows
the first one and the images themselves are among the followers' new rows."""
import copy

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES
from test_generate_batch_gpu import _alone, _batch, _requests
from test_generate_gpu import CASES, LOGITS_FP32_TOL, _engine, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu
N_NEW = 12
PREFIX = (np.arange(300) * 37 % 900 + 50).astype(np.int64)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _with_text(p, where):
    """The prompt with the common text after its image token ("after"; a text-only prompt: in front) or in front of everything."""
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    k = np.flatnonzero(p == IMAGE_TOKEN_INDEX)
    if where == "front" or k.size == 0:
        return np.concatenate([PREFIX, p])
    return np.concatenate([p[:k[0] + 1], PREFIX, p[k[0] + 1:]])


def _questions(g, images, sizes, case, where="after"):
    """2 images x 3 questions, then 1 text-only request: (prompt, image, size) each."""
    from radvlm_amd.splice import IMAGE_TOKEN_INDEX
    reqs = []
    for b in range(2):
        p = _prompt(g, b) if case != "toy" else _with_text(_prompt(g, b), where)
        for q in (p, p[:-2], np.concatenate([p[:-1], [7 + b, 9, 11]])):
            reqs.append((q, images[b], sizes[b]))
    p0 = _prompt(g, 0)
    text = p0[p0 != IMAGE_TOKEN_INDEX]
    reqs.append((text if case != "toy" else _with_text(text, where), None, None))
    return reqs


def _spliced_records(eng, reqs):
    from radvlm_amd.generation import position_records
    uid = {}
    out = []
    for p, im, s in reqs:
        ims, ss = ([], None) if im is None else ([im], [s])
        plan = eng.plan(p[None], None, None, ims, ss)
        out.append(position_records(plan, [uid.setdefault(id(im), len(uid))] if ims else [])[0])
    return out


# ------------------------------------------------------------------------------------------------ engine: extend into slots
@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_extend_into_slots_is_bit_identical(golden_dir, case):
    from radvlm_amd.generation import reuse_lengths
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    reqs = _questions(g, images, sizes, case)
    old, new = [reqs[0], reqs[3]], [reqs[2], reqs[4]]                # per image: the full question, then another question / a shorter one
    rec = _spliced_records(eng, old + new)
    r = reuse_lengths(rec[:2], rec[2:])
    assert (r >= 128).all() and r[0] != r[1]
    ims, szs = [q[1] for q in old], [q[2] for q in old]
    ids0, am0 = (a.numpy() for a in _pad_batch([q[0] for q in old], "right"))
    ids1, am1 = (a.numpy() for a in _pad_batch([q[0] for q in new], "right"))
    compact, _ = eng.prefill(ids0, am0, ims, szs, max_new_tokens=16)
    L_max = compact.L_max
    big = eng.new_kv_cache(8, L_max)
    for i, t in enumerate(big.layers):
        t.copy_(torch.randn(t.shape, device=t.device).to(t.dtype))   # stale contents everywhere
        for b, s in enumerate((5, 2)):
            t[s, :r[b]] = compact.layers[i][b, :r[b]]
    big.lens[:] = [3, 0, int(r[1]), 7, 0, int(r[0]) + 2, 1, 0]
    before = [t.clone() for t in big.layers]
    _, want = eng.extend(compact, ids1, am1, ims, szs, reuse=r, max_new_tokens=4)
    assert compact.L_max == L_max                                     # no growth: the same RoPE table and chunk grid on both sides
    _, got = eng.extend(big, ids1, am1, ims, szs, reuse=r, max_new_tokens=4, slots=[5, 2])
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    lens = compact.lens
    assert big.lens.tolist() == [3, 0, int(lens[1]), 7, 0, int(lens[0]), 1, 0]
    for i in range(len(big.layers)):
        for b, s in enumerate((5, 2)):
            n = int(lens[b])
            assert torch.equal(big.layers[i][s, :n], compact.layers[i][b, :n]), (i, b)
            assert torch.equal(big.layers[i][s, n:], before[i][s, n:])
        for s in (0, 1, 3, 4, 6, 7):
            assert torch.equal(big.layers[i][s], before[i][s])
    with pytest.raises(ValueError):
        eng.extend(big, ids1, am1, ims, szs, reuse=r, slots=[2, 2])
    with pytest.raises(ValueError):
        eng.extend(big, ids1, am1, ims, szs, reuse=r, slots=[5, 8])
    with pytest.raises(ValueError):                                   # no growth under slots=
        eng.extend(big, ids1, am1, ims, szs, reuse=r, max_new_tokens=L_max, slots=[5, 2])


# ------------------------------------------------------------------------------------------------ engine: decode_step(shared=)
def _shared_cache(eng, reqs, slots, S, extra=0, L_max=None):
    """Leader reqs[0] prefilled into slots[0] of a stale S-row cache; the others copied from it and extended.  Returns (cache, plan, P)."""
    from radvlm_amd.generation import reuse_lengths, shared_tiles
    rec = _spliced_records(eng, reqs)
    P = reuse_lengths([rec[0]] * (len(reqs) - 1), rec[1:])
    cache = eng.new_kv_cache(S, L_max or max(len(r) for r in rec) + extra)
    for t in cache.layers:
        t.copy_(torch.randn(t.shape, device=t.device).to(t.dtype))
    lead = reqs[0]
    eng.prefill(lead[0][None], None, None if lead[1] is None else [lead[1]], None if lead[2] is None else [lead[2]], cache=cache, slots=slots[:1])
    for t in cache.layers:
        for s, p in zip(slots[1:], P):
            t[s, :p] = t[slots[0], :p]
    cache.lens[slots[1:]] = P
    ids, am = (a.numpy() for a in _pad_batch([q[0] for q in reqs[1:]], "right"))
    ims = [q[1] for q in reqs[1:] if q[1] is not None]
    szs = [q[2] for q in reqs[1:] if q[1] is not None]
    eng.extend(cache, ids, am, ims or None, szs or None, reuse=P, slots=slots[1:])
    lineage, Ps = np.full(S, -1), np.zeros(S, dtype=np.int64)
    lineage[slots] = 0
    Ps[slots[0]], Ps[slots[1:]] = P.max(), P
    c0, tile = shared_tiles(slots, lineage, Ps, eng.shared_rows_per_tile, cache.chunk, S)
    return cache, eng.shared_plan(c0, tile), P


def _clone(eng, cache):
    c = eng.new_kv_cache(cache.B, cache.L_max)
    for a, b in zip(c.layers, cache.layers):
        a.copy_(b)
    c.lens[:] = cache.lens
    return c


def _three_steps(eng, cache, plan, slots, route):
    toks = np.random.default_rng(7).integers(0, eng.vocab, (3, cache.B))
    idle = np.array([s not in slots for s in range(cache.B)])
    out = []
    eng.shared_route = route
    try:
        for t in range(3):
            cache.lens[idle] = 0
            feed = np.where(idle, 0, toks[t])
            out.append((eng.decode_step(cache, feed) if plan is None else eng.decode_step(cache, feed, shared=plan)).clone())
            cache.lens[idle] = 0
    finally:
        eng.shared_route = None
    return out


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_decode_steps_with_a_plan_equal_the_plain_steps(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    reqs = _questions(g, images, sizes, case)[:3]
    slots = [4, 1, 3]
    cache, plan, P = _shared_cache(eng, reqs, slots, 6, extra=4)
    assert (P >= 2 * cache.chunk).all() and int(plan.c0_host.max()) >= 2 and (plan.c0_host[[0, 2, 5]] == 0).all()
    plain = _clone(eng, cache)
    want = _three_steps(eng, plain, None, slots, None)
    got = _three_steps(eng, cache, plan, slots, "shared")
    n0 = plain.lens[slots] - 3
    for a, b in zip(got, want):
        assert torch.equal(a[slots], b[slots]) and bool(torch.isfinite(a[slots]).all())
    for x, y in zip(cache.layers, plain.layers):
        for s, n in zip(slots, n0):
            assert torch.equal(x[s, n:n + 3], y[s, n:n + 3]) and torch.equal(x[s, :n], y[s, :n])


# ------------------------------------------------------------------------------------------------ generate_batch(share_prefix=True)
def _counted(model):
    """Wrap the engine's tower and prompt passes: the images each encode_images call saw, the rows of each prefill and extend."""
    eng = model.engine
    seen = dict(tower=[], prefill=[], extend=[])
    enc, pre, ext = eng.encode_images, eng.prefill, eng.extend

    def encode_images(pixels, *a, **k):
        seen["tower"].append(int(pixels.shape[0]))
        return enc(pixels, *a, **k)

    def prefill(ids, *a, **k):
        seen["prefill"].append(int(np.asarray(ids).shape[0]))
        return pre(ids, *a, **k)

    def extend(cache, ids, *a, **k):
        seen["extend"].append(int(np.asarray(ids).shape[0]))
        return ext(cache, ids, *a, **k)

    eng.encode_images, eng.prefill, eng.extend = encode_images, prefill, extend
    return seen


def _uncounted(model):
    for name in ("encode_images", "prefill", "extend"):
        model.engine.__dict__.pop(name, None)


def _route(model, route, reqs, **kw):
    model.engine.shared_route = route
    try:
        return _batch(model, reqs, max_batch_size=7, max_new_tokens=N_NEW, eos_token_id=None, return_logprobs=True, **kw)
    finally:
        model.engine.shared_route = None


def _against_unshared(got, ref, one):
    """The rule of test_generate_batch_gpu._compare, between two runs: log-probs within 2 x LOGITS_FP32_TOL x max|logit| and tokens equal
    up to the first step whose top-1 / top-2 margin (the scores of generate() on the request alone) is below 3 x that.  Returns the
    steps compared."""
    for t in range(len(one.scores)):
        s1 = one.scores[t][0].cpu()
        fin = s1[torch.isfinite(s1)]
        scale = LOGITS_FP32_TOL * float(fin.abs().max())
        top = torch.topk(fin, 2).values
        if float(top[0] - top[1]) < 3 * scale:
            return t
        assert got.generated_tokens[t] == ref.generated_tokens[t], (t, got.generated_tokens, ref.generated_tokens)
        assert abs(got.logprobs[t] - ref.logprobs[t]) <= 2 * scale, (t, got.logprobs[t], ref.logprobs[t])
    return len(one.scores)


@pytest.mark.parametrize("case,where", [("toy", "after"), ("toy_qwen", "after"), ("toy", "front")])
def test_generate_batch_shared_routes_and_unshared(golden_dir, case, where):
    from conftest import record_measurement
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    reqs = _questions(g, images, sizes, case, where)
    ref = _route(model, None, reqs)                                   # sharing off
    seen = _counted(model)
    try:
        shared = _route(model, "shared", reqs, share_prefix=True)
    finally:
        _uncounted(model)
    plain = _route(model, "plain", reqs, share_prefix=True)
    # (a) the two routes: exactly equal
    for k in shared:
        assert shared[k].generated_tokens == plain[k].generated_tokens and len(shared[k].generated_tokens) == N_NEW
        assert shared[k].logprobs == plain[k].logprobs and len(shared[k].logprobs) == N_NEW
    # (b) against sharing off
    steps = sum(_against_unshared(shared[f"req_{i}"], ref[f"req_{i}"], _alone(model, r, N_NEW, eos_token_id=None)) for i, r in enumerate(reqs))
    record_measurement("share_prefix_vs_unshared", case=case, where=where, steps_compared=steps, of=N_NEW * len(reqs))
    # how far the rule compares is the model's doing: behind 300 arbitrary tokens the random-weight toy model's top two scores are
    # near ties from the first steps on (9 and 5 of 84 steps compared in the two toy sets, 72 of 84 with toy_qwen)
    assert steps >= (len(reqs) if case == "toy_qwen" else 1)
    # (c) the tower runs once per distinct image and prefill only for leaders
    if where == "after":
        assert seen["prefill"] == [3] and seen["extend"] == [4]      # leaders: each image's first question and the text-only request
        assert seen["tower"] == [2]
    else:                                                             # the text in front: one leader; the followers' new rows hold their images
        assert seen["prefill"] == [1] and seen["extend"] == [6] and seen["tower"] == [1, 5]
    # (d) sampling: the two routes draw identical tokens
    a = _route(model, "shared", reqs, share_prefix=True, do_sample=True, seed=3)
    b = _route(model, "plain", reqs, share_prefix=True, do_sample=True, seed=3)
    for k in a:
        assert a[k].generated_tokens == b[k].generated_tokens and a[k].logprobs == b[k].logprobs and len(a[k].generated_tokens) == N_NEW
    assert any(a[k].generated_tokens != shared[k].generated_tokens for k in a)


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_nothing_in_common_is_the_call_without_the_keyword(golden_dir, case):
    from radvlm_amd.generation import BatchScheduler, batch_requests, parse_batch_kwargs
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw)
    reqs = _requests(g, images, sizes, case)
    if case == "toy_qwen":                                            # one request per image and the text-only ones: no image twice
        reqs = [reqs[0], reqs[2], reqs[3], reqs[6]]
    budgets = [6, 9, 1, 12, 4, 7, 10, 5][:len(reqs)]
    runs = []
    for extra in ({}, dict(share_prefix=True)):
        cfg = parse_batch_kwargs(dict(max_new_tokens=budgets, eos_token_id=None, **extra), len(reqs))
        sch = BatchScheduler(model.engine, batch_requests([r[0] for r in reqs], [r[1] for r in reqs], [r[2] for r in reqs]), cfg, 3,
                             return_logprobs=True)
        out = sch.run()
        runs.append((sch.events, [(o.generated_tokens, o.logprobs) for o in out.values()]))
    assert runs[0] == runs[1] and not any(e[0] == "share" for e in runs[1][0])
    assert [len(t) for t, _ in runs[1][1]] == budgets


def test_model_level_refusals(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    reqs = _requests(g, images, sizes, "toy")[:2]
    with pytest.raises(NotImplementedError):
        _batch(model, reqs, max_new_tokens=2, share_prefix=True, kv_cache_dtype="int8")
    with pytest.raises(NotImplementedError):
        _batch(model, reqs, max_new_tokens=2, share_prefix=True, guidance_scale=2.0)
    with pytest.raises(ValueError):
        _batch(model, reqs, max_new_tokens=2, share_prefix=1)
    p, im, s = reqs[0]
    with pytest.raises(TypeError):
        model.generate(torch.from_numpy(p[None]), images=[im], image_sizes=[s], max_new_tokens=2, share_prefix=True)
    with pytest.raises(TypeError):
        model.generate_beams(torch.from_numpy(p[None]), images=[im], image_sizes=[s], num_beams=2, max_new_tokens=2, share_prefix=True)


# ------------------------------------------------------------------------------------------------ full width
@pytest.mark.parametrize("gname", ["llava15_7b", "llava_ov_qwen2_7b"])
def test_full_width_layer_shared_equals_plain(gname):
    """One 7B-width decoder layer + the full head, L_max 384, B = 8, one lineage of 8 with two whole shared chunks: three decode steps
    through the shared kernel give the plain kernel's logits and cache rows."""
    _need_gpu()
    from radvlm_amd.engine import LlavaEngine
    geo = copy.deepcopy(GEOMETRIES[gname])
    geo["lm"]["layers"] = 1
    geo["vision"]["layers"] = 2
    eng = LlavaEngine(geo, device="cuda:0", init="fast", seed=0)
    rng = np.random.default_rng(0)
    common = rng.integers(0, eng.vocab, 300)
    reqs = [(np.concatenate([common, rng.integers(0, eng.vocab, 20 + 3 * b)]), None, None) for b in range(8)]
    slots = list(range(8))
    cache, plan, P = _shared_cache(eng, reqs, slots, 8, L_max=384)
    assert cache.L_max == 384 and (P == 300).all() and (plan.c0_host == 2).all()
    assert int((plan.tile_host[:, 0] >= 0).sum()) == 8 // min(eng.shared_rows_per_tile, 8)
    plain = _clone(eng, cache)
    want = _three_steps(eng, plain, None, slots, None)
    got = _three_steps(eng, cache, plan, slots, "shared")
    for a, b in zip(got, want):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(cache.layers[0][:, :360], plain.layers[0][:, :360])

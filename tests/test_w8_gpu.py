"""GPU tests of the int8 decoder weights (load_8bit): rv_quantize_rows_w8_bf16 bit-exact against the numpy restatement
(tests/w8_ref.py), rv_gemv_w8_bf16 bit-identical to rv_gemv_bf16 on the dequantised weight, and the engine / model / loader on the toy
goldens: every comparison is exact, and the oracle is the existing bf16 path run on the dequantised weights."""
import copy

import numpy as np
import pytest
import torch

import w8_ref
from radvlm_amd import portable_rng
from radvlm_amd.config import GEOMETRIES
from test_generate_gpu import CASES, _engine, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(t):
    """uint16 bit patterns of a bf16 tensor (host numpy)."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32_bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _toy_shapes():
    out = []
    for geo in ("toy", "toy_qwen"):
        l = GEOMETRIES[geo]["lm"]
        d, F, H = l["d"], l["ffn"], l["heads"]
        kvd = l.get("kv_heads", H) * (d // H)
        out += [(d + 2 * kvd, d), (d, d), (2 * F, d), (d, F)]
    return sorted(set(out))


# the 7B Llama and Qwen2-7B decoder matrices, the toy geometries' matrices, N not a multiple of 64 and a K that ends inside a 32-deep step
BIG = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (4608, 3584), (37888, 3584), (3584, 18944)]
SHAPES = BIG + _toy_shapes() + [(1000, 4096), (100, 40)]


def _special_rows(w, K):
    """Row 1 zeros, row 2 an outlier (40 sigma), row 3 built so that w / s lands on .5 ties: its maximum 127 * 2^e gives s = 2^e exactly,
    and (n + 1/2) 2^e is a bf16 number for |n| <= 100."""
    w[1] = 0.0
    w[2, K // 3] = 0.8
    n = portable_rng.integers(9, K, (K,), -100, 101).astype(np.float32)
    w[3] = (n + np.float32(0.5)) * np.float32(2.0 ** -9)
    w[3, K // 2] = np.float32(127.0 * 2.0 ** -9)
    return w


@pytest.fixture(scope="module", params=SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def qcase(request):
    """One weight per shape, drawn by portable_rng, quantised once by the kernel: (N, K, W bits before, W^ device, packed, scale)."""
    _need_gpu()
    from radvlm_amd import ops
    N, K = request.param
    w = portable_rng.normal(11, portable_rng.name_tag(f"w8_{N}x{K}"), (N, K), 0.02)
    w = _special_rows(w, K)
    wd = torch.from_numpy(w).to(BF16).cuda()
    before = _bits(wd)
    packed, scale = ops.quantize_rows_w8(wd)
    torch.cuda.synchronize()
    return N, K, before, wd, packed, scale


def test_quantize_kernel_bit_exact(qcase):
    N, K, before, what, packed, scale = qcase
    q, s, ref = w8_ref.quantize_rows(before)
    assert np.array_equal(_f32_bits(scale), s.view(np.uint32))
    assert np.array_equal(_bits(what), ref)
    assert packed.shape == (N, w8_ref.packed_row_bytes(K))
    assert np.array_equal(packed.cpu().numpy(), w8_ref.pack_rows(q))
    assert s[1] == np.float32(1.0) and not ref[1].any()                    # the zero row
    assert s[3] == np.float32(2.0 ** -9)                                    # the tie row: every entry but the maximum sits on a tie
    assert (q[3].astype(np.int32) % 2 == 0).sum() == K - 1


@pytest.mark.parametrize("M", [1, 2, 8, 16, 17, 32])
def test_gemv_w8_bit_identical_to_bf16_on_dequantised(qcase, M):
    from radvlm_amd import ops
    N, K, _, what, packed, scale = qcase
    g = torch.Generator().manual_seed(N * 7 + K)
    x = torch.randn(32, K, generator=g).to(BF16).cuda()
    bias = (torch.randn(N, generator=g) * 0.02).to(BF16).cuda()
    res = torch.randn(32, N, generator=g).to(BF16).cuda()
    for kw in (dict(), dict(bias=bias), dict(residual=res[:M]), dict(bias=bias, residual=res[:M]), dict(out_dtype=torch.float32),
               dict(bias=bias, out_dtype=torch.float32)):
        want = ops.gemv(x[:M], what, **kw)
        got = ops.gemv_w8(x[:M], packed, scale, K, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), (M, sorted(kw))
    if M > 1:                                                               # row r of an M-row launch is the M = 1 launch of that row
        y = ops.gemv_w8(x[:M], packed, scale, K, bias=bias, out_dtype=torch.float32)
        for r in sorted({0, M // 2, M - 1}):
            assert torch.equal(ops.gemv_w8(x[r:r + 1].contiguous(), packed, scale, K, bias=bias, out_dtype=torch.float32)[0], y[r]), r


def test_quantize_strided_fused_view():
    """A row-major view with a row stride inside a larger store (as the fused q|k|v and gate|up views of the flat parameters): the
    rows of the view are quantised, everything around them keeps its bits."""
    _need_gpu()
    from radvlm_amd import ops
    N, K, ld = 96, 448, 512
    store = torch.from_numpy(portable_rng.normal(12, 5, (N + 2, ld), 0.02)).to(BF16).cuda()
    keep = _bits(store)
    view = store[1:N + 1, 16:16 + K]
    assert view.stride(0) == ld and not view.is_contiguous()
    packed, scale = ops.quantize_rows_w8(view)
    q, s, ref = w8_ref.quantize_rows(keep[1:N + 1, 16:16 + K])
    want = keep.copy()
    want[1:N + 1, 16:16 + K] = ref
    assert np.array_equal(_bits(store), want)
    assert np.array_equal(_f32_bits(scale), s.view(np.uint32)) and np.array_equal(packed.cpu().numpy(), w8_ref.pack_rows(q))
    x = torch.randn(5, K, generator=torch.Generator().manual_seed(1)).to(BF16).cuda()
    assert torch.equal(ops.gemv_w8(x, packed, scale, K), ops.gemv(x, view))


def test_kernels_refuse_bad_arguments():
    _need_gpu()
    from radvlm_amd import lib, ops
    w = torch.zeros(8, 64, dtype=BF16, device="cuda")
    packed, scale = ops.quantize_rows_w8(w)
    x = torch.zeros(2, 64, dtype=BF16, device="cuda")
    y = torch.zeros(2, 8, dtype=BF16, device="cuda")
    with pytest.raises(lib.RadvlmHipError):                                 # a packed row stride that is not the layout's
        lib.call("rv_gemv_w8_bf16", x, 64, packed, 32, scale, y, 8, None, None, 0, 2, 8, 64, 0, None, 0)
    with pytest.raises(lib.RadvlmHipError):                                 # M > 32
        lib.call("rv_gemv_w8_bf16", x, 64, packed, 64, scale, y, 8, None, None, 0, 33, 8, 64, 0, None, 0)
    with pytest.raises(lib.RadvlmHipError):                                 # K % 8 != 0
        lib.call("rv_quantize_rows_w8_bf16", w, 64, packed, 64, scale, 8, 60)
    with pytest.raises(AssertionError):
        ops.quantize_rows_w8(w.cpu())


# ------------------------------------------------------------------------------------------------ engine
def _routes(eng, fn):
    """fn() with the int8 route and with the bf16 route forced on the same quantised engine."""
    out = []
    for flag in (True, False):
        eng.w8_decode = flag
        try:
            out.append(fn())
        finally:
            eng.w8_decode = True
    return out


def _count_w8_calls(monkeypatch):
    from radvlm_amd import ops
    calls = []
    real = ops.gemv_w8
    monkeypatch.setattr(ops, "gemv_w8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_decode_step_both_routes_bit_identical(golden_dir, case, monkeypatch):
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    assert not eng.is_quantized
    eng.quantize_decoder_()
    assert eng.is_quantized and len(eng.w8) == eng.l["layers"] and set(eng.w8[0]) == {"qkv", "o", "gu", "down"}
    calls = _count_w8_calls(monkeypatch)
    prompts = [_prompt(g, 0), _prompt(g, 1)[:-2]]
    ids, am = _pad_batch(prompts, "right")
    toks = np.random.default_rng(5).integers(0, eng.vocab, (4, 2))

    def run():
        cache, lg = eng.prefill(ids.numpy(), am.numpy(), images[:2], sizes[:2], max_new_tokens=5)
        seq = [lg.clone()]
        for t in range(4):
            seq.append(eng.decode_step(cache, toks[t].tolist()).clone())
        return seq, [l.clone() for l in cache.layers], cache.lens.copy()

    n0 = len(calls)
    (la, kva, lena), (lb, kvb, lenb) = _routes(eng, run)
    assert len(calls) - n0 == 4 * 4 * eng.l["layers"]                     # the int8 arm ran the int8 kernel, the other arm never
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert np.array_equal(lena, lenb)
    for a, b in zip(kva, kvb):
        for r in range(2):
            assert torch.equal(a[r, :lena[r]], b[r, :lena[r]])


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generation_same_tokens_on_both_routes_and_on_a_plain_engine(golden_dir, case):
    """generate() with processors, a two-turn GenerationCache conversation and generate_batch(): identical on the int8 route, on the
    bf16 route of the same engine, and on a second model that never quantised and was given the dequantised weights by
    load_state_dict(quantised.state_dict()) -- that leg runs none of the new code."""
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    model = _model(geo, kw)
    assert model.quantize_decoder_() is model and model.is_quantized
    plain = _model(geo, kw)
    missing, unexpected = plain.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    assert not missing and not unexpected and not plain.is_quantized
    p1 = _prompt(g, 0)
    proc = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, eos_token_id=None)

    def gen(m, ids, n, **k):
        return m.generate(torch.from_numpy(np.asarray(ids)[None]), images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=n,
                          output_logits=True, return_dict_in_generate=True, **k)

    def conversation(m):
        a = gen(m, p1, 12, **proc)
        cache = GenerationCache()
        t1 = gen(m, p1, 8, eos_token_id=None, past_key_values=cache)
        p2 = np.concatenate([p1, t1.sequences[0].cpu().numpy(), np.arange(5, 25, dtype=np.int64)])
        t2 = gen(m, p2, 6, eos_token_id=None, past_key_values=cache)
        reqs = [(_prompt(g, b)[:len(_prompt(g, b)) - c], images[b], sizes[b]) for b, c in ((0, 0), (1, 0), (0, 3), (1, 2))]
        out = m.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=3,
                               max_new_tokens=[6, 9, 4, 7], return_logprobs=True, **proc)
        return a, t1, t2, out

    (a8, s8, t8, o8), (ab, sb, tb, ob) = _routes(model.engine, lambda: conversation(model))
    ap, sp, tp, op = conversation(plain)
    for x, y, z in ((a8, ab, ap), (s8, sb, sp), (t8, tb, tp)):
        assert torch.equal(x.sequences, y.sequences) and torch.equal(x.sequences, z.sequences)
        assert all(torch.equal(u, v) for u, v in zip(x.logits, y.logits)) and all(torch.equal(u, v) for u, v in zip(x.logits, z.logits))
    for k in o8:
        assert o8[k].generated_tokens == ob[k].generated_tokens == op[k].generated_tokens
        assert o8[k].logprobs == ob[k].logprobs == op[k].logprobs and len(o8[k].logprobs) == len(o8[k].generated_tokens)


def test_quantised_model_differs_from_the_original_but_state_dict_is_dequantised(golden_dir):
    """quantize_decoder_ changes the four matrices of every layer (and nothing else) to W^ of the restatement."""
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    eng = _engine("toy_qwen", **kw)
    sd0 = {k: v.clone() for k, v in eng.state_dict().items()}
    eng.quantize_decoder_()
    sd1 = eng.state_dict()
    assert set(sd0) == set(sd1)
    changed = 0
    for k in sd0:
        linear = k.startswith("model.layers.") and k.endswith("_proj.weight")
        if not linear:
            assert torch.equal(sd0[k], sd1[k]), k
            continue
        changed += 1
        assert not torch.equal(sd0[k], sd1[k]), k
    assert changed == 7 * eng.l["layers"]
    # the scale is per output row, so the fused q|k|v and gate|up stores quantise as their seven separate matrices would
    for k in sd0:
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            _, _, ref = w8_ref.quantize_rows(_bits(sd0[k]))
            assert np.array_equal(_bits(sd1[k]), ref), k


# ------------------------------------------------------------------------------------------------ state
def test_quantize_twice_and_unmerged_lora_raise(golden_dir):
    from test_lora_merge_gpu import _model as _lora_model
    model = _model("toy", {})
    model.quantize_decoder_()
    with pytest.raises(RuntimeError, match="already quantised"):
        model.quantize_decoder_()
    lora = _lora_model("toy", lora=dict(r=8, alpha=16, dropout=0.0))
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        lora.quantize_decoder_()
    assert not lora.is_quantized
    lora.merge_and_unload().quantize_decoder_()                             # merged: the base store is quantised
    assert lora.is_quantized


@pytest.mark.parametrize("change", ["load_state_dict", "optimizer_step", "merge_lora_", "resize_token_embeddings"])
def test_weight_change_drops_the_int8_copies(golden_dir, change, monkeypatch):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    eng = model.engine
    model.quantize_decoder_()
    v = eng.weights_version
    what = {k: t.clone() for k, t in eng.state_dict().items()}
    if change == "load_state_dict":
        eng.load_state_dict({k: t.clone() for k, t in eng.state_dict().items()})
    elif change == "optimizer_step":
        eng.optimizer_step(lr=1e-3)                                         # zero gradients: the values stay, the version moves
    elif change == "merge_lora_":
        d = eng.l["d"]
        A = torch.from_numpy(portable_rng.normal(3, 1, (8, d), 0.05)).to(BF16)
        B = torch.from_numpy(portable_rng.normal(3, 2, (d, 8), 0.05)).to(BF16)
        eng.merge_lora_({"model.layers.0.self_attn.o_proj": (A, B)}, 0.5)
    else:
        eng.resize_token_embeddings(eng.vocab + 8)
    assert not model.is_quantized and eng.w8 is None and eng.weights_version > v
    if change in ("load_state_dict", "optimizer_step"):                    # the values stay the dequantised ones (the fp32 master copy too)
        after = eng.state_dict()
        assert all(torch.equal(what[k], after[k]) for k in what)
    calls = _count_w8_calls(monkeypatch)
    p = _prompt(g, 0)
    model.generate(torch.from_numpy(p[None]), images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=4, eos_token_id=None)
    assert not calls                                                        # a plain bf16 engine again


def test_generation_cache_from_before_quantisation_is_emptied(golden_dir):
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    p1 = _prompt(g, 0)
    gen = lambda ids, n, **k: model.generate(torch.from_numpy(np.asarray(ids)[None]), images=[images[0]], image_sizes=[sizes[0]],
                                             max_new_tokens=n, eos_token_id=None, output_logits=True, return_dict_in_generate=True, **k)
    cache = GenerationCache()
    t1 = gen(p1, 8, past_key_values=cache)
    model.quantize_decoder_()
    p2 = np.concatenate([p1, t1.sequences[0].cpu().numpy(), np.arange(5, 25, dtype=np.int64)])
    got = gen(p2, 6, past_key_values=cache)                                 # the cached K|V are of the unquantised weights: dropped
    fresh = gen(p2, 6)
    assert torch.equal(got.sequences, fresh.sequences)
    assert all(torch.equal(a, b) for a, b in zip(got.logits, fresh.logits))


# ------------------------------------------------------------------------------------------------ loader
def test_load_pretrained_model_load_8bit(golden_dir, tmp_path):
    from radvlm_amd.llava.model.builder import load_pretrained_model
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    src = _model("toy_qwen", kw)
    prompt = torch.from_numpy(_prompt(g, 0)[None])
    gen = lambda m: m.generate(prompt, images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=12, eos_token_id=None).cpu()
    want_plain = gen(src)
    ckpt = str(tmp_path / "ckpt")
    src.save_pretrained(ckpt)
    _, m8, _, _ = load_pretrained_model(ckpt, device="cuda:0", load_8bit=True)
    assert m8.is_quantized
    _, later, _, _ = load_pretrained_model(ckpt, device="cuda:0")
    assert not later.is_quantized
    assert torch.equal(gen(later), want_plain)                              # without the flag: the model as it was
    _, off, _, _ = load_pretrained_model(ckpt, device="cuda:0", load_8bit=False, load_4bit=True)
    assert not off.is_quantized and torch.equal(gen(off), want_plain)
    later.quantize_decoder_()
    assert torch.equal(gen(m8), gen(later))
    sd8, sdl = m8.state_dict(), later.state_dict()
    assert all(torch.equal(sd8[k], sdl[k]) for k in sd8)


# ------------------------------------------------------------------------------------------------ full width
@pytest.mark.parametrize("gname", ["llava15_7b", "llava_ov_qwen2_7b"])
def test_full_width_decode_step_both_routes(gname):
    """One 7B-width decoder layer + the full head: a decode step on the int8 route and on the bf16 route, bit-identical."""
    _need_gpu()
    from radvlm_amd.engine import LlavaEngine
    geo = copy.deepcopy(GEOMETRIES[gname])
    geo["lm"]["layers"] = 1
    geo["vision"]["layers"] = 2
    eng = LlavaEngine(geo, device="cuda:0", init="fast", seed=0)
    eng.quantize_decoder_()
    ids = np.random.default_rng(0).integers(0, eng.vocab, (8, 48))
    toks = np.random.default_rng(1).integers(0, eng.vocab, (2, 8))

    def run():
        cache, lg = eng.prefill(ids, None, None, None, max_new_tokens=3)
        out = [lg.clone()] + [eng.decode_step(cache, toks[t].tolist()).clone() for t in range(2)]
        return out, cache.layers[0].clone()

    (la, kva), (lb, kvb) = _routes(eng, run)
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and torch.equal(kva, kvb)
    assert all(bool(torch.isfinite(a).all()) for a in la)

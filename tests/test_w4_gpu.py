"""GPU tests of the MXFP4 decoder weights (quantization="mxfp4"): rv_quantize_rows_mxfp4_bf16 bit-exact against the numpy restatement
(tests/w4_ref.py), rv_gemv_w4_bf16 bit-identical to rv_gemv_bf16 on the quantised weight, and the engine / model / loader on the toy
goldens: every comparison is exact, and the oracle is the existing bf16 path run on the quantised weights."""
import copy

import numpy as np
import pytest
import torch

import w4_ref
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


def _toy_shapes():
    out = []
    for geo in ("toy", "toy_qwen"):
        l = GEOMETRIES[geo]["lm"]
        d, F, H = l["d"], l["ffn"], l["heads"]
        kvd = l.get("kv_heads", H) * (d // H)
        out += [(d + 2 * kvd, d), (d, d), (2 * F, d), (d, F)]
    return sorted(set(out))


# (100, 40): K ends inside a step and ks = 2, so two of the four waves have empty ranges; (8, 8): one short block; (72, 416): ks = 13, the
# waves start at step residues 0, 3, 2, 1 mod 4; (130, 1184): rv_gemv_split = 2 with ragged unit starts; the toy geometries' matrices;
# the 7B down_proj.  WIDE: the two widest 7B-width decoder shapes, GEMV at M = 1 and 32 only.
SHAPES = [(100, 40), (8, 8), (72, 416), (130, 1184)] + _toy_shapes() + [(4096, 11008)]
WIDE = [(22016, 4096), (3584, 18944)]
TIE = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
TIE_CODES = [0, 2, 2, 4, 4, 6, 6]


def _special_blocks(w, K):
    """The first block (k < min(K, 32)) of rows 1..6.  Row 1: zeros.  Row 2: a 40 sigma outlier.  Row 3: saturation, 7.5 * 2^-4 with
    5.5 * 2^-4 beside it.  Rows 4 and 5: 4 * 2^-9 and the seven ties of the value grid times 2^-9 (the block's largest entry is the
    tie 5 * 2^-9, in the binade of 4 * 2^-9, so e = -9), positive in row 4 and negative in row 5, the rest of the block zero.  Row 6:
    negative values that round to zero (a tie at -0.25, a small one and -0.0) under a maximum of 2^-5."""
    nb = min(K, 32)
    w[1, :nb] = 0.0
    w[2, 2] = 0.8
    w[3, 0], w[3, 1] = 7.5 * 2.0 ** -4, -5.5 * 2.0 ** -4
    for r, sgn in ((4, 1.0), (5, -1.0)):
        w[r, :nb] = 0.0
        w[r, 0] = 4.0 * 2.0 ** -9
        w[r, 1:8] = sgn * TIE * np.float32(2.0 ** -9)
    w[6, :nb] = 0.0
    w[6, :4] = [2.0 ** -5, -(2.0 ** -9), -(2.0 ** -13), -0.0]
    return w


def _weight(N, K):
    w = portable_rng.normal(11, portable_rng.name_tag(f"w4_{N}x{K}"), (N, K), 0.02)
    return torch.from_numpy(_special_blocks(w, K)).to(BF16).cuda()


@pytest.fixture(scope="module", params=SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def qcase(request):
    """One weight per shape, drawn by portable_rng, quantised once by the kernel: (N, K, W bits before, W^ device, packed, scales)."""
    _need_gpu()
    from radvlm_amd import ops
    N, K = request.param
    wd = _weight(N, K)
    before = _bits(wd)
    packed, scales = ops.quantize_rows_mxfp4(wd)
    torch.cuda.synchronize()
    return N, K, before, wd, packed, scales


@pytest.fixture(scope="module", params=WIDE, ids=[f"{n}x{k}" for n, k in WIDE])
def widecase(request):
    _need_gpu()
    from radvlm_amd import ops
    N, K = request.param
    wd = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.02).to(BF16).cuda()
    packed, scales = ops.quantize_rows_mxfp4(wd)
    return N, K, None, wd, packed, scales


def test_quantize_kernel_bit_exact(qcase):
    N, K, before, what, packed, scales = qcase
    nib, sb, ref = w4_ref.quantize_rows(before)
    assert np.array_equal(_bits(what), ref)
    assert packed.shape == (N, w4_ref.packed_row_bytes(K)) and scales.shape == (N, w4_ref.scale_row_bytes(K))
    want_p, want_s = w4_ref.pack_rows(nib, sb)
    assert np.array_equal(scales.cpu().numpy(), want_s)
    assert np.array_equal(packed.cpu().numpy(), want_p)
    nb = min(K, 32)
    assert sb[1, 0] == 127 and not nib[1, :nb].any() and not ref[1, :nb].any()                 # the zero block
    assert sb[2, 0] == 127 - 3 and nib[2, 2] == 7                                               # the outlier block: 0.8 = 6.4 * 2^-3 saturates
    assert sb[3, 0] == 127 - 4 and nib[3, 0] == 7 and nib[3, 1] == (8 | 7)                      # 7.5 and 5.5 both go to code 7
    for r, s in ((4, 0), (5, 8)):                                                               # the ties go to the even code
        assert sb[r, 0] == 127 - 9 and nib[r, 0] == 6
        assert nib[r, 1:8].tolist() == [c | s if c else 0 for c in TIE_CODES]
    assert nib[6, :4].tolist() == [6, 0, 0, 0] and ref[6, 1:4].tolist() == [0, 0, 0]           # negative values that round to zero: +0.0


def _gemv_identity(case, M, kws):
    from radvlm_amd import ops
    N, K, _, what, packed, scales = case
    g = torch.Generator().manual_seed(N * 7 + K)
    x = torch.randn(32, K, generator=g).to(BF16).cuda()
    bias = (torch.randn(N, generator=g) * 0.02).to(BF16).cuda()
    res = torch.randn(32, N, generator=g).to(BF16).cuda()
    named = dict(plain=dict(), bias=dict(bias=bias), res=dict(residual=res[:M]), both=dict(bias=bias, residual=res[:M]),
                 f32=dict(out_dtype=torch.float32), bias_f32=dict(bias=bias, out_dtype=torch.float32))
    for name in kws:
        kw = named[name]
        want = ops.gemv(x[:M], what, **kw)
        got = ops.gemv_w4(x[:M], packed, scales, K, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), (M, name)
    if M > 1:                                                               # row r of an M-row launch is the M = 1 launch of that row
        y = ops.gemv_w4(x[:M], packed, scales, K, bias=bias, out_dtype=torch.float32)
        for r in sorted({0, M // 2, M - 1}):
            assert torch.equal(ops.gemv_w4(x[r:r + 1].contiguous(), packed, scales, K, bias=bias, out_dtype=torch.float32)[0], y[r]), r


@pytest.mark.parametrize("M", [1, 5, 16, 17, 32])
def test_gemv_w4_bit_identical_to_bf16_on_quantised(qcase, M):
    _gemv_identity(qcase, M, ("plain", "bias", "res", "both", "f32", "bias_f32"))


@pytest.mark.parametrize("M", [1, 32])
def test_gemv_w4_bit_identical_at_7b_width(widecase, M):
    _gemv_identity(widecase, M, ("plain", "bias_f32"))


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
    packed, scales = ops.quantize_rows_mxfp4(view)
    nib, sb, ref = w4_ref.quantize_rows(keep[1:N + 1, 16:16 + K])
    want = keep.copy()
    want[1:N + 1, 16:16 + K] = ref
    assert np.array_equal(_bits(store), want)
    want_p, want_s = w4_ref.pack_rows(nib, sb)
    assert np.array_equal(packed.cpu().numpy(), want_p) and np.array_equal(scales.cpu().numpy(), want_s)
    x = torch.randn(5, K, generator=torch.Generator().manual_seed(1)).to(BF16).cuda()
    assert torch.equal(ops.gemv_w4(x, packed, scales, K), ops.gemv(x, view))


def test_kernels_refuse_bad_arguments():
    _need_gpu()
    from radvlm_amd import lib, ops
    w = torch.zeros(8, 64, dtype=BF16, device="cuda")
    packed, scales = ops.quantize_rows_mxfp4(w)
    assert packed.shape == (8, 64) and scales.shape == (8, 4)
    x = torch.zeros(2, 64, dtype=BF16, device="cuda")
    y = torch.zeros(2, 8, dtype=BF16, device="cuda")
    lib.call("rv_gemv_w4_bf16", x, 64, packed, 64, scales, 4, y, 8, None, None, 0, 2, 8, 64, 0, None, 0)        # the accepted call
    with pytest.raises(lib.RadvlmHipError):                                 # a packed row stride that is not the layout's
        lib.call("rv_gemv_w4_bf16", x, 64, packed, 32, scales, 4, y, 8, None, None, 0, 2, 8, 64, 0, None, 0)
    with pytest.raises(lib.RadvlmHipError):                                 # a scale row stride that is not the layout's
        lib.call("rv_gemv_w4_bf16", x, 64, packed, 64, scales, 2, y, 8, None, None, 0, 2, 8, 64, 0, None, 0)
    with pytest.raises(lib.RadvlmHipError):                                 # M > 32
        lib.call("rv_gemv_w4_bf16", x, 64, packed, 64, scales, 4, y, 8, None, None, 0, 33, 8, 64, 0, None, 0)
    with pytest.raises(lib.RadvlmHipError):                                 # K % 8 != 0
        lib.call("rv_quantize_rows_mxfp4_bf16", w, 64, packed, 64, scales, 4, 8, 60)
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_quantize_rows_mxfp4_bf16", w, 64, packed, 32, scales, 4, 8, 64)
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_quantize_rows_mxfp4_bf16", w, 64, packed, 64, scales, 8, 8, 64)
    with pytest.raises(AssertionError):
        ops.quantize_rows_mxfp4(w.cpu())
    with pytest.raises(AssertionError):
        ops.gemv_w4(x.cpu(), packed, scales, 64)


# ------------------------------------------------------------------------------------------------ engine
def _routes(eng, fn):
    """fn() with the 4-bit route and with the bf16 route forced on the same quantised engine."""
    out = []
    for flag in (True, False):
        eng.w4_decode = flag
        try:
            out.append(fn())
        finally:
            eng.w4_decode = True
    return out


def _count_w4_calls(monkeypatch):
    from radvlm_amd import ops
    calls = []
    real = ops.gemv_w4
    monkeypatch.setattr(ops, "gemv_w4", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_decode_step_and_verify_step_both_routes_bit_identical(golden_dir, case, monkeypatch):
    g, images, sizes, kw = _load(golden_dir, case)
    eng = _engine(CASES[case]["geo"], **kw)
    assert not eng.is_quantized
    eng.quantize_decoder_("mxfp4")
    assert eng.is_quantized and eng.w8 is None and len(eng.w4) == eng.l["layers"] and set(eng.w4[0]) == {"qkv", "o", "gu", "down"}
    assert all(p.dtype == torch.uint8 and s.dtype == torch.uint8 for p, s in eng.w4[0].values())
    calls = _count_w4_calls(monkeypatch)
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
    assert len(calls) - n0 == 4 * 4 * eng.l["layers"]                     # the 4-bit arm ran the 4-bit kernel, the other arm never
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert np.array_equal(lena, lenb)
    for a, b in zip(kva, kvb):
        for r in range(2):
            assert torch.equal(a[r, :lena[r]], b[r, :lena[r]])

    def verify():
        cache, lg = eng.prefill(ids.numpy()[:1], am.numpy()[:1], images[:1], sizes[:1], max_new_tokens=8)
        out = eng.verify_step(cache, toks[:, 0].tolist() + [3]).clone()
        n = int(cache.lens[0]) + 5
        return out, [l[0, :n].clone() for l in cache.layers]

    n0 = len(calls)
    (va, ca), (vb, cb) = _routes(eng, verify)
    assert len(calls) - n0 == 4 * eng.l["layers"]
    assert torch.equal(va, vb) and all(torch.equal(a, b) for a, b in zip(ca, cb))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generation_same_tokens_on_both_routes_and_on_a_plain_engine(golden_dir, case):
    """generate() with processors, a two-turn GenerationCache conversation, generate_batch() on an int8 KV cache and two-beam search:
    identical on the 4-bit route, on the bf16 route of the same engine, and on a second model that never quantised and was given the
    quantised weights by load_state_dict(quantised.state_dict()) -- that leg runs none of the new code."""
    from radvlm_amd.generation import GenerationCache
    g, images, sizes, kw = _load(golden_dir, case)
    geo = CASES[case]["geo"]
    model = _model(geo, kw)
    assert model.quantize_decoder_("mxfp4") is model and model.is_quantized
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
                               max_new_tokens=[6, 9, 4, 7], return_logprobs=True, kv_cache_dtype="int8", **proc)
        beams = m.generate_beams(torch.from_numpy(p1[None]), images=[images[0]], image_sizes=[sizes[0]], num_beams=2, max_new_tokens=6,
                                 eos_token_id=None, return_dict_in_generate=True, output_scores=True, output_logits=True)
        return a, t1, t2, out, beams

    (a4, s4, t4, o4, b4), (ab, sb, tb, ob, bb) = _routes(model.engine, lambda: conversation(model))
    ap, sp, tp, op, bp = conversation(plain)
    for x, y, z in ((a4, ab, ap), (s4, sb, sp), (t4, tb, tp)):
        assert torch.equal(x.sequences, y.sequences) and torch.equal(x.sequences, z.sequences)
        assert all(torch.equal(u, v) for u, v in zip(x.logits, y.logits)) and all(torch.equal(u, v) for u, v in zip(x.logits, z.logits))
    for k in o4:
        assert o4[k].generated_tokens == ob[k].generated_tokens == op[k].generated_tokens
        assert o4[k].logprobs == ob[k].logprobs == op[k].logprobs and len(o4[k].logprobs) == len(o4[k].generated_tokens)
    for field in ("sequences", "sequences_scores", "scores", "logits"):
        x = getattr(b4, field)
        assert x is not None and _same(x, getattr(bb, field)) and _same(x, getattr(bp, field)), field


def test_quantised_model_differs_from_the_original_but_state_dict_is_the_restatement(golden_dir):
    """quantize_decoder_("mxfp4") changes the seven matrices of every layer (and nothing else) to W^ of the restatement."""
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    eng = _engine("toy_qwen", **kw)
    sd0 = {k: v.clone() for k, v in eng.state_dict().items()}
    eng.quantize_decoder_("mxfp4")
    sd1 = eng.state_dict()
    assert set(sd0) == set(sd1)
    changed = 0
    for k in sd0:
        if not (k.startswith("model.layers.") and k.endswith("_proj.weight")):
            assert torch.equal(sd0[k], sd1[k]), k
            continue
        changed += 1
        assert not torch.equal(sd0[k], sd1[k]), k
        # the scale is per block of a row, so the fused q|k|v and gate|up stores quantise as their seven separate matrices would
        _, _, ref = w4_ref.quantize_rows(_bits(sd0[k]))
        assert np.array_equal(_bits(sd1[k]), ref), k
    assert changed == 7 * eng.l["layers"]


# ------------------------------------------------------------------------------------------------ state
def test_quantize_twice_in_either_format_and_unmerged_lora_raise(golden_dir):
    from test_lora_merge_gpu import _model as _lora_model
    for first in ("mxfp4", "int8"):
        model = _model("toy", {})
        model.quantize_decoder_(first)
        for second in ("mxfp4", "int8"):
            with pytest.raises(RuntimeError, match="already quantised"):
                model.quantize_decoder_(second)
        assert (model.engine.w4 is None) == (first == "int8") and (model.engine.w8 is None) == (first == "mxfp4")
    with pytest.raises(ValueError, match="fmt"):
        _model("toy", {}).quantize_decoder_("nf4")
    lora = _lora_model("toy", lora=dict(r=8, alpha=16, dropout=0.0))
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        lora.quantize_decoder_("mxfp4")
    assert not lora.is_quantized
    lora.merge_and_unload().quantize_decoder_("mxfp4")                     # merged: the base store is quantised
    assert lora.is_quantized and lora.engine.w4 is not None


@pytest.mark.parametrize("change", ["load_state_dict", "optimizer_step", "merge_lora_", "resize_token_embeddings"])
def test_weight_change_drops_the_4bit_copies(golden_dir, change, monkeypatch):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    eng = model.engine
    model.quantize_decoder_("mxfp4")
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
    assert not model.is_quantized and eng.w4 is None and eng.w8 is None and eng.weights_version > v
    if change in ("load_state_dict", "optimizer_step"):                    # the values stay the quantised ones (the fp32 master copy too)
        after = eng.state_dict()
        assert all(torch.equal(what[k], after[k]) for k in what)
    calls = _count_w4_calls(monkeypatch)
    p = _prompt(g, 0)
    model.generate(torch.from_numpy(p[None]), images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=4, eos_token_id=None)
    assert not calls                                                        # a plain bf16 engine again


# ------------------------------------------------------------------------------------------------ loader
def test_load_pretrained_model_quantization(golden_dir, tmp_path):
    from radvlm_amd.llava.model.builder import load_pretrained_model
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    src = _model("toy_qwen", kw)
    prompt = torch.from_numpy(_prompt(g, 0)[None])
    gen = lambda m: m.generate(prompt, images=[images[0]], image_sizes=[sizes[0]], max_new_tokens=12, eos_token_id=None).cpu()
    want_plain = gen(src)
    ckpt = str(tmp_path / "ckpt")
    src.save_pretrained(ckpt)
    _, m4, _, _ = load_pretrained_model(ckpt, device="cuda:0", quantization="mxfp4")
    assert m4.is_quantized and m4.engine.w4 is not None and m4.engine.w8 is None
    _, later, _, _ = load_pretrained_model(ckpt, device="cuda:0")
    assert not later.is_quantized and torch.equal(gen(later), want_plain)
    _, off, _, _ = load_pretrained_model(ckpt, device="cuda:0", load_4bit=True)                # still accepted and ignored
    assert not off.is_quantized and torch.equal(gen(off), want_plain)
    later.quantize_decoder_("mxfp4")
    assert torch.equal(gen(m4), gen(later))
    sd4, sdl = m4.state_dict(), later.state_dict()
    assert all(torch.equal(sd4[k], sdl[k]) for k in sd4)
    _, a8, _, _ = load_pretrained_model(ckpt, device="cuda:0", quantization="int8")
    _, b8, _, _ = load_pretrained_model(ckpt, device="cuda:0", load_8bit=True)
    _, c8, _, _ = load_pretrained_model(ckpt, device="cuda:0", load_8bit=True, quantization="int8")
    for m in (a8, b8, c8):
        assert m.is_quantized and m.engine.w8 is not None and m.engine.w4 is None
    sda, sdb, sdc = a8.state_dict(), b8.state_dict(), c8.state_dict()
    assert all(torch.equal(sda[k], sdb[k]) and torch.equal(sda[k], sdc[k]) for k in sda) and torch.equal(gen(a8), gen(b8))
    with pytest.raises(ValueError, match="load_8bit"):
        load_pretrained_model(ckpt, device="cuda:0", load_8bit=True, quantization="mxfp4")
    for bad in ("nf4", "fp4", "4bit", ""):
        with pytest.raises(ValueError, match="quantization"):
            load_pretrained_model(ckpt, device="cuda:0", quantization=bad)


# ------------------------------------------------------------------------------------------------ full width
@pytest.mark.parametrize("gname", ["llava15_7b", "llava_ov_qwen2_7b"])
def test_full_width_decode_step_both_routes(gname):
    """One 7B-width decoder layer + the full head: a decode step on the 4-bit route and on the bf16 route, bit-identical."""
    _need_gpu()
    from radvlm_amd.engine import LlavaEngine
    geo = copy.deepcopy(GEOMETRIES[gname])
    geo["lm"]["layers"] = 1
    geo["vision"]["layers"] = 2
    eng = LlavaEngine(geo, device="cuda:0", init="fast", seed=0)
    eng.quantize_decoder_("mxfp4")
    ids = np.random.default_rng(0).integers(0, eng.vocab, (8, 48))
    toks = np.random.default_rng(1).integers(0, eng.vocab, (2, 8))

    def run():
        cache, lg = eng.prefill(ids, None, None, None, max_new_tokens=3)
        out = [lg.clone()] + [eng.decode_step(cache, toks[t].tolist()).clone() for t in range(2)]
        return out, cache.layers[0].clone()

    (la, kva), (lb, kvb) = _routes(eng, run)
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and torch.equal(kva, kvb)
    assert all(bool(torch.isfinite(a).all()) for a in la)

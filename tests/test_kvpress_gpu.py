"""GPU tests of prompt cache compression (prompt_kv_budget / prompt_kv_window / prompt_kv_pool) on the toy goldens: `toy` (llava heads,
hd 128, one query head per kv head) and `toy_qwen` (GQA, hd 64, two query heads per kv head).  A budget no prompt exceeds changes no
bit and launches none of the three kernels.  Below it, the call is replayed by hand: the device votes of each layer go through
tests/kvpress_ref.select, the plain prompt pass's full cache is indexed with torch into a compact one, pos_off is set and decode_step
is called by hand -- every step's raw logits and the compact cache rows must be generate()'s bit for bit, which pins the gather, the
slot / position split and the RoPE offset whatever the votes' last bits are.  The batch is two left-padded prompts of different
lengths, so that one budget leaves one of them whole."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import kvpress_ref as R
from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu
CASES = {"toy": "toy_e2e", "toy_qwen": "toy_qwen_e2e"}
T_NEW = 4
W, K = 8, 3


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def _new_model(geo):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
    l = GEOMETRIES[geo]["lm"]
    cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0))
    return Model(cfg, device="cuda:0", init="portable", seed=0).eval()


@functools.lru_cache(maxsize=None)
def _model(geo):
    return _new_model(geo)


@functools.lru_cache(maxsize=None)
def _inputs(geo):
    """Two prompts of different lengths, left-padded, with their images: generate()'s arguments."""
    golden_dir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(golden_dir, CASES[geo] + ".npz"))
    json.load(open(os.path.join(golden_dir, CASES[geo] + "_gradnorms.json")))
    prompts = [g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64) for b in range(2)]
    prompts[1] = prompts[1][:-3]
    T = max(p.size for p in prompts)
    ids, am = np.zeros((2, T), dtype=np.int64), np.zeros((2, T), dtype=bool)
    for b, p in enumerate(prompts):
        ids[b, T - p.size:], am[b, T - p.size:] = p, True
    images = [torch.from_numpy(g[f"image{i}"]) for i in range(2)]
    sizes = [tuple(s) for s in g["image_sizes"].tolist()][:2]
    return dict(inputs=torch.from_numpy(ids), attention_mask=torch.from_numpy(am), images=images, image_sizes=sizes)


def _lens(model, geo):
    inp = _inputs(geo)
    plan = model.engine.plan(inp["inputs"].numpy(), inp["attention_mask"].numpy(), None, inp["images"], inp["image_sizes"])
    return plan["lens"].astype(np.int64)


def _budget(model, geo, which):
    """mixed: the shorter prompt's length, so it stays whole and the longer one is compressed; both: 24 (less under a short prompt)."""
    lens = _lens(model, geo)
    assert lens.min() < lens.max() and lens.min() > W + 3
    return int(lens.min()) if which == "mixed" else int(min(24, lens.min() - 2))


def _generate(model, geo, **kw):
    kw.setdefault("eos_token_id", None)
    return model.generate(**_inputs(geo), max_new_tokens=T_NEW, return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)


def _prefill(eng, geo, **kw):
    inp = _inputs(geo)
    return eng.prefill(inp["inputs"].numpy(), inp["attention_mask"].numpy(), inp["images"], inp["image_sizes"], max_new_tokens=T_NEW, **kw)


def _count(monkeypatch, name):
    from radvlm_amd import ops
    calls = []
    real = getattr(ops, name)
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


# ------------------------------------------------------------------------------------------------ a budget no prompt exceeds
@pytest.mark.parametrize("geo", list(CASES))
def test_budget_at_least_every_prompt_changes_nothing(geo, monkeypatch):
    model = _model(geo)
    eng = model.engine
    longest = int(_lens(model, geo).max())
    base = _generate(model, geo)
    c0, l0 = _prefill(eng, geo)
    calls = [_count(monkeypatch, n) for n in ("kv_votes", "kv_select", "kv_gather")]
    for N in (longest, longest + 100):
        out = _generate(model, geo, prompt_kv_budget=N, prompt_kv_window=W, prompt_kv_pool=K)
        assert torch.equal(out.sequences, base.sequences)
        for x, y in zip(out.scores + out.logits, base.scores + base.logits):
            assert torch.equal(_bits(x), _bits(y))
        c1, l1 = _prefill(eng, geo, compress=(N, W, K))
        assert c1.pos_off is None and c1.L_max == c0.L_max and np.array_equal(c1.lens, c0.lens) and torch.equal(_bits(l1), _bits(l0))
        for a, b in zip(c1.layers, c0.layers):
            assert torch.equal(_bits(a), _bits(b))
    assert not any(calls)                                                   # none of the three kernels was launched


# ------------------------------------------------------------------------------------------------ replay
def _replay(model, geo, N, **kw):
    """generate(prompt_kv_budget=N, ...) against the hand-built compact cache; returns the output."""
    eng = model.engine
    d, kvd, hd, Hkv, L = eng.l["d"], eng.kvd, eng.hd, eng.Hkv, eng.l["layers"]
    lens = _lens(model, geo)
    kept = np.minimum(lens, N)
    assert (lens > N).any()
    out = _generate(model, geo, prompt_kv_budget=N, prompt_kv_window=W, prompt_kv_pool=K, **kw)
    # the engine's own compressed prompt pass, with the votes of every layer
    eng.kvpress_trace = []
    try:
        cc, lc = _prefill(eng, geo, compress=(N, W, K))
        trace = eng.kvpress_trace
    finally:
        eng.kvpress_trace = None
    assert [t[0] for t in trace] == list(range(L))
    assert np.array_equal(cc.lens, kept) and np.array_equal(cc.pos_off, lens - kept) and cc.L_max == int(kept.max()) + T_NEW
    # the plain prompt pass: the full cache and the first step's logits
    full, lf = _prefill(eng, geo)
    assert torch.equal(_bits(lf), _bits(lc)) and torch.equal(_bits(lf), _bits(out.logits[0]))
    from radvlm_amd.engine import KVCache
    layers = []
    for i in range(L):
        votes = trace[i][1].cpu().numpy()
        kv = torch.zeros(2, cc.L_max, 2 * kvd, dtype=torch.bfloat16, device=full.layers[i].device)
        for b in range(2):
            P = int(lens[b])
            if P <= N:
                kv[b, :P] = full.layers[i][b, :P]
                continue
            for g in range(Hkv):
                keep = R.select(votes[b, g, :P - W], N, W, K)
                assert np.array_equal(trace[i][2][b, g].cpu().numpy(), keep)        # the device selection on the same votes
                idx = torch.from_numpy(keep).to(kv.device)
                for off in (0, kvd):
                    kv[b, :N, off + g * hd:off + (g + 1) * hd] = full.layers[i][b][idx, off + g * hd:off + (g + 1) * hd]
            assert (np.diff(keep) > 0).all() and keep[-W:].tolist() == list(range(P - W, P))
        # the compact cache rows are the engine's, bit for bit (rows past a sequence's slots are zeros in both)
        assert torch.equal(_bits(kv), _bits(cc.layers[i])), i
        layers.append(kv)
    mine = KVCache(layers, kept, cc.L_max)
    mine.pos_off = (lens - kept).astype(np.int64)
    seq = out.sequences.cpu().numpy()
    assert seq.shape == (2, T_NEW)
    for t in range(T_NEW - 1):
        lg = eng.decode_step(mine, seq[:, t])
        assert torch.equal(_bits(lg), _bits(out.logits[t + 1])), t
        assert np.array_equal(mine.lens, kept + t + 1)
    return out


@pytest.mark.parametrize("which", ["mixed", "both"])
@pytest.mark.parametrize("geo", list(CASES))
def test_replay(geo, which):
    model = _model(geo)
    N = _budget(model, geo, which)
    out = _replay(model, geo, N)
    base = _generate(model, geo)
    assert torch.equal(_bits(out.logits[0]), _bits(base.logits[0]))         # the first token comes from the uncompressed prompt pass
    lens = _lens(model, geo)
    dropped = [b for b in range(2) if lens[b] > N]
    # later steps read fewer keys: the compressed rows' logits move (the mode is lossy), a whole row's do not
    for b in range(2):
        same = all(torch.equal(_bits(x[b]), _bits(y[b])) for x, y in zip(out.logits[1:], base.logits[1:]))
        if b not in dropped and torch.equal(out.sequences[b], base.sequences[b]):
            assert same
    assert any(not torch.equal(_bits(out.logits[1][b]), _bits(base.logits[1][b])) for b in dropped)


def test_rope_offset_matters():
    """The same compact cache with pos_off zeroed gives other logits: the replay above would not pass on slot positions."""
    geo = "toy_qwen"
    model = _model(geo)
    eng = model.engine
    N = _budget(model, geo, "both")
    tok = np.array([5, 7])
    a, _ = _prefill(eng, geo, compress=(N, W, K))
    b, _ = _prefill(eng, geo, compress=(N, W, K))
    assert a.pos_off.min() > 0
    b.pos_off[:] = 0
    assert not torch.equal(_bits(eng.decode_step(a, tok)), _bits(eng.decode_step(b, tok)))


# ------------------------------------------------------------------------------------------------ composition
def _choices():
    return [[5, 6, 7, 8, 9, 10, 11], [5, 6, 12, 13, 14, 15, 16], [17, 18, 19, 20, 21, 22, 23]]


def _compose(mode):
    if mode == "sampled":
        return dict(do_sample=True, seed=11, top_k=20)
    if mode == "processed":
        return dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[3]])
    from radvlm_amd.constraints import TokenConstraint
    return dict(eos_token_id=999, constraint=TokenConstraint.from_choices(_choices(), eos=[999]))


@pytest.mark.parametrize("mode", ["sampled", "processed", "constrained"])
@pytest.mark.parametrize("geo", list(CASES))
def test_composition_replays(geo, mode):
    model = _model(geo)
    out = _replay(model, geo, _budget(model, geo, "both"), **_compose(mode))
    if mode == "constrained":
        for row in out.sequences.cpu().tolist():
            assert any(row == c[:T_NEW] for c in _choices())


def test_composition_quantized_decoder_replays():
    model = _new_model("toy")
    model.quantize_decoder_()
    _replay(model, "toy", _budget(model, "toy", "both"))


def test_composition_live_lora_adapters_replays():
    """Decoding on live, unmerged adapters (r = 8, the non-zero adapters of test_lora_merge_gpu) with a compressed prompt cache."""
    from test_lora_merge_gpu import _model as lora_model, _set_adapters
    model = lora_model("toy_qwen", lora=dict(r=8, alpha=16, dropout=0.0)).enable_adapter_decoding()
    _set_adapters(model.engine)
    _replay(model, "toy_qwen", _budget(model, "toy_qwen", "both"))


# ------------------------------------------------------------------------------------------------ generate_batch
@pytest.mark.parametrize("geo", list(CASES))
def test_generate_batch_equals_generate_alone(geo, monkeypatch):
    """Three requests on two slots: each request's tokens are those of generate() on it alone with the same three values, up to the
    alone run's first near tie (the rule of test_generate_batch_gpu._compare), and the slots' cache is smaller than without the keyword."""
    from test_generate_batch_gpu import _compare
    model = _model(geo)
    eng = model.engine
    inp = _inputs(geo)
    ids, am = inp["inputs"].numpy(), inp["attention_mask"].numpy()
    p = [ids[b][am[b]] for b in range(2)]
    reqs = [(p[0], inp["images"][0], inp["image_sizes"][0]), (p[1], inp["images"][1], inp["image_sizes"][1]),
            (p[0][:-2], inp["images"][0], inp["image_sizes"][0])]
    N = _budget(model, geo, "both")
    kw = dict(prompt_kv_budget=N, prompt_kv_window=W, prompt_kv_pool=K, eos_token_id=None)
    made = []
    real = eng.new_kv_cache
    monkeypatch.setattr(eng, "new_kv_cache", lambda B, L, *a: (made.append((B, L)), real(B, L, *a))[1])
    budgets = [6, 3, 5]

    def batch(**k):
        return model.generate_batch([r[0] for r in reqs], images=[r[1] for r in reqs], image_sizes=[r[2] for r in reqs], max_batch_size=2,
                                    max_new_tokens=budgets, **k)
    out = batch(**kw)
    batch(eos_token_id=None)
    assert made[0] == (2, N + max(budgets)) and made[1][0] == 2 and made[1][1] > made[0][1]
    steps = 0
    for i, (q, im, sz) in enumerate(reqs):
        one = model.generate(torch.from_numpy(q[None]), images=[im], image_sizes=[sz], max_new_tokens=budgets[i], output_scores=True,
                             return_dict_in_generate=True, **kw)
        got = out[f"req_{i}"].generated_tokens
        assert len(got) == budgets[i]
        steps += _compare(got, one)[0]
    assert steps >= len(reqs)


# ------------------------------------------------------------------------------------------------ refusals
def test_engine_refusals_leave_the_cache_alone():
    geo = "toy"
    model = _model(geo)
    eng = model.engine
    N = _budget(model, geo, "both")
    cache, _ = _prefill(eng, geo, compress=(N, W, K))
    lens0, off0 = cache.lens.copy(), cache.pos_off.copy()
    inp = _inputs(geo)
    tok = np.array([5, 7])
    marker = object()
    for call in (lambda: eng.verify_step(cache, np.array([[5, 6], [7, 8]])),
                 lambda: eng.extend(cache, inp["inputs"].numpy(), inp["attention_mask"].numpy(), inp["images"], inp["image_sizes"],
                                    reuse=np.array([4, 4])),
                 lambda: eng.score_tails(cache, np.array([0, 1]), [np.array([5, 6]), np.array([7])], None),
                 lambda: eng.decode_step(cache, tok, beams=marker),
                 lambda: eng.decode_step(cache, tok, shared=marker),
                 lambda: eng.decode_step(cache, tok, attn_layers=(0,))):
        with pytest.raises(NotImplementedError, match="prompt_kv_budget"):
            call()
        assert np.array_equal(cache.lens, lens0) and np.array_equal(cache.pos_off, off0)
    for bad in (dict(attn_layers=(0,)), dict(tap_layers=(1,)), dict(kv_dtype="int8")):
        with pytest.raises(NotImplementedError, match="prompt_kv_budget"):
            _prefill(eng, geo, compress=(N, W, K), **bad)
    for bad in ((N, 0, K), (N, 65, K), (W, W, K), (N, W, 4), (N, W, 65)):
        with pytest.raises(ValueError, match="compress"):
            _prefill(eng, geo, compress=bad)
    eng.decode_step(cache, tok)                                             # the plain step still runs
    assert np.array_equal(cache.lens, lens0 + 1)

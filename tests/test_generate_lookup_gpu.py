"""GPU tests of generate(prompt_lookup_num_tokens=k): bit-identical sequences, raw logits and processed scores to plain greedy
generate() on the toy (hd 128) and toy_qwen (hd 64, GQA, bias) models, for the default drafter and for injected ones whose acceptance
is known (so that the equality is never vacuous), under the logits processors, with an EOS inside an accepted run, on int8 weights,
across a two-turn GenerationCache conversation; verify_step never leaves the skinny GEMM; the training state is not touched."""
import math
import os

import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES

pytestmark = pytest.mark.gpu

CASES = {"toy": dict(golden="toy_e2e", geo="toy"), "toy_qwen": dict(golden="toy_qwen_e2e", geo="toy_qwen")}
KS = (1, 3, 7, 31)
TS = (1, 2, 12, 40)
_MODELS, _PLAIN = {}, {}


def _setup(golden_dir, case):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if case not in _MODELS:
        from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
        c = CASES[case]
        g = np.load(os.path.join(golden_dir, c["golden"] + ".npz"))
        geo = c["geo"]
        Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in geo else (LlavaConfig, LlavaLlamaForCausalLM)
        l = GEOMETRIES[geo]["lm"]
        cfg = Config(geometry=GEOMETRIES[geo], rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0),
                     mm_patch_merge_type="flat", image_aspect_ratio="square", image_grid_pinpoints=None)
        model = Model(cfg, device="cuda:0", init="portable", seed=0).eval()
        ids = g["input_ids"][0][g["attention_mask"][0].astype(bool)].astype(np.int64)
        _MODELS[case] = (model, ids, torch.from_numpy(g["image0"]), tuple(g["image_sizes"].tolist()[0]))
    return _MODELS[case]


def _run(setup, drafter=None, ids=None, **kw):
    """greedy_generate as model.generate() calls it, with an injected drafter when one is given."""
    from radvlm_amd.generation import greedy_generate, parse_generate_kwargs
    model, prompt, image, size = setup
    kw = dict(dict(eos_token_id=None, output_scores=True, output_logits=True, return_dict_in_generate=True), **kw)
    cfg = parse_generate_kwargs(kw, lookup=True)
    cfg.drafter = drafter
    with torch.no_grad():
        return greedy_generate(model.engine, np.asarray(prompt if ids is None else ids)[None], None, [image], [size], cfg)


def _plain(golden_dir, case, T):
    if (case, T) not in _PLAIN:
        _PLAIN[case, T] = _run(_setup(golden_dir, case), max_new_tokens=T)
    return _PLAIN[case, T]


def _same(got, want):
    assert torch.equal(got.sequences, want.sequences), (got.sequences.tolist(), want.sequences.tolist())
    n = want.sequences.shape[1]
    assert len(got.logits) == len(want.logits) == n and len(got.scores) == len(want.scores) == n
    for t in range(n):
        assert got.logits[t].shape == want.logits[t].shape and torch.equal(got.logits[t], want.logits[t]), ("logits", t)
        assert got.scores[t].shape == want.scores[t].shape and torch.equal(got.scores[t], want.scores[t]), ("scores", t)


class Scripted:
    """Proposes the reference run's next j tokens and then wrong ones, k in all (j >= k: the oracle, j = 0: never right); `poison`
    replaces the draft's entries from that index on (an image placeholder, say)."""

    def __init__(self, ref, prompt_len, j, k, vocab, poison=None):
        self.ref, self.P, self.j, self.k, self.V, self.poison = [int(v) for v in ref], prompt_len, j, k, vocab, poison

    def propose(self, seq):
        t = len(seq) - self.P
        out = []
        for i in range(self.k):
            r = self.ref[t + i] if t + i < len(self.ref) else 0
            out.append(r if i < self.j else (r + 1) % self.V)
        out = np.array(out, dtype=np.int64)
        if self.poison is not None:
            out[self.poison[0]:] = self.poison[1]
        return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(CASES))
def test_bit_identical_to_plain_generate(golden_dir, case, k):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    V, P = model.engine.vocab, len(prompt)
    ref = _plain(golden_dir, case, max(TS)).sequences[0].tolist()
    for T in TS:
        want = _plain(golden_dir, case, T)
        assert want.sequences[0].tolist() == ref[:T]
        # the default drafter, through the public interface
        got = model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], max_new_tokens=T, eos_token_id=None,
                             output_scores=True, output_logits=True, return_dict_in_generate=True, prompt_lookup_num_tokens=k)
        _same(got, want)
        assert set(got.lookup_stats) == {"steps", "drafted", "accepted"} and got.lookup_stats["steps"] <= max(T - 1, 0)
        # the oracle: every draft is right
        got = _run(setup, Scripted(ref, P, k, k, V), max_new_tokens=T)
        _same(got, want)
        s = got.lookup_stats
        assert s["accepted"] == s["drafted"] and s["steps"] <= math.ceil((T - 1) / (k + 1)) + 1, (T, s)
        assert s["drafted"] > 0 or T < 3, (T, s)
        # never right: every verify step is wasted
        got = _run(setup, Scripted(ref, P, 0, k, V), max_new_tokens=T)
        _same(got, want)
        s = got.lookup_stats
        assert s["accepted"] == 0 and s["steps"] == max(T - 1, 0) and (s["drafted"] > 0 or T < 3), (T, s)
        # right for j, then wrong
        j = k // 2
        got = _run(setup, Scripted(ref, P, j, k, V), max_new_tokens=T)
        _same(got, want)
        assert 0 < got.lookup_stats["accepted"] < got.lookup_stats["drafted"] or j == 0 or T - 2 <= j, (T, got.lookup_stats)
        # a draft with the image placeholder in it: cut before it, never fed
        got = _run(setup, Scripted(ref, P, k, k, V, poison=(1, -200)), max_new_tokens=T)
        _same(got, want)
        assert got.lookup_stats["accepted"] == got.lookup_stats["drafted"] <= got.lookup_stats["steps"]


@pytest.mark.parametrize("case", list(CASES))
def test_eos_inside_an_accepted_run_and_inside_a_draft(golden_dir, case):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    ref = _plain(golden_dir, case, max(TS)).sequences[0].tolist()
    # the EOS id is a token of the plain run that first occurs at step 3 or later, so the run with it as EOS ends inside the first
    # verify round.  A toy model whose greedy output is one token repeated (toy_qwen) has no such token: its runs, the plain one
    # included, then go under no_repeat_ngram_size=1, which makes every token a first occurrence.
    extra = {}
    firsts = [p for p in range(3, 30) if ref[p] not in ref[:p]]
    if not firsts:
        extra = dict(no_repeat_ngram_size=1)
        ref = _run(setup, max_new_tokens=40, **extra).sequences[0].tolist()
        firsts = [p for p in range(3, 30) if ref[p] not in ref[:p]]
    pos = firsts[0]
    want = _run(setup, max_new_tokens=40, eos_token_id=ref[pos], **extra)
    assert want.sequences.shape[1] == pos + 1
    for k in (3, 7, 31):
        # the injected oracle does not cut at EOS: the draft holds it, the emission ends on it
        got = _run(setup, Scripted(ref, len(prompt), k, k, model.engine.vocab), max_new_tokens=40, eos_token_id=ref[pos], **extra)
        _same(got, want)
        assert got.lookup_stats["accepted"] == got.lookup_stats["drafted"] > 0
        got = model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], max_new_tokens=40, eos_token_id=ref[pos],
                             output_scores=True, output_logits=True, return_dict_in_generate=True, prompt_lookup_num_tokens=k, **extra)
        _same(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_logits_processors(golden_dir, case):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    ref = _plain(golden_dir, case, max(TS)).sequences[0].tolist()
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=5, bad_words_ids=[[ref[0]], [ref[1], ref[2]], [ref[3]]],
              begin_suppress_tokens=[ref[0], 5], eos_token_id=ref[4], max_new_tokens=24)
    want = _run(setup, **kw)
    seq = want.sequences[0].tolist()
    assert len(seq) >= 5
    for k in (1, 3, 7, 31):
        for j in (k, k // 2, 0):
            got = _run(setup, Scripted(seq, len(prompt), j, k, model.engine.vocab), **kw)
            _same(got, want)
            if j == k:                                    # (past an EOS that ends the run the script has nothing right to offer)
                assert got.lookup_stats["accepted"] > 0
        got = model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], output_scores=True, output_logits=True,
                             return_dict_in_generate=True, prompt_lookup_num_tokens=k, **kw)
        _same(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_quantized_engine(golden_dir, case):
    setup = _setup(golden_dir, case)
    from radvlm_amd.llava.model import LlavaLlamaForCausalLM, LlavaQwenForCausalLM
    model, prompt, image, size = setup
    q = (LlavaQwenForCausalLM if "qwen" in case else LlavaLlamaForCausalLM)(model.config, device="cuda:0", init="portable", seed=0).eval()
    q.quantize_decoder_()
    qs = (q, prompt, image, size)
    want = _run(qs, max_new_tokens=24)
    ref = want.sequences[0].tolist()
    for k, j in ((7, 7), (7, 3), (31, 31), (3, 0)):
        got = _run(qs, Scripted(ref, len(prompt), j, k, q.engine.vocab), max_new_tokens=24)
        _same(got, want)
        assert (got.lookup_stats["accepted"] > 0) == (j > 0)
    got = q.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], max_new_tokens=24, eos_token_id=None,
                     output_scores=True, output_logits=True, return_dict_in_generate=True, prompt_lookup_num_tokens=7)
    _same(got, want)


@pytest.mark.parametrize("case", list(CASES))
def test_two_turn_generation_cache(golden_dir, case):
    from radvlm_amd.generation import GenerationCache
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    V = model.engine.vocab
    runs = {}
    for tag in ("plain", "lookup"):
        gc = GenerationCache()
        outs = []
        ids = prompt
        for turn, T in enumerate((9, 7)):
            if tag == "plain":
                o = _run(setup, ids=ids, max_new_tokens=T, past_key_values=gc)
            else:
                ref = runs["plain"][0][turn].sequences[0].tolist()
                o = _run(setup, Scripted(ref, len(ids), 2, 4, V), ids=ids, max_new_tokens=T, past_key_values=gc)
                assert o.lookup_stats["accepted"] > 0 and o.lookup_stats["accepted"] < o.lookup_stats["drafted"]
            outs.append(o)
            ids = np.concatenate([ids, o.sequences[0].cpu().numpy(), np.array([11, 12, 13])])
        n = gc.get_seq_length()
        runs[tag] = (outs, n, [kv[:, :n].clone() for kv in gc.kv.layers], gc.kv.lens.copy(), [r.copy() for r in gc.records])
    for a, b in zip(runs["plain"][0], runs["lookup"][0]):
        _same(b, a)
    assert runs["plain"][1] == runs["lookup"][1] and (runs["plain"][3] == runs["lookup"][3]).all()
    for a, b in zip(runs["plain"][2], runs["lookup"][2]):
        assert torch.equal(a, b)
    for a, b in zip(runs["plain"][4], runs["lookup"][4]):
        assert (a == b).all()


@pytest.mark.parametrize("case", list(CASES))
def test_verify_step_never_leaves_the_skinny_gemm(golden_dir, case, monkeypatch):
    from radvlm_amd import ops
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    eng = model.engine
    want = _plain(golden_dir, case, 12)
    ref = want.sequences[0].tolist()
    state = dict(inside=False, tiled=0, verify=0)
    real_gemm, real_verify = ops.gemm_nt, eng.verify_step

    def gemm_nt(*a, **k):
        state["tiled"] += state["inside"]
        return real_gemm(*a, **k)

    def verify_step(*a, **k):
        state["inside"], state["verify"] = True, state["verify"] + 1
        try:
            return real_verify(*a, **k)
        finally:
            state["inside"] = False

    monkeypatch.setattr(ops, "gemm_nt", gemm_nt)
    monkeypatch.setattr(eng, "verify_step", verify_step, raising=False)
    monkeypatch.setattr(eng, "gemv_max_m", 1, raising=False)           # instance level: every multi-row product would go to the tiled GEMM
    got = _run(setup, Scripted(ref, len(prompt), 3, 5, eng.vocab), max_new_tokens=12)
    _same(got, want)
    assert state["verify"] > 0 and state["tiled"] == 0, state


@pytest.mark.parametrize("route", ["verify", "beam"])
@pytest.mark.parametrize("case", list(CASES))
def test_both_attention_routes_give_the_plain_bits(golden_dir, case, route, monkeypatch):
    """verify_step sends some (head shape, R, key count) cells to rv_attn_decode_beam_bf16 (the measured table in engine.py); forced
    either way the result is the plain run's."""
    from radvlm_amd import ops
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    want = _plain(golden_dir, case, 40)
    ref = want.sequences[0].tolist()
    calls = dict(verify=0, beam=0)
    real = dict(verify=ops.attn_decode_verify, beam=ops.attn_decode_beam)
    for name in calls:
        def spy(*a, _n=name, **k):
            calls[_n] += 1
            return real[_n](*a, **k)
        monkeypatch.setattr(ops, "attn_decode_" + name, spy)
    monkeypatch.setattr(model.engine, "verify_route", route, raising=False)
    for k, j in ((31, 31), (7, 3), (1, 1)):
        _same(_run(setup, Scripted(ref, len(prompt), j, k, model.engine.vocab), max_new_tokens=40), want)
    other = "beam" if route == "verify" else "verify"
    assert calls[route] > 0 and calls[other] == 0, calls


@pytest.mark.parametrize("case", list(CASES))
def test_training_state_and_a_following_plain_call_are_unchanged(golden_dir, case):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    eng = model.engine
    want = _plain(golden_dir, case, 12)
    before = (model.training, eng.weights_version, eng.ctx is None, eng.lm.flat.clone())
    got = model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], max_new_tokens=12, eos_token_id=None,
                         prompt_lookup_num_tokens=5)
    assert torch.is_tensor(got) and torch.equal(got, want.sequences)
    assert (model.training, eng.weights_version, eng.ctx is None) == before[:3] and torch.equal(eng.lm.flat, before[3])
    again = _run(setup, max_new_tokens=12)
    _same(again, want)
    with pytest.raises(ValueError):
        model.generate(torch.from_numpy(np.stack([prompt, prompt])), images=[image, image], image_sizes=[size, size], max_new_tokens=2,
                       prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError):
        model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], max_new_tokens=2, prompt_lookup_num_tokens=3,
                       do_sample=True, seed=1)
    with pytest.raises(TypeError):
        model.generate_batch([prompt], images=[image], image_sizes=[size], max_new_tokens=2, prompt_lookup_num_tokens=3)
    with pytest.raises(TypeError):
        model.generate_beams(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], num_beams=2, max_new_tokens=2,
                             prompt_lookup_num_tokens=3)

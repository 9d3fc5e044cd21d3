"""GPU tests of generate(assistant_model=m, num_assistant_tokens=k).  Greedy: sequences, raw logits and processed scores are the plain
call's bit for bit, for draft models that are always right (the model itself), mostly wrong (another seed, a one-layer decoder) and
right some of the time (a copy with a perturbed lm_head), on toy and toy_qwen, under the logits processors, with an EOS inside an
accepted run and with an int8-weight target.  Sampled: reproducible, every draft of the model itself accepted, no rejected draft
leaks out, and the emitted tokens replayed through prefill + decode_step give the raw logits rows bit for bit (the cache rollback is
sound).  The training state of both engines is untouched."""
import numpy as np
import pytest
import torch

from radvlm_amd.config import GEOMETRIES
from test_generate_lookup_gpu import CASES, _plain, _run, _same, _setup

pytestmark = pytest.mark.gpu

KS = (1, 5, 31)
TS = (1, 2, 12, 40)
ASSISTANTS = ("self", "other_seed", "one_layer", "perturbed_head")
_DRAFTS = {}


def _build(case, seed=0, layers=None):
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    geo = dict(GEOMETRIES[CASES[case]["geo"]])
    if layers is not None:
        geo["lm"] = dict(geo["lm"], layers=layers)
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in case else (LlavaConfig, LlavaLlamaForCausalLM)
    l = geo["lm"]
    cfg = Config(geometry=geo, rms_norm_eps=l.get("rms_eps", 1e-5), rope_theta=l.get("rope_theta", 10000.0), mm_patch_merge_type="flat",
                 image_aspect_ratio="square", image_grid_pinpoints=None)
    return Model(cfg, device="cuda:0", init="portable", seed=seed).eval()


def _draft(golden_dir, case, kind):
    model = _setup(golden_dir, case)[0]
    if kind == "self":
        return model
    if (case, kind) not in _DRAFTS:
        if kind == "other_seed":
            m = _build(case, seed=1)
        elif kind == "one_layer":
            m = _build(case, seed=0, layers=1)
        else:                                   # the model's weights, the lm_head perturbed: right often, not always
            m = _build(case, seed=0)
            head = m.engine.W("lm_head.weight")
            g = torch.Generator(device="cpu").manual_seed(3)
            noise = torch.randn(head.shape, generator=g).to(head.device) * head.float().std() * _HEAD_NOISE[case]
            head.copy_((head.float() + noise).to(head.dtype))
            m.engine.weights_changed(tower=False)
        _DRAFTS[case, kind] = m
    return _DRAFTS[case, kind]


# the noise on the copy's lm_head, in units of the head's standard deviation.  toy_qwen's greedy output is one token repeated, which
# any copy gets right: its perturbed-head runs, the plain one included, go under no_repeat_ngram_size=1 (as
# test_generate_lookup_gpu does for this model), where every step's choice is a close call between neighbouring ranks
_HEAD_NOISE = {"toy": 0.5, "toy_qwen": 0.1}
_MIX_EXTRA = {"toy": {}, "toy_qwen": dict(no_repeat_ngram_size=1)}


def _gen(setup, assistant, k, **kw):
    model, prompt, image, size = setup
    kw = dict(dict(eos_token_id=None, output_scores=True, output_logits=True, return_dict_in_generate=True), **kw)
    return model.generate(torch.from_numpy(prompt[None]), images=[image], image_sizes=[size], assistant_model=assistant,
                          num_assistant_tokens=k, **kw)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ASSISTANTS)
@pytest.mark.parametrize("case", list(CASES))
def test_greedy_is_bit_identical_to_plain_generate(golden_dir, case, kind, k):
    from conftest import record_measurement
    setup = _setup(golden_dir, case)
    m = _draft(golden_dir, case, kind)
    tot = dict(drafted=0, accepted=0)
    extra = _MIX_EXTRA[case] if kind == "perturbed_head" else {}
    for T in TS:
        want = _run(setup, max_new_tokens=T, **extra) if extra else _plain(golden_dir, case, T)
        got = _gen(setup, m, k, max_new_tokens=T, **extra)
        _same(got, want)
        s = got.assist_stats
        assert set(s) == {"steps", "drafted", "accepted"} and not hasattr(got, "lookup_stats")
        assert 0 <= s["accepted"] <= s["drafted"] and s["steps"] <= max(T - 1, 0)
        if kind == "self":
            assert s["accepted"] == s["drafted"] and (s["drafted"] > 0 or T < 3), (T, s)
        tot = {name: tot[name] + s[name] for name in tot}
    record_measurement("assist_greedy_acceptance", case=case, kind=kind, k=k, **tot)
    if kind == "perturbed_head":
        assert 0 < tot["accepted"] < tot["drafted"], tot                 # the mix is not vacuous


@pytest.mark.parametrize("case", list(CASES))
def test_logits_processors_and_eos_inside_an_accepted_run(golden_dir, case):
    setup = _setup(golden_dir, case)
    model = setup[0]
    ref = _plain(golden_dir, case, max(TS)).sequences[0].tolist()
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_new_tokens=5, bad_words_ids=[[ref[0]], [ref[1], ref[2]], [ref[3]]],
              begin_suppress_tokens=[ref[0], 5], eos_token_id=ref[4], max_new_tokens=24)
    want = _run(setup, **kw)
    for kind in ("self", "perturbed_head", "one_layer"):
        for k in (1, 5, 31):
            got = _gen(setup, _draft(golden_dir, case, kind), k, **kw)
            _same(got, want)
            if kind == "self":                   # the draft rows went through the same processors: every draft is the model's choice
                assert got.assist_stats["accepted"] == got.assist_stats["drafted"] > 0
    # an EOS inside an accepted run: the emission ends on it
    extra = dict(no_repeat_ngram_size=1)
    seq = _run(setup, max_new_tokens=40, **extra).sequences[0].tolist()
    pos = next(p for p in range(3, 30) if seq[p] not in seq[:p])
    want = _run(setup, max_new_tokens=40, eos_token_id=seq[pos], **extra)
    assert want.sequences.shape[1] == pos + 1
    for k in (5, 31):
        got = _gen(setup, model, k, max_new_tokens=40, eos_token_id=seq[pos], **extra)
        _same(got, want)
        assert got.assist_stats["accepted"] == got.assist_stats["drafted"] > 0


@pytest.mark.parametrize("case", list(CASES))
def test_int8_weight_target(golden_dir, case):
    model, prompt, image, size = _setup(golden_dir, case)
    q = _build(case, seed=0)
    q.quantize_decoder_()
    qs = (q, prompt, image, size)
    want = _run(qs, max_new_tokens=24)
    for kind, k in (("self", 5), ("perturbed_head", 5), ("other_seed", 31)):
        m = q if kind == "self" else _draft(golden_dir, case, kind)
        got = _gen(qs, m, k, max_new_tokens=24)
        _same(got, want)
        if kind == "self":
            assert got.assist_stats["accepted"] == got.assist_stats["drafted"] > 0
    got = _gen(qs, model, 5, max_new_tokens=24)                          # a bf16 draft of an int8 target
    _same(got, want)


SAMPLING = dict(do_sample=True, temperature=0.8, top_k=4)


@pytest.mark.parametrize("case", list(CASES))
def test_sampled(golden_dir, case):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    eng = model.engine
    T = 24
    for kind, k, seed in (("self", 5, 11), ("other_seed", 5, 12), ("perturbed_head", 31, 13), ("one_layer", 1, 14)):
        m = _draft(golden_dir, case, kind)
        a = _gen(setup, m, k, max_new_tokens=T, seed=seed, **SAMPLING)
        b = _gen(setup, m, k, max_new_tokens=T, seed=seed, **SAMPLING)
        assert torch.equal(a.sequences, b.sequences) and a.assist_stats == b.assist_stats        # reproducible
        assert all(torch.equal(x, y) for x, y in zip(a.scores + a.logits, b.scores + b.logits))
        s = a.assist_stats
        assert a.sequences.shape == (1, T) and s["drafted"] > 0
        if kind == "self":
            assert s["accepted"] == s["drafted"], s
        seq = a.sequences[0].tolist()
        # every emitted token is one its own warped row kept: no rejected draft leaks out
        for t, tok in enumerate(seq):
            row = a.scores[t][0]
            assert bool(torch.isfinite(row[tok])), (kind, t, tok)
        # the emitted tokens replayed one by one: the raw rows are the call's, so no stale or rejected K|V row was ever read
        cache, logits = eng.prefill(prompt[None], None, [image], [size], max_new_tokens=T)
        for t, tok in enumerate(seq):
            assert torch.equal(logits, a.logits[t]), (kind, t)
            if t + 1 < T:
                logits = eng.decode_step(cache, np.asarray([tok]))

@pytest.mark.parametrize("case", list(CASES))
def test_training_state_and_refusals(golden_dir, case):
    setup = _setup(golden_dir, case)
    model, prompt, image, size = setup
    m = _draft(golden_dir, case, "other_seed")
    want = _plain(golden_dir, case, 12)
    before = [(x.training, x.engine.weights_version, x.engine.ctx is None, x.engine.lm.flat.clone()) for x in (model, m)]
    inp = dict(images=[image], image_sizes=[size])
    got = model.generate(torch.from_numpy(prompt[None]), max_new_tokens=12, eos_token_id=None, assistant_model=m, **inp)
    assert torch.is_tensor(got) and torch.equal(got, want.sequences)
    model.generate(torch.from_numpy(prompt[None]), max_new_tokens=12, eos_token_id=None, assistant_model=m, do_sample=True, seed=4, **inp)
    for x, b in zip((model, m), before):
        assert (x.training, x.engine.weights_version, x.engine.ctx is None) == b[:3] and torch.equal(x.engine.lm.flat, b[3])
    with pytest.raises(ValueError, match="one prompt row"):
        model.generate(torch.from_numpy(np.stack([prompt, prompt])), images=[image, image], image_sizes=[size, size], max_new_tokens=2,
                       assistant_model=m)
    with pytest.raises(NotImplementedError):
        model.generate(torch.from_numpy(prompt[None]), max_new_tokens=2, assistant_model=m, prompt_lookup_num_tokens=3, **inp)
    with pytest.raises(TypeError):
        model.generate_batch([prompt], images=[image], image_sizes=[size], max_new_tokens=2, assistant_model=m)
    with pytest.raises(TypeError):
        model.generate_beams(torch.from_numpy(prompt[None]), num_beams=2, max_new_tokens=2, assistant_model=m, **inp)
    other = "toy_qwen" if case == "toy" else "toy"
    if _setup(golden_dir, other)[0].engine.vocab != model.engine.vocab:
        with pytest.raises(ValueError, match="vocabulary"):
            model.generate(torch.from_numpy(prompt[None]), max_new_tokens=2, assistant_model=_setup(golden_dir, other)[0], **inp)

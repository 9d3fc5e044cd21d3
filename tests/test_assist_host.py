"""CPU tests of assisted generation's host side (radvlm_amd/generation.py, radvlm_amd/assist.py): the assistant_model /
num_assistant_tokens keywords and their refusals, the vocabulary / image mismatch errors, and ModelDrafter's cache bookkeeping on a fake
engine -- what it feeds is exactly the emitted tokens, its cache never counts a rejected draft, and the greedy result is the plain
run's for draft engines that are always, sometimes and never right."""
import numpy as np
import pytest
import torch

from radvlm_amd import ops
from radvlm_amd.assist import ModelDrafter, check_assistant
from radvlm_amd.generation import (FEATURES, REFUSALS, features_of, greedy_generate, parse_batch_kwargs, parse_beam_kwargs,
                                   parse_generate_kwargs)
from test_lookup_host import PROMPT, FakeEngine, V, same


class FakeModel:
    def __init__(self, engine=None):
        self.engine = engine or FakeEngine()


@pytest.fixture(autouse=True)
def host_argmax(monkeypatch):
    monkeypatch.setattr(ops, "argmax_rows", lambda x, n, out=None: x[:, :n].argmax(1))


# ------------------------------------------------------------------------------------------------ keywords
def test_keywords_parse():
    m = FakeModel()
    cfg = parse_generate_kwargs(dict(assistant_model=m), lookup=True)
    assert cfg.assistant.model is m and cfg.assistant.k == 5 and cfg.drafter is None and cfg.lookup is None
    assert parse_generate_kwargs(dict(assistant_model=m, num_assistant_tokens=31), lookup=True).assistant.k == 31
    assert parse_generate_kwargs({}, lookup=True).assistant is None
    assert parse_generate_kwargs(dict(assistant_model=None), lookup=True).assistant is None
    for bad in (0, 32, -1, 2.0, "3", True, [3]):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            parse_generate_kwargs(dict(assistant_model=m, num_assistant_tokens=bad), lookup=True)
    with pytest.raises(ValueError, match="without `assistant_model`"):
        parse_generate_kwargs(dict(num_assistant_tokens=3), lookup=True)
    with pytest.raises(ValueError, match="assistant_model"):
        parse_generate_kwargs(dict(assistant_model=object()), lookup=True)
    # generate_batch / generate_beams reject the names as they reject any unknown keyword
    for name, v in (("assistant_model", m), ("num_assistant_tokens", 3)):
        with pytest.raises(TypeError):
            parse_batch_kwargs({name: v}, 2)
        with pytest.raises(TypeError):
            parse_beam_kwargs({name: v, "num_beams": 2})
        with pytest.raises(TypeError):
            parse_generate_kwargs({name: v})


def test_feature_and_refusals():
    m = FakeModel()
    assert FEATURES["assistant"] == "assistant_model"
    cfg = parse_generate_kwargs(dict(assistant_model=m, do_sample=True, seed=3), lookup=True)          # sampling composes
    assert features_of(cfg) == {"assistant", "sampling"}
    cfg.drafter = object()                   # the drafter greedy_generate builds must not turn the call into a lookup call
    assert features_of(cfg) == {"assistant", "sampling"}
    # the lookup's own row stays, and a drafter set by hand still counts as the lookup
    assert ("lookup", "sampling", "speculative sampling is not implemented") in REFUSALS
    with pytest.raises(NotImplementedError, match="speculative sampling"):
        parse_generate_kwargs(dict(prompt_lookup_num_tokens=3, do_sample=True, seed=1), lookup=True)
    hand = parse_generate_kwargs({}, lookup=True)
    hand.drafter = object()
    assert features_of(hand) == {"lookup"}
    # refused with the lookup, with everything the lookup is refused with but sampling, and with past_key_values
    with_lookup = {(a if b == "lookup" else b) for a, b, _ in REFUSALS if "lookup" in (a, b)} - {"sampling", "assistant"}
    with_assistant = {(a if b == "assistant" else b) for a, b, _ in REFUSALS if "assistant" in (a, b)}
    assert with_assistant == with_lookup | {"lookup", "past_key_values"}
    from radvlm_amd.constraints import TokenConstraint
    from radvlm_amd.generation import GenerationCache
    for kw, word in ((dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"), (dict(kv_cache_dtype="int8"), "int8"),
                     (dict(guidance_scale=2.0), "guidance_scale"), (dict(dola_layers="low"), "dola_layers"),
                     (dict(past_key_values=GenerationCache()), "past_key_values"), (dict(prompt_kv_budget=64), "prompt_kv_budget"),
                     (dict(output_attentions=True, return_dict_in_generate=True), "output_attentions"),
                     (dict(constraint=TokenConstraint.from_choices([[1, 2]], 0)), "constraint")):
        with pytest.raises(NotImplementedError, match="assistant_model") as e:
            parse_generate_kwargs(dict(kw, assistant_model=m), lookup=True, attentions=True)
        assert word in str(e.value)


def test_more_than_one_prompt_row_is_refused():
    cfg = parse_generate_kwargs(dict(assistant_model=FakeModel(), max_new_tokens=4), lookup=True)
    with pytest.raises(ValueError, match="one prompt row"):
        greedy_generate(FakeEngine(), np.concatenate([PROMPT, PROMPT]), None, None, None, cfg)


class Geo:
    def __init__(self, vocab=V, **v):
        self.vocab = vocab
        self.v = dict(dict(kind="clip", image=336, patch=14), **v)
        self.merge_type, self.aspect, self.pinpoints = "flat", "square", None


def test_mismatch_errors_name_what_differs():
    check_assistant(Geo(), Geo())
    with pytest.raises(ValueError, match=r"vocabulary holds 24 ids, the model's 23"):
        check_assistant(Geo(), Geo(vocab=V + 1))
    with pytest.raises(ValueError, match=r"image 224 vs 336"):
        check_assistant(Geo(), Geo(image=224))
    with pytest.raises(ValueError, match=r"tower 'siglip' vs 'clip'.*patch 16 vs 14"):
        check_assistant(Geo(), Geo(kind="siglip", patch=16))
    other = Geo()
    other.merge_type = "spatial_unpad"
    with pytest.raises(ValueError, match="mm_patch_merge_type"):
        check_assistant(Geo(), other)


# ------------------------------------------------------------------------------------------------ the drafter on a fake engine
class HostEngine(FakeEngine):
    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))


class SaltedEngine(HostEngine):
    """A draft engine whose logits agree with FakeEngine's except at the positions in `wrong` (counted in emitted tokens), so a greedy
    draft is right until it reaches one."""

    def __init__(self, wrong=(), prompt_len=PROMPT.shape[1]):
        super().__init__()
        self.wrong, self.P = set(wrong), prompt_len

    def logits_of(self, seq):
        x = super().logits_of(seq)
        if len(seq) - self.P in self.wrong:
            x = x.clone()
            x[int(x.argmax())] = -1e9
        return x


def run(draft_engine, k, T, **kw):
    eng = HostEngine()
    cfg = parse_generate_kwargs(dict(kw, max_new_tokens=T, assistant_model=FakeModel(draft_engine), num_assistant_tokens=k,
                                     return_dict_in_generate=True, output_scores=True, output_logits=True), lookup=True)
    cfg.drafter = ModelDrafter(draft_engine, k, cfg, T, PROMPT.shape[1])
    cfg.drafter.start(PROMPT, None, None, None)
    drafter, propose = cfg.drafter, cfg.drafter.propose
    drafter.rounds = []                      # (index of the round's first draft-engine call, tokens emitted before it)

    def spy(seq):
        before = len(draft_engine.calls)
        out = propose(seq)
        if len(draft_engine.calls) > before:
            drafter.rounds.append((before, len(seq) - PROMPT.shape[1]))
        return out
    drafter.propose = spy
    return greedy_generate(eng, PROMPT, None, None, None, cfg), eng, cfg.drafter


def plain(T, **kw):
    cfg = parse_generate_kwargs(dict(kw, max_new_tokens=T, return_dict_in_generate=True, output_scores=True, output_logits=True), lookup=True)
    return greedy_generate(HostEngine(), PROMPT, None, None, None, cfg)


@pytest.mark.parametrize("k", [1, 3, 5, 31])
@pytest.mark.parametrize("wrong", [(), (4, 5, 11), tuple(range(1, 40)), (2,), (7, 8, 9, 10)])
def test_cache_bookkeeping_and_result(k, wrong):
    T, P = 24, PROMPT.shape[1]
    want = plain(T)
    seq = want.sequences[0].tolist()
    d = SaltedEngine(wrong)
    got, eng, drafter = run(d, k, T)
    same(got, want)
    assert not hasattr(got, "lookup_stats") and set(got.assist_stats) == {"steps", "drafted", "accepted"}
    s = got.assist_stats
    if not wrong:
        assert s["accepted"] == s["drafted"] > 0
    elif len(wrong) > 30:
        assert s["accepted"] == 0 and s["drafted"] > 0
    elif k >= 3:
        assert 0 < s["accepted"] < s["drafted"]
    # replay the draft engine's calls round by round.  The first call of a round is the catch-up: below its position the cache row
    # holds exactly the emitted tokens (lens never counts a rejected draft) and it feeds the emitted tokens that follow, up to the
    # last one; the later calls of the round feed the round's own drafts, one each, right behind it.
    row = {}
    for r, (c0, n_emitted) in enumerate(drafter.rounds):
        calls = d.calls[c0:drafter.rounds[r + 1][0] if r + 1 < len(drafter.rounds) else len(d.calls)]
        kind, n0, toks = calls[0]
        pos = n0 - P
        assert 0 <= pos < n_emitted and [row[i] for i in range(pos)] == seq[:pos], (r, pos)
        assert toks == seq[pos:n_emitted] and (kind == "decode") == (len(toks) == 1), (r, kind, toks)
        for i, tok in enumerate(toks):
            row[pos + i] = tok
        nxt = n_emitted
        for kind, n0, toks in calls[1:]:
            assert kind == "decode" and n0 - P == nxt and len(toks) == 1
            row[nxt] = toks[0]
            nxt += 1
        assert len(calls) <= k and nxt <= T - 1
    assert 0 < len(drafter.rounds) <= s["steps"]
    # after a fully accepted round the catch-up is two tokens in one verify_step
    if not wrong and k < T - 2:
        assert any(kind == "verify" and len(toks) == 2 for kind, _, toks in d.calls)
    # no position past the budget is ever fed, on either engine
    for e in (eng, d):
        assert max(n0 + len(toks) for _, n0, toks in e.calls) <= P + T - 1 + 1


def test_processors_run_on_the_drafts_own_history(monkeypatch):
    """Under the logits processors the draft rows go through the rows kernel with the draft's own history and steps."""
    seen = []

    def rows(x, n, hist, slot, t, min_new, rep_penalty=1.0, ngram=0, ban_always=None, ban_begin=None, ban_eos=None, bad_tok=None,
             bad_off=None, out=None, logprob=None):
        for r in range(x.shape[0]):
            seen.append((int(t[r]), hist[int(slot[r]), :int(t[r])].tolist()))
            if int(t[r]) < int(min_new[r]) and ban_eos is not None:
                x[r, ban_eos.long()] = -float("inf")
        return x[:, :n].argmax(1)
    monkeypatch.setattr(ops, "logits_process_argmax_rows", rows)

    def uniform(x, n, hist, t, rep_penalty, ngram, ban, bad_tok, bad_off):
        if ban is not None:
            x[:, ban.long()] = -float("inf")
        return x[:, :n].argmax(1)
    monkeypatch.setattr(ops, "logits_process_argmax", uniform)
    T = 12
    first = plain(T).sequences[0].tolist()
    kw = dict(min_new_tokens=6, eos_token_id=first[2])
    want = plain(T, **kw)
    got, eng, drafter = run(SaltedEngine(), 4, T, **kw)
    same(got, want)
    seq = want.sequences[0].tolist()
    assert got.assist_stats["accepted"] == got.assist_stats["drafted"] > 0
    assert seen and all(h == seq[:t] for t, h in seen)

"""CPU tests of prompt-lookup decoding's host side (radvlm_amd/generation.py): PromptLookupDrafter against the installed transformers'
PromptLookupCandidateGenerator, its extra cuts, the accept loop of greedy_generate driven by a fake engine (sequences, scores and
lookup_stats against the plain loop for drafters that are right for j tokens and then wrong; EOS, budget and stopping-criterion edges)
and the keyword validation."""
import numpy as np
import pytest
import torch

from radvlm_amd import ops
from radvlm_amd.engine import KVCache
from radvlm_amd.generation import (PromptLookupDrafter, clamp_draft, greedy_generate, parse_batch_kwargs, parse_beam_kwargs,
                                   parse_generate_kwargs)

V = 23


# ------------------------------------------------------------------------------------------------ drafter
def _hf_candidates(seq, k, max_ngram, eos):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=None if not eos else torch.tensor(eos), num_output_tokens=k,
                                         max_matching_ngram_size=max_ngram, max_length=10 ** 6)
    ids = torch.tensor(seq, dtype=torch.long)[None]
    out, _ = gen.get_candidates(ids)
    return out[0, len(seq):].numpy()


def test_drafter_matches_transformers():
    rng = np.random.default_rng(0)
    cases = nonempty = 0
    for trial in range(540):
        alphabet = int(rng.integers(3, 13))
        n = 1 + trial % 60
        seq = rng.integers(0, alphabet, n).tolist()
        k = (1, 3, 10)[trial % 3]
        max_ngram = (1, 2, 4)[(trial // 3) % 3]
        eos = [] if trial % 2 else sorted(set(rng.integers(0, alphabet, 1 + trial % 2).tolist()))
        want = _hf_candidates(seq, k, max_ngram, eos)
        got = PromptLookupDrafter(k, max_ngram, eos, vocab=alphabet).propose(np.array(seq))
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), (seq, k, max_ngram, eos, got, want)
        cases += 1
        nonempty += bool(len(want))
    assert cases >= 500 and nonempty * 3 >= cases, (cases, nonempty)


def test_drafter_lengths_one_and_two_have_no_draft_or_a_unigram_one():
    assert PromptLookupDrafter(3, 2).propose([5]).size == 0
    assert PromptLookupDrafter(3, 2).propose([5, 5]).tolist() == [5]
    assert PromptLookupDrafter(3, 2).propose([5, 6]).size == 0


def test_drafter_cuts():
    d = PromptLookupDrafter(10, 2, eos=[], vocab=50)
    # "7 8" occurs at the start; its continuation holds the image placeholder: cut before it
    assert d.propose([7, 8, 9, 10, -200, 11, 12, 7, 8]).tolist() == [9, 10]
    # an id >= vocab is cut before it as well
    assert d.propose([7, 8, 9, 50, 11, 7, 8]).tolist() == [9]
    assert d.propose([7, 8, 49, 11, 7, 8]).tolist() == [49, 11, 7, 8]
    # a placeholder may be part of the matched n-gram: the text after it still drafts
    assert d.propose([3, -200, 4, 5, 6, 1, 3, -200]).tolist() == [4, 5, 6, 1, 3]
    # EOS: cut before the first one; a match cut to nothing ends the search (HF does not try the next match)
    e = PromptLookupDrafter(10, 2, eos=[9], vocab=50)
    assert e.propose([7, 8, 1, 2, 9, 3, 7, 8]).tolist() == [1, 2]
    assert e.propose([7, 8, 9, 3, 7, 8, 4, 4, 7, 8]).size == 0
    # the continuation ends where the sequence ends and is at most k tokens
    assert PromptLookupDrafter(2, 2).propose([7, 8, 1, 2, 3, 7, 8]).tolist() == [1, 2]
    with pytest.raises(ValueError):
        PromptLookupDrafter(0, 2)
    with pytest.raises(ValueError):
        PromptLookupDrafter(3, 0)


def test_clamp_draft_budget_and_vocab():
    assert clamp_draft([1, 2, 3, 4], 2, 10).tolist() == [1, 2]
    assert clamp_draft([1, 2, 3, 4], 0, 10).size == 0
    assert clamp_draft([1, 2, 3, 4], -3, 10).size == 0
    assert clamp_draft([1, 2, -200, 4], 9, 10).tolist() == [1, 2]
    assert clamp_draft([1, 10, 3], 9, 10).tolist() == [1]
    assert clamp_draft([], 9, 10).size == 0


# ------------------------------------------------------------------------------------------------ accept loop on a fake engine
class FakeEngine:
    """Stands in for LlavaEngine on the CPU.  The "KV cache" holds the fed tokens as values and the logits at a position are a
    pseudo-random function of that position and of every token up to it, so a row that reads a stale or a wrong position changes.
    verify_step is R decode steps on one cache row that does not advance lens, as the real one."""
    vocab = V
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def logits_of(self, seq):
        h = len(seq)
        for v in seq:
            h = (h * 1000003 + int(v) + 7) % (1 << 61)
        return torch.from_numpy(np.random.default_rng(h).standard_normal(V).astype(np.float32))

    def prefill(self, ids, am, images, sizes, max_new_tokens=0):
        seq = [int(v) for v in ids[0]]
        L = len(seq) + max_new_tokens
        cache = KVCache([np.full((1, L), -7, dtype=np.int64)], np.array([len(seq)], dtype=np.int64), L)
        cache.layers[0][0, :len(seq)] = seq
        return cache, self.logits_of(seq)[None]

    def decode_step(self, cache, tokens):
        tokens = np.asarray(tokens).reshape(-1)
        assert tokens.shape[0] == 1 and cache.lens[0] < cache.L_max
        self.calls.append(("decode", int(cache.lens[0]), tokens.tolist()))
        cache.layers[0][0, cache.lens[0]] = tokens[0]
        cache.lens += 1
        return self.logits_of(cache.layers[0][0, :cache.lens[0]])[None]

    def verify_step(self, cache, tokens):
        tokens = np.asarray(tokens).reshape(-1)
        n0, R = int(cache.lens[0]), tokens.shape[0]
        assert 2 <= R <= 32 and n0 + R <= cache.L_max, (n0, R, cache.L_max)
        assert ((tokens >= 0) & (tokens < V)).all(), tokens
        self.calls.append(("verify", n0, tokens.tolist()))
        cache.layers[0][0, n0:n0 + R] = tokens
        return torch.stack([self.logits_of(cache.layers[0][0, :n0 + i + 1]) for i in range(R)])


@pytest.fixture(autouse=True)
def host_argmax(monkeypatch):
    monkeypatch.setattr(ops, "argmax_rows", lambda x, n, out=None: x[:, :n].argmax(1))


PROMPT = np.array([[3, 1, 4, 1, 5, 9, 2, 6]])


def run(drafter=None, eng=None, **kw):
    eng = eng or FakeEngine()
    cfg = parse_generate_kwargs(dict(kw, return_dict_in_generate=True, output_scores=True, output_logits=True), lookup=True)
    cfg.drafter = drafter
    return greedy_generate(eng, PROMPT, None, None, None, cfg), eng


class RightThenWrong:
    """Proposes the plain run's next j tokens, then tokens that are wrong, k in all -- whatever room the loop has left."""

    def __init__(self, plain, j, k, prompt_len=PROMPT.shape[1]):
        self.plain, self.j, self.k, self.P = [int(v) for v in plain], j, k, prompt_len
        self.seen = []

    def propose(self, seq):
        t = len(seq) - self.P
        self.seen.append([int(v) for v in seq])
        out = []
        for i in range(self.k):
            if t + i >= len(self.plain):
                out.append(0)
            else:
                out.append(self.plain[t + i] if i < self.j else (self.plain[t + i] + 1) % V)
        return np.array(out, dtype=np.int64)


def expected_stats(T, j, k):
    t, steps, drafted, accepted = 1, 0, 0, 0
    while t < T:
        nd = min(k, T - t - 1)
        acc = min(j, nd)
        steps, drafted, accepted, t = steps + 1, drafted + nd, accepted + acc, t + acc + 1
    return dict(steps=steps, drafted=drafted, accepted=accepted)


def same(a, b):
    assert torch.equal(a.sequences, b.sequences)
    assert len(a.scores) == len(b.scores) == a.sequences.shape[1] and len(a.logits) == len(b.logits) == a.sequences.shape[1]
    for x, y in zip(a.scores + a.logits, b.scores + b.logits):
        assert x.shape == (1, V) and torch.equal(x, y)


@pytest.mark.parametrize("k", [1, 3, 7])
def test_right_for_j_then_wrong(k):
    T = 24
    plain, _ = run(max_new_tokens=T)
    assert not hasattr(plain, "lookup_stats")
    seq = plain.sequences[0].tolist()
    for j in range(k + 1):
        d = RightThenWrong(seq, j, k)
        got, eng = run(d, max_new_tokens=T)
        same(got, plain)
        assert got.lookup_stats == expected_stats(T, j, k), (j, got.lookup_stats)
        # every call sees the prompt as passed followed by the emitted tokens
        assert all(s == PROMPT[0].tolist() + seq[:len(s) - PROMPT.shape[1]] for s in d.seen)
        # accepted == j in every step with room for it, and no position past the budget is fed
        for kind, n0, toks in eng.calls:
            assert n0 + len(toks) <= PROMPT.shape[1] + T - 1 + (kind == "decode")


def test_empty_draft_is_a_plain_decode_step():
    T = 9
    plain, _ = run(max_new_tokens=T)

    class Never:
        def propose(self, seq):
            return np.zeros(0, dtype=np.int64)
    got, eng = run(Never(), max_new_tokens=T)
    same(got, plain)
    assert got.lookup_stats == dict(steps=T - 1, drafted=0, accepted=0)
    assert [c[0] for c in eng.calls] == ["decode"] * (T - 1)


def test_default_drafter_is_built_from_the_kwargs():
    T = 16
    plain, _ = run(max_new_tokens=T)
    got, eng = run(None, max_new_tokens=T, prompt_lookup_num_tokens=4, max_matching_ngram_size=1)
    same(got, plain)
    assert got.lookup_stats["drafted"] > 0 and got.lookup_stats["steps"] <= T - 1
    assert any(c[0] == "verify" for c in eng.calls)


def test_unfit_ids_in_a_draft_are_never_fed():
    T = 12
    plain, _ = run(max_new_tokens=T)
    seq = plain.sequences[0].tolist()

    class Placeholder(RightThenWrong):
        def propose(self, s):
            out = super().propose(s)
            out[2:] = -200
            return out
    got, eng = run(Placeholder(seq, 7, 7), max_new_tokens=T)         # FakeEngine.verify_step asserts the ids
    same(got, plain)
    assert all(len(toks) <= 3 for kind, _, toks in eng.calls if kind == "verify")


def test_eos_inside_an_accepted_run_and_as_the_bonus_token():
    T = 24
    plain, _ = run(max_new_tokens=T)
    seq = plain.sequences[0].tolist()
    # first verify round of an oracle with k = 7 covers emitted positions 1 .. 8: EOS at position 4 lies inside the accepted run
    pos = next(p for p in range(3, 8) if seq[p] not in seq[:p])
    ref, _ = run(max_new_tokens=T, eos_token_id=seq[pos])
    assert ref.sequences.shape[1] == pos + 1
    got, eng = run(RightThenWrong(seq, 7, 7), max_new_tokens=T, eos_token_id=seq[pos])
    same(got, ref)
    assert got.lookup_stats["steps"] == 1
    # right for pos - 1 drafts, then wrong: the EOS is the choice after the accepted drafts
    got, eng = run(RightThenWrong(seq, pos - 1, 7), max_new_tokens=T, eos_token_id=seq[pos])
    same(got, ref)
    assert got.lookup_stats == dict(steps=1, drafted=7, accepted=pos - 1)
    # several EOS ids; the oracle's draft holds the EOS itself (an injected drafter need not cut it): the emission still ends there
    other = next(v for v in range(V) if v not in seq)
    got, eng = run(RightThenWrong(seq, 7, 7), max_new_tokens=T, eos_token_id=[other, seq[pos]])
    same(got, ref)
    assert seq[pos] in eng.calls[0][2]


def test_budget_ends_mid_draft():
    for T in (3, 5, 6):
        plain, _ = run(max_new_tokens=T)
        got, eng = run(RightThenWrong(plain.sequences[0].tolist() + [0] * 8, 7, 7), max_new_tokens=T)
        same(got, plain)
        assert got.lookup_stats == expected_stats(T, 7, 7)
        assert max(n0 + len(toks) for _, n0, toks in eng.calls) <= PROMPT.shape[1] + T - 1


@pytest.mark.parametrize("T", [0, 1, 2])
def test_tiny_budgets(T):
    plain, _ = run(max_new_tokens=T)
    got, eng = run(RightThenWrong([1] * 8, 0, 3), max_new_tokens=T)
    same(got, plain)
    assert got.sequences.shape == (1, T)
    assert got.lookup_stats == dict(steps=max(T - 1, 0), drafted=0, accepted=0)


def test_stopping_criterion_fires_mid_run():
    T = 24
    seen = {}

    def make(tag, stop_at):
        seen[tag] = []

        def crit(ids, scores):
            seen[tag].append((ids[0].tolist(), scores.clone()))
            return ids.shape[1] >= stop_at
        return crit
    full, _ = run(max_new_tokens=T)
    seq = full.sequences[0].tolist()
    plain, _ = run(max_new_tokens=T, stopping_criteria=[make("plain", 4)])
    got, eng = run(RightThenWrong(seq, 7, 7), max_new_tokens=T, stopping_criteria=[make("lookup", 4)])
    same(got, plain)
    assert got.sequences.shape[1] == 4 and got.lookup_stats == dict(steps=1, drafted=7, accepted=7)
    # once per emitted token, in order, with that token's own score row
    assert [c[0] for c in seen["lookup"]] == [seq[:i] for i in range(1, 5)]
    assert len(seen["plain"]) == len(seen["lookup"]) == 4
    for (ia, sa), (ib, sb) in zip(seen["plain"], seen["lookup"]):
        assert ia == ib and sa.shape == sb.shape == (1, V) and torch.equal(sa, sb)


# ------------------------------------------------------------------------------------------------ keywords
def test_kwarg_validation():
    cfg = parse_generate_kwargs(dict(prompt_lookup_num_tokens=5), lookup=True)
    assert (cfg.lookup.k, cfg.lookup.max_ngram) == (5, 2) and cfg.drafter is None
    cfg = parse_generate_kwargs(dict(prompt_lookup_num_tokens=31, max_matching_ngram_size=4), lookup=True)
    assert (cfg.lookup.k, cfg.lookup.max_ngram) == (31, 4)
    assert parse_generate_kwargs({}, lookup=True).lookup is None
    assert parse_generate_kwargs(dict(prompt_lookup_num_tokens=None), lookup=True).lookup is None
    for bad in (0, 32, -1, 2.0, "3", True, [3]):
        with pytest.raises(ValueError):
            parse_generate_kwargs(dict(prompt_lookup_num_tokens=bad), lookup=True)
    for bad in (0, -2, 1.5, "2"):
        with pytest.raises(ValueError):
            parse_generate_kwargs(dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=bad), lookup=True)
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(prompt_lookup_num_tokens=3, do_sample=True, seed=1), lookup=True)
    # generate_batch / generate_beams reject the names as they reject any unknown keyword
    for name in ("prompt_lookup_num_tokens", "max_matching_ngram_size"):
        with pytest.raises(TypeError):
            parse_batch_kwargs({name: 3}, 2)
        with pytest.raises(TypeError):
            parse_beam_kwargs({name: 3, "num_beams": 2})
        with pytest.raises(TypeError):
            parse_generate_kwargs({name: 3})


def test_more_than_one_prompt_row_is_refused():
    cfg = parse_generate_kwargs(dict(prompt_lookup_num_tokens=3, max_new_tokens=4), lookup=True)
    with pytest.raises(ValueError, match="one prompt row"):
        greedy_generate(FakeEngine(), np.concatenate([PROMPT, PROMPT]), None, None, None, cfg)

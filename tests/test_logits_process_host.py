"""CPU tests of generate()'s greedy logits processors: the numpy restatement (tests/logits_ref.py) against transformers' own processor
classes, keyword parsing and validation, the per-step ban lists, and the C-ABI declaration of rv_logits_process_argmax_f32."""
import os

import numpy as np
import pytest
import torch

from logits_ref import argmax, process_row, same_values
from radvlm_amd.generation import LogitsProcessors, min_new_length, parse_generate_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(rng, B, V):
    x = (rng.standard_normal((B, V)) * 4).astype(np.float32)
    x[:, rng.integers(0, V, 5)] = -np.inf                          # -inf entries
    x[0, 3] = x[0, 7] = x[0].max() + 1                              # a tie at the top
    x[1 % B, :] = np.round(x[1 % B, :])                             # many ties, zeros (signed) among them
    return x


def _hist(rng, B, t, V, pad):
    h = rng.integers(0, 12, (B, t))                                 # small ids: duplicates and repeated n-grams
    if t >= 4:
        h[:, t // 2:t // 2 + 2] = h[:, :2]                          # a guaranteed repeat
        h[-1, t - 2:] = pad                                         # a finished row's pads
    return h


@pytest.mark.parametrize("t", [0, 1, 2, 3, 6, 17])
@pytest.mark.parametrize("ngram", [1, 2, 3])
@pytest.mark.parametrize("penalty", [0.7, 1.3])
def test_restatement_matches_transformers(t, ngram, penalty):
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as LP
    rng = np.random.default_rng(1000 * t + 10 * ngram + int(penalty * 10))
    B, V, eos, pad, m = 4, 64, 5, 2, 4
    x = _rows(rng, B, V)
    h = _hist(rng, B, t, V, pad)
    bad = [[9], [3, 4], [1, 2, 3], [eos], [h[0, -1] if t else 6, 8]]
    kept = [w for w in bad if w != [eos]]
    suppress, begin = [11, 70, 13], [0, 12]
    procs = LP.LogitsProcessorList([
        LP.RepetitionPenaltyLogitsProcessor(penalty=penalty),
        LP.NoRepeatNGramLogitsProcessor(ngram),
        LP.NoBadWordsLogitsProcessor([[int(i) for i in w] for w in bad], eos_token_id=eos),
        LP.MinLengthLogitsProcessor(m, eos),
        LP.MinNewTokensLengthLogitsProcessor(0, m, eos),
        LP.SuppressTokensLogitsProcessor(suppress),
        LP.SuppressTokensAtBeginLogitsProcessor(begin, 0),
    ])
    want = procs(torch.from_numpy(h.astype(np.int64)).reshape(B, t), torch.from_numpy(x.copy())).numpy()
    for b in range(B):
        got = process_row(x[b], h[b], penalty=penalty, ngram=ngram, bad_words=kept, eos=[eos], min_new=m, suppress=suppress,
                          begin_suppress=begin)
        assert same_values(got, want[b]), (b, np.flatnonzero(~((got == want[b]) | (np.isnan(got) & np.isnan(want[b])))))
        assert argmax(got) == int(torch.argmax(torch.from_numpy(want[b])))


def test_restatement_penalty_alone_matches_transformers():
    """Every single processor alone on rows with penalties on both sides of 1 (IEEE fp32 x / p and x * p, no reciprocal)."""
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as LP
    rng = np.random.default_rng(7)
    B, V, t = 8, 4096, 300
    x = (rng.standard_normal((B, V)) * 30).astype(np.float32)
    h = rng.integers(0, V, (B, t))
    for p in (0.3, 0.9, 1.1, 1.2, 1.7, 3.0):
        want = LP.RepetitionPenaltyLogitsProcessor(penalty=p)(torch.from_numpy(h), torch.from_numpy(x.copy())).numpy()
        for b in range(B):
            assert same_values(process_row(x[b], h[b], penalty=p), want[b]), p
    for n in (1, 2, 3):
        hh = rng.integers(0, 5, (B, t))
        want = LP.NoRepeatNGramLogitsProcessor(n)(torch.from_numpy(hh), torch.from_numpy(x.copy())).numpy()
        for b in range(B):
            assert same_values(process_row(x[b], hh[b], ngram=n), want[b]), n


def test_disabled_values_leave_processors_off():
    for kw in ({}, dict(repetition_penalty=None), dict(repetition_penalty=1.0), dict(repetition_penalty=1), dict(no_repeat_ngram_size=0),
               dict(no_repeat_ngram_size=None), dict(min_new_tokens=0), dict(min_length=0), dict(suppress_tokens=[]),
               dict(begin_suppress_tokens=None), dict(min_new_tokens=5), dict(min_length=50)):
        cfg = parse_generate_kwargs(kw)                             # min constraints without an EOS id: off
        assert not LogitsProcessors(cfg, 1000, 10).active, kw
    cfg = parse_generate_kwargs(dict(min_new_tokens=0, eos_token_id=3))
    assert not LogitsProcessors(cfg, 1000).active
    assert LogitsProcessors(parse_generate_kwargs(dict(repetition_penalty=1.2)), 1000).active
    assert LogitsProcessors(parse_generate_kwargs(dict(no_repeat_ngram_size=3)), 1000).active
    assert LogitsProcessors(parse_generate_kwargs(dict(min_new_tokens=2, eos_token_id=3)), 1000).active


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=2),
                                dict(repetition_penalty="1.2"), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0),
                                dict(bad_words_ids=[]), dict(bad_words_ids=[3, 4]), dict(bad_words_ids=[[3], []]),
                                dict(bad_words_ids=[[3, -1]]), dict(bad_words_ids=[[3.0]]), dict(bad_words_ids=((3,),)),
                                dict(bad_words_ids=[[2]], eos_token_id=2), dict(min_new_tokens=-1), dict(min_length=1.5),
                                dict(suppress_tokens=[1.5]), dict(begin_suppress_tokens=3)])
def test_bad_values_raise_value_error(kw):
    with pytest.raises(ValueError):
        parse_generate_kwargs(kw)


@pytest.mark.parametrize("name", ["sequence_bias", "forced_bos_token_id", "forced_eos_token_id", "exponential_decay_length_penalty",
                                  "renormalize_logits", "logits_processor", "prefix_allowed_tokens_fn", "generation_config"])
def test_out_of_scope_names_still_raise_type_error(name):
    with pytest.raises(TypeError):
        parse_generate_kwargs({name: 1})


def test_new_names_are_accepted():
    cfg = parse_generate_kwargs(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, bad_words_ids=[[5], [6, 7]], min_length=4,
                                     min_new_tokens=2, suppress_tokens=[1], begin_suppress_tokens=[2], output_logits=True,
                                     eos_token_id=9))
    assert cfg.repetition_penalty == 1.2 and cfg.no_repeat_ngram_size == 3 and cfg.bad_words_ids == [(5,), (6, 7)]
    assert cfg.output_logits and cfg.suppress_tokens == [1] and cfg.begin_suppress_tokens == [2]


def test_eos_sequences_dropped_from_bad_words():
    cfg = parse_generate_kwargs(dict(bad_words_ids=[[2], [2, 3], [4], [4]], eos_token_id=[2, 8]))
    assert cfg.bad_words_ids == [(2, 3), (4,)]                      # [eos] dropped, [eos, x] kept, duplicates merged
    cfg = parse_generate_kwargs(dict(bad_words_ids=[[2]]))          # no EOS known: nothing to drop
    assert cfg.bad_words_ids == [(2,)]


def test_min_length_counts_the_prompt_and_min_new_tokens_wins():
    mk = lambda **k: parse_generate_kwargs(dict(eos_token_id=3, **k))
    assert min_new_length(mk(min_length=30), 20) == 10              # inputs_embeds generation: min_length - S
    assert min_new_length(mk(min_length=10), 20) == 0
    assert min_new_length(mk(min_new_tokens=4, min_length=30), 20) == 4
    assert min_new_length(mk(min_new_tokens=0, min_length=30), 20) == 0
    assert min_new_length(mk(), 20) == 0
    assert min_new_length(parse_generate_kwargs(dict(min_new_tokens=4)), 20) == 0        # no EOS: ignored
    assert min_new_length(parse_generate_kwargs(dict(min_length=40)), 20) == 0


def test_static_ban_lists_per_step():
    cfg = parse_generate_kwargs(dict(eos_token_id=[3, 2000], min_new_tokens=2, suppress_tokens=[7, -1, 5000], begin_suppress_tokens=[1],
                                     bad_words_ids=[[9], [4, 5]]))
    lp = LogitsProcessors(cfg, 1000)
    assert lp.static_ban(0) == [1, 3, 7, 9]                         # ids outside the vocabulary are ignored
    assert lp.static_ban(1) == [3, 7, 9]
    assert lp.static_ban(2) == [7, 9]
    tok, off = lp.bad_csr()
    assert tok.tolist() == [4, 5] and off.tolist() == [0, 2]
    with pytest.raises(ValueError):
        LogitsProcessors(parse_generate_kwargs(dict(bad_words_ids=[[4, 1000]])), 1000)   # HF: ids >= vocab raise


def test_logits_process_symbol_declared_and_bound():
    from radvlm_amd import lib
    assert "rv_logits_process_argmax_f32" in lib.SIGNATURES
    from radvlm_amd import ops
    assert callable(ops.logits_process_argmax)
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if os.path.exists(so):
        assert hasattr(lib.load(), "rv_logits_process_argmax_f32")

"""Host tests of prompt cache compression (prompt_kv_budget / prompt_kv_window / prompt_kv_pool; no GPU): the keywords are accepted,
defaulted, refused or rejected by the parsers, the needle input of the kernel tests meets its condition in fp64, tests/kvpress_ref.py's
pool and select do what the rule says on hand-written rows, and BatchScheduler sizes its cache and its memory check with
min(spliced, N) + budget and hands the engine compress= only when the keyword was given."""
import numpy as np
import pytest
import torch

import kvpress_ref as R
from radvlm_amd.engine import KVCache
from radvlm_amd.generation import (BatchScheduler, GenerationCache, batch_requests, parse_batch_kwargs, parse_beam_kwargs,
                                   parse_generate_kwargs, parse_prompt_kv)
from test_generate_batch_host import FakeEngine, HostPicker, _prompts


# ------------------------------------------------------------------------------------------------ parsers
def test_defaults_and_accepted_values():
    assert parse_generate_kwargs({}).kvpress is None and parse_batch_kwargs({}, 2).kvpress is None
    assert parse_generate_kwargs(dict(prompt_kv_budget=1024)).kvpress == (1024, 32, 7)
    assert parse_generate_kwargs(dict(prompt_kv_budget=np.int64(40), prompt_kv_window=8, prompt_kv_pool=3)).kvpress == (40, 8, 3)
    assert parse_generate_kwargs(dict(prompt_kv_budget=2, prompt_kv_window=1, prompt_kv_pool=1)).kvpress == (2, 1, 1)
    assert parse_generate_kwargs(dict(prompt_kv_budget=65, prompt_kv_window=64, prompt_kv_pool=63)).kvpress == (65, 64, 63)
    assert parse_batch_kwargs(dict(prompt_kv_budget=24, prompt_kv_window=8, max_new_tokens=[1, 2]), 2).kvpress == (24, 8, 7)
    assert parse_prompt_kv(dict(prompt_kv_budget=None)) is None


@pytest.mark.parametrize("kw", [
    dict(prompt_kv_budget=True), dict(prompt_kv_budget=100.0), dict(prompt_kv_budget="100"), dict(prompt_kv_budget=[100]),
    dict(prompt_kv_budget=32), dict(prompt_kv_budget=8, prompt_kv_window=8), dict(prompt_kv_budget=0, prompt_kv_window=1),
    dict(prompt_kv_budget=100, prompt_kv_window=0), dict(prompt_kv_budget=100, prompt_kv_window=65),
    dict(prompt_kv_budget=100, prompt_kv_window=True), dict(prompt_kv_budget=100, prompt_kv_window=8.0),
    dict(prompt_kv_budget=100, prompt_kv_pool=4), dict(prompt_kv_budget=100, prompt_kv_pool=0), dict(prompt_kv_budget=100, prompt_kv_pool=65),
    dict(prompt_kv_budget=100, prompt_kv_pool=-1), dict(prompt_kv_budget=100, prompt_kv_pool=False), dict(prompt_kv_budget=100, prompt_kv_pool=3.0),
    dict(prompt_kv_window=8), dict(prompt_kv_pool=3), dict(prompt_kv_window=8, prompt_kv_pool=3)])
def test_value_errors(kw):
    with pytest.raises(ValueError, match="prompt_kv_"):
        parse_generate_kwargs(dict(kw))
    with pytest.raises(ValueError, match="prompt_kv_"):
        parse_batch_kwargs(dict(kw), 2)


def test_beams_and_score_reject_the_names():
    for name in ("prompt_kv_budget", "prompt_kv_window", "prompt_kv_pool"):
        with pytest.raises(TypeError, match=name):
            parse_beam_kwargs({"num_beams": 2, name: 9})
    from radvlm_amd.llava.model.llava_llama import LlavaLlamaForCausalLM
    for name in ("prompt_kv_budget", "prompt_kv_window", "prompt_kv_pool"):
        with pytest.raises(TypeError, match=name):                          # score() refuses every keyword before it touches the model
            LlavaLlamaForCausalLM.score(None, [], [], **{name: 9})


def _refused(kw, other):
    with pytest.raises(NotImplementedError) as e:
        parse_generate_kwargs(dict(kw, prompt_kv_budget=100), lookup=True, attentions=True)
    assert "prompt_kv_budget" in str(e.value) and other in str(e.value)


def test_refuses_past_key_values():
    _refused(dict(past_key_values=GenerationCache()), "past_key_values")


def test_refuses_prompt_lookup():
    _refused(dict(prompt_lookup_num_tokens=4), "prompt_lookup_num_tokens")


def test_refuses_guidance():
    _refused(dict(guidance_scale=2.0, negative_prompt_ids=np.array([[1, 2]])), "guidance_scale")


def test_refuses_dola():
    _refused(dict(dola_layers="high"), "dola_layers")


def test_refuses_output_attentions():
    _refused(dict(output_attentions=True, return_dict_in_generate=True), "output_attentions")


def test_refuses_int8_cache():
    _refused(dict(kv_cache_dtype="int8"), "kv_cache_dtype")
    with pytest.raises(NotImplementedError, match="prompt_kv_budget"):
        parse_batch_kwargs(dict(prompt_kv_budget=100, kv_cache_dtype="int8"), 2)


def test_refuses_share_prefix():
    with pytest.raises(NotImplementedError) as e:
        parse_batch_kwargs(dict(prompt_kv_budget=100, share_prefix=True), 2)
    assert "prompt_kv_budget" in str(e.value) and "share_prefix" in str(e.value)
    assert parse_batch_kwargs(dict(prompt_kv_budget=100, share_prefix=False), 2).kvpress == (100, 32, 7)


def test_composes_with_sampling_processors_constraint():
    from radvlm_amd.constraints import TokenConstraint
    cfg = parse_generate_kwargs(dict(prompt_kv_budget=100, do_sample=True, seed=3, top_k=5, repetition_penalty=1.2,
                                     constraint=TokenConstraint.from_choices([[1, 2]], eos=[3])))
    assert cfg.kvpress == (100, 32, 7) and cfg.sampling is not None and cfg.constraint is not None


# ------------------------------------------------------------------------------------------------ the needle input
def _bf16(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("j_star", [3, 127, 128, 300])
def test_needle_condition_fp64(hd, j_star):
    """On the bf16-rounded inputs the kernel test uses (scale 1), the needle's vote exceeds every other prefix vote by 10x in fp64."""
    w, P = 8, 330
    q, k = R.needle(P, w, hd, j_star, seed=j_star)
    v = R.votes(_bf16(q), _bf16(k), w, 1.0)[0]
    others = np.delete(v, j_star)
    assert v[j_star] > 10.0 * others.max()
    assert R.select(v, w + 1, w, 1)[0] == j_star


# ------------------------------------------------------------------------------------------------ kvpress_ref
def test_pool_hand_rows():
    v = np.array([0., 5., 1., 0., 0., 2., 0.])
    assert R.pool(v, 1).tolist() == v.tolist()
    assert R.pool(v, 3).tolist() == [5., 5., 5., 1., 2., 2., 2.]
    assert R.pool(v, 5).tolist() == [5., 5., 5., 5., 2., 2., 2.]
    assert R.pool(v, 63).tolist() == [5.] * 7
    assert R.pool(np.float32([1, 2]), 3).dtype == np.float32               # a max: the values pass through unrounded


def test_select_hand_rows():
    v = np.array([0., 5., 1., 0., 0., 2., 0.])
    # k = 1: raw votes; the best two are positions 1 and 5; the window (w = 2) follows at 7, 8
    assert R.select(v, 4, 2, 1).tolist() == [1, 5, 7, 8]
    assert R.select(v, 5, 2, 1).tolist() == [1, 2, 5, 7, 8]
    # k = 3: pooled [5 5 5 1 2 2 2]: the plateau of 5s wins, lower positions first
    assert R.select(v, 4, 2, 3).tolist() == [0, 1, 7, 8]
    assert R.select(v, 6, 2, 3).tolist() == [0, 1, 2, 4, 7, 8]              # the cut falls inside the plateau of 2s: lowest position


def test_select_plateau_straddles_the_cut():
    v = np.array([1., 3., 3., 3., 3., 1., 3.])
    assert R.select(v, 1 + 3, 1, 1).tolist() == [1, 2, 3, 7]
    assert R.select(v, 1 + 5, 1, 1).tolist() == [1, 2, 3, 4, 6, 7]
    assert R.select(v, 1 + 6, 1, 1).tolist() == [0, 1, 2, 3, 4, 6, 7]       # the 1s tie too: position 0 before 5


def test_select_edges_one_kept_and_one_dropped():
    v = np.array([0.5, 0.25, 4., 0.125, 0.75])
    w = 3
    assert R.select(v, w + 1, w, 1).tolist() == [2, 5, 6, 7]                # N - w = 1
    assert R.select(v, w + 4, w, 1).tolist() == [0, 1, 2, 4, 5, 6, 7]       # N - w = n - 1: only the smallest leaves
    with pytest.raises(AssertionError):
        R.select(v, w + 5, w, 1)                                            # N = P: not a compressed sequence


def test_select_all_equal_keeps_the_lowest_positions():
    for k in (1, 3, 7):
        assert R.select(np.full(9, 0.25), 2 + 4, 2, k).tolist() == [0, 1, 2, 3, 9, 10]
        assert R.select(np.zeros(9), 2 + 4, 2, k).tolist() == [0, 1, 2, 3, 9, 10]


def test_votes_sum_and_causality():
    rng = np.random.default_rng(0)
    P, w, H, Hkv, hd = 11, 3, 4, 2, 8
    q, k = rng.standard_normal((P, H, hd)), rng.standard_normal((P, Hkv, hd))
    v = R.votes(q, k, w, 0.5)
    assert v.shape == (Hkv, P - w) and (v > 0).all()
    # each (head, window row) hands out one unit of probability, part of it to the window's own keys
    assert (v.sum(1) < (H // Hkv) * w).all()
    # causality: the last key is seen by the last window row alone, so with w = 1 fewer rows ... a window of the first w - 1 rows
    # (the same prompt cut by one position, window moved) never reads it
    k2 = k.copy()
    k2[P - 1] += 100.0
    assert not np.array_equal(R.votes(q, k, w, 0.5), R.votes(q, k2, w, 0.5))
    assert np.array_equal(R.votes(q[:P - 1], k[:P - 1], w - 1, 0.5), R.votes(q[:P - 1], k2[:P - 1], w - 1, 0.5))
    # one window row, one head, two keys: the vote is the softmax weight of key 0
    q1, k1 = np.zeros((2, 1, 1)), np.zeros((2, 1, 1))
    q1[1], k1[0], k1[1] = 1.0, np.log(3.0), 0.0
    assert np.allclose(R.votes(q1, k1, 1, 1.0), [[0.75]], rtol=1e-15)


# ------------------------------------------------------------------------------------------------ scheduler
class PressEngine(FakeEngine):
    """The fake engine with a prefill that takes compress=: a slot keeps the LAST min(len, N) spliced values (a stand-in for the kept
    positions) and the cache carries pos_off as the real one does."""

    def __init__(self, free=None):
        super().__init__(free)
        self.bytes_calls, self.cache_calls, self.compress_calls = [], [], []

    def kv_cache_bytes(self, B, L):
        self.bytes_calls.append((B, L))
        return super().kv_cache_bytes(B, L)

    def new_kv_cache(self, B, L):
        self.cache_calls.append((B, L))
        c = KVCache([np.full((B, L), -7, dtype=np.int64)], np.zeros(B, np.int64), L)
        return c

    def prefill(self, ids, am, images, sizes, max_new_tokens=0, cache=None, slots=None, compress=None):
        self.compress_calls.append(compress)
        N = compress[0]
        imgs = list(images or [])
        rows, k = [], 0
        if cache.pos_off is None:
            cache.pos_off = np.zeros(cache.B, dtype=np.int64)
        for b in range(ids.shape[0]):
            p = ids[b][am[b]]
            n_img = int((p == -200).sum())
            seq = self._splice(p, imgs[k:k + n_img])
            k += n_img
            s, kept = slots[b], seq[-N:]
            assert len(kept) <= cache.L_max
            cache.layers[0][s, :len(kept)] = kept
            cache.lens[s], cache.pos_off[s] = len(kept), len(seq) - len(kept)
            rows.append(self.logits_of(seq))
        self.prefills.append((tuple(slots), [len(r) for r in rows]))
        return cache, torch.stack(rows)


def _schedule(eng, n=5, slots=2, **kw):
    ps, ims = _prompts(n, 1)
    cfg = parse_batch_kwargs(dict(kw, max_new_tokens=4, eos_token_id=None), n)
    sch = BatchScheduler(eng, batch_requests(ps, ims), cfg, slots, picker=HostPicker(cfg))
    return sch, sch.run()


def test_scheduler_sizes_the_cache_with_the_budget():
    base, _ = _schedule(FakeEngine())
    longest = max(base.spliced)
    N = longest - 5
    assert N > 3
    eng = PressEngine()
    sch, out = _schedule(eng, prompt_kv_budget=N, prompt_kv_window=3, prompt_kv_pool=3)
    assert sch.L_max == max(min(s, N) + 4 for s in sch.spliced) == N + 4 < base.L_max
    assert eng.bytes_calls == [(2, sch.L_max)] and eng.cache_calls == [(2, sch.L_max)]
    assert eng.compress_calls and all(c == (N, 3, 3) for c in eng.compress_calls)
    assert all(len(o.generated_tokens) == 4 for o in out.values())


def test_scheduler_memory_check_uses_the_smaller_cache():
    base, _ = _schedule(FakeEngine())
    N = max(base.spliced) - 5
    need, need_full = 2 * (N + 4) * 8, 2 * base.L_max * 8
    _schedule(PressEngine(free=need), prompt_kv_budget=N, prompt_kv_window=3)       # fits exactly
    with pytest.raises(ValueError, match=f"needs {need} bytes"):
        _schedule(PressEngine(free=need - 1), prompt_kv_budget=N, prompt_kv_window=3)
    with pytest.raises(ValueError, match=f"needs {need_full} bytes"):              # the same memory does not hold the full cache
        _schedule(FakeEngine(free=need))


def test_scheduler_without_the_keyword_keeps_the_old_signature():
    """FakeEngine.prefill has no compress=: every call without the keyword still runs on it, and a budget no prompt exceeds changes
    neither L_max nor the tokens."""
    sch, want = _schedule(FakeEngine())
    big = max(sch.spliced) + 1
    sch2, same = _schedule(PressEngine(), prompt_kv_budget=big, prompt_kv_window=3)
    assert sch2.L_max == sch.L_max
    assert {k: v.generated_tokens for k, v in want.items()} == {k: v.generated_tokens for k, v in same.items()}

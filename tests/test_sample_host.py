"""CPU tests of seeded sampling's host side: the float64 restatement (tests/sample_ref.py) against transformers' warpers, keyword
parsing and the seed rule, the counter-based uniform, the scheduler handing each request its own seed and step, and the C ABI of
rv_sample_rows_f32."""
import os
import re

import numpy as np
import pytest
import torch

import sample_ref
from radvlm_amd import portable_rng
from radvlm_amd.generation import BatchScheduler, batch_requests, parse_batch_kwargs, parse_generate_kwargs
from test_generate_batch_host import FakeEngine, V, _prompts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,scale", [(1000, 1.0), (1000, 4.0), (32000, 1.0), (32000, 4.0)])
def test_restatement_keeps_what_transformers_keeps(n, scale):
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as LP
    has_min_p = hasattr(LP, "MinPLogitsWarper")                          # absent before transformers 4.41: only its settings are left out
    x = portable_rng.normal(11, n, (n,), scale)
    for T, k, p, mp in ((0.7, 0, 1.0, 0.0), (1.0, 50, 1.0, 0.0), (1.0, n + 5, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (1.0, 0, 0.5, 0.0),
                        (1.0, 0, 1.0, 0.05), (0.2, 50, 0.7, 0.0), (0.7, 50, 0.9, 0.05)):
        if mp > 0.0 and not has_min_p:
            continue
        s, kept, tail, q = sample_ref.warp_row(x, T, k, p, mp)
        sc = torch.from_numpy(x.copy())[None]
        ids = torch.zeros(1, 0, dtype=torch.long)
        sc = LP.TemperatureLogitsWarper(float(T))(ids, sc)
        assert np.array_equal(sc[0].numpy().view(np.uint32), s.view(np.uint32))          # the fp32 quotient
        if k:
            sc = LP.TopKLogitsWarper(top_k=k)(ids, sc)
        if p < 1.0:
            sc = LP.TopPLogitsWarper(top_p=float(p))(ids, sc)
        if mp > 0.0:
            sc = LP.MinPLogitsWarper(min_p=float(mp))(ids, sc)
        hf = torch.isfinite(sc[0]).numpy()
        # entries within 1e-4 of the cut (the largest band the GPU test may use) can fall either way in HF's fp32 softmax and cumsum
        band = 1e-4
        near = np.zeros(n, dtype=bool)
        if p < 1.0:
            near |= np.abs(tail - (1.0 - p)) <= band
        if mp > 0.0:
            e = np.exp(s.astype(np.float64) - float(s.max()))
            near |= np.abs(e - mp) <= band
        assert near.sum() <= max(1, n // 1000), (T, k, p, mp, int(near.sum()))
        assert np.array_equal(hf[~near], kept[~near]), (T, k, p, mp, np.flatnonzero(hf != kept)[:8])
        assert abs(q.sum() - 1.0) < 1e-12 and (q[~kept] == 0).all()


def test_draw_walks_the_cdf_in_id_order():
    q = np.array([0.1, 0.0, 0.4, 0.5])
    kept = np.array([True, False, True, True])
    assert [sample_ref.draw(q, kept, u) for u in (0.0, 0.0999, 0.1, 0.4999, 0.5, 0.999999)] == [0, 0, 2, 2, 3, 3]


# ------------------------------------------------------------------------------------------------ keywords
def test_sampling_defaults_follow_hf():
    c = parse_generate_kwargs(dict(do_sample=True, seed=7))
    sm = c.sampling
    assert (sm.temperature, sm.top_k, sm.top_p, sm.min_p, sm.seed) == (1.0, 50, 1.0, 0.0, 7)
    sm = parse_generate_kwargs(dict(do_sample=True, seed=7, temperature=0.2, top_p=0.7, top_k=None, min_p=0.05)).sampling
    assert (sm.temperature, sm.top_k, sm.top_p, sm.min_p) == (0.2, 0, 0.7, 0.05)
    assert parse_generate_kwargs(dict(do_sample=True, seed=0, top_k=0)).sampling.top_k == 0
    assert parse_generate_kwargs(dict(do_sample=True, seed=0, top_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)).sampling.top_p == 1.0
    assert parse_generate_kwargs(dict(max_new_tokens=3)).sampling is None
    # greedy: the sampling knobs are accepted and ignored, as before
    assert parse_generate_kwargs(dict(do_sample=False, temperature=0.2, top_p=0.7, top_k=3, min_p=0.1)).sampling is None


def test_sampling_validation():
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature="hot"), dict(temperature=float("inf")), dict(temperature=1e-50),
                dict(temperature=1e39), dict(top_k=-1),
                dict(top_k=2.5), dict(top_p=1.5), dict(top_p=-0.1), dict(min_p=2.0), dict(min_p=-0.5)):
        with pytest.raises(ValueError):
            parse_generate_kwargs(dict(do_sample=True, seed=1, **bad))
    for bad in (dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=1e-3)):
        with pytest.raises(NotImplementedError):
            parse_generate_kwargs(dict(do_sample=True, seed=1, **bad))
    for bad in (dict(seed=-1), dict(seed=1 << 63), dict(seed="abc"), dict(seed=1.5), dict(seed=[1, 2.5]), dict(seed=True)):
        with pytest.raises(ValueError):
            parse_generate_kwargs(dict(do_sample=True, **bad))
    with pytest.raises(NotImplementedError) as e:
        parse_generate_kwargs(dict(do_sample=True))
    assert "seed=" in str(e.value) and "global RNG" in str(e.value)
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(do_sample=True, temperature=0.2, top_p=0.7))
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs(dict(do_sample=True), 3)
    for kw in (dict(seed=3), dict(seed=3, do_sample=False), dict(seed=[1, 2])):
        with pytest.raises(ValueError):
            parse_generate_kwargs(kw)
    # what was out of scope stays out of scope with sampling on
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(do_sample=True, seed=1, num_beams=2))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(do_sample=True, seed=1, num_return_sequences=2))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(do_sample=True, seed=1, streamer=object()))


def test_seed_forms():
    from radvlm_amd.generation import sampling_seeds
    sm = parse_generate_kwargs(dict(do_sample=True, seed=10)).sampling
    assert sampling_seeds(sm, 4) == [10, 11, 12, 13]
    sm = parse_generate_kwargs(dict(do_sample=True, seed=[5, 5, 9])).sampling
    assert sampling_seeds(sm, 3) == [5, 5, 9]
    with pytest.raises(ValueError):
        sampling_seeds(sm, 2)
    sm = parse_generate_kwargs(dict(do_sample=True, seed=np.array([4, 2]))).sampling
    assert sampling_seeds(sm, 2) == [4, 2]
    assert parse_batch_kwargs(dict(do_sample=True, seed=[1, 2, 3]), 3).sampling.seed == [1, 2, 3]
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(do_sample=True, seed=[1, 2]), 3)
    with pytest.raises(ValueError):
        sampling_seeds(parse_generate_kwargs(dict(do_sample=True, seed=(1 << 63) - 2)).sampling, 4)     # s + i leaves the range


# ------------------------------------------------------------------------------------------------ the uniform
def test_uniform_is_the_portable_stream_and_exact():
    from radvlm_amd.generation import sample_uniform
    for seed in (0, 1, 7, 123456789, (1 << 40) + 3, (1 << 63) - 1):
        for t in (0, 1, 2, 63, 1000, 99999):
            u = sample_uniform(seed, t)
            assert 0.0 < u < 1.0 and (u * 2.0 ** 25) % 2 == 1                        # an odd multiple of 2^-25, exact in float64
            if seed * 1000003 < 1 << 64:                                              # where the numpy stream takes the seed
                bits = int(portable_rng._stream(seed, 0, t + 1)[t])
                assert u == ((bits >> 40) + 0.5) * 2.0 ** -24 == sample_ref.uniform(seed, t)
    us = np.array([sample_uniform(3, t) for t in range(4000)])
    assert abs(us.mean() - 0.5) < 0.02 and len(set(us.tolist())) > 3990


def test_library_restates_the_uniform():
    from radvlm_amd import lib
    from radvlm_amd.generation import sample_uniform
    if not os.path.exists(os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")):
        pytest.skip("library not built")
    L = lib.load()
    for seed in (0, 1, 7, 123456789, (1 << 40) + 3, (1 << 63) - 1):
        for t in (0, 1, 2, 63, 1000, 99999, (1 << 31) - 1):
            assert (L.rv_sample_uniform24(seed, t) + 0.5) * 2.0 ** -24 == sample_uniform(seed, t), (seed, t)


# ------------------------------------------------------------------------------------------------ the scheduler
class SamplingPicker:
    """Draws with the float64 restatement, each row with the seed and step the scheduler hands it; records every call."""

    def __init__(self, sm):
        self.sm, self.calls = sm, []

    def __call__(self, logits, slot, t, min_new, seed=None):
        assert seed is not None and len(seed) == logits.shape[0]
        self.calls.append((slot.tolist(), t.tolist(), [int(s) for s in seed]))
        sm, tok, lp = self.sm, [], []
        for r in range(logits.shape[0]):
            s, kept, _, q = sample_ref.warp_row(logits[r].numpy(), sm.temperature, sm.top_k, sm.top_p, sm.min_p)
            k = sample_ref.draw(q, kept, sample_ref.uniform(int(seed[r]), int(t[r])))
            tok.append(k)
            lp.append(float(np.log(q[k])))
        return np.array(tok), np.array(lp)


def _sampled_alone(eng, ids, images, budget, sm, seed):
    seq, out = eng._splice(ids, images), []
    for t in range(budget):
        s, kept, _, q = sample_ref.warp_row(eng.logits_of(seq).numpy(), sm.temperature, sm.top_k, sm.top_p, sm.min_p)
        k = sample_ref.draw(q, kept, sample_ref.uniform(seed, t))
        out.append(k)
        seq = seq + [k]
    return out


@pytest.mark.parametrize("seed", [100, [9, 9, 4, 77, 3, 12, 5]])
def test_scheduler_hands_each_request_its_seed_and_step(seed):
    n = 7
    budgets = [5, 1, 9, 3, 7, 2, 6]
    ps, ims = _prompts(n, 4)
    cfg = parse_batch_kwargs(dict(do_sample=True, seed=seed, temperature=0.8, top_k=12, top_p=0.9, max_new_tokens=budgets), n)
    eng = FakeEngine()
    picker = SamplingPicker(cfg.sampling)
    sch = BatchScheduler(eng, batch_requests(ps, ims), cfg, 2, return_logprobs=True, picker=picker)
    out = sch.run()
    seeds = [seed + i for i in range(n)] if isinstance(seed, int) else seed
    # every row of every call carries the seed of the request that owns its slot at that time, and that request's own step
    owner, done = {}, {}
    calls = iter(picker.calls)
    for ev in sch.events:
        if ev[0] == "admit":
            for q, s in zip(ev[1], ev[2]):
                owner[s] = q
                done[q] = 0
            slots, ts, sd = next(calls)
            assert sorted(slots) == sorted(ev[2])
        elif ev[0] == "decode":
            slots, ts, sd = next(calls)
        else:
            owner = {s: q for s, q in owner.items() if q != ev[1]}
            continue
        for s, t, v in zip(slots, ts, sd):
            if s in owner:
                assert v == seeds[owner[s]] and t == done[owner[s]], (ev, s, t, v)
                done[owner[s]] += 1
    assert len({tuple(e[1]) for e in sch.events if e[0] == "admit"}) > 2         # admissions did reorder the slots
    for i in range(n):
        o = out[f"req_{i}"]
        want = _sampled_alone(eng, ps[i], [] if ims[i] is None else [ims[i]], budgets[i], cfg.sampling, seeds[i])
        assert o.generated_tokens == want, i
        assert len(o.logprobs) == budgets[i] and all(v <= 0 for v in o.logprobs)
    assert len({tuple(out[f"req_{i}"].generated_tokens) for i in range(n)}) > 1


def test_greedy_pickers_are_called_as_before():
    """Without sampling the picker gets no seed (older pickers keep working)."""
    seen = []

    def picker(logits, slot, t, min_new):
        seen.append(len(slot))
        return np.zeros(len(slot), dtype=np.int64), np.zeros(len(slot))

    ps, ims = _prompts(3, 1)
    cfg = parse_batch_kwargs(dict(max_new_tokens=2), 3)
    BatchScheduler(FakeEngine(), batch_requests(ps, ims), cfg, 2, picker=picker).run()
    assert seen


# ------------------------------------------------------------------------------------------------ the C ABI
def test_sample_symbol_declared_and_bound():
    from radvlm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "radvlm_hip.h")).read()
    assert {"rv_sample_rows_f32", "rv_sample_uniform24"} <= set(lib.SIGNATURES)
    assert re.search(r"depth = (\d+)", hdr) and int(re.search(r"depth = (\d+)", hdr).group(1)) == sample_ref.DEPTH
    assert "sample" in open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read().split('SRCS="')[1].split('"')[0].split()
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if os.path.exists(so):
        L = lib.load()
        assert hasattr(L, "rv_sample_rows_f32") and hasattr(L, "rv_sample_uniform24")

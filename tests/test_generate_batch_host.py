"""CPU tests of generate_batch()'s host side: argument handling, the continuous-batching scheduler driven by a fake engine and a host
token picker (admission order and grouping, slot reuse, per-request budgets and EOS minima, stopping criteria, determinism), and the
C-ABI declaration of rv_logits_process_argmax_rows_f32."""
import os

import numpy as np
import pytest
import torch

from logits_ref import argmax, process_row
from radvlm_amd.engine import KVCache
from radvlm_amd.generation import BatchScheduler, batch_requests, parse_batch_kwargs
from radvlm_amd.splice import IMAGE_TOKEN_INDEX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 61
IMG_ROWS = 3


class FakeEngine:
    """Stands in for LlavaEngine on the CPU.  Its "KV cache" holds each slot's spliced positions as values (an image token becomes
    IMG_ROWS values derived from the image), and the logits of a sequence are a pseudo-random function of every position it holds --
    so a row's output changes if it reads another slot's or a stale position."""
    vocab = V
    device = torch.device("cpu")

    def __init__(self, free=None):
        self.free = free
        self.prefills, self.decodes = [], []

    def _splice(self, ids, images):
        out, k = [], 0
        for v in ids:
            if v == IMAGE_TOKEN_INDEX:
                base = int(float(images[k].float().sum()) * 1000) % 997
                out += [1000 + base + j for j in range(IMG_ROWS)]
                k += 1
            else:
                out.append(int(v))
        return out

    def logits_of(self, seq):
        h = 0
        for v in seq:
            h = (h * 1000003 + int(v) + 7) % (1 << 61)
        return torch.from_numpy(np.random.default_rng(h).standard_normal(V).astype(np.float32))

    def plan(self, ids, am, labels, images, sizes):
        ids = np.asarray(ids)
        k = int((ids[0] == IMAGE_TOKEN_INDEX).sum())
        n = ids.shape[1] + (IMG_ROWS - 1) * k
        return dict(lens=np.array([n]), S=n)

    def kv_cache_bytes(self, B, L):
        return B * L * 8

    def free_device_bytes(self):
        return self.free

    def new_kv_cache(self, B, L):
        return KVCache([np.full((B, L), -7, dtype=np.int64)], np.zeros(B, np.int64), L)

    def prefill(self, ids, am, images, sizes, max_new_tokens=0, cache=None, slots=None):
        imgs = list(images or [])
        rows, k = [], 0
        for b in range(ids.shape[0]):
            p = ids[b][am[b]]
            n_img = int((p == IMAGE_TOKEN_INDEX).sum())
            seq = self._splice(p, imgs[k:k + n_img])
            k += n_img
            s = slots[b]
            assert len(seq) <= cache.L_max
            cache.layers[0][s, :len(seq)] = seq
            cache.lens[s] = len(seq)
            rows.append(self.logits_of(seq))
        self.prefills.append((tuple(slots), [len(r) for r in rows]))
        return cache, torch.stack(rows)

    def decode_step(self, cache, tokens):
        tokens = np.asarray(tokens)
        self.decodes.append((cache.lens.copy(), tokens.copy()))
        assert (cache.lens < cache.L_max).all()
        rows = []
        for b in range(cache.B):
            cache.layers[0][b, cache.lens[b]] = tokens[b]
            rows.append(self.logits_of(cache.layers[0][b, :cache.lens[b] + 1]))
        cache.lens += 1
        return torch.stack(rows)


class HostPicker:
    """Token choice through the numpy restatement of the processors (tests/logits_ref.py), each row at its own step; the processed row
    is written back (criteria see it).  Records every call."""

    def __init__(self, cfg):
        self.cfg, self.hist, self.calls = cfg, {}, []

    def __call__(self, logits, slot, t, min_new):
        self.calls.append((slot.tolist(), t.tolist(), min_new.tolist()))
        c = self.cfg
        tok, lp = [], []
        for r in range(logits.shape[0]):
            s, tt = int(slot[r]), int(t[r])
            h = self.hist.get(s, [])[:tt]
            x = process_row(logits[r].numpy(), h, penalty=c.repetition_penalty, ngram=c.no_repeat_ngram_size, bad_words=c.bad_words_ids,
                            eos=c.eos, min_new=int(min_new[r]), suppress=c.suppress_tokens, begin_suppress=c.begin_suppress_tokens)
            logits[r] = torch.from_numpy(x)
            k = argmax(x)
            tok.append(k)
            x64 = x.astype(np.float64)
            lp.append(x64[k] - (x64.max() + np.log(np.exp(x64 - x64.max()).sum())))
            self.hist[s] = h + [k]
        return np.array(tok), np.array(lp)


def alone(eng, ids, images, budget, cfg, min_new=0):
    """One request by itself: the greedy loop of generate() at B = 1 on the fake engine."""
    seq = eng._splice(ids, images)
    out = []
    for t in range(budget):
        x = process_row(eng.logits_of(seq).numpy(), out, penalty=cfg.repetition_penalty, ngram=cfg.no_repeat_ngram_size,
                        bad_words=cfg.bad_words_ids, eos=cfg.eos, min_new=min_new, suppress=cfg.suppress_tokens,
                        begin_suppress=cfg.begin_suppress_tokens)
        k = argmax(x)
        out.append(k)
        if k in cfg.eos:
            break
        seq = seq + [k]
    return out


def _prompts(n, seed=0):
    rng = np.random.default_rng(seed)
    ps, ims = [], []
    for i in range(n):
        p = rng.integers(0, V, int(rng.integers(3, 12))).astype(np.int64)
        if i % 3 != 2:
            p[1] = IMAGE_TOKEN_INDEX
            ims.append(torch.full((3, 4, 4), float(i % 4)))
        else:
            ims.append(None)
        ps.append(p)
    return ps, ims


def _run(n=9, slots=3, admit=None, free=None, seed=0, **kw):
    ps, ims = _prompts(n, seed)
    cfg = parse_batch_kwargs(kw, n)
    eng = FakeEngine(free=free)
    picker = HostPicker(cfg)
    sch = BatchScheduler(eng, batch_requests(ps, ims), cfg, slots, return_logprobs=True, admit_free=admit, picker=picker)
    out = sch.run()
    return out, sch, eng, picker, ps, ims, cfg


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs(dict(do_sample=True), 2)
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs(dict(num_beams=3), 2)
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs(dict(streamer=object()), 2)
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs(dict(inputs_embeds=torch.zeros(1, 2, 8)), 2)
    with pytest.raises(NotImplementedError):
        parse_batch_kwargs({}, 2, lora=True)
    for name in ("attention_mask", "past_key_values", "position_ids", "output_scores", "output_logits", "return_dict_in_generate"):
        with pytest.raises(TypeError):
            parse_batch_kwargs({name: torch.ones(1) if name == "attention_mask" else True}, 2)
    with pytest.raises(TypeError):
        parse_batch_kwargs(dict(no_such_option=1), 2)
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(max_new_tokens=[1, 2, 3]), 2)
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(max_new_tokens=[1, -2]), 2)
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(max_new_tokens=-1), 2)
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(repetition_penalty=-1.0), 2)
    c = parse_batch_kwargs(dict(max_new_tokens=[4, 0], pad_token_id=5, do_sample=False, num_beams=1, temperature=0.3, use_cache=True), 2)
    assert c.budgets == [4, 0] and c.max_new_tokens is None and c.pad == 5
    c = parse_batch_kwargs(dict(max_new_tokens=6, output_scores=False, attention_mask=None), 2)
    assert c.budgets is None and c.max_new_tokens == 6


def test_request_errors():
    img = torch.zeros(3, 4, 4)
    with_img = np.array([1, IMAGE_TOKEN_INDEX, 2])
    with pytest.raises(ValueError):
        batch_requests([with_img, [1, 2]], images=[img])                         # a list of the wrong length
    with pytest.raises(ValueError):
        batch_requests([with_img], image_sizes=[(4, 4), (4, 4)])
    with pytest.raises(ValueError):
        batch_requests([with_img])                                                # image token, no image
    with pytest.raises(ValueError):
        batch_requests([with_img], images=[[img, img]])                           # two images, one token
    with pytest.raises(ValueError):
        batch_requests([[1, 2]], images=[img])                                    # an image without a token
    with pytest.raises(ValueError):
        batch_requests([np.zeros((2, 3), np.int64)])                              # not 1-D
    with pytest.raises(ValueError):
        batch_requests([[]])
    with pytest.raises(ValueError):
        batch_requests([with_img, with_img], images=[img, img], image_sizes=[(4, 4), None])
    r = batch_requests([torch.tensor([1, 2]), [3, IMAGE_TOKEN_INDEX, IMAGE_TOKEN_INDEX], np.array([4])],
                       images=[None, [img, img], None], image_sizes=[None, [(4, 4), (5, 6)], None])
    assert [q.ids.tolist() for q in r] == [[1, 2], [3, IMAGE_TOKEN_INDEX, IMAGE_TOKEN_INDEX], [4]]
    assert len(r[1].images) == 2 and r[1].sizes == [(4, 4), (5, 6)] and r[0].images == []
    assert batch_requests([with_img], images=[img], image_sizes=[(4, 5)])[0].sizes == [(4, 5)]


def test_no_requests():
    cfg = parse_batch_kwargs({}, 0)
    eng = FakeEngine()
    assert BatchScheduler(eng, batch_requests([]), cfg, 4).run() == {}
    assert eng.prefills == [] and eng.decodes == []
    with pytest.raises(ValueError):
        BatchScheduler(eng, batch_requests([]), cfg, 0)


# ------------------------------------------------------------------------------------------------ the scheduler
def test_every_request_equals_its_alone_run():
    budgets = [5, 0, 9, 1, 3, 12, 7, 2, 6]
    out, sch, eng, _, ps, ims, cfg = _run(max_new_tokens=budgets)
    assert list(out) == [f"req_{i}" for i in range(9)]
    for i, p in enumerate(ps):
        o = out[f"req_{i}"]
        assert o.request_id == f"req_{i}" and o.prompt_ids == p.tolist() and o.error is None and o.is_finished()
        assert o.generated_tokens == alone(eng, p, [] if ims[i] is None else [ims[i]], budgets[i], cfg), i
        assert len(o.logprobs) == len(o.generated_tokens) and all(v <= 0 for v in o.logprobs)
    assert out["req_1"].generated_tokens == []                                   # budget 0: never runs
    assert all(1 not in ev[1] for ev in sch.events if ev[0] == "admit")


def test_admission_order_grouping_and_slot_reuse():
    budgets = [4, 9, 2, 7, 3, 5, 8, 6, 1]
    out, sch, eng, picker, *_ = _run(slots=3, admit=2, max_new_tokens=budgets)
    admits = [ev for ev in sch.events if ev[0] == "admit"]
    order = [q for ev in admits for q in ev[1]]
    assert order == list(range(9))                                              # input order
    assert admits[0][1] == (0, 1, 2) and admits[0][2] == (0, 1, 2)              # nothing decoding: the first group fills every slot
    assert all(len(ev[1]) >= 2 or ev is admits[-1] for ev in admits[1:])       # later groups wait for 2 free slots (or take the rest)
    assert sorted(s for ev in admits for s in ev[2]) != sorted(set(s for ev in admits for s in ev[2]))   # slots were reused
    # each group is one prefill, into exactly its slots (image requests first within the group)
    assert [sorted(p[0]) for p in eng.prefills] == [sorted(ev[2]) for ev in admits]
    # the first pick of an admitted group runs every row at t = 0 with its request's EOS minimum
    first = [c for c in picker.calls if len(c[0]) != 3 or c[0] != [0, 1, 2]]
    assert all(all(t == 0 for t in c[1]) for c in first)
    # idle slots are fed token 0 at position 0; decode events list the active slots
    decodes = [ev for ev in sch.events if ev[0] == "decode"]
    assert len(decodes) == len(eng.decodes)
    for ev, (lens, toks) in zip(decodes, eng.decodes):
        idle = [s for s in range(3) if s not in ev[1]]
        assert all(lens[s] == 0 and toks[s] == 0 for s in idle)
        assert all(lens[s] > 0 for s in ev[1])
    # a finished request frees its slot; every request finished exactly once with its budget (no EOS set)
    fin = [ev for ev in sch.events if ev[0] == "finish"]
    assert sorted(ev[1] for ev in fin) == list(range(9)) and all(ev[3] == budgets[ev[1]] for ev in fin)


def test_threshold_groups_admissions():
    budgets = [3, 30, 30, 30, 4, 5, 6, 30, 30, 30, 2, 2]
    _, sch1, *_ = _run(n=12, slots=4, admit=1, max_new_tokens=budgets)
    _, sch3, *_ = _run(n=12, slots=4, admit=3, max_new_tokens=budgets)
    g1 = [len(ev[1]) for ev in sch1.events if ev[0] == "admit"]
    g3 = [len(ev[1]) for ev in sch3.events if ev[0] == "admit"]
    assert g1[0] == g3[0] == 4 and len(g3) < len(g1)
    assert all(g >= 3 for g in g3[1:-1])


def test_budgets_from_int_list_and_max_length():
    out, sch, eng, _, ps, ims, cfg = _run(max_new_tokens=4)
    assert all(len(o.generated_tokens) == 4 for o in out.values())
    out, sch, *_ = _run(max_length=12)                                          # counts each request's own spliced prompt
    assert [len(o.generated_tokens) for o in out.values()] == [max(0, 12 - n) for n in sch.spliced]
    out, sch, *_ = _run()                                                       # HF's default of 20
    assert all(len(o.generated_tokens) == 20 for o in out.values())
    assert sch.L_max == max(n + 20 for n in sch.spliced) and sch.slots == 3


def test_per_request_eos_minimum_and_eos():
    out0, sch, eng, _, ps, ims, cfg0 = _run(max_new_tokens=16)
    eos = out0["req_0"].generated_tokens[2]
    out, sch, eng, picker, ps, ims, cfg = _run(max_new_tokens=16, eos_token_id=eos, min_length=9)
    for i, p in enumerate(ps):
        mn = max(9 - sch.spliced[i], 0)
        assert sch.min_new[i] == mn
        got = out[f"req_{i}"].generated_tokens
        assert got == alone(eng, p, [] if ims[i] is None else [ims[i]], 16, cfg, min_new=mn), i
        assert eos not in got[:mn] and (got[-1] == eos or len(got) == 16)
        assert eos not in got[:-1]
    assert any(mn > 0 for mn in sch.min_new) and any(mn == 0 for mn in sch.min_new)
    out, *_ = _run(max_new_tokens=16, eos_token_id=eos, min_new_tokens=5)
    assert all(eos not in o.generated_tokens[:5] for o in out.values())


def test_processors_per_request():
    kw = dict(repetition_penalty=1.5, no_repeat_ngram_size=2, bad_words_ids=[[3], [4, 5]], suppress_tokens=[6], begin_suppress_tokens=[7])
    budgets = [8, 3, 11, 0, 6, 9, 2, 10, 4]
    out, sch, eng, _, ps, ims, cfg = _run(max_new_tokens=budgets, **kw)
    for i, p in enumerate(ps):
        assert out[f"req_{i}"].generated_tokens == alone(eng, p, [] if ims[i] is None else [ims[i]], budgets[i], cfg), i


def test_stopping_criteria_per_request():
    seen = []

    def crit(ids, scores):
        seen.append((tuple(ids.shape), tuple(scores.shape)))
        return ids.shape[1] >= 3 and int(ids[0, 0]) % 2 == 0

    out, sch, eng, _, ps, ims, cfg = _run(max_new_tokens=8, stopping_criteria=[crit])
    assert all(s[0][0] == 1 and s[1] == (1, V) for s in seen)
    for i, p in enumerate(ps):
        free = alone(eng, p, [] if ims[i] is None else [ims[i]], 8, cfg)
        got = out[f"req_{i}"].generated_tokens
        assert got == (free[:3] if free[0] % 2 == 0 else free), i
    assert sum(len(o.generated_tokens) for o in out.values()) == len(seen)


def test_identical_schedules_and_outputs():
    kw = dict(max_new_tokens=[5, 2, 9, 1, 3, 12, 7, 2, 6], repetition_penalty=1.2)
    a, sa, ea, *_ = _run(**kw)
    b, sb, eb, *_ = _run(**kw)
    assert sa.events == sb.events and ea.prefills == eb.prefills
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(ea.decodes, eb.decodes))
    assert {k: (v.generated_tokens, v.logprobs) for k, v in a.items()} == {k: (v.generated_tokens, v.logprobs) for k, v in b.items()}


def test_stale_positions_are_never_read():
    """One slot, prompts of decreasing length: the slot's later positions still hold the previous request's tokens."""
    ps = [np.arange(20) % V, np.arange(12) % V + 3, np.arange(5) % V + 9]
    cfg = parse_batch_kwargs(dict(max_new_tokens=6), 3)
    eng = FakeEngine()
    out = BatchScheduler(eng, batch_requests(ps), cfg, 1, picker=HostPicker(cfg)).run()
    for i, p in enumerate(ps):
        assert out[f"req_{i}"].generated_tokens == alone(eng, p, [], 6, cfg)


def test_cache_size_is_checked_before_allocation():
    with pytest.raises(ValueError, match="bytes"):
        _run(free=100, max_new_tokens=5)
    out, sch, *_ = _run(free=10 ** 9, max_new_tokens=5)
    assert len(out) == 9


def test_rows_symbol_declared_and_bound():
    from radvlm_amd import lib, ops
    name = "rv_logits_process_argmax_rows_f32"
    assert name in lib.SIGNATURES
    assert callable(ops.logits_process_argmax_rows)
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if os.path.exists(so):
        assert hasattr(lib.load(), name)

"""The call trace of radvlm_amd/generation.py, pinned: a recording fake engine and recording stand-ins for the ops entry points run a
matrix of small generate() / generate_batch() calls on the CPU, and every call's ordered list of engine and op calls -- name, row
count, step(s), which optional tensors were None, the keywords passed, the engine._dev uploads and .cpu() syncs since the entry
before -- and its returned tokens have to equal tests/golden/generation_call_trace.json.

The fixture is recorded by running this file as a script with --record; it is recorded from the commit BEFORE a refactor of
generation.py and has to pass unmodified after it.  A trace entry that has to change is a behaviour change."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from constraint_ref import constrain_rows_ref
from logits_ref import process_row
from radvlm_amd import ops
from radvlm_amd.constraints import TokenConstraint
from radvlm_amd.engine import KVCache
from radvlm_amd.generation import (BatchScheduler, GenerationCache, batch_requests, greedy_generate, parse_batch_kwargs,
                                   parse_generate_kwargs, sample_uniform)
from radvlm_amd.splice import IMAGE_TOKEN_INDEX

GOLDEN = os.path.join(ROOT, "tests", "golden", "generation_call_trace.json")
V, EOS, IMG_ROWS = 32, 2, 3
PROMPTS = np.array([[3, 1, 4, 1, 5], [9, 2, 6, 5, 3], [5, 8, 9, 7, 9]], dtype=np.int64)
SYS = (np.arange(130) * 7 % V).astype(np.int64)               # a shared "system prompt" longer than one decode chunk


class Rec:
    """The ordered trace of one call.  dev / cpu count the engine._dev uploads and the .cpu() syncs since the entry before."""

    def __init__(self):
        self.log, self.dev, self.cpu = [], 0, 0

    def add(self, f, rows, t=None, none=(), kw=(), **extra):
        e = dict(f=f, rows=int(rows))
        if t is not None:
            e["t"] = _val(t)
        for k, v in (("none", list(none)), ("kw", sorted(kw)), ("dev", self.dev), ("cpu", self.cpu)):
            if v:
                e[k] = v
        e.update({k: _val(v) for k, v in extra.items() if v is not None})
        self.dev = self.cpu = 0
        self.log.append(e)


REC = Rec()


def _val(v):
    """A JSON value for what a trace entry holds."""
    if torch.is_tensor(v):
        return v.tolist()
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.integer, np.bool_)):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    if isinstance(v, (list, tuple)):
        return [_val(x) for x in v]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return type(v).__name__


def _rows_of(seqs, salt=0):
    """fp32 [len(seqs), V]: a pseudo-random function of every value of each sequence; the last layer's rows (salt 0) favour EOS at
    about every third position, so that rows finish at different steps."""
    out = []
    for seq in seqs:
        h = len(seq) + 31 * salt
        for v in seq:
            h = (h * 1000003 + int(v) + 7) % (1 << 61)
        x = 2 * np.random.default_rng(h).standard_normal(V).astype(np.float32)
        if salt == 0 and h % 3 == 0:
            x[EOS] += 50
        out.append(x)
    return torch.from_numpy(np.stack(out))


class RecEngine:
    """Stands in for LlavaEngine on the CPU and records what generation asks of it.  The "KV cache" holds each row's spliced positions
    as values (an image token becomes IMG_ROWS values derived from the image) and a row's logits depend on every one of them.  Every
    method takes *args / **kw so that the trace holds exactly the keywords that were passed."""
    vocab, device, l, lora, weights_version, shared_rows_per_tile = V, torch.device("cpu"), {"layers": 4}, False, 0, 16

    def _dev(self, a):
        REC.dev += 1
        return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a

    def _seqs(self, ids, am, images):
        ids, imgs, k, out = np.asarray(ids), list(images) if images is not None else [], 0, []
        for b in range(ids.shape[0]):
            seq = []
            for v in (ids[b] if am is None else ids[b][np.asarray(am).reshape(ids.shape)[b].astype(bool)]):
                if v == IMAGE_TOKEN_INDEX:
                    base = int(float(imgs[k].float().sum()) * 1000) % 997
                    seq += [1000 + base + j for j in range(IMG_ROWS)]
                    k += 1
                else:
                    seq.append(int(v))
            out.append(seq)
        assert k == len(imgs)
        return out

    def plan(self, ids, am, labels, images, sizes):
        ids = np.asarray(ids)
        REC.add("plan", ids.shape[0], none=[n for n, v in (("am", am), ("sizes", sizes)) if v is None], n_images=len(images))
        rows, k = [], 0
        for b in range(ids.shape[0]):
            idx = []
            for v in (ids[b] if am is None else ids[b][np.asarray(am).reshape(ids.shape)[b].astype(bool)]):
                if v == IMAGE_TOKEN_INDEX:
                    idx += [-(2 + k * IMG_ROWS + j) for j in range(IMG_ROWS)]
                    k += 1
                else:
                    idx.append(int(v))
            rows.append(idx)
        S, nfr = max(len(r) for r in rows), k * IMG_ROWS
        idx, m = np.zeros((len(rows), S), dtype=np.int64), np.zeros((len(rows), S), dtype=bool)
        for b, r in enumerate(rows):
            idx[b, :len(r)], m[b, :len(r)] = r, True
        return dict(lens=np.array([len(r) for r in rows]), S=S, idx=idx, attention_mask=m, n_feat_rows=nfr,
                    image_rows=[(i * IMG_ROWS, (i + 1) * IMG_ROWS, nfr, nfr) for i in range(k)])

    def kv_cache_bytes(self, B, L, *a):
        REC.add("kv_cache_bytes", B, L, extra=list(a))
        return B * L * 8

    def free_device_bytes(self):
        return 1 << 40

    def new_kv_cache(self, B, L, *a):
        REC.add("new_kv_cache", B, L, extra=list(a))
        return KVCache([np.full((B, L), -7, dtype=np.int64)], np.zeros(B, np.int64), L)

    def _outputs(self, cache, seqs, kw):
        out = [_rows_of(seqs)]
        if "tap_layers" in kw:
            out.append(torch.stack([_rows_of(seqs, 1 + c) for c in kw["tap_layers"]]))
        if "attn_layers" in kw:
            L = max(len(s) for s in seqs)
            out.append(tuple(torch.full((len(seqs), L) if kw.get("attn_mean") else (len(seqs), 2, L), float(c)) for c in kw["attn_layers"]))
        return out

    def _fill(self, name, args, kw, cache, slots):
        ids, am, images = np.asarray(args[0]), args[1], args[2]
        seqs = self._seqs(ids, am, images)
        REC.add(name, ids.shape[0], [len(s) for s in seqs], none=[n for n, v in zip(("am", "images", "sizes"), args[1:]) if v is None],
                kw=kw, shape=ids.shape, n_images=None if images is None else len(images),
                **{k: v for k, v in kw.items() if k not in ("cache", "plan")})
        if cache is None or (slots is None and cache.L_max < max(len(s) for s in seqs) + kw.get("max_new_tokens", 0)):
            cache = KVCache([np.full((ids.shape[0], max(len(s) for s in seqs) + kw.get("max_new_tokens", 0)), -7, dtype=np.int64)],
                            np.zeros(ids.shape[0], np.int64), max(len(s) for s in seqs) + kw.get("max_new_tokens", 0))
        for s, seq in zip(range(ids.shape[0]) if slots is None else slots, seqs):
            if "compress" in kw:
                seq = seq[-kw["compress"][0]:]
            assert len(seq) <= cache.L_max
            cache.layers[0][s, :len(seq)] = seq
            cache.lens[s] = len(seq)
        return cache, seqs

    def prefill(self, *args, **kw):
        assert len(args) == 4
        cache, seqs = self._fill("prefill", args, kw, kw.get("cache"), kw.get("slots"))
        return (cache, *self._outputs(cache, seqs, kw))

    def extend(self, *args, **kw):
        assert len(args) == 5
        cache, seqs = self._fill("extend" if args[0] is not None else "extend(None)", args[1:], kw, args[0], kw.get("slots"))
        return (cache, *self._outputs(cache, seqs, kw))

    def decode_step(self, *args, **kw):
        cache, tokens = args
        tok = (tokens.numpy() if torch.is_tensor(tokens) else np.asarray(tokens)).reshape(-1)
        REC.add("decode_step", tok.shape[0], cache.lens, kw=kw, feed=type(tokens).__name__, dtype=str(tokens.dtype).replace("torch.", ""),
                tok=tok, **{k: v for k, v in kw.items() if k != "shared"})
        assert tok.shape[0] == cache.B and (cache.lens < cache.L_max).all()
        seqs = []
        for b in range(cache.B):
            cache.layers[0][b, cache.lens[b]] = tok[b]
            seqs.append(cache.layers[0][b, :cache.lens[b] + 1])
        cache.lens += 1
        out = self._outputs(cache, seqs, kw)
        return out[0] if len(out) == 1 else tuple(out)

    def verify_step(self, *args, **kw):
        cache, tokens = args
        tok = np.asarray(tokens).reshape(-1)
        n0, R = int(cache.lens[0]), tok.shape[0]
        REC.add("verify_step", R, cache.lens, kw=kw, tok=tok)
        assert 2 <= R <= 32 and n0 + R <= cache.L_max and ((tok >= 0) & (tok < V)).all()
        cache.layers[0][0, n0:n0 + R] = tok
        return _rows_of([cache.layers[0][0, :n0 + i + 1] for i in range(R)])

    def shared_plan(self, c0, tile):
        REC.add("shared_plan", len(c0), c0, tile=tile)
        return (c0.copy(), tile.copy())


# ------------------------------------------------------------------------------------------------ recording stand-ins for ops
_LISTS = ("ban", "ban_always", "ban_begin", "ban_eos", "bad_tok", "bad_off", "seed", "slot", "min_new")
OPS = {}


def _op(params, tensors=()):
    """Registers fn as the stand-in of ops.<fn's name>.  params: the positional names of the real entry point; tensors: its optional
    tensor arguments, recorded when None.  The int lists a call carries (bans, seeds, slots) are recorded by value."""
    def deco(fn):
        def wrapped(*args, **kw):
            b = dict(zip(params, args), **kw)
            REC.add(fn.__name__, args[0].shape[0] if torch.is_tensor(args[0]) else args[0], b.get("t"), [p for p in tensors if b.get(p) is None], kw,
                    **{p: b[p] for p in _LISTS if torch.is_tensor(b.get(p))},
                    **{p: b[p] for p in ("rep_penalty", "ngram", "write_scores", "g") if p in b})
            return fn(**b)
        OPS[fn.__name__] = wrapped
        return wrapped
    return deco


def _ints(v):
    return [] if v is None else [int(i) for i in v]


def _words(bad_tok, bad_off):
    return [] if bad_tok is None else [_ints(bad_tok[int(a):int(b)]) for a, b in zip(bad_off[:-1], bad_off[1:])]


@_op(("x", "n", "out"))
def argmax_rows(x, n, out=None):
    return x[:, :n].argmax(1)


@_op(("x", "n", "hist", "t", "rep_penalty", "ngram", "ban", "bad_tok", "bad_off", "out"), ("hist", "ban", "bad_tok", "bad_off"))
def logits_process_argmax(x, n, hist, t, rep_penalty=1.0, ngram=0, ban=None, bad_tok=None, bad_off=None, out=None):
    for r in range(x.shape[0]):
        h = [] if hist is None else _ints(hist[r, :t])
        x[r, :n] = torch.from_numpy(process_row(x[r, :n].numpy(), h, penalty=rep_penalty, ngram=ngram, bad_words=_words(bad_tok, bad_off),
                                                suppress=_ints(ban)))
    return x[:, :n].argmax(1)


@_op(("x", "n", "hist", "slot", "t", "min_new", "rep_penalty", "ngram", "ban_always", "ban_begin", "ban_eos", "bad_tok", "bad_off", "out",
      "logprob"), ("hist", "ban_always", "ban_begin", "ban_eos", "bad_tok", "bad_off", "logprob"))
def logits_process_argmax_rows(x, n, hist, slot, t, min_new, rep_penalty=1.0, ngram=0, ban_always=None, ban_begin=None, ban_eos=None,
                               bad_tok=None, bad_off=None, out=None, logprob=None):
    for r in range(x.shape[0]):
        h = [] if hist is None else _ints(hist[int(slot[r]), :int(t[r])])
        x[r, :n] = torch.from_numpy(process_row(x[r, :n].numpy(), h, penalty=rep_penalty, ngram=ngram, bad_words=_words(bad_tok, bad_off),
                                                eos=_ints(ban_eos), min_new=int(min_new[r]), suppress=_ints(ban_always),
                                                begin_suppress=_ints(ban_begin)))
    tok = x[:, :n].argmax(1)
    if logprob is not None:
        logprob.copy_(torch.log_softmax(x[:, :n].double(), -1).gather(1, tok[:, None])[:, 0].float())
    return tok


@_op(("rows", "device"))
def sample_rows_workspace(rows, device):
    return None


@_op(("x", "n", "seed", "t", "temperature", "top_k", "top_p", "min_p", "write_scores", "out", "logprob", "ws"), ("logprob", "ws"))
def sample_rows(x, n, seed, t, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, write_scores=False, out=None, logprob=None, ws=None):
    toks = []
    for r in range(x.shape[0]):
        s = x[r, :n].double() / temperature
        if 0 < top_k < n:
            s = torch.where(s < s.topk(top_k).values[-1], torch.full_like(s, -float("inf")), s)
        if torch.isnan(s).any() or not torch.isfinite(s).any():
            toks.append(-1)
            continue
        p = torch.softmax(s, -1).numpy()
        k = min(int(np.searchsorted(np.cumsum(p), sample_uniform(int(seed[r]), int(t[r])), side="right")), n - 1)
        if write_scores:
            x[r, :n] = s.float()
        if logprob is not None:
            logprob[r] = float(np.log(max(p[k], 1e-300)))
        toks.append(k)
    return torch.tensor(toks, dtype=torch.int64)


@_op(("rows", "device"))
def cfg_guide_workspace(rows, device):
    return None


@_op(("c", "u", "n", "g", "ws", "route"), ("ws",))
def cfg_guide_rows(c, u, n, g, ws=None, route=None):
    assert c.shape[0] == u.shape[0]
    lc, lu = torch.log_softmax(c[:, :n], -1), torch.log_softmax(u[:, :n], -1)
    c[:, :n] = g * (lc - lu) + lu
    return c


@_op(("rows", "n_layers", "device"))
def dola_workspace(rows, n_layers, device):
    return None


@_op(("f", "c", "n", "ws", "want_jsd"), ("ws",))
def dola_contrast_rows(f, c, n, ws=None, want_jsd=False):
    lf, lq = torch.log_softmax(f[:, :n], -1), torch.log_softmax(c[:, :, :n], -1)
    ch = (lf[None] - lq).abs().mean(-1).argmax(0)
    f[:, :n] = lf - lq[ch, torch.arange(f.shape[0])]
    return f, ch.to(torch.int32)


@_op(("x", "n", "state", "tables", "tok", "slot"), ("tok", "slot"))
def constrain_rows(x, n, state, tables, tok=None, slot=None):
    bits, new = constrain_rows_ref(x.numpy(), n, state.numpy(), *(t.numpy() for t in tables), tok=None if tok is None else tok.numpy(),
                                   slot=None if slot is None else slot.numpy())
    x.copy_(torch.from_numpy(bits.view(np.float32)))
    state.copy_(torch.from_numpy(new))
    return x


def traced(case):
    """Run one case with the stand-ins installed; returns its JSON record."""
    global REC
    REC = Rec()
    with pytest.MonkeyPatch.context() as mp:
        for name, fn in OPS.items():
            mp.setattr(ops, name, fn)
        real_cpu = torch.Tensor.cpu

        def cpu(self, *a, **k):
            REC.cpu += 1
            return real_cpu(self, *a, **k)
        mp.setattr(torch.Tensor, "cpu", cpu)
        out = case(RecEngine())
    return dict(trace=REC.log, tail=[REC.dev, REC.cpu], out=out)


# ------------------------------------------------------------------------------------------------ the matrix: generate()
def _gen_out(out):
    if torch.is_tensor(out):
        return dict(seq=out.tolist())
    d = dict(seq=out.sequences.tolist(), n_scores=None if out.scores is None else len(out.scores),
             n_logits=None if out.logits is None else len(out.logits), pkv=type(out.past_key_values).__name__)
    if hasattr(out, "lookup_stats"):
        d["lookup_stats"] = out.lookup_stats
    if hasattr(out, "attentions"):
        d["attentions"] = [[list(a.shape) for a in step] for step in out.attentions]
        d["attention_layers"] = list(out.attention_layers)
    if hasattr(out, "dola_premature_layers"):
        d["dola"] = out.dola_premature_layers.tolist()
    return d


def gen(B, ids=None, **kw):
    def case(eng):
        cfg = parse_generate_kwargs(dict(kw), lookup=True, attentions=True)
        return _gen_out(greedy_generate(eng, PROMPTS[:B] if ids is None else ids, cfg.attention_mask, None, None, cfg))
    return case


def gen_turns(B, **kw):
    """Two turns of a conversation over one GenerationCache: the second prompt continues the first with its answer and a question."""
    def case(eng):
        gc, outs, ids = GenerationCache(), [], PROMPTS[:B]
        for turn in range(2):
            cfg = parse_generate_kwargs(dict(kw, past_key_values=gc, return_dict_in_generate=True), lookup=True, attentions=True)
            out = greedy_generate(eng, ids, None, None, None, cfg)
            outs.append(_gen_out(out))
            ids = np.concatenate([ids, out.sequences.numpy(), np.full((B, 2), 11 + turn)], 1)
        return outs
    return case


class _Drafter:
    """Proposes the plain run's next token and a wrong one after it."""

    def __init__(self, plain, P):
        self.plain, self.P = plain, P

    def propose(self, seq):
        t = len(seq) - self.P
        return np.array([self.plain[t] if t < len(self.plain) else 0, (self.plain[t + 1] + 1) % V if t + 1 < len(self.plain) else 0], dtype=np.int64)


def gen_lookup(drafted, **kw):
    def case(eng):
        kw2 = dict(kw, return_dict_in_generate=True, output_scores=True, output_logits=True)
        plain = greedy_generate(eng, PROMPTS[:1], None, None, None, parse_generate_kwargs(dict(kw2), lookup=True)).sequences[0].tolist()
        cfg = parse_generate_kwargs(dict(kw2, prompt_lookup_num_tokens=2), lookup=True)
        if drafted:
            cfg.drafter = _Drafter(plain, PROMPTS.shape[1])
        out = _gen_out(greedy_generate(eng, PROMPTS[:1], None, None, None, cfg))
        assert out["seq"] == [plain]
        return out
    return case


FULL = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)
PROCS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=2, bad_words_ids=[[5, 6], [7], [EOS, 9]], suppress_tokens=[3],
             begin_suppress_tokens=[4, 8])
SAMPLE = dict(do_sample=True, seed=11, top_k=8, temperature=0.9)
CHOICES = [[5, 6], [7], [5, 6, 8, 9]]


def _constraint(B):
    c = TokenConstraint.from_choices(CHOICES, eos=[EOS])
    return c if B == 1 else [c, None, TokenConstraint.from_choices([[7, 7, 7, 7]], eos=[EOS])]


def _never(ids, scores):
    return False


# family -> (keywords, needs an EOS id)
GEN = {
    "plain": (dict(max_new_tokens=4), False),
    "plain_full": (dict(max_new_tokens=5, **FULL), False),
    "plain_max_length": (dict(max_length=9, min_length=7, **FULL), False),
    "zero_budget": (dict(max_new_tokens=0, **FULL), False),
    "criteria": (dict(max_new_tokens=5, stopping_criteria=[lambda ids, scores: ids.shape[1] >= 4], **FULL), False),
    "procs": (dict(max_new_tokens=6, **PROCS, **FULL), True),
    "procs_no_eos_min": (dict(max_new_tokens=4, repetition_penalty=1.2), False),
    "sampling": (dict(max_new_tokens=5, **SAMPLE), False),
    "sampling_criteria": (dict(max_new_tokens=4, stopping_criteria=[_never], **SAMPLE, **FULL), False),
    "sampling_procs": (dict(max_new_tokens=6, **SAMPLE, **PROCS, **FULL), True),
    "guided": (dict(max_new_tokens=4, guidance_scale=1.5), False),
    "guided_negative": (dict(max_new_tokens=5, guidance_scale=2.0, negative_prompt_ids=[[4, 5, 6], [7, 8, 9], [1, 2, 3]],
                             negative_prompt_attention_mask=[[1, 1, 1], [0, 1, 1], [1, 1, 0]], **FULL), False),
    "guided_procs_sampling": (dict(max_new_tokens=6, guidance_scale=0.5, **SAMPLE, **PROCS, **FULL), True),
    "guided_max_length": (dict(max_length=10, guidance_scale=1.5, kv_cache_dtype="int8"), False),
    "dola": (dict(max_new_tokens=4, dola_layers=[0, 2], **FULL), False),
    "dola_high_procs": (dict(max_new_tokens=5, dola_layers="high", **PROCS, **FULL), True),
    "dola_sampling_int8": (dict(max_new_tokens=4, dola_layers=[1], kv_cache_dtype="int8", **SAMPLE), False),
    "attentions": (dict(max_new_tokens=4, output_attentions=True, return_dict_in_generate=True), False),
    "attentions_mean": (dict(max_new_tokens=5, output_attentions=True, attention_layers=[1, -1], attention_reduce="mean_heads", **FULL), False),
    "int8": (dict(max_new_tokens=4, kv_cache_dtype="int8", **FULL), False),
    "kvpress": (dict(max_new_tokens=4, prompt_kv_budget=4, prompt_kv_window=2, prompt_kv_pool=1), False),
    "kvpress_sampling": (dict(max_new_tokens=5, prompt_kv_budget=3, prompt_kv_window=1, **SAMPLE, **FULL), False),
}
CASES = {}
for _name, (_kw, _needs_eos) in GEN.items():
    for _B, _eos in ((1, None), (3, None), (3, EOS)):
        if _eos is None and _needs_eos:
            _eos = EOS
            if _B == 3:
                continue
        _kw2 = dict(_kw, eos_token_id=_eos, pad_token_id=0)
        if "negative_prompt_ids" in _kw2:
            _kw2.update(negative_prompt_ids=np.array(_kw["negative_prompt_ids"][:_B]),
                        negative_prompt_attention_mask=np.array(_kw["negative_prompt_attention_mask"][:_B]))
        CASES[f"generate/{_name}/B{_B}/eos{int(_eos is not None)}"] = gen(_B, **_kw2)
for _B in (1, 3):
    CASES[f"generate/constraint/B{_B}"] = gen(_B, max_new_tokens=6, constraint=_constraint(_B), eos_token_id=EOS, pad_token_id=0, **FULL)
    CASES[f"generate/constraint_procs/B{_B}"] = gen(_B, max_new_tokens=6, constraint=_constraint(_B), eos_token_id=EOS, pad_token_id=0,
                                                    repetition_penalty=1.3)
    CASES[f"generate/constraint_sampling/B{_B}"] = gen(_B, max_new_tokens=6, constraint=_constraint(_B), eos_token_id=EOS, pad_token_id=0,
                                                       **SAMPLE, **FULL)
    CASES[f"generate/constraint_attentions/B{_B}"] = gen(_B, max_new_tokens=5, constraint=_constraint(_B), eos_token_id=EOS, pad_token_id=0,
                                                         output_attentions=True, attention_layers=[0], return_dict_in_generate=True)
    CASES[f"generate/constraint_int8_criteria/B{_B}"] = gen(_B, max_new_tokens=5, constraint=_constraint(_B), eos_token_id=EOS, pad_token_id=0,
                                                            kv_cache_dtype="int8", stopping_criteria=[_never])
    for _eos in (None, EOS):
        CASES[f"generate/past_key_values/B{_B}/eos{int(_eos is not None)}"] = gen_turns(_B, max_new_tokens=4, eos_token_id=_eos, pad_token_id=0)
    CASES[f"generate/past_key_values_procs_sampling/B{_B}"] = gen_turns(_B, max_new_tokens=5, eos_token_id=EOS, pad_token_id=0, output_scores=True,
                                                                       **PROCS, **SAMPLE)
    CASES[f"generate/past_key_values_constraint/B{_B}"] = gen_turns(_B, max_new_tokens=6, eos_token_id=EOS, pad_token_id=0,
                                                                   constraint=_constraint(_B))
CASES["generate/masked_prompt/B3"] = gen(3, max_new_tokens=4, eos_token_id=EOS, pad_token_id=0, guidance_scale=None,
                                         attention_mask=np.array([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 1, 1, 1, 1]]))
CASES["generate/guided_masked_prompt/B3"] = gen(3, max_new_tokens=4, eos_token_id=EOS, pad_token_id=0, guidance_scale=3.0,
                                                attention_mask=np.array([[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 1, 1, 1, 0]]))
for _drafted in (False, True):
    for _eos in (None, EOS):
        _tag = f"drafter{int(_drafted)}/eos{int(_eos is not None)}"
        CASES[f"generate/lookup/{_tag}"] = gen_lookup(_drafted, max_new_tokens=6, eos_token_id=_eos, pad_token_id=0)
        CASES[f"generate/lookup_procs/{_tag}"] = gen_lookup(_drafted, max_new_tokens=6, eos_token_id=_eos, pad_token_id=0, **PROCS)
    CASES[f"generate/lookup_criteria/drafter{int(_drafted)}"] = gen_lookup(_drafted, max_new_tokens=6, eos_token_id=None,
                                                                          stopping_criteria=[lambda ids, scores: ids.shape[1] >= 4])


# ------------------------------------------------------------------------------------------------ the matrix: generate_batch()
def _img(i):
    return torch.full((3, 4, 4), float(i))


def _requests(n, share):
    """n unpadded prompts, some with an image; share: they begin with the same image and system prompt, or with the system prompt alone."""
    rng = np.random.default_rng(5)
    ps, ims = [], []
    for i in range(n):
        q = rng.integers(3, V, int(rng.integers(2, 6))).astype(np.int64)
        has = i % 3 != 1
        body = np.concatenate([SYS, q]) if share else q
        ps.append(np.concatenate([[IMAGE_TOKEN_INDEX], body]).astype(np.int64) if has else body)
        ims.append(_img(1 if share else i) if has else None)
    return ps, ims


BUDGETS = [3, 5, 4, 6, 3]


def batch(n=5, slots=2, share=False, logprobs=False, negatives=False, **kw):
    def case(eng):
        ps, ims = _requests(n, share)
        kw2 = dict(kw, max_new_tokens=BUDGETS[:n])
        if share:
            kw2["share_prefix"] = True
        if negatives:
            neg = np.array([4, IMAGE_TOKEN_INDEX, 6, 7, 8, 9, 10, 11, 12], dtype=np.int64)
            kw2.update(negative_prompt_ids=[None, [4, 5], neg, None, [6]][:n], negative_images=[None, None, _img(9), None, None][:n])
        cfg = parse_batch_kwargs(kw2, n)
        sch = BatchScheduler(eng, batch_requests(ps, ims, None, getattr(cfg, "guidance", None)), cfg, slots, return_logprobs=logprobs,
                             admit_free=1)
        out = sch.run()
        return dict(tokens=[o.generated_tokens for o in out.values()], n_logprobs=[len(o.logprobs) for o in out.values()],
                    events=_val(sch.events))
    return case


def _batch_constraint():
    c = TokenConstraint.from_choices(CHOICES, eos=[EOS])
    return [c, None, TokenConstraint.from_choices([[7, 7]], eos=[EOS]), c, None]


BATCH = {
    "plain": dict(),
    "logprobs": dict(logprobs=True),
    "procs": dict(**PROCS),
    "procs_logprobs_criteria": dict(logprobs=True, stopping_criteria=[_never], **PROCS),
    "sampling": dict(**SAMPLE),
    "sampling_procs_logprobs": dict(logprobs=True, **SAMPLE, **PROCS),
    "guided": dict(guidance_scale=1.5),
    "guided_negatives_procs_sampling": dict(guidance_scale=2.0, negatives=True, logprobs=True, **SAMPLE, **PROCS),
    "guided_int8": dict(guidance_scale=0.5, negatives=True, kv_cache_dtype="int8"),
    "dola": dict(dola_layers=[0, 2]),
    "dola_procs_logprobs": dict(dola_layers="high", logprobs=True, **PROCS),
    "constraint": dict(constraint=_batch_constraint()),
    "constraint_sampling_logprobs": dict(constraint=_batch_constraint(), logprobs=True, **SAMPLE),
    "share_prefix": dict(share=True, slots=3),
    "share_prefix_constraint_procs": dict(share=True, slots=3, constraint=_batch_constraint(), repetition_penalty=1.3),
    "int8": dict(kv_cache_dtype="int8"),
    "kvpress": dict(prompt_kv_budget=4, prompt_kv_window=2),
    "one_slot": dict(slots=1, n=3),
    "all_fit": dict(slots=8),
}
for _name, _kw in BATCH.items():
    for _eos in (None, EOS):
        if _eos is None and ("constraint" in _kw or "min_new_tokens" in _kw):
            continue
        CASES[f"generate_batch/{_name}/eos{int(_eos is not None)}"] = batch(eos_token_id=_eos, pad_token_id=0, **_kw)


# ------------------------------------------------------------------------------------------------ the test
@functools.lru_cache(None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_matrix_is_the_recorded_one():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_call_trace_is_the_recorded_one(name):
    got, want = json.loads(json.dumps(traced(CASES[name]))), _golden()[name]
    assert got["out"] == want["out"]
    for i, (a, b) in enumerate(zip(got["trace"], want["trace"])):
        assert a == b, f"{name}: entry {i} of {len(want['trace'])}"
    assert len(got["trace"]) == len(want["trace"]) and got["tail"] == want["tail"]


def test_every_family_sees_a_row_finish_early():
    """The recorded EOS variants really finish a row (a request) before the others: a pad after the EOS, or fewer tokens than the budget."""
    gold = _golden()
    for name, rec in gold.items():
        if name.startswith("generate/") and name.endswith("B3/eos1"):
            outs = rec["out"] if isinstance(rec["out"], list) else [rec["out"]]
            assert any(EOS in row[:-1] for o in outs for row in o["seq"]) or "zero_budget" in name, name
        if name.startswith("generate_batch/") and name.endswith("eos1"):
            assert any(t and t[-1] == EOS and len(t) < b for t, b in zip(rec["out"]["tokens"], BUDGETS)), name
            assert sum(e[0] == "admit" for e in rec["out"]["events"]) > 1 or "all_fit" in name, name


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_generation_trace_host.py --record   (on the commit before the refactor)")
    with open(GOLDEN, "w") as f:
        json.dump({name: traced(case) for name, case in sorted(CASES.items())}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} calls into {GOLDEN}")

"""CPU tests of DoLa's host side: candidate resolution and validation (radvlm_amd/generation.py against tests/dola_ref.py and
hand-written lists), the refusals, the reference against itself, greedy_generate's loop on a fake engine (the contrast op replaced by
the reference), and the build plumbing."""
import os

import numpy as np
import pytest
import torch

import dola_ref
from radvlm_amd import lib, ops
from radvlm_amd.engine import KVCache
from radvlm_amd.generation import (GenerationCache, greedy_generate, parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs,
                                   resolve_dola_layers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 29


# ------------------------------------------------------------------------------------------------ candidate layers
HAND = {
    (2, "low"): [0], (2, "high"): [1],
    (12, "low"): [0, 2, 4], (12, "high"): [6, 8, 10],
    (28, "low"): [0, 2, 4, 6, 8, 10, 12], (28, "high"): [14, 16, 18, 20, 22, 24, 26],
    (32, "low"): [0, 2, 4, 6, 8, 10, 12, 14], (32, "high"): [16, 18, 20, 22, 24, 26, 28, 30],
    (40, "low"): [0, 2, 4, 6, 8, 10, 12, 14, 16, 18], (40, "high"): [20, 22, 24, 26, 28, 30, 32, 34, 36, 38],
    (80, "low"): [0, 2, 4, 6, 8, 10, 12, 14, 16, 18], (80, "high"): [60, 62, 64, 66, 68, 70, 72, 74, 76, 78],
}


@pytest.mark.parametrize("L,spec", sorted(HAND))
def test_buckets_against_hand_written_lists(L, spec):
    cfg = parse_generate_kwargs(dict(dola_layers=spec))
    assert cfg.dola == spec
    assert list(resolve_dola_layers(cfg.dola, L)) == HAND[(L, spec)] == dola_ref.candidate_layers(spec, L)


def test_bucket_sizes_of_the_shipped_geometries():
    assert len(resolve_dola_layers("high", 32)) == 8 and len(resolve_dola_layers("high", 28)) == 7 and len(resolve_dola_layers("high", 40)) == 10


def test_tied_embeddings_follow_hf():
    assert list(resolve_dola_layers("low", 12, tied=True)) == [2, 4] == dola_ref.candidate_layers("low", 12, tied=True)
    assert list(resolve_dola_layers("low", 80, tied=True)) == list(range(2, 20, 2))
    assert list(resolve_dola_layers("high", 2, tied=True)) == [1]
    with pytest.raises(ValueError):
        resolve_dola_layers("low", 2, tied=True)                       # range(1, 1): empty


def test_lists_keep_their_order():
    cfg = parse_generate_kwargs(dict(dola_layers=[5, 1, 3]))
    assert cfg.dola == (5, 1, 3) and resolve_dola_layers(cfg.dola, 6) == (5, 1, 3)
    assert parse_generate_kwargs(dict(dola_layers=(0,))).dola == (0,)
    assert parse_generate_kwargs(dict(dola_layers=[np.int64(2)])).dola == (2,)


@pytest.mark.parametrize("bad", [[], (), "middle", "", [1, 1], [0, 2, 0], [1.0], ["1"], [True], [None], True, 3, 1.5, {"low"}, [-1],
                                 list(range(17))])
def test_value_errors_at_parse_time(bad):
    with pytest.raises(ValueError):
        parse_generate_kwargs(dict(dola_layers=bad))
    with pytest.raises(ValueError):
        parse_batch_kwargs(dict(dola_layers=bad), 2)
    with pytest.raises(ValueError):
        dola_ref.candidate_layers(bad, 64)


@pytest.mark.parametrize("spec,L", [([4], 4), ([0, 7], 7), ([32], 32), ("low", 1), ("low", 0), ("high", 0), ([0, 1, -1], 4)])
def test_value_errors_once_the_depth_is_known(spec, L):
    with pytest.raises(ValueError):
        resolve_dola_layers(spec if isinstance(spec, str) else tuple(spec), L)
    with pytest.raises(ValueError):
        dola_ref.candidate_layers(spec, L)


def test_sixteen_candidates_is_the_limit():
    assert resolve_dola_layers(tuple(range(16)), 16) == tuple(range(16))
    assert ops.DOLA_MAX_LAYERS == 16 == dola_ref.MAX_LAYERS
    with pytest.raises(ValueError):
        resolve_dola_layers(tuple(range(17)), 40)


def test_off_is_off():
    assert parse_generate_kwargs({}).dola is None and parse_generate_kwargs(dict(dola_layers=None)).dola is None
    assert parse_batch_kwargs(dict(dola_layers=None), 3).dola is None
    parse_beam_kwargs(dict(dola_layers=None, num_beams=2))


def test_refusals():
    for extra in (dict(guidance_scale=1.5), dict(past_key_values=GenerationCache())):
        with pytest.raises(NotImplementedError, match="dola_layers"):
            parse_generate_kwargs(dict(dola_layers="high", **extra))
    with pytest.raises(NotImplementedError, match="dola_layers"):
        parse_generate_kwargs(dict(dola_layers=[0], prompt_lookup_num_tokens=3), lookup=True)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        parse_batch_kwargs(dict(dola_layers="low", share_prefix=True), 2)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        parse_batch_kwargs(dict(dola_layers="low", guidance_scale=2.0), 2)
    with pytest.raises(NotImplementedError, match="dola_layers"):
        parse_beam_kwargs(dict(dola_layers="high", num_beams=2))
    with pytest.raises(NotImplementedError, match="LoRA"):             # the existing refusal stays what it was
        parse_generate_kwargs(dict(dola_layers="high"), lora=True)
    assert parse_batch_kwargs(dict(dola_layers="low", share_prefix=False, kv_cache_dtype="int8", do_sample=True, seed=3), 2).dola == "low"


# ------------------------------------------------------------------------------------------------ the reference against itself
def _rows(seed, n, V=V, B=3):
    g = torch.Generator().manual_seed(seed)
    f = 4 * torch.randn(B, V, generator=g)
    c = torch.stack([f + 0.25 * 2 ** (k / 2) * torch.randn(B, V, generator=g) for k in range(n)])
    return torch.log_softmax(f, -1), torch.log_softmax(c, -1)


def test_single_candidate_skips_the_divergence():
    lf, lq = _rows(0, 1)
    out, ch, J = dola_ref.dola_rows(lf, lq)
    assert J is None and ch.tolist() == [0, 0, 0]
    assert torch.equal(out, dola_ref.contrast(lf, lq[0]))


def test_exact_tie_goes_to_the_lower_index():
    lf, lq = _rows(1, 3)
    lq = torch.stack([lq[0], lq[2], lq[2], lq[1]])                      # 1 and 2 are the same row
    J = torch.stack([dola_ref.jsd64(lf, lq[k]) for k in range(4)], 1).numpy()
    assert np.array_equal(J[:, 1], J[:, 2])
    _, ch, _ = dola_ref.dola_rows(lf, lq)
    assert (ch != 2).all()
    assert dola_ref.select(np.array([[0.1, 0.3, 0.3], [0.2, 0.2, 0.1]])).tolist() == [1, 0]


def test_filter_keeps_the_maximum_and_thresh_is_fp32():
    lf, lq = _rows(2, 2, V=257)
    out, ch, _ = dola_ref.dola_rows(lf, lq)
    am = lf.argmax(-1)
    assert torch.isfinite(out[torch.arange(3), am]).all()
    thresh = (lf.max(-1).values + torch.tensor(dola_ref.LOG_RT)).float()
    assert dola_ref.LOG_RT.dtype == np.float32 and float(dola_ref.LOG_RT) == float(np.float32(np.log(0.1)))
    kept = torch.isfinite(out)
    assert torch.equal(kept, lf >= thresh[:, None]) and 0 < int(kept.sum()) < kept.numel()
    # an entry exactly at the fp32 threshold is kept, one ulp below it is not
    row = torch.full((1, 8), -30.0)
    row[0, 0] = 0.0
    t = torch.tensor(0.0) + torch.tensor(dola_ref.LOG_RT)
    row[0, 1], row[0, 2] = t, torch.nextafter(t, torch.tensor(-float("inf")))
    o = dola_ref.contrast(row, torch.zeros(1, 8))
    assert torch.isfinite(o[0, :2]).all() and o[0, 2] == -float("inf")


def test_equal_rows_give_zero():
    lf, _ = _rows(3, 1)
    lq = torch.stack([lf, lf])
    out, ch, J = dola_ref.dola_rows(lf, lq)
    # log(exp(l)) is l up to float64 rounding: J is 0 to 2^-52 and both candidates give the same bits, so the tie rule decides
    assert (np.abs(J) <= 2.0 ** -52).all() and np.array_equal(J[:, 0], J[:, 1]) and ch.tolist() == [0, 0, 0]
    assert (out[torch.isfinite(out)] == 0).all() and torch.isfinite(out).any(-1).all()
    assert (dola_ref.jsd_error_bound(lf, lf) > 0).all()                 # the inputs' own rounding still moves J


def test_jsd_is_the_textbook_divergence():
    lf, lq = _rows(4, 1, V=64)
    p, q = lf[0].double().exp(), lq[0, 0].double().exp()
    m = 0.5 * (p + q)
    kl = lambda a, b: float((a * (a / b).log()).sum())
    want = 0.5 * (kl(p, m) + kl(q, m)) / 64                            # HF's kl_div(reduction="none").mean(-1): the sum over V, / V
    # J = 0.5 (mean M (log M - lf) + mean M (log M - lq)) is HF's expression (kl_div(input, target) = target (log target - input))
    hf = 0.5 * (float((m * (m.log() - lf[0].double())).mean()) + float((m * (m.log() - lq[0, 0].double())).mean()))
    got = float(dola_ref.jsd64(lf[0], lq[0, 0]))
    assert abs(got - hf) <= 1e-15
    assert want != got                                                   # and HF's is NOT the textbook JSD: its KL terms are reversed
    b = float(dola_ref.jsd_error_bound(lf[0], lq[0, 0]))
    assert 0 < b < 1e-3 * abs(got)                                       # the bound is small beside J


# ------------------------------------------------------------------------------------------------ greedy_generate on a fake engine
class FakeEngine:
    """Stands in for LlavaEngine on the CPU: 4 "layers"; the logits of the last layer and of every tapped layer are pseudo-random
    functions of the fed tokens, the tapped ones near the last layer's."""
    vocab = V
    device = torch.device("cpu")
    l = {"layers": 4}

    def __init__(self):
        self.calls = []

    def _rows(self, seqs, taps):
        f, c = [], []
        for seq in seqs:
            h = len(seq)
            for v in seq:
                h = (h * 1000003 + int(v) + 7) % (1 << 61)
            rng = np.random.default_rng(h)
            row = 4 * rng.standard_normal(V).astype(np.float32)
            noise = rng.standard_normal((4, V)).astype(np.float32)
            f.append(row)
            c.append([row + np.float32(0.3 * (k + 1)) * noise[k] for k in taps])
        return torch.from_numpy(np.stack(f)), torch.from_numpy(np.array(c)).transpose(0, 1).contiguous()

    def prefill(self, ids, am, images, sizes, max_new_tokens=0, tap_layers=None):
        ids = np.asarray(ids)
        self.calls.append(("prefill", tap_layers))
        L = ids.shape[1] + max_new_tokens
        cache = KVCache([np.full((ids.shape[0], L), -7, dtype=np.int64)], np.full(ids.shape[0], ids.shape[1], dtype=np.int64), L)
        cache.layers[0][:, :ids.shape[1]] = ids
        f, c = self._rows([r[:ids.shape[1]] for r in cache.layers[0]], tap_layers or ())
        return (cache, f) if tap_layers is None else (cache, f, c)

    def decode_step(self, cache, tokens, tap_layers=None):
        tokens = np.asarray(tokens).reshape(-1)
        self.calls.append(("decode", tap_layers))
        n = int(cache.lens[0])
        cache.layers[0][:, n] = tokens
        cache.lens += 1
        f, c = self._rows([r[:n + 1] for r in cache.layers[0]], tap_layers or ())
        return f if tap_layers is None else (f, c)


def _host_contrast(f, c, n, ws=None, want_jsd=False):
    lf = torch.log_softmax(f[:, :n], -1)
    lqs = torch.log_softmax(c[:, :, :n], -1)
    out, ch, _ = dola_ref.dola_rows(lf, lqs)
    f[:, :n] = out
    return f, torch.from_numpy(ch.astype(np.int32))


@pytest.fixture(autouse=True)
def host_ops(monkeypatch):
    monkeypatch.setattr(ops, "argmax_rows", lambda x, n, out=None: x[:, :n].argmax(1))
    monkeypatch.setattr(ops, "dola_contrast_rows", _host_contrast)
    monkeypatch.setattr(ops, "dola_workspace", lambda rows, n_layers, device: None)


PROMPTS = np.array([[3, 1, 4, 1, 5], [9, 2, 6, 5, 3], [5, 8, 9, 7, 9]])


def _run(eng=None, **kw):
    eng = eng or FakeEngine()
    cfg = parse_generate_kwargs(dict(kw, return_dict_in_generate=True, output_scores=True, output_logits=True))
    return greedy_generate(eng, PROMPTS, None, None, None, cfg), eng


def test_loop_matches_the_reference_loop():
    T = 9
    out, eng = _run(dola_layers=[3, 0, 2], max_new_tokens=T, eos_token_id=None)
    ref = dola_ref.dola_generate_ref(FakeEngine(), PROMPTS, [3, 0, 2], T)
    assert np.array_equal(out.sequences.numpy(), ref["sequences"]) and out.sequences.shape == (3, T)
    assert all(torch.equal(a, b) for a, b in zip(out.logits, ref["logits"])) and len(out.logits) == T          # the raw mature rows
    assert all(torch.equal(a, b) for a, b in zip(out.scores, ref["scores"])) and len(out.scores) == T          # the contrasted rows
    lay = out.dola_premature_layers
    assert lay.dtype == torch.int64 and tuple(lay.shape) == (3, T) and np.array_equal(lay.numpy(), ref["layers"])
    assert set(lay.numpy().ravel().tolist()) <= {3, 0, 2} and len(set(lay.numpy().ravel().tolist())) > 1
    assert eng.calls == [("prefill", (3, 0, 2))] + [("decode", (3, 0, 2))] * (T - 1)
    plain, _ = _run(max_new_tokens=T, eos_token_id=None)
    assert not hasattr(plain, "dola_premature_layers")
    assert all(torch.equal(a, b) for a, b in zip(out.logits[:1], plain.logits[:1]))       # the same raw rows at the first step
    assert not torch.equal(out.scores[0], plain.scores[0])


def test_minus_one_after_eos_and_pad_tokens():
    T = 9
    free, _ = _run(dola_layers="high", max_new_tokens=T, eos_token_id=None)              # 4 layers: "high" is [2]
    eos = int(free.sequences[1, 2])
    out, eng = _run(dola_layers="high", max_new_tokens=T, eos_token_id=eos, pad_token_id=0)
    ref = dola_ref.dola_generate_ref(FakeEngine(), PROMPTS, [2], T, eos=[eos], pad=0)
    assert np.array_equal(out.sequences.numpy(), ref["sequences"])
    lay = out.dola_premature_layers.numpy()
    assert np.array_equal(lay, ref["layers"]) and lay.shape == out.sequences.shape
    seq = out.sequences.numpy()
    for b in range(3):
        hit = np.flatnonzero(seq[b] == eos)
        end = int(hit[0]) + 1 if hit.size else seq.shape[1]
        assert (lay[b, :end] == 2).all() and (lay[b, end:] == -1).all() and (seq[b, end:] == 0).all()
    assert (lay[1, 3:] == -1).all() and lay[1, 2] == 2
    assert eng.calls[0] == ("prefill", (2,))


def test_processors_see_the_contrasted_row(monkeypatch):
    seen = []

    def fake_process(logits, n, hist, t, penalty, ngram, *args):
        seen.append(logits.clone())
        logits[:, 7] = -float("inf")                                    # what a processor does: in place, before output_scores
        return logits[:, :n].argmax(1)

    monkeypatch.setattr(ops, "logits_process_argmax", fake_process)
    T = 5
    out, _ = _run(dola_layers=[1, 2], max_new_tokens=T, eos_token_id=None, suppress_tokens=[7])
    ref = dola_ref.dola_generate_ref(FakeEngine(), PROMPTS, [1, 2], T, process=lambda row, hist: np.where(np.arange(V) == 7, -np.inf, row)
                                     .astype(np.float32))
    assert len(seen) == T and np.array_equal(out.sequences.numpy(), ref["sequences"])
    for t in range(T):
        contrasted = ref["scores"][t].clone()
        assert torch.equal(out.scores[t], contrasted)                   # processed contrasted rows
        assert torch.equal(out.logits[t], ref["logits"][t])             # raw mature rows
        lf = torch.log_softmax(ref["logits"][t], -1)
        assert torch.equal(torch.isfinite(seen[t]), lf >= lf.max(-1, keepdim=True).values + torch.tensor(dola_ref.LOG_RT))


def test_stopping_criterion_gets_the_contrasted_scores():
    got = []

    def crit(ids, scores):
        got.append(scores.clone())
        return ids.shape[1] >= 3

    out, _ = _run(dola_layers=[0, 1], max_new_tokens=8, eos_token_id=None, stopping_criteria=[crit])
    assert out.sequences.shape[1] == 3 and len(got) == 3
    assert all(torch.equal(a, b) for a, b in zip(got, out.scores))
    assert tuple(out.dola_premature_layers.shape) == (3, 3)


def test_a_layer_outside_the_decoder_raises_when_the_call_starts():
    with pytest.raises(ValueError):
        _run(dola_layers=[0, 4], max_new_tokens=3)


def test_off_runs_todays_calls():
    _, eng = _run(max_new_tokens=4, eos_token_id=None, dola_layers=None)
    assert eng.calls == [("prefill", None)] + [("decode", None)] * 3


# ------------------------------------------------------------------------------------------------ build plumbing
def test_header_and_bindings_agree():
    assert len(lib.SIGNATURES["rv_dola_contrast_rows_f32"][1]) == 14
    assert len(lib.SIGNATURES["rv_dola_ws_bytes"][1]) == 2
    assert callable(ops.dola_contrast_rows) and callable(ops.dola_workspace)
    assert ops.DOLA_LOG_RT == float(dola_ref.LOG_RT)


def test_build_lists_the_source_under_the_scratch_gate():
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "dola" in build.split('SRCS="')[1].split('"')[0].split()
    assert 'grep -h -B8 "ScratchSize \\[bytes/lane\\]: [1-9]" $(printf "$OBJ/%s.res " $SRCS) | grep "Function Name"' in build
    src = open(os.path.join(ROOT, "radvlm_amd", "csrc", "dola.hip")).read()
    assert '#include "log_softmax.h"' in src and "ls_row_max(" in src and "ls_block_logsum(" in src      # the statistics are shared, not restated

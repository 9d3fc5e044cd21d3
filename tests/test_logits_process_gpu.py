"""GPU tests of the greedy logits processors: rv_logits_process_argmax_f32 against the numpy restatement (tests/logits_ref.py), and
generate() with repetition_penalty / no_repeat_ngram_size / min_new_tokens / bad_words_ids / begin_suppress_tokens end to end."""
import numpy as np
import pytest
import torch

from logits_ref import argmax, has_repeated_ngram, process_row, same_values
from test_generate_gpu import LOGITS_FP32_TOL, _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu

SETTINGS = {
    "penalty_up": dict(repetition_penalty=1.2),
    "penalty_down": dict(repetition_penalty=0.8),
    "ngram1": dict(no_repeat_ngram_size=1),
    "ngram2": dict(no_repeat_ngram_size=2),
    "ngram3": dict(no_repeat_ngram_size=3),
    "bad_words": dict(bad_words_ids=[[4], [1, 2], [3, 1, 2], [7, 7], [5, 6, 7, 8]]),
    "min_new": dict(min_new_tokens=50, eos_token_id=[2, 9]),
    "suppress": dict(suppress_tokens=[0, 3, 11, 10 ** 7]),
    "begin_suppress": dict(begin_suppress_tokens=[1, 6]),
    "all": dict(repetition_penalty=1.3, no_repeat_ngram_size=3, bad_words_ids=[[4], [1, 2], [3, 1, 2]], min_new_tokens=50,
                eos_token_id=[2, 9], suppress_tokens=[0, 11], begin_suppress_tokens=[1, 6]),
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ref_kwargs(cfg, lp):
    return dict(penalty=cfg.repetition_penalty, ngram=cfg.no_repeat_ngram_size, bad_words=cfg.bad_words_ids, eos=cfg.eos,
                min_new=lp.min_new, suppress=cfg.suppress_tokens, begin_suppress=cfg.begin_suppress_tokens)


def _rows(rng, B, n, pad_cols=8):
    full = (rng.standard_normal((B, n + pad_cols)) * 5).astype(np.float32)
    full[:, rng.integers(0, n, 16)] = -np.inf
    full[:, 1] = full[:, 5] = full.max() + 2                        # ties at the top (lowest index wins)
    return full


def _hist(rng, B, t, n, pad=2):
    h = rng.integers(0, 12, (B, t))                                 # small ids: duplicates and repeated n-grams
    if t > 8:
        h[:, rng.integers(0, t, 4)] = rng.integers(0, n, 4)           # a few ids from the whole vocabulary
        h[:, t - 3:t - 1] = h[:, 2:4]                                # a guaranteed 3-gram prefix match
        h[B - 1, t - 4:] = pad                                       # a finished row's pads
    return h.astype(np.int32)


def _run(x_full, n, h, t, cfg):
    from radvlm_amd import ops
    from radvlm_amd.generation import LogitsProcessors
    lp = LogitsProcessors(cfg, n)
    xd = torch.from_numpy(x_full).cuda()
    view = xd[:, :n]                                                 # strided rows: the [:, :vocab] view of a padded lm_head output
    hd = torch.from_numpy(np.ascontiguousarray(h)).cuda() if t > 0 else None
    tok = ops.logits_process_argmax(view, n, hd, t, lp.penalty, lp.ngram, *lp.device_args(t, xd.device))
    torch.cuda.synchronize()
    return xd.cpu().numpy(), tok.cpu().numpy(), lp


@pytest.mark.parametrize("n,B", [(1000, 1), (1000, 7), (32000, 7), (32000, 32), (152064, 1), (152064, 32)])
@pytest.mark.parametrize("name", list(SETTINGS))
def test_kernel_matches_restatement(n, B, name):
    _need_gpu()
    from radvlm_amd.generation import parse_generate_kwargs
    cfg = parse_generate_kwargs(SETTINGS[name])
    rng = np.random.default_rng(n + B)
    for t in (0, 1, 3, 40, 300):
        x = _rows(rng, B, n)
        h = _hist(rng, B, t, n)
        got, tok, lp = _run(x, n, h, t, cfg)
        assert np.array_equal(got[:, n:], x[:, n:], equal_nan=True)  # columns >= n are never touched
        for b in range(B):
            want = process_row(x[b, :n], h[b], **_ref_kwargs(cfg, lp))
            assert same_values(got[b, :n], want), (name, t, b, np.flatnonzero(~((got[b, :n] == want) | np.isnan(want)))[:8])
            assert int(tok[b]) == argmax(want), (name, t, b)


def test_ban_everything_and_nan_rows():
    _need_gpu()
    from radvlm_amd.generation import parse_generate_kwargs
    n, B, t = 32000, 3, 20
    rng = np.random.default_rng(3)
    x = _rows(rng, B, n)
    x[1, 777] = np.nan
    x[2, 100] = x[2, 50] = np.nan
    h = _hist(rng, B, t, n)
    got, tok, lp = _run(x, n, h, t, parse_generate_kwargs(dict(repetition_penalty=1.5, suppress_tokens=list(range(n)))))
    assert np.all(got[:, :n] == -np.inf) and tok.tolist() == [0, 0, 0]       # every id banned: argmax of an all -inf row is 0
    got, tok, lp = _run(x, n, h, t, parse_generate_kwargs(dict(repetition_penalty=1.5, no_repeat_ngram_size=2)))
    for b in range(B):
        want = process_row(x[b, :n], h[b], penalty=1.5, ngram=2)
        assert same_values(got[b, :n], want) and int(tok[b]) == argmax(want)
    assert tok[1] == 777 and tok[2] == 50


def test_row_result_independent_of_batch_neighbours():
    _need_gpu()
    from radvlm_amd.generation import parse_generate_kwargs
    cfg = parse_generate_kwargs(SETTINGS["all"])
    n, t = 152064, 64
    rng = np.random.default_rng(11)
    x = _rows(rng, 32, n)
    h = _hist(rng, 32, t, n)
    alone, tok1, _ = _run(x[3:4].copy(), n, h[3:4], t, cfg)
    for seed in (1, 2):
        r = np.random.default_rng(seed)
        x2, h2 = _rows(r, 32, n), _hist(r, 32, t, n)
        x2[3], h2[3] = x[3], h[3]
        got, tok, _ = _run(x2, n, h2, t, cfg)
        assert np.array_equal(got[3], alone[0], equal_nan=True) and tok[3] == tok1[0]


def test_entry_rejects_out_of_bound_vocabulary():
    _need_gpu()
    from radvlm_amd import lib, ops
    x = torch.zeros(1, ops.LOGITS_PROCESS_MAX_N + 64, device="cuda")
    out = torch.empty(1, dtype=torch.int64, device="cuda")
    with pytest.raises(lib.RadvlmHipError):
        lib.call("rv_logits_process_argmax_f32", x, x.stride(0), 1, ops.LOGITS_PROCESS_MAX_N + 1, None, 0, 0, 1.0, 0, None, 0, None, None, 0, out)
    ops.logits_process_argmax(x, ops.LOGITS_PROCESS_MAX_N, None, 0, 1.0, 0, torch.tensor([5], dtype=torch.int32, device="cuda"), out=out)
    assert int(out[0]) == 0 and float(x[0, 5]) == -np.inf


def test_torch_scalar_division_on_gpu_recorded():
    """HF run on a GPU divides by a scalar through its reciprocal; the CPU processors (the pin) divide.  Recorded, not asserted."""
    _need_gpu()
    from conftest import record_measurement
    x = torch.from_numpy((np.random.default_rng(0).standard_normal(1 << 20) * 10).astype(np.float32))
    diff = int(((x.cuda() / 1.2).cpu() != x / 1.2).sum())
    record_measurement("torch_gpu_scalar_div", p=1.2, n=x.numel(), entries_differing_from_cpu=diff)


# ------------------------------------------------------------------------------------------------ generate() end to end
def _gen(model, g, images, sizes, b=0, **kw):
    prompt = torch.from_numpy(_prompt(g, b)[None])
    return model.generate(prompt, images=[images[b]], image_sizes=[sizes[b]], **kw)


def _repeating_budget(model, g, images, sizes, n):
    for T in (32, 64, 128, 256):
        free = _gen(model, g, images, sizes, max_new_tokens=T, eos_token_id=None)[0].cpu().numpy()
        if has_repeated_ngram(free, n):
            return T, free
    pytest.fail("plain greedy never repeats an n-gram: the no-repeat test would show nothing")


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_generate_scores_are_processed_logits(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(case, kw)
    T, free = _repeating_budget(model, g, images, sizes, 3)
    out = _gen(model, g, images, sizes, max_new_tokens=T, eos_token_id=None, repetition_penalty=1.3, no_repeat_ngram_size=3,
               output_scores=True, output_logits=True, return_dict_in_generate=True)
    seq = out.sequences[0].cpu().numpy()
    assert len(out.scores) == len(out.logits) == seq.size == T
    for t in range(T):
        raw, sc = out.logits[t][0].cpu().numpy(), out.scores[t][0].cpu().numpy()
        want = process_row(raw, seq[:t], penalty=1.3, ngram=3)
        assert same_values(sc, want), t
        assert int(seq[t]) == argmax(want), t
    assert not has_repeated_ngram(seq, 3)
    plain = _gen(model, g, images, sizes, max_new_tokens=4, eos_token_id=None, output_scores=True, output_logits=True,
                 return_dict_in_generate=True)
    for t in range(4):                                               # no processor: scores are the raw logits
        assert torch.equal(plain.scores[t], plain.logits[t])
    assert _gen(model, g, images, sizes, max_new_tokens=4, return_dict_in_generate=True).logits is None


def test_min_new_tokens_delays_eos(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    free = _gen(model, g, images, sizes, max_new_tokens=24, eos_token_id=None)[0].cpu().numpy()
    k = next((i for i in range(2, 24) if free[i] not in free[:i]), 0)       # first emitted at step k
    eos = int(free[k])
    stop = _gen(model, g, images, sizes, max_new_tokens=24, eos_token_id=eos)[0].cpu().numpy()
    assert stop.size == k + 1 and stop[-1] == eos and np.array_equal(stop, free[:k + 1])
    m = k + 3
    out = _gen(model, g, images, sizes, max_new_tokens=24, eos_token_id=eos, min_new_tokens=m)[0].cpu().numpy()
    assert np.array_equal(out[:k], free[:k]) and eos not in out[:m].tolist()
    assert out.size >= m + 1 or out.size == 24


def test_bad_words_and_begin_suppress(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    free = _gen(model, g, images, sizes, max_new_tokens=16, eos_token_id=None)[0].cpu().numpy()
    one, pair = int(free[1]), [int(free[2]), int(free[3])]
    out = _gen(model, g, images, sizes, max_new_tokens=16, eos_token_id=None, bad_words_ids=[[one], pair],
               begin_suppress_tokens=[int(free[0])])[0].cpu().numpy()
    assert one not in out.tolist() and out[0] != free[0]
    assert not any(out[i] == pair[0] and out[i + 1] == pair[1] for i in range(out.size - 1))


@pytest.mark.parametrize("side", ["right", "left"])
def test_batch_rows_with_processors_generate_as_if_alone(golden_dir, side):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    prompts = [_prompt(g, b) for b in range(3)]
    prompts[1] = prompts[1][:-3]
    ids, am = _pad_batch(prompts, side)
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, eos_token_id=None, max_new_tokens=24, output_scores=True,
                return_dict_in_generate=True)
    out = model.generate(ids, images=images[:3], image_sizes=sizes[:3], attention_mask=am, **proc)
    for b in range(3):
        one = model.generate(torch.from_numpy(prompts[b][None]), images=[images[b]], image_sizes=[sizes[b]], **proc)
        row = out.sequences[b].cpu().numpy()
        assert not has_repeated_ngram(row, 2)
        for t in range(24):
            s1 = one.scores[t][0].cpu()
            fin = s1[torch.isfinite(s1)]
            top = torch.topk(fin, 2).values
            if float(top[0] - top[1]) < 3 * LOGITS_FP32_TOL * float(fin.abs().max()):
                break                                                # a near tie: the rest of the row may differ legitimately
            assert int(row[t]) == int(one.sequences[0, t]), (b, t)

"""GPU tests of generate_beams() end to end on the toy models: the returned hypotheses are what BeamState gives on the returned scores
(numpy top-K), the scores are the log-softmax of the raw logits, teacher forcing through the plain decode_step reproduces every raw
logits row bit for bit (which pins the ancestry lookup through the whole model), the shared prompt is never copied, the logits
processors see each beam's own history, and the int8 identity carries over."""
import numpy as np
import pytest
import torch

from logits_ref import process_row, same_values
from test_beam_host import np_topk
from test_beam_kernels_gpu import lsm_bound, lsm_exact
from test_generate_gpu import _load, _model, _pad_batch, _prompt

pytestmark = pytest.mark.gpu

NB, T_NEW, PAD = 3, 10, 1


def _batch(g, images, sizes):
    prompts = [_prompt(g, 0), _prompt(g, 1)[:-3]]                            # two prompts of different lengths
    ids, am = _pad_batch(prompts, "left")
    return ids, dict(images=images[:2], image_sizes=sizes[:2], attention_mask=am)


def _early_eos(model, ids, args):
    """The greedy token of row 0 at step 2: as an EOS id it ends a hypothesis well before the budget."""
    return int(model.generate(ids, max_new_tokens=3, eos_token_id=None, **args)[0, 2])


def _replay(out, B, nb, V, T, eos, fill, length_penalty=1.0, early_stopping=False):
    """BeamState driven by the returned per-step scores with the numpy top-K; also returns the running sequences before each step."""
    from radvlm_amd.generation import BeamState
    st = BeamState(B, nb, V, T, [eos] if eos is not None else [], length_penalty, early_stopping, fill)
    before = []
    st.finished_early = False                                                # a hypothesis entered the finished set before the last step
    for s in out.scores:
        assert not st.done
        before.append(st.running_sequences.copy())
        vals, flat = np_topk(s.cpu().numpy().reshape(B, nb, V), st.running_scores, st.K)
        st.step(vals, flat)
        st.finished_early |= st.cur < T and bool(st.is_sent_finished.any())
    assert st.done
    return st, before


# "early": the EOS id of the run is the greedy token of row 0 at step 2, so hypotheses finish (and the loop may end) early;
# "full": no EOS id, every hypothesis runs the whole budget and the ancestry tables grow to T_NEW - 1 entries
@pytest.fixture(scope="module", params=[("toy", "early"), ("toy_qwen", "early"), ("toy", "full"), ("toy_qwen", "full")],
                ids=lambda p: "-".join(p))
def beam_run(request, golden_dir):
    case, mode = request.param
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(case, kw)
    ids, args = _batch(g, images, sizes)
    eos = _early_eos(model, ids, args) if mode == "early" else None
    out = model.generate_beams(ids, num_beams=NB, num_return_sequences=NB, max_new_tokens=T_NEW, eos_token_id=eos, pad_token_id=PAD,
                               output_scores=True, output_logits=True, return_dict_in_generate=True, **args)
    return model, ids, args, eos, out


def test_hypotheses_are_beam_state_on_the_returned_scores(beam_run):
    model, ids, args, eos, out = beam_run
    V = model.engine.vocab
    assert V < 65536 and 2 * NB <= 32                                        # every projection takes the skinny-GEMM route
    assert len(out.scores) == len(out.logits) and 1 <= len(out.scores) <= T_NEW
    assert all(tuple(s.shape) == (2 * NB, V) and s.dtype == torch.float32 for s in out.scores + out.logits)
    st, _ = _replay(out, 2, NB, V, T_NEW, eos, PAD if eos is not None else -1)
    seq, sc, bi = st.finalize(NB)
    assert out.sequences.dtype == torch.int64 and np.array_equal(out.sequences.cpu().numpy(), seq)
    assert np.array_equal(out.beam_indices.cpu().numpy(), bi)
    assert np.array_equal(out.sequences_scores.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    # (e) best first within each prompt
    s = out.sequences_scores.cpu().numpy().reshape(2, NB)
    assert (np.diff(s, axis=1) <= 0).all(), s
    lengths = (bi != -1).sum(axis=1)
    if eos is None:
        assert (lengths == T_NEW).all() and len(out.scores) == T_NEW
    else:                                                                    # the EOS id chosen at run time ends a hypothesis before the budget
        assert st.finished_early
        for h in np.flatnonzero(lengths < T_NEW):
            assert seq[h, lengths[h] - 1] == eos
        assert (seq[bi == -1] == PAD).all()


def test_scores_are_the_log_softmax_of_the_raw_logits(beam_run):
    model, ids, args, eos, out = beam_run
    V = model.engine.vocab
    from conftest import record_measurement
    worst = 0.0
    for t, (s, raw) in enumerate(zip(out.scores, out.logits)):
        s, raw = s.cpu().numpy(), raw.cpu().numpy()
        for r in range(s.shape[0]):
            want = lsm_exact(raw[r])
            err = np.abs(s[r].astype(np.float64) - want)
            assert (err <= lsm_bound(want, V)).all(), (t, r, float(err.max()))
            worst = max(worst, float(err.max()))
    record_measurement("beam_scores_vs_float64_log_softmax", vocab=V, max_abs_err=worst)


def test_teacher_forcing_reproduces_every_logits_row_bit_for_bit(beam_run):
    """Hypothesis j of both prompts is fed token by token through prefill + the plain decode_step (no beams, batch of 2).  The raw
    logits that predict its token t must be the bits of the beam run's logits[t] at the row beam_indices names: same K|V bits in other
    places of the cache, reached through the ancestry table."""
    model, ids, args, eos, out = beam_run
    eng = model.engine
    seq, bi = out.sequences.cpu().numpy(), out.beam_indices.cpu().numpy()
    lengths = (bi != -1).sum(axis=1)
    am = args["attention_mask"].numpy()
    compared = 0
    for j in range(NB):
        hyp = [b * NB + j for b in range(2)]
        cache, logits = eng.prefill(ids.numpy(), am, args["images"], args["image_sizes"], max_new_tokens=T_NEW)
        for t in range(int(lengths[hyp].max())):
            for b, h in enumerate(hyp):
                if t < lengths[h]:
                    want = out.logits[t][int(bi[h, t])]
                    assert torch.equal(logits[b], want), (j, b, t, float((logits[b] - want).abs().max()))
                    compared += 1
            if t + 1 < int(lengths[hyp].max()):
                tok = [int(seq[h, t]) if t < lengths[h] else 0 for h in hyp]          # a finished row is fed a filler, its logits are not read
                logits = eng.decode_step(cache, tok)
        del cache
    assert compared == int(lengths.sum()) and compared >= 2 * NB                 # every token of every returned hypothesis
    if eos is None:
        assert compared == 2 * NB * T_NEW
    # step 0: every beam row of a prompt carries the batch prefill's logits
    _, l0 = eng.prefill(ids.numpy(), am, args["images"], args["image_sizes"], max_new_tokens=T_NEW)
    for r in range(2 * NB):
        assert torch.equal(out.logits[0][r], l0[r // NB])


def test_prompt_rows_of_non_root_beams_are_never_written(beam_run):
    model, ids, args, eos, out = beam_run
    cache = out.past_key_values
    plan = model.engine.plan(ids.numpy(), args["attention_mask"].numpy(), None, list(args["images"]), args["image_sizes"])
    lens = plan["lens"]
    steps = len(out.scores) - 1                                              # decode steps run: positions lens[b] .. lens[b] + steps - 1
    assert cache.B == 2 * NB and (cache.lens == np.repeat(lens, NB) + steps).all()
    for layer in cache.layers:
        for r in range(2 * NB):
            b = r // NB
            if r % NB:
                assert not layer[r, :int(lens[b])].any(), r                  # the shared prompt lives in the root row only
            else:
                assert layer[r, :int(lens[b])].any()
            if steps:
                assert layer[r, int(lens[b]):int(lens[b]) + steps].any()     # every beam appended to its own row
            assert not layer[r, int(lens[b]) + steps:].any()


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_processors_see_each_beams_own_history(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(case, kw)
    from radvlm_amd import ops
    ids, args = _batch(g, images, sizes)
    eos = _early_eos(model, ids, args)
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=3)
    out = model.generate_beams(ids, num_beams=NB, num_return_sequences=NB, max_new_tokens=T_NEW, eos_token_id=eos, pad_token_id=PAD,
                               output_scores=True, output_logits=True, return_dict_in_generate=True, **proc, **args)
    V = model.engine.vocab
    st, before = _replay(out, 2, NB, V, T_NEW, eos, PAD)
    touched = 0
    for t, (s, raw) in enumerate(zip(out.scores, out.logits)):
        lsm = ops.log_softmax_rows(raw.clone(), V).cpu().numpy()             # the kernel's bits: a row does not depend on its launch
        hist = before[t].reshape(2 * NB, T_NEW)[:, :t]
        s = s.cpu().numpy()
        for r in range(2 * NB):
            want = process_row(lsm[r], hist[r], penalty=1.3, ngram=2, eos=[eos], min_new=3)
            assert same_values(s[r], want), (t, r, np.flatnonzero(s[r] != want)[:8])
            touched += int((want != lsm[r]).sum())
            if t < 3:
                assert s[r, eos] == -np.inf
    assert touched > 0
    seq, sc, bi = st.finalize(NB)
    assert np.array_equal(out.sequences.cpu().numpy(), seq) and np.array_equal(out.beam_indices.cpu().numpy(), bi)
    assert not (seq[:, :3] == eos).any()                                     # min_new_tokens held the EOS id back on every beam


def test_generate_still_refuses_beams_and_one_beam_runs_the_budget(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    ids, args = _batch(g, images, sizes)
    with pytest.raises(NotImplementedError, match="generate_beams"):
        model.generate(ids, num_beams=2, **args)
    with pytest.raises(NotImplementedError):
        model.generate_beams(ids, num_beams=2, do_sample=True, **args)
    one = model.generate_beams(ids, num_beams=1, eos_token_id=None, max_new_tokens=7, **args)
    assert one.dtype == torch.int64 and tuple(one.shape) == (2, 7)
    # one beam without an EOS id and without a length effect is greedy decoding
    greedy = model.generate(ids, eos_token_id=None, max_new_tokens=7, **args)
    assert torch.equal(one, greedy)
    plain = model.generate_beams(ids, num_beams=2, eos_token_id=None, max_new_tokens=4, return_dict_in_generate=True, **args)
    assert plain.sequences_scores is None and plain.scores is None and plain.logits is None and tuple(plain.sequences.shape) == (2, 4)

    seen = []

    def crit(cand, scores):
        seen.append((tuple(cand.shape), scores))
        return torch.full((cand.shape[0],), cand.shape[1] >= 2, dtype=torch.bool)

    out = model.generate_beams(ids, num_beams=2, eos_token_id=None, max_new_tokens=6, stopping_criteria=[crit], **args)
    assert seen[0] == ((2 * 4, 1), None) and tuple(out.shape) == (2, 2)      # K = 4 candidates per prompt, flattened


def test_int8_identity_carries_over(golden_dir):
    """On a quantised model the decode steps read the int8 copies; the bf16 kernel on the same (dequantised) weights gives the same bits."""
    g, images, sizes, kw = _load(golden_dir, "toy_qwen")
    model = _model("toy_qwen", kw)
    model.quantize_decoder_()
    ids, args = _batch(g, images, sizes)
    kwargs = dict(num_beams=NB, num_return_sequences=NB, max_new_tokens=6, eos_token_id=None, output_scores=True,
                  return_dict_in_generate=True, **args)
    assert model.engine.w8_decode is True
    q = model.generate_beams(ids, **kwargs)
    model.engine.w8_decode = False
    try:
        d = model.generate_beams(ids, **kwargs)
    finally:
        model.engine.w8_decode = True
    assert torch.equal(q.sequences, d.sequences) and torch.equal(q.sequences_scores, d.sequences_scores)
    assert all(torch.equal(a, b) for a, b in zip(q.scores, d.scores))

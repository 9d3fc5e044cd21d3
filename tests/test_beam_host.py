"""Host tests of beam search's bookkeeping (radvlm_amd/generation.py: BeamState, parse_beam_kwargs, advance_tail_src): no device.

BeamState is replayed on the per-step scores transformers itself recorded for a tiny random Llama on the CPU and must give the same
sequences, beam indices and fp32 score bits; the top-K of every step is computed here, independently (np.lexsort: value descending,
then flat index ascending)."""
import itertools

import numpy as np
import pytest

from radvlm_amd.generation import BeamState, advance_tail_src, beams_to_keep, parse_beam_kwargs

VOCAB, PROMPT, MAX_NEW = 50, 4, 6
MODEL_SEED, LM_HEAD_GAIN = 3, 40.0
# EOS ids picked on the CPU from what this model generates (seed 3): 12 and 45 are the second tokens of the two prompts' best first
# beams, so hypotheses finish early, some loops end before the budget and the returned hypothesis is often not the top running beam
EOS_CHOICES = (None, [12], [12, 45])


def np_topk(x, score, K):
    """x fp32 [B, nb, V], score fp32 [B, nb] -> (vals [B, K], flat [B, K]) of fl(x + score): value descending, then flat index ascending."""
    B, nb, V = x.shape
    v = (np.float32(x) + np.float32(score)[:, :, None]).reshape(B, nb * V)
    vals, flat = np.empty((B, K), np.float32), np.empty((B, K), np.int64)
    for b in range(B):
        order = np.lexsort((np.arange(nb * V), -v[b]))[:K]
        vals[b], flat[b] = v[b][order], order
    return vals, flat


def replay(scores, B, nb, V, T, eos, length_penalty, early_stopping, fill):
    """Drive BeamState with recorded per-step scores ([B * nb, V] each); returns the state after the last recorded step."""
    st = BeamState(B, nb, V, T, eos or [], length_penalty, early_stopping, fill)
    for t, s in enumerate(scores):
        assert not st.done, f"BeamState stopped after {t} steps, the recording has {len(scores)}"
        vals, flat = np_topk(np.asarray(s, dtype=np.float32).reshape(B, nb, V), st.running_scores, st.K)
        st.step(vals, flat)
    return st


# ------------------------------------------------------------------------------------------------ 1. against transformers itself
@pytest.fixture(scope="module")
def hf_model():
    transformers = pytest.importorskip("transformers")
    import torch
    cfg = transformers.LlamaConfig(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=64, bos_token_id=None, eos_token_id=None, pad_token_id=None)
    torch.manual_seed(MODEL_SEED)
    model = transformers.LlamaForCausalLM(cfg).eval().float()
    with torch.no_grad():
        model.lm_head.weight.mul_(LM_HEAD_GAIN)           # a random init gives nearly uniform scores: sharpen them so beams compete
    ids = torch.from_numpy(np.random.default_rng(0).integers(0, VOCAB, size=(2, PROMPT)))
    return model, ids


def hf_grid():
    for nb, eos, pen, es in itertools.product((1, 2, 4), EOS_CHOICES, (0.0, 1.0, 2.0, -1.0), (False, True, "never")):
        for nrs in sorted({1, nb}):
            yield nb, eos, pen, es, nrs


def run_hf(model, ids, nb, eos, pen, es, nrs):
    """transformers' own beam search.  generate() routes num_beams = 1 to its greedy loop, which is not _beam_search with one beam (a
    single beam still keeps 2 candidates and a finished set), so for that case the dispatch alone is patched to the beam search mode."""
    import torch
    from transformers.generation.configuration_utils import GenerationConfig, GenerationMode
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        if nb == 1:
            mp.setattr(GenerationConfig, "get_generation_mode", lambda self, assistant_model=None: GenerationMode.BEAM_SEARCH)
        return model.generate(ids, attention_mask=torch.ones_like(ids), num_beams=nb, num_return_sequences=nrs, length_penalty=pen,
                              early_stopping=es, eos_token_id=eos, pad_token_id=None, max_new_tokens=MAX_NEW, do_sample=False,
                              output_scores=True, output_logits=True, return_dict_in_generate=True)


def test_beam_state_matches_transformers(hf_model):
    model, ids = hf_model
    B = ids.shape[0]
    seen = dict(eos_before_budget=0, stopped_before_budget=0, not_top_running=0)
    for nb, eos, pen, es, nrs in hf_grid():
        out = run_hf(model, ids, nb, eos, pen, es, nrs)
        what = f"num_beams={nb} eos={eos} length_penalty={pen} early_stopping={es!r} num_return_sequences={nrs}"
        fill = eos[0] if eos else -1                      # HF: pad_token_id (set to the first EOS id by generate) else -1
        st = replay([s.numpy() for s in out.scores], B, nb, VOCAB, MAX_NEW, eos, pen, es, fill)
        assert st.done, what
        top_running = st.running_sequences[:, 0].copy()
        seq, sc, bi = st.finalize(nrs)
        want_seq = out.sequences[:, PROMPT:].numpy()
        assert seq.shape == want_seq.shape and (seq == want_seq).all(), what
        assert bi.shape == tuple(out.beam_indices.shape) and (bi == out.beam_indices.numpy()).all(), what
        want_sc = out.sequences_scores.numpy()
        assert want_sc.dtype == np.float32 and (sc.view(np.uint32) == want_sc.view(np.uint32)).all(), (what, sc, want_sc)
        lengths = (bi != -1).sum(axis=1)
        if eos and ((lengths < MAX_NEW) & np.isin(seq[np.arange(len(seq)), lengths - 1], eos)).any():
            seen["eos_before_budget"] += 1
        if len(out.scores) < MAX_NEW:
            seen["stopped_before_budget"] += 1
        best = seq[::nrs]
        if any((best[b, :seq.shape[1]] != top_running[b, :seq.shape[1]]).any() for b in range(B)):
            seen["not_top_running"] += 1
    # the grid must exercise: a hypothesis finished by EOS before the budget, a loop that stopped early, a returned hypothesis that is
    # not the final top running beam
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------ 2. a hand-worked case
def test_beam_state_hand_worked():
    """2 beams, 3 steps, vocabulary 4, EOS id 3, length_penalty 1, early_stopping False, K = 4.  Scores are multiples of 0.5 so every
    sum and every quotient below is exact in fp32 (by 1, 2 and 3: -4.5 / 3 = -1.5)."""
    st = BeamState(1, 2, 4, 3, eos=[3], length_penalty=1.0, early_stopping=False, fill=9)
    assert st.K == 4
    f = np.float32
    # step 0: both rows carry the prefill scores; beam 1 starts at -1e9, so every candidate comes from beam 0
    lp0 = np.array([-1.0, -2.0, -4.0, -1.5], dtype=f)
    x = np.stack([lp0, lp0])[None]
    vals, flat = np_topk(x, st.running_scores, 4)
    assert flat.tolist() == [[0, 3, 1, 2]] and vals.tolist() == [[-1.0, -1.5, -2.0, -4.0]]
    parent, tok = st.step(vals, flat)
    # candidate 1 is EOS and within the first 2: it finishes with -1.5 / 1; the running beams are tokens 0 and 1
    assert parent.tolist() == [[0, 0]] and tok.tolist() == [[0, 1]]
    assert st.running_scores.tolist() == [[-1.0, -2.0]]
    assert st.beam_scores.tolist() == [[-1.5, -1e9]] and st.is_sent_finished.tolist() == [[True, False]]
    assert st.sequences[0, 0].tolist() == [3, 9, 9] and st.beam_indices[0, 0].tolist() == [0, -1, -1]
    assert not st.done and st.unsat.all()
    # step 1: beam 0 ([0], -1.0) and beam 1 ([1], -2.0)
    x = np.array([[[-0.5, -3.0, -3.0, -2.0], [-0.5, -1.0, -3.0, -3.0]]], dtype=f)
    vals, flat = np_topk(x, st.running_scores, 4)
    # accumulated: beam 0 -> -1.5, -4, -4, -3; beam 1 -> -2.5, -3, -5, -5.  Two candidates tie at -3.0: flat 3 (beam 0, token 3) before 5
    assert flat.tolist() == [[0, 4, 3, 5]] and vals.tolist() == [[-1.5, -2.5, -3.0, -3.0]]
    parent, tok = st.step(vals, flat)
    # the EOS candidate (slot 2) is outside the first 2, so nothing finishes; it is only barred from running
    assert parent.tolist() == [[0, 1]] and tok.tolist() == [[0, 0]]
    assert st.running_sequences[0, :, :2].tolist() == [[0, 0], [1, 0]] and st.running_scores.tolist() == [[-1.5, -2.5]]
    assert st.running_beam_indices[0, :, :2].tolist() == [[0, 0], [0, 1]]
    assert st.beam_scores.tolist() == [[-1.5, -1e9]]
    # heuristic: best running -1.5 / 2 = -0.75 > -1e9 (slot 1 is still open): improvement stays possible
    assert not st.done and st.unsat.all()
    # step 2, the last of the budget: every candidate finishes; only the first 2 may enter the finished set
    x = np.array([[[-3.0, -1.0, -3.0, -3.0], [-0.5, -3.0, -3.0, -3.0]]], dtype=f)
    vals, flat = np_topk(x, st.running_scores, 4)
    # beam 0 -> -4.5, -2.5, -4.5, -4.5; beam 1 -> -3, -5.5, -5.5, -5.5
    assert flat.tolist() == [[1, 4, 0, 2]] and vals.tolist() == [[-2.5, -3.0, -4.5, -4.5]]
    st.step(vals, flat)
    assert st.done
    # finished candidates: [0, 0, 1] at -2.5 / 3 and [1, 0, 0] at -3 / 3 = -1.0; merged with {-1.5, -1e9}: the best two are -2.5 / 3, -1.0
    seq, sc, bi = st.finalize(2)
    assert seq.tolist() == [[0, 0, 1], [1, 0, 0]]
    assert sc.tolist() == [float(f(-2.5) / f(3.0)), -1.0]
    assert bi.tolist() == [[0, 0, 0], [0, 1, 1]]
    # the early EOS hypothesis [3] at -1.5 dropped out of the best two; with one return sequence only the best is returned
    seq1, sc1, bi1 = st.finalize(1)
    assert seq1.tolist() == [[0, 0, 1]] and bi1.tolist() == [[0, 0, 0]]


def test_beam_state_user_criteria_and_candidates():
    st = BeamState(2, 2, 5, 4, eos=[], length_penalty=1.0, early_stopping=False, fill=-1)
    x = np.tile(np.array([-1.0, -2.0, -3.0, -4.0, -5.0], np.float32), (2, 2, 1))
    vals, flat = np_topk(x, st.running_scores, st.K)
    cand = st.candidates(flat)
    assert cand.shape == (2 * st.K, 1) and cand[:, 0].tolist() == [0, 1, 2, 3] * 2
    hit = np.zeros((2, st.K), bool)
    hit[0, 0] = True                                        # the user's criterion stops prompt 0's best candidate
    parent, tok = st.step(vals, flat, hit.reshape(-1))
    assert tok.tolist() == [[1, 2], [0, 1]]
    assert st.is_sent_finished.tolist() == [[True, False], [False, False]] and st.sequences[0, 0].tolist() == [0, -1, -1, -1]


# ------------------------------------------------------------------------------------------------ 3. parse_beam_kwargs
def test_parse_beam_kwargs_defaults_and_values():
    cfg = parse_beam_kwargs(dict(num_beams=3, max_new_tokens=5), config_eos=2)
    assert (cfg.num_beams, cfg.num_return_sequences, cfg.length_penalty, cfg.early_stopping, cfg.K) == (3, 1, 1.0, False, 6)
    assert cfg.eos == [2] and cfg.fill == 2 and cfg.max_new_tokens == 5 and cfg.sampling is None
    cfg = parse_beam_kwargs(dict(num_beams=4, num_return_sequences=4, length_penalty=2, early_stopping="never", eos_token_id=[5, 6, 7],
                                 pad_token_id=1))
    assert (cfg.num_return_sequences, cfg.length_penalty, cfg.early_stopping, cfg.K, cfg.fill) == (4, 2.0, "never", 16, 1)
    assert parse_beam_kwargs(dict(num_beams=2, early_stopping=True)).early_stopping is True
    assert parse_beam_kwargs({}).num_beams == 1 and parse_beam_kwargs({}).K == 2
    # HF's output_fill_value: without an EOS id it is -1 whatever the pad; a pad of 0 falls through to the first EOS id
    assert parse_beam_kwargs(dict(num_beams=2, pad_token_id=4)).fill == -1
    assert parse_beam_kwargs(dict(num_beams=2, pad_token_id=0, eos_token_id=9)).fill == 9
    assert beams_to_keep(5, 0) == 10 and beams_to_keep(5, 1) == 10 and beams_to_keep(5, 2) == 15


def test_parse_beam_kwargs_ignores_greedy_sampling_knobs():
    cfg = parse_beam_kwargs(dict(num_beams=2, temperature=0.3, top_p=0.5, top_k=7, typical_p=0.2, min_p=0.1, epsilon_cutoff=0.1,
                                 eta_cutoff=0.1, do_sample=False))
    assert cfg.sampling is None and cfg.num_beams == 2


def test_parse_beam_kwargs_errors():
    with pytest.raises(ValueError, match=r"\[1, 16\]"):
        parse_beam_kwargs(dict(num_beams=17))
    for bad in (0, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="num_beams"):
            parse_beam_kwargs(dict(num_beams=bad))
    with pytest.raises(ValueError, match="limit is 64"):
        parse_beam_kwargs(dict(num_beams=13, eos_token_id=[1, 2, 3, 4]))             # K = 5 * 13 = 65
    assert parse_beam_kwargs(dict(num_beams=16, eos_token_id=[1, 2, 3])).K == 64
    with pytest.raises(ValueError, match="num_return_sequences"):
        parse_beam_kwargs(dict(num_beams=2, num_return_sequences=3))
    with pytest.raises(ValueError, match="num_return_sequences"):
        parse_beam_kwargs(dict(num_beams=2, num_return_sequences=0))
    with pytest.raises(ValueError, match="length_penalty"):
        parse_beam_kwargs(dict(num_beams=2, length_penalty="1"))
    with pytest.raises(ValueError, match="early_stopping"):
        parse_beam_kwargs(dict(num_beams=2, early_stopping="always"))
    with pytest.raises(NotImplementedError, match="beam sampling"):
        parse_beam_kwargs(dict(num_beams=2, do_sample=True))
    with pytest.raises(NotImplementedError, match="beam sampling"):
        parse_beam_kwargs(dict(num_beams=2, do_sample=True, seed=1))
    with pytest.raises(NotImplementedError, match="past_key_values"):
        parse_beam_kwargs(dict(num_beams=2, past_key_values=object()))
    with pytest.raises(NotImplementedError, match="streamer"):
        parse_beam_kwargs(dict(num_beams=2, streamer=object()))
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        parse_beam_kwargs(dict(num_beams=2, inputs_embeds=np.zeros((1, 2, 3))))
    with pytest.raises(NotImplementedError, match="LoRA"):
        parse_beam_kwargs(dict(num_beams=2), lora=True)
    with pytest.raises(TypeError, match="diversity_penalty"):
        parse_beam_kwargs(dict(num_beams=2, diversity_penalty=0.5))
    with pytest.raises(ValueError, match="repetition_penalty"):
        parse_beam_kwargs(dict(num_beams=2, repetition_penalty=-1.0))
    with pytest.raises(ValueError, match="max_new_tokens"):
        parse_beam_kwargs(dict(num_beams=2, max_new_tokens=-1))


def test_generate_keeps_raising_for_beams():
    from radvlm_amd.generation import parse_batch_kwargs, parse_generate_kwargs
    with pytest.raises(NotImplementedError, match="generate_beams"):
        parse_generate_kwargs(dict(num_beams=4))
    with pytest.raises(NotImplementedError, match="generate_beams"):
        parse_batch_kwargs(dict(num_beams=3), 2)


# ------------------------------------------------------------------------------------------------ 4. the ancestry table
def test_advance_tail_src_follows_copy_the_parent_simulation():
    """Simulation: every row keeps the list of (row, position) cells that hold its generated positions; a beam step copies the parent's
    list and appends the row's own cell.  advance_tail_src must list the same rows, for several prompts and random parents."""
    rng = np.random.default_rng(5)
    B, nb, T = 3, 4, 9
    rows = B * nb
    tail = np.zeros((rows, T), dtype=np.int32)
    sim = [[] for _ in range(rows)]
    for i in range(T):
        parent = rng.integers(0, nb, size=(B, nb))
        if i == 0:
            parent[:] = 0                                   # step 0: every running beam descends from beam 0
        prow = (np.arange(B)[:, None] * nb + parent).reshape(-1)
        before = tail.copy()
        new = advance_tail_src(tail, prow, i)
        assert (tail == before).all()                       # the input is not modified
        tail = new
        sim = [sim[prow[r]] + [r] for r in range(rows)]
        for r in range(rows):
            assert tail[r, :i + 1].tolist() == sim[r], (i, r)
            assert (tail[r, :i + 1] // nb == r // nb).all()                              # ancestry never leaves the prompt's rows
    # every cell (row, position) is written by exactly one beam step: position i of row r is only ever row r's own
    assert all(sim[r][-1] == r for r in range(rows))

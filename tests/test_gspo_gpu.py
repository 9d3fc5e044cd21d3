"""GPU tests of GRPO with sequence-level importance ratios (importance_sampling_level="sequence", GSPO) on the toy goldens.  The anchor
is bit for bit: whenever the sequence ratio is exactly 1 -- on-policy, or old log-probs from token_logps() -- the coefficient
rv_gspo_seqs_f64 writes is the fp32 product the token kernel forms, so both levels leave the same gradient buffer.  Where the levels
differ (old log-probs alternating half a nat around the policy's) the coefficients are held to tests/gspo_ref.py."""
import numpy as np
import pytest
import torch

import gspo_ref
from preference_ref import fp32_ulp
from test_generate_gpu import CASES, _load, _model
from test_policy_gpu import _args, _batch, _bits, _counts, _dataset, _even_fraction, _grads, _strip_times

pytestmark = pytest.mark.gpu

ADV = [0.7, -1.3, 0.4]
SEQ = dict(importance_sampling_level="sequence")


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_anchor_padded_packed_and_head_rows(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw).train()
    batch = _batch(g, images, sizes)
    B = len(ADV)
    for packed in (False, True):
        for head_rows in ("labeled", "all"):
            model.engine.packed, model.engine.head_rows = packed, head_rows
            old = model.token_logps(**batch)
            for terms in (dict(), dict(old_logps=old), dict(ref_logps=old, beta=0.04), dict(old_logps=old, ref_logps=old, beta=0.04)):
                tok, out_t = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, **terms))
                seq, out = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, **terms, **SEQ))
                where = (case, packed, head_rows, sorted(terms))
                assert float(tok.float().abs().max()) > 0, where
                assert torch.equal(_bits(seq), _bits(tok)), where
                assert (out.seq_ratio == 1.0).all() and out.seq_ratio.dtype == torch.float64 and tuple(out.seq_ratio.shape) == (B,), where
                assert not bool(out.seq_clip.any()) and not bool(out.clip.any()) and not bool(out.kl.any()), where
                assert torch.equal(_bits(out.logps), _bits(out_t.logps)) and torch.equal(_bits(out.logps), _bits(old)), where
                # the surrogate's value at s = 1 is -A per token, under either level; the two sums differ in order and precision
                assert abs(float(out.loss.detach()) - float(out_t.loss.detach())) <= 1e-5, where


def test_levels_differ_where_the_ratios_do(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    eng = model.engine
    batch = _batch(g, images, sizes)
    counts = np.asarray(_counts(model, batch))
    n = int(counts.sum())
    logp = model.token_logps(**batch)
    # old log-probs half a nat below and above the policy's, alternating over each sample's tokens: every token ratio is e^+-0.5, far
    # outside [0.8, 1.2], while a sample's mean log-ratio is 0 or +-0.5 / n
    sign = np.concatenate([np.where(np.arange(c) % 2 == 0, 1.0, -1.0) for c in counts]).astype(np.float32)
    old = logp - 0.5 * torch.from_numpy(sign).to(logp.device)
    for head_rows in ("labeled", "all"):
        eng.head_rows = head_rows
        tok, out_t = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old))
        seq, out = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old, **SEQ))
        assert bool((out_t.clip != 0).any()) and float(out_t.stats["clip_ratio/high"]) + float(out_t.stats["clip_ratio/low"]) > 0
        assert out.seq_clip.cpu().tolist() == [0.0] * len(ADV) and not bool(out.clip.any())
        assert float(out.stats["clip_ratio/high"]) == 0.0 and float(out.stats["clip_ratio/low"]) == 0.0
        assert not torch.equal(_bits(seq), _bits(tok)) and float(seq.float().abs().max()) > 0
        w = np.full(n, 1.0 / n)
        ref = gspo_ref.gspo(out.logps.cpu().numpy(), counts, ADV, w.astype(np.float32), (w * eng.loss_scale).astype(np.float32),
                            old_logp=old.cpu().numpy(), eps_low=0.2, eps_high=0.2)
        want = ref["coef"].astype(np.float32)
        err = np.abs(out.coefs.cpu().numpy().astype(np.float64) - want.astype(np.float64)) / fp32_ulp(want)
        print(f"head_rows={head_rows}: coefs against gspo_ref, worst {err.max():.3g} fp32 ulp")
        assert err.max() <= 1.0
        assert np.array_equal(out.seq_logratio.cpu().numpy(), ref["m"]) and np.abs(out.seq_ratio.cpu().numpy() / ref["s"] - 1).max() <= 8 * 2.0 ** -52
        # loss and clip repeat the sample's term over its tokens
        assert np.abs(out.loss.detach().cpu().item() - ref["L"]) <= 1e-6 * max(1.0, abs(ref["L"]))
        assert np.allclose(eng.last_policy["loss"].cpu().numpy(), np.repeat(ref["l"], counts), rtol=2.0 ** -22, atol=0)


def test_uniform_shift_clips_whole_sequences(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    batch = _batch(g, images, sizes)
    counts = np.asarray(_counts(model, batch))
    old = model.token_logps(**batch)
    # old log-probs half a nat lower: s = e^0.5 > 1 + eps, so the positive-advantage samples clip high and the negative one stays active
    grads, out = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old - 0.5, **SEQ))
    assert out.seq_clip.cpu().tolist() == [2.0, 0.0, 2.0]
    assert out.clip.cpu().tolist() == np.repeat([2.0, 0.0, 2.0], counts).tolist()
    assert float(out.stats["clip_ratio/high"]) == pytest.approx(2.0 / 3.0) and float(out.stats["clip_ratio/low"]) == 0.0
    # only the active sample carries a gradient coefficient
    coefs = out.coefs.cpu().numpy()
    live = np.repeat([False, True, False], counts)
    assert not coefs[~live].any() and (coefs[live] < 0).all() and float(grads.float().abs().max()) > 0
    # per-token advantages that vary inside a sample have no sequence-level meaning
    per_token = [np.linspace(0.5, 1.0, int(c)) for c in counts]
    with pytest.raises(ValueError, match="one advantage per sample"):
        model.policy_loss(**batch, advantages=per_token, **SEQ)
    with pytest.raises(ValueError, match="importance_sampling_level"):
        model.policy_loss(**batch, advantages=ADV, importance_sampling_level="sentence")


def test_empty_sample(golden_dir):
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw).train()
    labels = np.array(g["labels"])
    labels[1] = -100                                           # a masked truncated completion: no scored token
    batch = dict(_batch(g, images, sizes), labels=labels)
    counts = np.asarray(_counts(model, batch))
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    for head_rows in ("labeled", "all"):
        model.engine.head_rows = head_rows
        old = model.token_logps(**batch)
        tok, _ = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old))
        seq, out = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old, **SEQ))
        assert torch.equal(_bits(seq), _bits(tok)) and float(seq.float().abs().max()) > 0
        assert out.seq_ratio.cpu().tolist() == [1.0, 1.0, 1.0] and out.seq_logratio.cpu().tolist() == [0.0, 0.0, 0.0]
        assert tuple(out.coefs.shape) == (int(counts.sum()),) == tuple(out.logps.shape)
        _, out = _grads(model, lambda: model.policy_loss(**batch, advantages=ADV, old_logps=old - 0.5, **SEQ))
        assert out.seq_clip.cpu().tolist() == [2.0, 0.0, 2.0] and out.seq_ratio.cpu().tolist()[1] == 1.0
        assert float(out.stats["clip_ratio/high"]) == pytest.approx(1.0)          # of the two samples that have a scored token


# ------------------------------------------------------------------------------------------------ the trainer
def _train(golden_dir, case, reward_funcs=_even_fraction, with_ref=False, **args):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(case, kw).train()
    extra = dict(ref_model=_model(case, kw)) if with_ref else {}
    state = GRPOTrainer(model, _args(**args), _dataset(g, images, sizes), reward_funcs, **extra).train()
    torch.cuda.synchronize()
    return model.engine.lm.flat.clone(), _strip_times(state["log_history"])


def test_trainer_levels_agree_on_policy(golden_dir):
    """num_iterations = 1: no old log-probs are taken, s = 1, and the two levels take the same steps."""
    w_tok, log_tok = _train(golden_dir, "toy", importance_sampling_level="token")
    w_seq, log_seq = _train(golden_dir, "toy", importance_sampling_level="sequence")
    assert torch.equal(_bits(w_seq), _bits(w_tok)) and len(log_seq) == 2
    for a, b in zip(log_tok, log_seq):
        assert a["completion_ids"] == b["completion_ids"] and a["grad_norm"] == b["grad_norm"] and b["grad_norm"] > 0
        assert b["clip_ratio/low"] == b["clip_ratio/high"] == b["kl"] == 0.0


def test_trainer_iterations_repeat(golden_dir):
    kw = dict(max_steps=1, num_iterations=2, beta=0.04, loss_type="grpo", learning_rate=3e-3, importance_sampling_level="sequence",
              epsilon=3e-4, epsilon_high=4e-4)
    (wa, la), (wb, lb) = (_train(golden_dir, "toy_qwen", with_ref=True, **kw) for _ in range(2))
    assert torch.equal(_bits(wa), _bits(wb)) and la == lb
    first, second = la[0]["iterations"]
    assert first["clip_ratio/low"] == first["clip_ratio/high"] == 0.0 and first["kl"] == 0.0       # s exactly 1, reference == policy
    assert np.isfinite([second["kl"], second["clip_ratio/low"], second["clip_ratio/high"], second["loss"]]).all() and second["kl"] > 0.0
    assert 0.0 <= second["clip_ratio/low"] <= 1.0 and 0.0 <= second["clip_ratio/high"] <= 1.0


def test_trainer_argument_check(golden_dir):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    model = _model("toy", kw)
    with pytest.raises(ValueError, match="importance_sampling_level"):
        GRPOTrainer(model, _args(importance_sampling_level="sentence"), _dataset(g, images, sizes), _even_fraction)
    assert GRPOTrainer(model, _args(importance_sampling_level="sequence"), _dataset(g, images, sizes), _even_fraction).importance_sampling_level == "sequence"
    assert GRPOTrainer(model, _args(), _dataset(g, images, sizes), _even_fraction).importance_sampling_level == "token"

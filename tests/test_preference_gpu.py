"""GPU tests of DPO preference training on the toy goldens: LlavaEngine.forward(preference=) / sequence_logps and the model's
preference_loss / sequence_logps.  Chosen = the golden rows; rejected = the same rows with every answer token replaced by
(id + 1) mod vocab in ids and labels and the last answer token dropped, so the two halves differ in length.  Every check is a property
that holds by construction: the step is policy_loss with the coefficients the pair kernel wrote (bit for bit); the pair terms are the
restatement's on token_logps(); a reference equal to the policy gives h = 0, loss = log 2 and closed-form coefficients exactly;
dpo_alpha = 0 leaves the SFT term; both weights 0 leave zero gradients."""
import math

import numpy as np
import pytest
import torch

import preference_ref as R
from radvlm_amd import preference as PF
from radvlm_amd.splice import shifted_labels
from test_generate_gpu import CASES, _load, _model

pytestmark = pytest.mark.gpu

LAYOUTS = [(packed, head_rows) for packed in (False, True) for head_rows in ("labeled", "all")]
PAIR_KEYS = ("chosen_input_ids", "chosen_attention_mask", "chosen_labels", "rejected_input_ids", "rejected_attention_mask", "rejected_labels")


def _bits(t):
    return t.contiguous().view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def _record(test, **kw):
    from conftest import record_measurement
    record_measurement(test, **kw)


def _pairs(g, vocab):
    ids, am, lab = g["input_ids"].astype(np.int64), g["attention_mask"].astype(bool), g["labels"].astype(np.int64)
    r_ids, r_am, r_lab = ids.copy(), am.copy(), lab.copy()
    for b in range(ids.shape[0]):
        ans = np.nonzero(lab[b] != -100)[0]
        assert ans.size >= 2, "the golden answer is too short to drop a token"
        r_ids[b, ans] = (ids[b, ans] + 1) % vocab
        r_lab[b, ans] = r_ids[b, ans]
        keep = np.delete(np.arange(ids.shape[1]), ans[-1])
        for a, fill in ((r_ids, 0), (r_am, False), (r_lab, -100)):
            a[b] = np.concatenate([a[b, keep], [fill]])
    return dict(zip(PAIR_KEYS, (ids, am, lab, r_ids, r_am, r_lab)))


def _setup(golden_dir, case):
    g, images, sizes, kw = _load(golden_dir, case)
    model = _model(CASES[case]["geo"], kw).train()
    pairs = _pairs(g, model.engine.vocab)
    ids, am, lab = PF.concatenate_pairs(*[pairs[k] for k in PAIR_KEYS])
    concat = dict(input_ids=ids, attention_mask=am, labels=lab, images=images + images, image_sizes=sizes + sizes)
    plan = model.engine.plan(ids, am, lab, concat["images"], concat["image_sizes"])
    counts = (shifted_labels(plan["labels"]) != -100).sum(1)
    return model, dict(pairs, images=images, image_sizes=sizes), concat, counts


def _grads(model, run):
    eng = model.engine
    eng.zero_grad()
    out = run()
    out.loss.backward()
    torch.cuda.synchronize()
    return eng.grads.clone(), out


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_composition_and_pair_terms(golden_dir, case):
    model, batch, concat, counts = _setup(golden_dir, case)
    P, n = counts.size // 2, int(counts.sum())
    assert (counts[:P] == counts[P:] + 1).all()                   # the halves differ in length
    ref_sums = -np.linspace(3.0, 9.0, 2 * P)                      # any finite reference
    kw = dict(ref_chosen_logps=ref_sums[:P], ref_rejected_logps=ref_sums[P:], beta=0.3, dpo_alpha=0.9, gamma=1.1)
    worst = {}
    for packed, head_rows in LAYOUTS:
        model.engine.packed, model.engine.head_rows = packed, head_rows
        for loss_type, eps in (("sigmoid", 0.1), ("ipo", 0.0)):
            tag = (case, packed, head_rows, loss_type)
            pref, out = _grads(model, lambda: model.preference_loss(**batch, loss_type=loss_type, label_smoothing=eps, **kw))
            assert float(pref.float().abs().max()) > 0 and out.coefs.dtype == torch.float32 and tuple(out.coefs.shape) == (n,)
            assert model.engine.last_preference["scored"].tolist() == counts.tolist()
            # (a) the step is policy_loss with the coefficients the pair kernel wrote
            pol, _ = _grads(model, lambda: model.policy_loss(**concat, advantages=out.coefs, weights=np.ones(n)))
            assert torch.equal(_bits(pol), _bits(pref)), tag
            # (b) the sequence sums: sequence_logps() of the same batch, and the restated order over token_logps()
            sums, cnt = model.sequence_logps(**concat)
            assert sums.dtype == torch.float64 and cnt.tolist() == counts.tolist()
            lp = _np(model.token_logps(**concat))
            want = np.array([R.ordered_sum(s) for s in np.split(lp, np.cumsum(counts)[:-1])])
            assert _np(sums).view(np.int64).tolist() == want.view(np.int64).tolist(), tag
            pi = torch.cat([out.chosen_logps, out.rejected_logps])
            if loss_type == "ipo":
                assert torch.equal(_bits(pi), _bits(sums / torch.from_numpy(counts.astype(np.float64)).to(sums.device))), tag
            else:
                assert torch.equal(_bits(pi), _bits(sums)), tag
            rho = ref_sums / counts if loss_type == "ipo" else ref_sums
            ref = R.dpo(lp, counts, ref=rho, beta=kw["beta"], dpo_alpha=kw["dpo_alpha"], gamma=kw["gamma"], loss_type=loss_type, label_smoothing=eps)
            got = dict(pi_c=_np(out.chosen_logps), pi_r=_np(out.rejected_logps), h=_np(out.margins), loss=_np(out.pair_loss),
                       reward_c=_np(out.rewards_chosen), reward_r=_np(out.rewards_rejected), coef=_np(out.coefs).astype(np.float64))
            for k, v in R.gate_ratios(got, ref, kw["beta"], rho).items():
                worst[k] = max(worst.get(k, 0.0), v)
            # the batch scalar and TRL's statistics
            assert abs(float(out.loss.detach()) - ref["L"]) <= 2.0 ** -23 * abs(ref["L"]) + 1e-12
            st = {k: float(v) for k, v in out.stats.items()}
            assert set(st) == {"rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins", "logps/chosen", "logps/rejected",
                               "dpo_loss", "sft_loss"}
            assert st["rewards/accuracies"] == float((ref["reward_c"] > ref["reward_r"]).mean())
            assert st["rewards/margins"] == pytest.approx(float((ref["reward_c"] - ref["reward_r"]).mean()), rel=1e-12)
            assert st["dpo_loss"] == pytest.approx(ref["dpo_loss"], rel=1e-12) and st["sft_loss"] == pytest.approx(ref["sft_loss"], rel=1e-12)
    print(f"{case}: worst gate ratios {worst}")
    _record(f"preference_model_pair_terms[{case}]", **{f"worst_ratio_{k}": v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_self_reference_is_exact(golden_dir, case):
    model, batch, concat, counts = _setup(golden_dir, case)
    P, n_c = counts.size // 2, int(counts[:counts.size // 2].sum())
    dpo_alpha, beta, gamma = 1.0, 0.1, 1.0
    for packed, head_rows in LAYOUTS:
        model.engine.packed, model.engine.head_rows = packed, head_rows
        sums, _ = model.sequence_logps(**concat)
        out = model.preference_loss(**batch, ref_chosen_logps=sums[:P], ref_rejected_logps=sums[P:], beta=beta, dpo_alpha=dpo_alpha, gamma=gamma)
        model.engine.ctx = None
        tag = (case, packed, head_rows)
        assert (_np(out.margins) == 0).all() and (_np(out.rewards_chosen) == 0).all() and (_np(out.rewards_rejected) == 0).all(), tag
        assert float(out.stats["rewards/accuracies"]) == 0.0 and float(out.stats["rewards/margins"]) == 0.0
        assert _np(out.pair_loss).tolist() == [math.log(2.0)] * P, tag
        coefs = _np(out.coefs)
        want = np.repeat([np.float32(dpo_alpha * beta / (2 * P) + gamma / n_c), np.float32(-dpo_alpha * beta / (2 * P))], [n_c, int(counts[P:].sum())])
        assert coefs.view(np.int32).tolist() == want.view(np.int32).tolist(), tag


@pytest.mark.parametrize("case", ["toy", "toy_qwen"])
def test_sft_only_zero_terms_and_refusals(golden_dir, case):
    model, batch, concat, counts = _setup(golden_dir, case)
    P, n_c = counts.size // 2, int(counts[:counts.size // 2].sum())
    for packed, head_rows in LAYOUTS:
        model.engine.packed, model.engine.head_rows = packed, head_rows
        # (d) dpo_alpha = 0: the loss is the chosen half's SFT loss
        lp = model.token_logps(**concat).double()[:n_c]
        _, out = _grads(model, lambda: model.preference_loss(**batch, reference_free=True, dpo_alpha=0.0, gamma=1.0))
        want = -float(lp.sum()) / n_c
        bound = n_c * 2.0 ** -23 * float(lp.abs().mean())
        print(f"{case} packed={packed} head_rows={head_rows}: |loss - SFT| = {abs(float(out.loss.detach()) - want):.3g}, bound {bound:.3g}")
        assert abs(float(out.loss.detach()) - want) <= bound and float(out.stats["dpo_loss"]) == 0.0
        assert (_np(out.coefs)[n_c:] == 0).all() and (_np(out.coefs)[:n_c] == np.float32(1.0 / n_c)).all()
        # (e) both weights 0: every gradient is zero
        model.engine.grads.fill_(1.0)
        zero, out = _grads(model, lambda: model.preference_loss(**batch, reference_free=True, dpo_alpha=0.0, gamma=0.0))
        assert float(zero.float().abs().max()) == 0.0 and float(out.loss.detach()) == 0.0
    # validation reaches the caller before any device work is kept
    with pytest.raises(ValueError, match="reference_free"):
        model.preference_loss(**batch)
    with pytest.raises(ValueError, match="ref_chosen_logps"):
        model.preference_loss(**batch, ref_chosen_logps=np.zeros(P + 1), ref_rejected_logps=np.zeros(P))
    no_answer = dict(batch, rejected_labels=np.where(np.arange(P)[:, None] == 1, -100, batch["rejected_labels"]))
    with pytest.raises(ValueError, match="pair 1: the rejected answer has no scored token"):
        model.preference_loss(**no_answer, reference_free=True)
    # (f) the raw DPO forward is still refused, and now names the entry point
    with pytest.raises(NotImplementedError, match="preference_loss"):
        model.eval()(input_ids=concat["input_ids"], attention_mask=concat["attention_mask"], labels=concat["labels"], images=concat["images"],
                     dpo_forward=True)


def test_lora_engine_trains_and_scores_in_eval_form(golden_dir):
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM
    _, batch, concat, counts = _setup(golden_dir, "toy")
    P = counts.size // 2
    lora = LlavaLlamaForCausalLM(LlavaConfig(geometry=GEOMETRIES["toy"], lora=dict(r=8, alpha=16, dropout=0.05)), device="cuda:0", init="portable", seed=0).train()
    eng = lora.engine
    step0 = eng.lora_step
    a, _ = lora.sequence_logps(**concat)
    b, _ = lora.sequence_logps(**concat)
    assert torch.equal(_bits(a), _bits(b)) and eng.lora_step == step0 and eng.ctx is None          # no adapter dropout, no training state touched
    grads, out = _grads(lora, lambda: lora.preference_loss(**batch, ref_chosen_logps=a[:P], ref_rejected_logps=a[P:]))
    assert eng.lora_step == step0 + 1 and float(grads.float().abs().max()) > 0 and math.isfinite(float(out.loss.detach()))
    assert float(out.margins.abs().max()) < 1.0          # the adapter starts as the identity: only its dropout separates policy and reference

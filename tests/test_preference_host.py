"""CPU tests of DPO preference training's host side: tests/preference_ref.py (the float64 restatement the GPU tests compare the kernels
with) pinned to torch autograd, radvlm_amd/preference.py (validation, the pair batch, offsets, the record contract) and the trainer's
argument checks.  No GPU is touched."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import preference_ref as R
from radvlm_amd import preference as PF

COUNTS = (3, 70, 1, 5, 64, 130)          # P = 3: chosen 3, 70, 1 and rejected 5, 64, 130 scored tokens


def _logps(seed, n, scale=0.4):
    return (-np.random.default_rng(seed).exponential(scale, n)).astype(np.float32)


def _autograd(x, counts, ref, beta, dpo_alpha, gamma, loss_type, eps):
    """L from a leaf tensor of token log-probs, written with torch's own functions (logsigmoid, relu), not with the restatement's."""
    P = len(counts) // 2
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    parts = torch.split(t, list(counts))
    pi = torch.stack([p.mean() if loss_type == "ipo" else p.sum() for p in parts])
    rho = torch.zeros(2 * P, dtype=torch.float64) if ref is None else torch.tensor(np.asarray(ref, dtype=np.float64))
    u = (pi[:P] - pi[P:]) - (rho[:P] - rho[P:])
    h = beta * u
    if loss_type == "sigmoid":
        l = -(1 - eps) * torch.nn.functional.logsigmoid(h) - eps * torch.nn.functional.logsigmoid(-h)
    elif loss_type == "hinge":
        l = torch.relu(1 - h)
    else:
        l = (u - 1 / (2 * beta)) ** 2
    sft = -torch.cat(parts[:P]).sum() / sum(counts[:P])
    L = dpo_alpha * l.mean() + gamma * sft
    L.backward()
    return float(L.detach()), l.detach().numpy(), h.detach().numpy(), -t.grad.numpy()


@pytest.mark.parametrize("loss_type,eps", [("sigmoid", 0.0), ("sigmoid", 0.1), ("hinge", 0.0), ("ipo", 0.0)])
@pytest.mark.parametrize("reference_free", [False, True])
def test_restatement_matches_autograd(loss_type, eps, reference_free):
    n = sum(COUNTS)
    x = _logps(1, n)
    P = len(COUNTS) // 2
    ref = None
    if not reference_free:
        ref = np.array([R.ordered_sum(s) for s in np.split(_logps(2, n), np.cumsum(COUNTS)[:-1])])
        if loss_type == "ipo":
            ref = ref / np.array(COUNTS, dtype=np.float64)
    kw = dict(beta=0.25, dpo_alpha=0.7, gamma=1.3)
    got = R.dpo(x, COUNTS, ref=ref, loss_type=loss_type, label_smoothing=eps, **kw)
    L, l, h, A = _autograd(x, COUNTS, ref, kw["beta"], kw["dpo_alpha"], kw["gamma"], loss_type, eps)
    tol = 1e-12 * (1 + np.abs(x.astype(np.float64)).sum())
    assert abs(got["L"] - L) <= tol * max(1.0, abs(L)) and np.allclose(got["loss"], l, rtol=1e-12, atol=1e-13) and np.allclose(got["h"], h, rtol=1e-12, atol=1e-13)
    assert np.allclose(got["coef"], A, rtol=1e-11, atol=1e-14)
    assert abs(got["L"] - (got["dpo_loss"] + kw["gamma"] * got["sft_loss"])) <= 1e-12 * max(1.0, abs(L))
    assert got["dpo_loss"] == pytest.approx(kw["dpo_alpha"] * got["loss"].mean(), rel=1e-13)
    # rewards, and the chosen / rejected split of the coefficient
    rho = np.zeros(2 * P) if ref is None else ref
    assert np.allclose(got["reward_c"], kw["beta"] * (got["pi_c"] - rho[:P])) and np.allclose(got["reward_r"], kw["beta"] * (got["pi_r"] - rho[P:]))
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    for b in range(2 * P):
        assert len(set(got["coef"][off[b]:off[b + 1]].tolist())) == 1            # one coefficient per sequence


def test_restatement_edges():
    # the documented order: an empty sequence sums to +0.0, a short one is its plain sum, 65 elements wrap into accumulator 0
    assert R.ordered_sum([]) == 0.0 and math.copysign(1.0, R.ordered_sum([])) == 1.0
    assert R.ordered_sum([1.5]) == 1.5
    x = _logps(3, 2049).astype(np.float64)
    assert abs(R.ordered_sum(x) - math.fsum(x)) <= 2.0 ** -52 * np.abs(x).sum()
    big = np.array([1e16, 1.0] + [0.0] * 62 + [-1e16])          # 1e16 + -1e16 meet in accumulator 0 before the 1.0 joins: order matters
    assert R.ordered_sum(big) == 1.0 and sum(big.tolist()) == 0.0
    # the stable log-sigmoid: finite at |h| = 800, and equal to log 2 at 0
    assert R.log_sigmoid(0.0) == -math.log(2.0) and R.log_sigmoid(800.0) == 0.0 and R.log_sigmoid(-800.0) == -800.0
    assert R.sigmoid(0.0) == 0.5 and R.sigmoid(-800.0) == 0.0 and R.sigmoid(800.0) == 1.0
    # self-reference: h = 0, loss = log 2, the coefficients of DESIGN 5e
    counts = (4, 2, 3, 5)
    x = _logps(4, sum(counts))
    sums = np.array([R.ordered_sum(s) for s in np.split(x, np.cumsum(counts)[:-1])])
    got = R.dpo(x, counts, ref=sums, beta=0.1)
    assert (got["h"] == 0).all() and (got["loss"] == math.log(2.0)).all() and (got["reward_c"] == 0).all()
    assert got["coef"][0] == 1.0 * 0.1 / (2 * 2) + 1.0 / 6 and got["coef"][-1] == -1.0 * 0.1 / (2 * 2)
    with pytest.raises(AssertionError, match="kink"):
        R.dpo(x, counts, ref=sums - np.array([10.0, 0, 0, 0]), beta=0.1, loss_type="hinge")          # h = 1 exactly


def test_terms_validation():
    T = PF.PreferenceTerms
    ok = T(ref_chosen_logps=[-1.0, -2.0], ref_rejected_logps=torch.tensor([-3.0, -4.0]), beta=0.1)
    P, seg, rho, a_P, g_N = ok.per_pair([3, 2, 4, 1])
    assert P == 2 and seg.dtype == np.int32 and seg.tolist() == [0, 3, 5, 9, 10] and rho.tolist() == [-1.0, -2.0, -3.0, -4.0]
    assert a_P == 0.5 and g_N == 1.0 / 5
    ipo = T(ref_chosen_logps=[-1.0, -2.0], ref_rejected_logps=[-3.0, -4.0], loss_type="ipo").per_pair([2, 2, 4, 1])
    assert ipo[2].tolist() == [-0.5, -1.0, -0.75, -4.0]                              # the reference's sums become means
    assert T(reference_free=True).per_pair([1, 1])[2] is None
    with pytest.raises(ValueError, match="pair 1: the chosen answer has no scored token"):
        ok.per_pair([3, 0, 4, 1])
    with pytest.raises(ValueError, match="pair 0: the rejected answer has no scored token"):
        ok.per_pair([3, 2, 0, 1])
    with pytest.raises(ValueError, match="2 P sequences"):
        ok.per_pair([3, 2, 1])
    with pytest.raises(ValueError, match="ref_rejected_logps: 1 entries for 2 pairs"):
        T(ref_chosen_logps=[-1.0, -2.0], ref_rejected_logps=[-3.0]).per_pair([3, 2, 4, 1])
    with pytest.raises(ValueError, match="ref_chosen_logps must be finite"):
        T(ref_chosen_logps=[-1.0, float("nan")], ref_rejected_logps=[-3.0, -4.0]).per_pair([3, 2, 4, 1])
    with pytest.raises(ValueError, match="reference_free"):
        T(ref_chosen_logps=[-1.0, -2.0]).per_pair([3, 2, 4, 1])
    for bad in (dict(beta=0.0), dict(beta=float("inf")), dict(beta=float("nan")), dict(label_smoothing=0.5), dict(label_smoothing=-0.1),
                dict(loss_type="kto_pair"), dict(loss_type="ipo", label_smoothing=0.1), dict(gamma=float("nan"))):
        with pytest.raises(ValueError):
            T(reference_free=True, **bad).per_pair([1, 1])


def test_concatenate_pairs_and_offsets_ragged():
    ci = np.array([[1, 5, 6, 7, 0], [1, 8, 9, 0, 0]])
    ri = np.array([[1, 5, 4], [1, 8, 3]])
    cl, rl = np.where(ci > 4, ci, -100), np.where(ri > 2, ri, -100)
    ids, am, lab = PF.concatenate_pairs(ci, ci != 0, cl, torch.tensor(ri), ri != 0, rl, pad_id=0)
    assert ids.shape == (4, 5) and ids.dtype == np.int64 and am.dtype == bool
    assert ids.tolist() == [[1, 5, 6, 7, 0], [1, 8, 9, 0, 0], [1, 5, 4, 0, 0], [1, 8, 3, 0, 0]]
    assert am.sum(1).tolist() == [4, 3, 3, 3] and (lab[2:, 3:] == -100).all() and lab[2].tolist() == [-100, 5, 4, -100, -100]
    ids2, _, _ = PF.concatenate_pairs(ri, ri != 0, rl, ci, ci != 0, cl, pad_id=9)          # the shorter half first
    assert ids2[:2, 3:].tolist() == [[9, 9], [9, 9]] and ids2[2:].tolist() == ci.tolist()
    with pytest.raises(ValueError, match="two halves"):
        PF.concatenate_pairs(ci, ci != 0, cl, ri[:1], ri[:1] != 0, rl[:1])
    with pytest.raises(ValueError, match="rejected"):
        PF.concatenate_pairs(ci, ci != 0, cl, ri, (ri != 0)[:, :2], rl)
    assert PF.pair_offsets([2, 0, 3]).tolist() == [0, 2, 2, 5] and PF.pair_offsets([2, 0, 3]).dtype == np.int32
    for bad in ([], [1, -1]):
        with pytest.raises(ValueError):
            PF.pair_offsets(bad)


class _Ids:
    def __init__(self, ids):
        self.input_ids = ids


class CharTok:
    """One id per character, BOS 1, </s> 2 (the v1 template's separator)."""
    bos_token_id, pad_token_id, model_max_length, legacy, padding_side = 1, 0, 2048, True, "right"

    def __call__(self, s, **kw):
        ids = [1]
        for k, piece in enumerate(s.split("</s>")):
            if k:
                ids.append(2)
            ids.extend(ord(c) for c in piece)
        return _Ids(ids)


RECORDS = [
    dict(prompt="Is there <image> a nodule?", chosen="Yes, in the left lung.", rejected="No.", image=[(torch.zeros(3, 4, 4), (40, 30), "image")]),
    dict(prompt="<image>\n<image>Describe.  ", chosen="Clear lungs.", rejected="Clear lungs, large heart, effusion.", image=[(torch.ones(3, 4, 4), (8, 8), "image")]),
    dict(prompt="Name the view.", chosen="PA", rejected="Lateral view", image=[(torch.zeros(2, 3, 4, 4), (100, 50), "image")]),
]


@pytest.mark.parametrize("template", ["v1", "qwen"])
def test_record_contract(golden_dir, template):
    from radvlm_amd.llava import conversation as conv_lib
    from radvlm_amd.llava.train import train as TR
    from radvlm_amd.llava.train.dpo_trainer import DPODataCollator, DPODataset
    if template == "qwen":
        sys.path.insert(0, golden_dir)
        import toy_chatml_tokenizer as T
        tok = T.build()
        tok.model_max_length = 2048
    else:
        tok = CharTok()
    assert PF.rewrite_prompt(RECORDS[0]["prompt"]) == "<image>\nIs there  a nodule?"
    assert PF.rewrite_prompt(RECORDS[1]["prompt"]) == "<image>\nDescribe." and PF.rewrite_prompt("Name the view.") == "<image>\nName the view."
    assert PF.make_conv("p", "a") == [{"from": "human", "value": "p"}, {"from": "gpt", "value": "a"}]
    ds = DPODataset(records=RECORDS, tokenizer=tok, data_args=SimpleNamespace(is_multimodal=True))
    assert len(ds) == 3 and ds.lengths == [PF.record_words(r) + 128 for r in RECORDS] and all(m > 0 for m in ds.modality_lengths)
    items = [ds[i] for i in range(3)]
    assert [it["index"] for it in items] == [0, 1, 2] and all(it["has_image"] and it["prompt"].startswith("<image>\n") for it in items)
    assert RECORDS[1]["prompt"] == "<image>\n<image>Describe.  "                    # the record itself is not modified
    saved = conv_lib.default_conversation
    conv_lib.default_conversation = conv_lib.conv_templates["v1" if template == "v1" else "qwen_1_5"]
    try:
        b = DPODataCollator(tokenizer=tok)(items)
        want = {k: [TR.preprocess([PF.make_conv(it["prompt"], it[k])], tok, has_image=True) for it in items] for k in ("chosen", "rejected")}
    finally:
        conv_lib.default_conversation = saved
    pad = tok.pad_token_id
    for k in ("chosen", "rejected"):
        ids, lab, am = b[f"{k}_input_ids"], b[f"{k}_labels"], b[f"{k}_attention_mask"]
        assert ids.shape == lab.shape == am.shape and ids.shape[0] == 3 and ids.shape[1] == max(w["input_ids"].shape[1] for w in want[k])
        for r, w in enumerate(want[k]):
            n = w["input_ids"].shape[1]
            assert ids[r, :n].tolist() == w["input_ids"][0].tolist() and lab[r, :n].tolist() == w["labels"][0].tolist()
            assert (ids[r, n:] == pad).all() and (lab[r, n:] == -100).all() and am[r].tolist() == (ids[r] != pad).tolist()
            assert (ids[r] == -200).sum() == 1 and (lab[r] != -100).sum() > 0          # one image mark, a scored answer
    # both halves share the prompt: identical up to the first answer token
    for r in range(3):
        first = int((b["chosen_labels"][r] != -100).nonzero()[0])
        assert b["chosen_input_ids"][r, :first].tolist() == b["rejected_input_ids"][r, :first].tolist()
    assert b["image_sizes"] == [(40, 30), (8, 8), (100, 50)] and b["modalities"] == ["image"] * 3 and b["indices"] == [0, 1, 2]
    assert [tuple(i.shape) for i in b["images"]] == [(3, 4, 4), (3, 4, 4), (2, 3, 4, 4)]
    with pytest.raises(ValueError, match="missing \\['rejected'\\]"):
        DPODataset(records=[dict(prompt="p", chosen="c")])
    with pytest.raises(NotImplementedError):
        DPODataset(records=[dict(prompt="p", chosen="c", rejected="r", video="v.mp4")])


def test_trainer_argument_checks():
    from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer
    from radvlm_amd.llava.train.train import parse_args_into_dataclasses
    from radvlm_amd.llava.train.train_dpo import DataArguments, DPOTrainingArguments, ModelArguments
    import dropin.llava.train.llava_trainer as D
    assert D.LLaVADPOTrainer is LLaVADPOTrainer
    model, args = SimpleNamespace(engine=None), SimpleNamespace(per_device_train_batch_size=1)
    with pytest.raises(ValueError, match="ref_model"):
        LLaVADPOTrainer(model=model, args=args, train_dataset=[])
    with pytest.raises(ValueError, match="policy itself"):
        LLaVADPOTrainer(model=model, ref_model=model, args=args, train_dataset=[])
    for bad in (dict(beta=0.0), dict(loss_type="kto_pair"), dict(label_smoothing=0.5), dict(loss_type="ipo", label_smoothing=0.1)):
        with pytest.raises(ValueError):
            LLaVADPOTrainer(model=model, args=args, train_dataset=[], reference_free=True, **bad)
    with pytest.raises(NotImplementedError, match="one rank"):
        LLaVADPOTrainer(model=model, args=SimpleNamespace(world_size=2), train_dataset=[], reference_free=True)
    for kw in (dict(reference_free=True), dict(precompute_ref_log_probs=True), dict(ref_model=SimpleNamespace())):
        t = LLaVADPOTrainer(model=model, args=args, train_dataset=[], **kw)
        assert t.terms == dict(beta=0.1, dpo_alpha=1.0, gamma=1.0, loss_type="sigmoid", label_smoothing=0.0)
    # the reference's argument names and defaults, on top of train.py's parser
    _, _, a = parse_args_into_dataclasses(["--beta", "0.2", "--precompute_ref_log_probs", "True", "--learning_rate", "5e-7"],
                                          (ModelArguments, DataArguments, DPOTrainingArguments))
    assert (a.dpo_alpha, a.beta, a.gamma, a.precompute_ref_log_probs, a.generate_during_eval, a.learning_rate) == (1.0, 0.2, 1.0, True, False, 5e-7)
    # the library's source list and the header carry the new entry points
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from radvlm_amd import lib
    build = open(os.path.join(root, "radvlm_amd", "csrc", "build.sh")).read()
    assert "preference" in build.split('SRCS="')[1].split('"')[0].split()
    assert {"rv_seq_logp_sums_f64", "rv_dpo_pairs_f64"} <= set(lib.SIGNATURES)

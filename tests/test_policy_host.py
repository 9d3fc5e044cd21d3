"""Host checks of GRPO training's planning (radvlm_amd.policy, radvlm_amd.rewards) and of the float64 kernel reference (tests/policy_ref.py),
which is pinned here to float64 autograd of the formula as written: torch.minimum, clamp and logsumexp.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import policy_ref as P
from radvlm_amd.data.create_instructions import format_boxes
from radvlm_amd.policy import PolicyTerms, assemble, group_advantages, sample_seeds, token_weights
from radvlm_amd.rewards import box_iou_reward, parse_boxes

V, ROWS = 11, 9
EPS_LO, EPS_HI = 0.2, 0.28


def _case(beta, with_old=True):
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(ROWS, V, generator=g) * 2).to(torch.bfloat16)
    labels = torch.tensor([0, 10, 3, 4, 5, 6, -100, 7, 2])
    adv = torch.tensor([1.0, -0.7, 2.0, -1.5, -0.5, 0.8, float("nan"), 0.0, 1.2], dtype=torch.float64)
    ratio = torch.tensor([1.0, 0.9, 1.5, 1.5, 0.5, 0.5, float("nan"), 1.1, 1.1], dtype=torch.float64)
    w = torch.tensor([0.1, 0.2, 0.3, 0.1, 0.05, 0.4, float("nan"), 0.25, 0.15], dtype=torch.float64)
    logp = torch.log_softmax(z.double(), -1)[torch.arange(ROWS), labels.clamp_min(0)]
    old = (logp - ratio.log()) if with_old else None
    ref = logp - torch.tensor([-0.3, 0.0, 0.5, -0.3, 0.0, 0.5, float("nan"), -0.3, 0.5], dtype=torch.float64) if beta > 0 else None
    return z, labels, adv, w, old, ref


@pytest.mark.parametrize("with_old", [True, False])
@pytest.mark.parametrize("beta", [0.0, 0.04])
def test_reference_is_autograd_of_the_formula(beta, with_old):
    z, labels, adv, w, old, ref = _case(beta, with_old)
    gw = w * 0.5
    out = P.policy_loss(z, labels, V, adv, w, gw, old, ref, EPS_LO, EPS_HI, beta)
    live = labels >= 0
    zl = z.double()[live].clone().requires_grad_(True)
    y = labels[live]
    logp = zl.gather(1, y[:, None])[:, 0] - torch.logsumexp(zl, -1)
    A = adv[live]
    r = torch.exp(logp - old[live]) if with_old else torch.exp(logp - logp.detach())
    loss = -torch.minimum(r * A, r.clamp(1 - EPS_LO, 1 + EPS_HI) * A)
    if beta > 0:
        q = ref[live] - logp
        kl = torch.exp(q) - q - 1
        loss = loss + beta * kl
        assert torch.allclose(out["kl"][live], kl.detach(), rtol=0, atol=1e-12)
    (gw[live] * loss).sum().backward()
    assert torch.allclose(out["logp"][live], logp.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(out["loss"][live], loss.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(out["wloss"][live], (w[live] * loss).detach(), rtol=0, atol=1e-12)
    assert torch.allclose(out["grad"][live], zl.grad, rtol=0, atol=1e-12)
    for k in ("logp", "loss", "wloss", "kl", "clip"):
        assert float(out[k][6]) == 0.0                                   # the ignored row, whose floats are NaN
    assert float(out["grad"][6].abs().max()) == 0.0 and float(out["A"][6].abs().max()) == 0.0
    want_clip = [0, 0, 2, 0, 1, 0, 0, 0, 0] if with_old else [0] * ROWS
    assert out["clip"].tolist() == [float(c) for c in want_clip]
    if beta == 0:
        for row in range(ROWS):
            if want_clip[row] or row == 7:                               # clipped rows and the A = 0 row: an all-zero gradient
                assert float(out["grad"][row].abs().max()) == 0.0
    assert bool((out["A"] >= out["grad"].abs() - 1e-15).all())


def test_reference_rejects_a_row_on_a_clip_edge():
    z, labels, adv, w, old, _ = _case(0.0)
    logp = torch.log_softmax(z.double(), -1)[torch.arange(ROWS), labels.clamp_min(0)]
    for edge in (1 - EPS_LO + 5e-4, 1 + EPS_HI - 5e-4):
        bad = old.clone()
        bad[1] = logp[1] - np.log(edge)
        with pytest.raises(AssertionError, match="clip edge"):
            P.policy_loss(z, labels, V, adv, w, w, bad, None, EPS_LO, EPS_HI, 0.0)


# ------------------------------------------------------------------------------------------------ advantages, weights
def test_group_advantages_hand_values():
    r = [1.0, 2.0, 3.0, 6.0, 2.0, 2.0, 2.0, 2.0]
    a = group_advantages(r, 4)
    s0 = np.sqrt(((np.array(r[:4]) - 3.0) ** 2).sum() / 3)               # ddof = 1
    np.testing.assert_allclose(a[:4], (np.array(r[:4]) - 3.0) / (s0 + 1e-4), rtol=1e-15)
    assert a[4:].tolist() == [0.0] * 4                                   # a zero-std group
    b = group_advantages(r, 4, "batch")
    sb = np.std(r, ddof=1)
    np.testing.assert_allclose(b[:4], (np.array(r[:4]) - 3.0) / (sb + 1e-4), rtol=1e-15)
    assert b[4:].tolist() == [0.0] * 4
    n = group_advantages(r, 4, "none")
    assert n.tolist() == [-2.0, -1.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0]
    assert group_advantages([0.0, 1.0], 2).tolist() == pytest.approx([-0.5 / (np.sqrt(0.5) + 1e-4), 0.5 / (np.sqrt(0.5) + 1e-4)])
    for bad in (dict(rewards=r, num_generations=1), dict(rewards=r, num_generations=3), dict(rewards=[1.0, float("nan")], num_generations=2),
                dict(rewards=[1.0, float("inf")], num_generations=2), dict(rewards=r, num_generations=4, scale_rewards="std"),
                dict(rewards=[], num_generations=2)):
        with pytest.raises(ValueError):
            group_advantages(**bad)


def test_token_weights_rules_sum_as_stated():
    n = [3, 0, 5, 2]
    N = len(n)
    w = token_weights(n, "grpo")
    assert w[1] == 0.0 and w.tolist() == [1 / (N * 3), 0.0, 1 / (N * 5), 1 / (N * 2)]
    assert sum(w[i] * n[i] for i in range(N)) == pytest.approx(3 / N)    # every live sequence contributes 1 / N
    for lt in ("dapo", "bnpo"):
        w = token_weights(n, lt)
        assert w[1] == 0.0 and sum(w[i] * n[i] for i in range(N)) == pytest.approx(1.0)
        assert w[0] == w[2] == w[3] == 1 / 10
    w = token_weights(n, "dr_grpo", max_completion_length=8)
    assert w.tolist() == [1 / 32, 0.0, 1 / 32, 1 / 32]
    assert sum(w[i] * n[i] for i in range(N)) == pytest.approx(10 / 32)
    assert token_weights([0, 0], "dapo").tolist() == [0.0, 0.0]
    for bad in (dict(lengths=n, loss_type="sum"), dict(lengths=n, loss_type="dr_grpo"), dict(lengths=[], loss_type="grpo"),
                dict(lengths=[1, -1], loss_type="grpo")):
        with pytest.raises(ValueError):
            token_weights(**bad)


def test_assemble_and_sample_seeds():
    ids, am, lab = assemble([[5, -200, 6], [7]], [[8, 9, 2], [3, 2, 4, 4, 2]], pad_id=0)
    assert ids.tolist() == [[5, -200, 6, 8, 9, 2], [7, 3, 2, 4, 4, 2]] and ids.dtype == np.int64
    assert am.tolist() == [[True] * 6, [True] * 6]
    assert lab.tolist() == [[-100, -100, -100, 8, 9, 2], [-100, 3, 2, 4, 4, 2]]
    ids, am, lab = assemble([[5, 6], [7]], [[8], []], pad_id=1)
    assert ids.tolist() == [[5, 6, 8], [7, 1, 1]] and am.tolist() == [[True, True, True], [True, False, False]]
    assert lab.tolist() == [[-100, -100, 8], [-100, -100, -100]]
    with pytest.raises(ValueError):
        assemble([[1]], [[2], [3]], 0)
    with pytest.raises(ValueError):
        assemble([[]], [[2]], 0)
    assert sample_seeds(100, 0, 2, 3) == [100, 101, 102, 103, 104, 105]
    assert sample_seeds(100, 2, 2, 3) == [112, 113, 114, 115, 116, 117]
    assert sample_seeds((1 << 63) - 6, 0, 2, 3)[-1] == (1 << 63) - 1
    for bad in ((-1, 0, 1, 2), ((1 << 63) - 5, 0, 2, 3), (0, -1, 1, 2), (0, 0, 0, 2)):
        with pytest.raises(ValueError):
            sample_seeds(*bad)


def test_policy_terms_validation():
    counts = [3, 0, 2]
    adv, w, old, ref = PolicyTerms(advantages=[1.0, 2.0, -1.0]).per_token(counts)
    assert adv.tolist() == [1.0, 1.0, 1.0, -1.0, -1.0] and w.tolist() == [0.2] * 5 and old is None and ref is None
    adv, w, old, ref = PolicyTerms(advantages=[np.array([1.0, 2.0, 3.0]), np.zeros(0), np.array([4.0, 5.0])], weights=np.arange(5) / 10.0,
                                   old_logps=[-np.ones(3), np.zeros(0), -np.ones(2)], ref_logps=torch.full((5,), -2.0), beta=0.1).per_token(counts)
    assert adv.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and w.tolist() == [0.0, 0.1, 0.2, 0.3, 0.4]
    assert old.tolist() == [-1.0] * 5 and ref.tolist() == [-2.0] * 5
    with pytest.raises(ValueError, match="sample 2"):
        PolicyTerms(advantages=[np.ones(3), np.zeros(0), np.ones(1)]).per_token(counts)
    with pytest.raises(ValueError, match="sample 2"):
        PolicyTerms(advantages=[1.0, 1.0, 1.0], weights=np.ones(4)).per_token(counts)
    with pytest.raises(ValueError, match="old_logps"):
        PolicyTerms(advantages=[1.0, 1.0, 1.0], old_logps=-np.ones(3)).per_token(counts)
    for bad in (dict(advantages=[1.0, float("nan"), 1.0]), dict(advantages=[1.0, 1.0]), dict(advantages=[1.0] * 3, epsilon=-0.1),
                dict(advantages=[1.0] * 3, epsilon_high=float("inf")), dict(advantages=[1.0] * 3, beta=-1.0),
                dict(advantages=[1.0] * 3, beta=0.1), dict(advantages=[1.0] * 3, weights=[-1.0, 1.0, 1.0]),
                dict(advantages=[1.0] * 3, old_logps=np.full(5, 0.5)), dict(advantages=[1.0] * 3, ref_logps=np.full(5, float("-inf")), beta=0.1)):
        with pytest.raises(ValueError):
            PolicyTerms(**bad).per_token(counts)
    assert PolicyTerms(advantages=[0.0], epsilon=0.1).eps_high == 0.1 and PolicyTerms(advantages=[0.0], epsilon_high=0.3).eps_high == 0.3


# ------------------------------------------------------------------------------------------------ rewards
def test_parse_boxes_inverts_format_boxes(golden_dir):
    G = json.load(open(os.path.join(golden_dir, "instruction_generators.json"), encoding="utf-8"))
    n = 0
    for rec in G["format_boxes"]:
        boxes, nf = rec["args"][0], rec["kwargs"].get("num_float", 2)
        text = format_boxes(boxes, nf)
        got = parse_boxes(text, nf)
        assert got == [[round(v, nf) for v in b] for b in boxes], (text, got)      # b, as far as the string holds it
        assert format_boxes(got, nf) == text
        n += 1
    assert n >= 6
    b = [[0.1, 0.25, 0.5, 0.75], [0.0, 0.05, 1.0, 0.4]]
    assert parse_boxes(format_boxes(b)) == b
    for bad in ("", "[0.1, 0.2, 0.3]", "[0.1, 0.2, 0.3, 0.4] ", " [0.1, 0.2, 0.3, 0.4]", "[0.1,0.2,0.3,0.4]", "[0.10, 0.2, 0.3, 0.4]",
                "[0.1, 0.2, 0.3, 1.5]", "[0.1, 0.2, 0.3, 0.4], [0.1, 0.2, 0.3, 0.4]", "[0.1, 0.2, 0.3, 0.4] and", "[0.1, 0.2, 0.3, 0.123]",
                "[.1, 0.2, 0.3, 0.4]", "the box is [0.1, 0.2, 0.3, 0.4]", "[0.1, 0.2, 0.3, 0.4, 0.5]", "[1, 0.2, 0.3, 0.4]", None, 7):
        assert parse_boxes(bad) is None, bad


def test_box_iou_reward_hand_cases():
    t = [[0.0, 0.0, 0.5, 0.5]]
    r = box_iou_reward(completions=["[0.0, 0.0, 0.5, 0.5]", "[0.0, 0.0, 0.5, 0.25]", "[0.5, 0.5, 1.0, 1.0]", "no box", "[0.0, 0.0, 0.5, 0.5] and [0.5, 0.5, 1.0, 1.0]"],
                       boxes=[t] * 5, prompts=None, completion_ids=None)
    assert r == [1.0, 0.5, 0.0, 0.0, 0.5]
    # two true boxes; the greedy match takes the best pair first: pred 0 ~ true 1 (IoU 1), then pred 1 ~ true 0 (IoU 0.5)
    truth = [[0.0, 0.0, 0.5, 0.25], [0.5, 0.5, 1.0, 1.0]]
    r = box_iou_reward(completions=["[0.5, 0.5, 1.0, 1.0] and [0.0, 0.0, 0.5, 0.5]", "[0.5, 0.5, 1.0, 1.0]"], boxes=[truth, truth])
    assert r == [pytest.approx(0.75), pytest.approx(0.5)]
    assert box_iou_reward(completions=["[0.5, 0.5, 0.5, 1.0]"], boxes=[t]) == [0.0]        # a degenerate box
    assert box_iou_reward(completions=["[0.0, 0.0, 0.5, 0.5]"], boxes=[[]]) == [0.0]

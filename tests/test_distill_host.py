"""Host checks of knowledge distillation's planning (radvlm_amd.distill), of GKDTrainer's argument validation and of the float64 kernel
reference (tests/distill_ref.py), which is pinned here to float64 autograd of TRL's generalized_jsd_loss written out literally:
log_softmax, logsumexp of the stacked mixture, kl_div(log_target=True).  Negative controls show that the kernel tests' gates are not
vacuous: a reference with a slightly different beta or temperature, or the neighbouring special case, fails them.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_ref as D
from radvlm_amd.distill import DistillTerms, check_same_scored, on_policy_step, step_uniform
from rowops_ref import ratios

VS = (8, 9, 2049, 32003)
BETAS = (0.0, 0.1, 0.5, 0.9, 1.0)
TAUS = (0.5, 1.0, 2.0)
INDEPENDENT = (0, 3, 4, 7, 8)             # rows whose teacher is drawn independently of the student (row 3: the dominant pair)


def _trl_generalized_jsd(student_logits, teacher_logits, beta, temperature):
    """trl.GKDTrainer.generalized_jsd_loss, reduction per token (the sum over the vocabulary)."""
    student_logits, teacher_logits = student_logits / temperature, teacher_logits / temperature
    student_log_probs, teacher_log_probs = F.log_softmax(student_logits, dim=-1), F.log_softmax(teacher_logits, dim=-1)
    if beta == 0:
        jsd = F.kl_div(student_log_probs, teacher_log_probs, reduction="none", log_target=True)
    elif beta == 1:
        jsd = F.kl_div(teacher_log_probs, student_log_probs, reduction="none", log_target=True)
    else:
        b = torch.tensor(beta, dtype=student_log_probs.dtype)
        mixture_log_probs = torch.logsumexp(torch.stack([student_log_probs + torch.log1p(-b), teacher_log_probs + torch.log(b)]), dim=0)
        kl_teacher = F.kl_div(mixture_log_probs, teacher_log_probs, reduction="none", log_target=True)
        kl_student = F.kl_div(mixture_log_probs, student_log_probs, reduction="none", log_target=True)
        jsd = b * kl_teacher + (1 - b) * kl_student
    return jsd.sum(-1)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("V", (8, 9, 2049))
def test_reference_is_autograd_of_trl_formula(V, beta, tau):
    z, u, labels, lw, gw = D.make_inputs(V)
    out = D.distill_loss(z, u, labels, V, lw, gw, beta, tau)
    live = labels >= 0
    zl = z.double()[live].clone().requires_grad_(True)
    L = _trl_generalized_jsd(zl, u.double()[live], beta, tau)
    (gw.double()[live] * L).sum().backward()
    assert torch.allclose(out["jsd"][live], L.detach(), rtol=1e-9, atol=1e-13)
    assert torch.allclose(out["wloss"][live], (lw.double()[live] * L).detach(), rtol=1e-9, atol=1e-13)
    scale = zl.grad.abs().amax(-1, keepdim=True)
    assert bool(((out["grad"][live] - zl.grad).abs() <= 1e-9 * scale + 1e-15).all())     # the floor: float64 rounding where the row's gradient cancels to 0
    if beta == 0:
        assert torch.equal(out["kl_teacher"], out["jsd"]) and float(out["kl_student"].abs().max()) == 0.0
    elif beta == 1:
        assert torch.equal(out["kl_student"], out["jsd"]) and float(out["kl_teacher"].abs().max()) == 0.0
    else:
        assert torch.allclose(out["jsd"], beta * out["kl_teacher"] + (1 - beta) * out["kl_student"], rtol=1e-12, atol=0)
    for k in ("jsd", "wloss", "kl_teacher", "kl_student"):
        assert float(out[k][D.IGNORED]) == 0.0                            # the ignored row, whose floats are NaN
    assert float(out["grad"][D.IGNORED].abs().max()) == 0.0 and float(out["A"][D.IGNORED].abs().max()) == 0.0
    assert float(out["grad"][D.ZERO_WEIGHT].abs().max()) == 0.0
    assert float(out["grad"][D.SAME].abs().max()) <= 1e-16 and abs(float(out["jsd"][D.SAME])) <= 1e-15
    assert bool((out["A"] >= out["grad"].abs() * (1 - 1e-12)).all())
    assert bool(torch.isfinite(out["grad"]).all() and torch.isfinite(out["jsd"]).all())


def test_reference_keeps_the_discontinuity_at_the_end_points():
    """beta 0 and 1 are TRL's special cases (a full KL), not the limits of the middle formula, which tends to 0 at both ends."""
    z, u, labels, lw, gw = D.make_inputs(9)
    near0, near1 = D.distill_loss(z, u, labels, 9, lw, gw, 1e-9, 1.0), D.distill_loss(z, u, labels, 9, lw, gw, 1 - 1e-9, 1.0)
    at0, at1 = D.distill_loss(z, u, labels, 9, lw, gw, 0.0, 1.0), D.distill_loss(z, u, labels, 9, lw, gw, 1.0, 1.0)
    assert float(near0["jsd"][0]) < 1e-6 and float(near1["jsd"][0]) < 1e-6 and float(at0["jsd"][0]) > 0.1 and float(at1["jsd"][0]) > 0.1


def test_reference_is_finite_for_log_ratios_of_two_hundred():
    z = torch.zeros(1, 16, dtype=torch.bfloat16)
    u = torch.zeros(1, 16, dtype=torch.bfloat16)
    z[0, 2], u[0, 5] = 100.0, 100.0
    one = torch.ones(1)
    for beta in BETAS:
        out = D.distill_loss(z, u, torch.tensor([0]), 16, one, one, beta, 0.5)       # |d| = 200 at columns 2 and 5
        assert bool(torch.isfinite(out["grad"]).all() and torch.isfinite(out["jsd"]).all() and torch.isfinite(out["A"]).all())
        assert float(out["jsd"][0]) > 0


@pytest.mark.parametrize("V", (8, 2049, 32003))
def test_the_gates_reject_a_neighbouring_objective(V):
    """The gradient gate separates beta 0.5 from 0.45, the middle formula from either special case, and temperature 1 from 1.05, on
    every row whose teacher is independent of the student."""
    z, u, labels, lw, gw = D.make_inputs(V)
    ref = lambda beta, tau: D.distill_loss(z, u, labels, V, lw, gw, beta, tau)
    for (b0, t0), (b1, t1) in (((0.5, 1.0), (0.45, 1.0)), ((0.0, 1.0), (0.1, 1.0)), ((1.0, 1.0), (0.9, 1.0)), ((0.5, 1.0), (0.5, 1.05)),
                               ((0.0, 1.0), (0.0, 1.05))):
        want, other = ref(b0, t0), ref(b1, t1)
        worst = ratios(other["grad"], want["grad"], want["A"]).amax(-1)
        for r in INDEPENDENT:
            assert float(worst[r]) > 1.0, (V, (b0, t0), (b1, t1), r, float(worst[r]))
        assert float(ratios(want["grad"], want["grad"], want["A"]).max()) == 0.0


# ------------------------------------------------------------------------------------------------ terms
def _bf16(n, v):
    return torch.zeros(n, v, dtype=torch.bfloat16)


def test_distill_terms_validation():
    counts = [3, 0, 2]
    w = DistillTerms(teacher_logits=_bf16(5, 16)).per_token(counts, 11)
    assert w.tolist() == [0.2] * 5
    w = DistillTerms(teacher_logits=_bf16(5, 11), weights=[1.0, 2.0, 0.5], beta=0.0, temperature=2.0).per_token(counts, 11)
    assert w.tolist() == [1.0, 1.0, 1.0, 0.5, 0.5]
    w = DistillTerms(teacher_logits=_bf16(5, 11), weights=np.arange(5) / 10.0, beta=1.0).per_token(counts, 11)
    assert w.tolist() == [0.0, 0.1, 0.2, 0.3, 0.4]
    assert DistillTerms(teacher_logits=_bf16(0, 11)).per_token([0, 0], 11).size == 0
    DistillTerms(teacher_logits=_bf16(5, 11), teacher_scored=[3, 0, 2]).per_token(counts, 11)
    with pytest.raises(ValueError, match="sample 2"):
        DistillTerms(teacher_logits=_bf16(5, 11), teacher_scored=[3, 0, 1]).per_token(counts, 11)
    with pytest.raises(ValueError, match="samples"):
        check_same_scored([1, 2], [1, 2, 3])
    for bad in (dict(beta=-0.1), dict(beta=1.1), dict(beta=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float("inf")), dict(temperature=float("nan"))):
        with pytest.raises(ValueError):
            DistillTerms(teacher_logits=_bf16(5, 11), **bad)
    for bad in (dict(teacher_logits=_bf16(4, 11)), dict(teacher_logits=_bf16(5, 10)), dict(teacher_logits=torch.zeros(5, 11)),
                dict(teacher_logits=_bf16(5, 11).reshape(5, 11, 1)), dict(teacher_logits=None), dict(teacher_logits=_bf16(5, 11), weights=[-1.0, 1.0, 1.0]),
                dict(teacher_logits=_bf16(5, 11), weights=np.ones(4)), dict(teacher_logits=_bf16(5, 11), weights=[1.0, float("nan"), 1.0])):
        with pytest.raises(ValueError):
            DistillTerms(**bad).per_token(counts, 11)


def test_on_policy_draw_is_a_function_of_seed_and_step():
    u = [step_uniform(42, s) for s in range(1, 10001)]
    assert u == [step_uniform(42, s) for s in range(1, 10001)] and all(0.0 < x < 1.0 for x in u)
    assert len(set(u)) == len(u) and u[:50] != [step_uniform(43, s) for s in range(1, 51)]
    for lmbda in (0.1, 0.5, 0.9):
        n = 10000
        hits = sum(on_policy_step(7, s, lmbda) for s in range(1, n + 1))
        assert abs(hits - n * lmbda) <= 3 * math.sqrt(n * lmbda * (1 - lmbda)), (lmbda, hits)
    assert not any(on_policy_step(7, s, 0.0) for s in range(1, 10001)) and all(on_policy_step(7, s, 1.0) for s in range(1, 10001))
    assert [on_policy_step(7, s, 0.5) for s in range(1, 6)] == [step_uniform(7, s) < 0.5 for s in range(1, 6)]
    for bad in (dict(seed=-1, step=0, lmbda=0.5), dict(seed=0, step=-1, lmbda=0.5), dict(seed=0, step=0, lmbda=1.5), dict(seed=0, step=0, lmbda=-0.1),
                dict(seed=0, step=0, lmbda=float("nan"))):
        with pytest.raises(ValueError):
            on_policy_step(**bad)
    assert 0.0 < step_uniform((1 << 63) - 1, 1 << 40) < 1.0


# ------------------------------------------------------------------------------------------------ the trainer's arguments
def _fake_model(vocab=64, lora=False, adapter_decoding=False):
    engine = SimpleNamespace(vocab=vocab, lora=dict(r=8) if lora else None, adapter_decoding=adapter_decoding, master=None, state_bits=32)
    return SimpleNamespace(engine=engine, config=SimpleNamespace())


def _args(**kw):
    return SimpleNamespace(**dict(dict(per_device_train_batch_size=2, learning_rate=1e-4, max_steps=1, seed=0), **kw))


def test_gkd_trainer_argument_validation():
    from radvlm_amd.llava.train.gkd_trainer import GKDTrainer
    import dropin.llava.train.gkd_trainer as shim
    assert shim.GKDTrainer is GKDTrainer
    data = [dict(prompt_ids=[1, 2], completion_ids=[3, 4])]
    t = GKDTrainer(_fake_model(), _fake_model(), _args(), data)
    assert (t.lmbda, t.beta, t.temperature, t.max_new_tokens) == (0.5, 0.5, 0.9, 128)            # TRL's defaults
    t = GKDTrainer(model=_fake_model(), teacher_model=_fake_model(), args=_args(lmbda=0.0, beta=1.0, temperature=2.0, max_new_tokens=7),
                   train_dataset=data)
    assert (t.lmbda, t.beta, t.temperature, t.max_new_tokens) == (0.0, 1.0, 2.0, 7)
    with pytest.raises(NotImplementedError, match="seq_kd"):
        GKDTrainer(_fake_model(), _fake_model(), _args(seq_kd=True), data)
    with pytest.raises(NotImplementedError, match="one rank"):
        GKDTrainer(_fake_model(), _fake_model(), _args(world_size=2), data)
    with pytest.raises(NotImplementedError, match="enable_adapter_decoding"):
        GKDTrainer(_fake_model(lora=True), _fake_model(), _args(), data)
    GKDTrainer(_fake_model(lora=True), _fake_model(), _args(lmbda=0.0), data)               # no sampling: the adapters may stay unmerged
    GKDTrainer(_fake_model(lora=True, adapter_decoding=True), _fake_model(), _args(), data)
    with pytest.raises(ValueError, match="vocabulary"):
        GKDTrainer(_fake_model(), _fake_model(vocab=65), _args(), data)
    with pytest.raises(ValueError, match="teacher_model"):
        GKDTrainer(_fake_model(), None, _args(), data)
    for bad in (dict(lmbda=1.5), dict(lmbda=-0.1), dict(beta=1.5), dict(beta=float("nan")), dict(temperature=0.0), dict(temperature=float("inf")),
                dict(max_new_tokens=0)):
        with pytest.raises(ValueError):
            GKDTrainer(_fake_model(), _fake_model(), _args(**bad), data)

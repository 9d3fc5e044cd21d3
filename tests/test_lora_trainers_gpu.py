"""GPU tests of GRPO and DPO on LoRA adapters: rollouts on the live adapters (model.enable_adapter_decoding()) and the reference taken
from the same model with the adapters switched off (model.disable_adapter()) -- no second copy of the model.  With peft's initial
B = 0 the policy and its reference run the same arithmetic, so step 1 logs kl == 0.0 / a zero margin exactly."""
import math

import pytest
import torch

from test_dpo_trainer_gpu import PairSet, _args as _dpo_args, _bits, _collate, _strip
from test_generate_gpu import _load, _model as _plain_model
from test_lora_merge_gpu import _model
from test_policy_gpu import _args as _grpo_args, _dataset, _even_fraction, _strip_times

pytestmark = pytest.mark.gpu
LORA = dict(r=8, alpha=16, dropout=0.0)


def _adapters(eng):
    return torch.cat([eng.lm.view(n).reshape(-1) for n in eng.lm.names() if ".lora_" in n]).clone()


def test_grpo_on_live_adapters_with_the_adapters_off_as_reference(golden_dir):
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    g, images, sizes, kw = _load(golden_dir, "toy")
    data = _dataset(g, images, sizes)
    args = dict(beta=0.04, loss_type="grpo", learning_rate=3e-3)
    with pytest.raises(NotImplementedError, match="merge_and_unload"):
        GRPOTrainer(_model("toy", lora=dict(LORA)), _grpo_args(), data, _even_fraction)
    with pytest.raises(ValueError, match="ref_model"):
        GRPOTrainer(_model("toy", lora=dict(LORA)), _grpo_args(**args), data, _even_fraction)          # no switch: as before
    with pytest.raises(ValueError, match="ref_model"):
        GRPOTrainer(_plain_model("toy", kw), _grpo_args(**args), data, _even_fraction)

    def run(steps):
        model = _model("toy", lora=dict(LORA)).enable_adapter_decoding().train()
        eng = model.engine
        base0, ad0 = eng.base.flat.clone(), _adapters(eng)
        state = GRPOTrainer(model, _grpo_args(max_steps=steps, **args), data, _even_fraction).train()
        torch.cuda.synchronize()
        assert torch.equal(_bits(eng.base.flat), _bits(base0)) and not eng.adapters_off and eng.opt_step == steps
        return _strip_times(state["log_history"]), _adapters(eng), ad0

    (one,), ad1, ad0 = run(1)
    assert one["kl"] == 0.0 and one["clip_ratio/low"] == one["clip_ratio/high"] == 0.0      # policy and reference: the same bits
    assert not torch.equal(_bits(ad1), _bits(ad0))                                           # step 1 moved the adapters, and only them
    (la, wa, _), (lb, wb, _) = run(2), run(2)
    assert la == lb and len(la) == 2 and la[0] == one and torch.equal(_bits(wa), _bits(wb))
    assert la[1]["kl"] > 0.0                                                                  # away from the frozen base


def _dpo_run(golden_dir, ref, **kw):
    from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer
    model = _model("toy", lora=dict(LORA)).train()
    data = PairSet(golden_dir, model.engine.vocab)
    trainer = LLaVADPOTrainer(model=model, ref_model=_plain_model("toy", {}) if ref else None, args=_dpo_args(max_steps=2), train_dataset=data,
                              data_collator=_collate, **kw)
    state = trainer.train()
    torch.cuda.synchronize()
    return model, _strip(state["log_history"]), trainer


def test_dpo_with_the_adapters_off_as_reference(golden_dir):
    from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer
    model, log, trainer = _dpo_run(golden_dir, False, reference_adapters_off=True)
    first = log[0]
    assert first["rewards/margins"] == 0.0 and first["rewards/chosen"] == 0.0 and first["dpo_loss"] == math.log(2.0)
    assert any(rec["rewards/margins"] != 0.0 for rec in log[1:]) and not model.engine.adapters_off
    # an explicit reference model holding the same base weights without adapters: the same first step (test_dpo_trainer_gpu's gate for
    # its explicit-reference case: the log records are equal)
    _, log_ref, _ = _dpo_run(golden_dir, True)
    print("dpo reference_adapters_off:", log, "explicit reference:", log_ref)
    assert log_ref[0] == first
    # without the new argument every refusal stands; with it, a model without adapters or a second reference is refused
    data = PairSet(golden_dir, model.engine.vocab)
    with pytest.raises(ValueError, match="ref_model"):
        LLaVADPOTrainer(model=model, ref_model=None, args=_dpo_args(), train_dataset=data, data_collator=_collate)
    with pytest.raises(ValueError, match="reference_adapters_off"):
        LLaVADPOTrainer(model=_plain_model("toy", {}), ref_model=None, args=_dpo_args(), train_dataset=data, data_collator=_collate,
                        reference_adapters_off=True)
    with pytest.raises(ValueError, match="reference_adapters_off"):
        LLaVADPOTrainer(model=model, ref_model=_plain_model("toy", {}), args=_dpo_args(), train_dataset=data, data_collator=_collate,
                        reference_adapters_off=True)

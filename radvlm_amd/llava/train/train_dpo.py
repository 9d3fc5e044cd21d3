"""Entry point of DPO preference training: train.py's setup (model, tokenizer, image processor, auto-resume, the final save) with the
reference's DPO arguments (train_dpo.py:137-168: dpo_alpha, beta, gamma, precompute_ref_log_probs, generate_during_eval) on top of
train.py's parser, DPODataset / DPODataCollator in the supervised data module's place and LLaVADPOTrainer in LLaVATrainer's.

The reference model is a second copy of the starting weights (train_dpo.py builds ref_model the same way), or -- with
--precompute_ref_log_probs, and always for LoRA runs, whose freshly initialised adapter is the identity -- the policy's own initial
weights, scored once before the first update."""
from dataclasses import dataclass

from .dpo_trainer import DPODataCollator, DPODataset, LLaVADPOTrainer
from .train import DataArguments, ModelArguments, TrainingArguments, train as _train


@dataclass
class DPOTrainingArguments(TrainingArguments):
    dpo_alpha: float = 1.0
    beta: float = 0.1
    gamma: float = 1.0
    generate_during_eval: bool = False      # accepted, ignored: there is no evaluation loop
    precompute_ref_log_probs: bool = False
    loss_type: str = "sigmoid"              # TRL DPOTrainer arguments the reference leaves at their defaults
    label_smoothing: float = 0.0
    reference_free: bool = False


def make_dpo_data_module(tokenizer, data_args):
    """train_dpo.py:1308-1311."""
    return DPODataset(tokenizer=tokenizer, data_path=data_args.data_path, data_args=data_args)


def _make_trainer(model, tokenizer, data_args, a, new_model):
    precompute = bool(a.precompute_ref_log_probs) or bool(a.lora_enable and not a.reference_free)
    ref = None if (precompute or a.reference_free) else new_model()
    return LLaVADPOTrainer(model=model, ref_model=ref, args=a, dpo_alpha=a.dpo_alpha, beta=a.beta, gamma=a.gamma,
                           train_dataset=make_dpo_data_module(tokenizer, data_args), data_collator=DPODataCollator(tokenizer=tokenizer),
                           tokenizer=tokenizer, precompute_ref_log_probs=precompute, loss_type=a.loss_type, label_smoothing=a.label_smoothing,
                           reference_free=a.reference_free)


def train(attn_implementation=None, argv=None, tokenizer=None):
    return _train(attn_implementation=attn_implementation, argv=argv, tokenizer=tokenizer,
                  arg_groups=(ModelArguments, DataArguments, DPOTrainingArguments), make_trainer=_make_trainer)


if __name__ == "__main__":
    train()

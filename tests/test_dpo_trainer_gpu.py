"""GPU tests of LLaVADPOTrainer on a four-pair toy set (the toy golden's rows as chosen answers, token-shifted shorter copies as
rejected ones), one pair per micro-batch.  With the policy's initial weights as the reference, step 1 sees h = 0 exactly -- the table
is taken from the same micro-batches the run trains on -- so it logs rewards/margins 0 and dpo_loss = dpo_alpha log 2; a seeded run
repeats bit for bit; an explicit reference copy logs the same first step; a resumed run continues bit for bit.  The loss trajectory
is recorded, not gated."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_generate_gpu import _load, _model
from test_preference_gpu import PAIR_KEYS, _pairs

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class PairSet:
    """Tokenised pairs: item i is row i % 3 of the toy golden; the fourth item shifts its rejected answer once more."""

    def __init__(self, golden_dir, vocab):
        g, self.images, self.sizes, self.kw = _load(golden_dir, "toy")
        self.pairs = _pairs(g, vocab)
        self.vocab = vocab

    def __len__(self):
        return 4

    def __getitem__(self, i):
        b = i % 3
        item = {k: self.pairs[k][b].copy() for k in PAIR_KEYS}
        if i == 3:
            ans = item["rejected_labels"] != -100
            item["rejected_input_ids"][ans] = (item["rejected_input_ids"][ans] + 1) % self.vocab
            item["rejected_labels"][ans] = item["rejected_input_ids"][ans]
        return dict(item, image=self.images[b], size=self.sizes[b], index=i)


def _collate(items):
    out = {k: torch.from_numpy(np.stack([it[k] for it in items])) for k in PAIR_KEYS}
    out.update(images=[it["image"] for it in items], image_sizes=[it["size"] for it in items], indices=[it["index"] for it in items])
    return out


def _args(**kw):
    base = dict(per_device_train_batch_size=1, gradient_accumulation_steps=1, max_steps=3, learning_rate=2e-3, weight_decay=0.0,
                lr_scheduler_type="constant", seed=5, max_grad_norm=1.0, dataloader_num_workers=0, logging_steps=1, save_steps=0, output_dir=None)
    return SimpleNamespace(**dict(base, **kw))


def _strip(log):
    return [{k: v for k, v in rec.items() if k not in ("step_time_s", "data_wait_s")} for rec in log]


def _run(golden_dir, args, ref=False, resume=None, **kw):
    from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer
    model = _model("toy", {}).train()
    data = PairSet(golden_dir, model.engine.vocab)
    ref_model = _model("toy", {}) if ref else None
    trainer = LLaVADPOTrainer(model=model, ref_model=ref_model, args=args, train_dataset=data, data_collator=_collate,
                              precompute_ref_log_probs=not ref, **kw)
    state = trainer.train(resume_from_checkpoint=resume)
    torch.cuda.synchronize()
    return model.engine.lm.flat.clone(), _strip(state["log_history"]), trainer


def test_first_step_repeat_and_explicit_reference(golden_dir):
    w0 = _model("toy", {}).engine.lm.flat.clone()
    (wa, la, ta), (wb, lb, _) = _run(golden_dir, _args()), _run(golden_dir, _args())
    assert torch.equal(_bits(wa), _bits(wb)) and la == lb and len(la) == 3 and not torch.equal(_bits(wa), _bits(w0))
    assert ta.ref_model is None and ta.ref_table.shape == (4, 2) and np.isfinite(ta.ref_table).all() and ta.model.engine.loss_scale == 1.0
    first = la[0]
    assert first["rewards/margins"] == 0.0 and first["rewards/chosen"] == 0.0 and first["rewards/accuracies"] == 0.0
    assert first["dpo_loss"] == math.log(2.0)
    assert set(first) >= {"loss", "grad_norm", "learning_rate", "step", "rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins",
                          "logps/chosen", "logps/rejected", "dpo_loss", "sft_loss"}
    assert first["loss"] == pytest.approx(first["dpo_loss"] + first["sft_loss"], rel=1e-6)
    assert any(rec["rewards/margins"] != 0.0 for rec in la[1:])                # the policy has moved away from its reference
    # an explicit copy of the starting weights as the reference: the same first step
    _, lc, tc = _run(golden_dir, _args(max_steps=1), ref=True)
    assert lc[0] == first and tc.ref_table is None and tc.ref_model.engine.opt_step == 0
    # another objective on the same loop, with accumulation: it runs and the scale is restored
    _, ld, td = _run(golden_dir, _args(max_steps=1, gradient_accumulation_steps=2), loss_type="ipo", beta=0.2)
    assert ld[0]["rewards/margins"] == 0.0 and ld[0]["dpo_loss"] == pytest.approx((1 / (2 * 0.2)) ** 2, rel=1e-12) and td.model.engine.loss_scale == 1.0
    from conftest import record_measurement
    record_measurement("dpo_trainer_toy_trajectory", loss=[rec["loss"] for rec in la], dpo_loss=[rec["dpo_loss"] for rec in la],
                       margins=[rec["rewards/margins"] for rec in la])


def test_checkpoint_resume_continues_bit_for_bit(golden_dir, tmp_path):
    wa, la, _ = _run(golden_dir, _args())
    out = str(tmp_path / "run")
    _run(golden_dir, _args(max_steps=2, save_steps=2, output_dir=out))
    wb, lb, tb = _run(golden_dir, _args(save_steps=2, output_dir=out), resume=True)
    assert tb.state["global_step"] == 3 and torch.equal(_bits(wa), _bits(wb)) and lb == la


def test_train_dpo_entry_point(tmp_path):
    """train_dpo.train() on json records through DPODataset / DPODataCollator at the toy geometry: with a reference copy built from the
    policy's starting weights, and with the precomputed table, the first step starts at a margin of exactly 0."""
    import json
    import math
    from PIL import Image
    from radvlm_amd.llava import conversation as conv_lib
    from radvlm_amd.llava.train.train_dpo import train
    from test_train_features_gpu import Tok, _train_args
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rng = np.random.default_rng(3)
    recs = []
    for i in range(4):
        Image.fromarray(rng.integers(0, 255, (64, 80, 3), dtype=np.uint8)).save(tmp_path / f"im{i}.png")
        recs.append(dict(id=f"s{i}", image=f"im{i}.png", prompt=f"What is <image> finding {i}?", chosen="A nodule " + "x" * i, rejected="Nothing."))
    (tmp_path / "d.json").write_text(json.dumps(recs))
    saved = conv_lib.default_conversation
    try:
        logs = []
        for extra in ([], ["--precompute_ref_log_probs", "True"]):
            state = train(argv=_train_args(tmp_path, str(tmp_path / "d.json"), ["--geometry", "toy", "--max_steps", "2", "--beta", "0.2", "--save_steps", "0",
                                                                               "--output_dir", str(tmp_path / f"out{len(logs)}")] + extra), tokenizer=Tok())
            logs.append(_strip(state["log_history"]))
    finally:
        conv_lib.default_conversation = saved
    first = logs[0][0]
    assert first["rewards/margins"] == 0.0 and first["dpo_loss"] == math.log(2.0) and first["grad_norm"] > 0
    assert logs[1][0]["rewards/margins"] == 0.0 and logs[1][0]["dpo_loss"] == math.log(2.0) and logs[1][0]["sft_loss"] == first["sft_loss"]
    assert logs[0][1]["rewards/margins"] != 0.0

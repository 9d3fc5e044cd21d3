"""DPO preference training over LlavaEngine: the reference's DPODataset / DPODataCollator record contract (train_dpo.py:955-1305) and
LLaVADPOTrainer (llava_trainer.py:466-481 on TRL's DPOTrainer) on LLaVATrainer's loop -- schedule, accumulation, clipping, checkpoints
and resume are that loop's; only the micro-batch's loss call differs (model.preference_loss).

A micro-batch of P records runs as 2 P sequences (TRL's concatenated_forward).  The reference log-probs are ref_model.sequence_logps()
of the same 2 P sequence batch, or -- precompute_ref_log_probs -- a table indexed by dataset item, filled once before the first
update from the micro-batches of the run's first epoch (items that epoch drops are taken one by one), after which ref_model is not
needed; with ref_model None the table is taken from the policy's own initial weights (TRL).  The table is kept in every checkpoint, so
a resumed run does not take it again from trained weights.  reference_adapters_off=True (a LoRA policy, ref_model None): the reference
is the policy itself under model.disable_adapter(), per micro-batch or into the table.  One rank only: a pair never straddles ranks and no collective is added;
N > 1 ranks are untested.
"""
import copy
import json
import os
from dataclasses import dataclass

import numpy as np
import torch
from torch.utils.data import Dataset

from ...preference import PreferenceTerms, check_record, concatenate_pairs, make_conv, record_words, rewrite_prompt
from ..constants import IGNORE_INDEX
from .llava_trainer import LLaVATrainer, LengthGroupedSampler, epoch_index_batches

STAT_KEYS = ("rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins", "logps/chosen", "logps/rejected", "dpo_loss",
             "sft_loss")


class DPODataset(Dataset):
    """Records {"prompt", "chosen", "rejected", "image"?} -> {"prompt" ("<image>\\n" + prompt, earlier marks removed), "chosen",
    "rejected", "image": [(tensor, size, modality)], "has_image", "index"} (train_dpo.py:1155-1183).  `records` is a list or the path
    of a json / jsonl file; images are loaded as LazySupervisedDataset loads them."""

    def __init__(self, data_path=None, tokenizer=None, data_args=None, records=None):
        from .train import _load_records
        self.tokenizer, self.data_args = tokenizer, data_args
        self.list_data_dict = [check_record(r, i) for i, r in enumerate(records if records is not None else _load_records(data_path, data_args))]

    def __len__(self):
        return len(self.list_data_dict)

    @property
    def lengths(self):
        return [record_words(r) + (128 if "image" in r else 0) for r in self.list_data_dict]

    @property
    def modality_lengths(self):
        return [record_words(r) * (1 if "image" in r else -1) for r in self.list_data_dict]

    def __getitem__(self, i):
        from .train import LazySupervisedDataset
        rec = self.list_data_dict[i]
        out = copy.deepcopy({k: v for k, v in rec.items() if k != "image"})
        out["prompt"] = rewrite_prompt(rec["prompt"])
        if "image" in rec:
            f = rec["image"]
            if isinstance(f, str) or (isinstance(f, list) and all(isinstance(x, str) for x in f)):
                files = f if isinstance(f, list) else [f]
                out["image"] = [LazySupervisedDataset.process_image(self, x, "pad" if len(files) > 1 else None) for x in files]
            else:                    # already (tensor, size, modality) tuples: in-memory records
                out["image"] = list(f)
        elif getattr(self.data_args, "is_multimodal", False):
            cs = self.data_args.image_processor.crop_size
            out["image"] = [(torch.zeros(1, 3, cs["height"], cs["width"]), (cs["width"], cs["height"]), "text")]
        out["has_image"] = "image" in rec
        out["index"] = i
        return out


@dataclass
class DPODataCollator:
    """train_dpo.py:1186-1305: each answer is templated as a two-turn conversation through preprocess(), then chosen_* / rejected_*
    input_ids, labels and attention_mask are right-padded per half, and images / image_sizes are flattened in record order."""
    tokenizer: object
    label_pad_token_id: int = IGNORE_INDEX

    def tokenize_batch_element(self, prompt, chosen, rejected, has_image=True):
        from .train import preprocess
        batch = {}
        for k, answer in (("chosen", chosen), ("rejected", rejected)):
            d = preprocess([make_conv(prompt, answer)], self.tokenizer, has_image=has_image)
            batch[f"{k}_input_ids"], batch[f"{k}_labels"] = d["input_ids"][0], d["labels"][0]
        return batch

    def __call__(self, features):
        tok = self.tokenizer
        if tok.pad_token_id is None:
            tok.pad_token_id = 0
        L = getattr(tok, "model_max_length", None) or (1 << 30)
        rows = [self.tokenize_batch_element(f["prompt"], f["chosen"], f["rejected"], has_image=f.get("has_image", True)) for f in features]
        out = {}
        for k in ("chosen", "rejected"):
            ids = [torch.as_tensor(r[f"{k}_input_ids"])[:L] for r in rows]
            labs = [torch.as_tensor(r[f"{k}_labels"])[:L] for r in rows]
            out[f"{k}_input_ids"] = torch.nn.utils.rnn.pad_sequence(ids, batch_first=True, padding_value=tok.pad_token_id)
            out[f"{k}_labels"] = torch.nn.utils.rnn.pad_sequence(labs, batch_first=True, padding_value=self.label_pad_token_id)
            out[f"{k}_attention_mask"] = out[f"{k}_input_ids"].ne(tok.pad_token_id)
        if "image" in features[0]:
            flat = [im for f in features for im in f["image"]]
            out["image_sizes"] = [im[1] for im in flat]
            out["modalities"] = [im[2] for im in flat]
            out["images"] = [im[0] for im in flat]
        out["prompts"] = [f["prompt"] for f in features]
        if "index" in features[0]:
            out["indices"] = [int(f["index"]) for f in features]
        return out


PAIR_KEYS = ("chosen_input_ids", "chosen_attention_mask", "chosen_labels", "rejected_input_ids", "rejected_attention_mask", "rejected_labels")


class LLaVADPOTrainer(LLaVATrainer):
    def __init__(self, model=None, ref_model=None, args=None, dpo_alpha=1.0, beta=0.1, gamma=1.0, train_dataset=None, data_collator=None,
                 tokenizer=None, precompute_ref_log_probs=False, loss_type="sigmoid", label_smoothing=0.0, reference_free=False,
                 reference_adapters_off=False, **_):
        super().__init__(model=model, tokenizer=tokenizer, args=args, train_dataset=train_dataset,
                         data_collator=data_collator if data_collator is not None else DPODataCollator(tokenizer=tokenizer))
        self.ref_model, self.precompute, self.reference_free = ref_model, bool(precompute_ref_log_probs), bool(reference_free)
        self.terms = dict(beta=beta, dpo_alpha=dpo_alpha, gamma=gamma, loss_type=loss_type, label_smoothing=label_smoothing)
        PreferenceTerms(reference_free=True, **self.terms).check()          # the scalar arguments, before any device work
        # reference_adapters_off (a LoRA policy, ref_model None): the reference is the policy with its adapters switched off
        # (model.disable_adapter(), peft's way) -- the frozen base it started from, without a second copy of the model
        self.ref_off = bool(reference_adapters_off)
        if self.ref_off and (ref_model is not None or not model.engine.lora):
            raise ValueError("reference_adapters_off=True takes the reference from the policy's own frozen base: it needs a model with "
                             "LoRA adapters and ref_model=None")
        if ref_model is None and not self.precompute and not self.reference_free and not self.ref_off:
            raise ValueError("LLaVADPOTrainer needs a ref_model, precompute_ref_log_probs=True (the policy's initial weights are the "
                             "reference) or reference_free=True")
        if ref_model is model and not self.precompute:
            raise ValueError("ref_model is the policy itself: pass a copy, or precompute_ref_log_probs=True")
        if getattr(args, "world_size", 1) > 1:
            raise NotImplementedError("DPO training runs on one rank (N > 1 untested)")
        self.ref_table = None            # float64 [len(dataset), 2]: the reference's summed log-prob of (chosen, rejected), NaN = not taken
        self._micro = []

    def _get_train_sampler(self):
        """llava_trainer.py:466-481: the DPO trainer groups by modality length only (world_size without the accumulation factor)."""
        a = self.args
        if getattr(a, "group_by_modality_length", False):
            return LengthGroupedSampler(batch_size=a.per_device_train_batch_size, world_size=getattr(a, "world_size", 1),
                                        lengths=self.train_dataset.modality_lengths, group_by_modality=True,
                                        generator=torch.Generator().manual_seed(getattr(a, "seed", 42)))
        return None

    # ------------------------------------------------------------------ reference log-probs
    @staticmethod
    def _pair_batch(batch):
        ids, am, lab = concatenate_pairs(*[batch[k].cpu().numpy() if torch.is_tensor(batch[k]) else batch[k] for k in PAIR_KEYS])
        images = list(batch["images"])
        sizes = batch.get("image_sizes")
        return dict(input_ids=ids, attention_mask=am, labels=lab, images=images + images, image_sizes=None if sizes is None else list(sizes) * 2)

    def _reference_sums(self, model, batch):
        """The reference's summed log-probs of the micro-batch's 2 P sequences: (chosen fp64 [P], rejected fp64 [P]) on the device."""
        if self.ref_off:
            with self.model.disable_adapter():
                sums, _ = self.model.sequence_logps(**self._pair_batch(batch))
        else:
            sums, _ = model.sequence_logps(**self._pair_batch(batch))
        P = sums.numel() // 2
        return sums[:P], sums[P:]

    def _before_train(self, start):
        if not self.precompute or self.reference_free or self.ref_table is not None:
            return
        a = self.args
        ref = self.ref_model if self.ref_model is not None else self.model
        n = len(self.train_dataset)
        table = np.full((n, 2), np.nan)
        accum = max(1, int(getattr(a, "gradient_accumulation_steps", 1) or 1))
        it, steps = epoch_index_batches(n, self._get_train_sampler(), getattr(a, "seed", 42), a.per_device_train_batch_size, 1, 0, accum,
                                        drop_last=bool(getattr(a, "dataloader_drop_last", False)))
        groups = [next(it) for _ in range(steps * accum)]
        seen = {i for g in groups for i in g}
        groups += [[i] for i in range(n) if i not in seen]
        for g in groups:
            if not np.isnan(table[g]).any():
                continue
            c, r = self._reference_sums(ref, self.data_collator([self.train_dataset[i] for i in g]))
            todo = [k for k, i in enumerate(g) if np.isnan(table[i, 0])]         # an item's first micro-batch is the one that counts
            c, r = c.cpu().numpy(), r.cpu().numpy()
            for k in todo:
                table[g[k]] = (c[k], r[k])
        self.ref_table = table
        self.ref_model = None             # not needed from here on

    def compute_loss(self, batch):
        kw = dict(self.terms, reference_free=self.reference_free)
        if self.reference_free:
            pass
        elif self.ref_table is not None:
            rows = self.ref_table[np.asarray(batch["indices"], dtype=np.int64)]
            kw.update(ref_chosen_logps=rows[:, 0], ref_rejected_logps=rows[:, 1])
        else:
            c, r = self._reference_sums(self.ref_model, batch)
            kw.update(ref_chosen_logps=c, ref_rejected_logps=r)
        out = self.model.preference_loss(*[batch[k] for k in PAIR_KEYS], batch["images"], batch.get("image_sizes"), **kw)
        self._micro.append(out.stats)
        return out

    def _extra_log(self):
        micro, self._micro = self._micro, []
        return {k: float(np.mean([float(m[k]) for m in micro])) for k in STAT_KEYS} if micro else {}

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path, rank=0):
        super().save_checkpoint(path, rank)
        if rank == 0 and self.ref_table is not None:
            with open(os.path.join(path, "ref_log_probs.json"), "w") as f:
                json.dump([[float(v).hex() for v in row] for row in self.ref_table], f)

    def _maybe_resume(self, resume_from_checkpoint):
        start = super()._maybe_resume(resume_from_checkpoint)
        path = resume_from_checkpoint
        if path is True and start:
            path = os.path.join(self.args.output_dir, f"checkpoint-{start}")
        if start and isinstance(path, str) and os.path.exists(os.path.join(path, "ref_log_probs.json")):
            with open(os.path.join(path, "ref_log_probs.json")) as f:
                self.ref_table = np.array([[float.fromhex(v) for v in row] for row in json.load(f)], dtype=np.float64).reshape(-1, 2)
        return start

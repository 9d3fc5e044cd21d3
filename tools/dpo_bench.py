"""DPO measurements: JSON lines appended to profiles/dpo_bench.jsonl.

  python tools/dpo_bench.py kernel  [--reps 20] [--out FILE]
  python tools/dpo_bench.py trainer [--geometry llava15_7b] [--pairs 8] [--answer-tokens 128] [--out FILE]

kernel   The three-launch DPO loss -- (A) rv_policy_loss_bf16 without dlogits, rv_dpo_pairs_f64, (C) rv_policy_loss_bf16 in place --
         against rv_cross_entropy (unchanged) on the same bf16 logits, in place, at [2048, 32000] and [2048, 152064]: 8 pairs as 16
         sequences over the live rows, scattered through row_idx as under the all-rows head.  Before any timing the composition is
         asserted: the gradients are bit for bit rv_policy_loss_bf16's with the coefficients as advantages.  The arms alternate;
         every repetition restores the logits outside the timed window and is timed between device events; reported: the median of
         --reps, every repetition, the CE arm's spread (max - min), and the pair kernel alone.
trainer  One LLaVADPOTrainer step at a full geometry with random weights and a reference engine: --pairs pairs in one micro-batch
         (2 x pairs sequences), prompts of 128 text tokens and one image (704 positions at llava15_7b), --answer-tokens answer tokens;
         a first step warms up, the second is reported, split into reference / policy forward / backward / optimizer seconds.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _src_hash():
    try:
        from radvlm_amd.build_id import kernel_source_sha256
        return kernel_source_sha256()
    except Exception:          # noqa: BLE001 -- the hash is a label, never a reason to lose a measurement
        return None


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def kernel_ab(reps, pairs=8):
    from radvlm_amd import lib, ops
    dev = torch.device("cuda:0")
    recs = []
    for rows, V in ((2048, 32000), (2048, 152064)):
        g = torch.Generator(device=dev).manual_seed(V)
        src = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
        labels = torch.randint(0, V, (rows,), device=dev, generator=g)
        labels[::17] = -100
        live = torch.nonzero(labels >= 0).flatten()
        n = int(live.numel())
        c = 1.0 / n
        seg = torch.from_numpy(np.linspace(0, n, 2 * pairs + 1).astype(np.int32)).to(dev)
        row_idx = live.to(torch.int32)
        rho = -torch.rand(2 * pairs, dtype=torch.float64, device=dev) * 500
        zero, ones = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
        coef = torch.zeros(rows, device=dev)
        work = src.clone()
        ce_rows = torch.empty(rows, device=dev)
        stats, stats_c = torch.empty(5, rows, device=dev), torch.empty(5, rows, device=dev)
        n_c = int(seg[pairs])
        out = {}

        def ce():
            lib.call("rv_cross_entropy", work, V, labels, ce_rows, work, V, rows, V, c)

        def logp_pass():
            lib.call("rv_policy_loss_bf16", work, V, labels, zero, zero, zero, None, None, 0.0, 0.0, 0.0, stats, None, 0, rows, V)

        def pair_pass():
            out["planes"], out["batch"] = ops.dpo_pairs(stats[0], seg, row_idx, rho, "sigmoid", 0.1, 0.0, 1.0 / pairs, 1.0 / n_c, coef)

        def grad_pass():
            lib.call("rv_policy_loss_bf16", work, V, labels, coef, ones, ones, None, None, 0.0, 0.0, 0.0, stats_c, work, V, rows, V)

        def dpo():
            logp_pass(), pair_pass(), grad_pass()

        dpo()
        got = work.clone()
        work.copy_(src)
        grad_pass()                                      # the same coefficients through the GRPO kernel alone
        torch.cuda.synchronize()
        assert torch.equal(work.view(torch.int16), got.view(torch.int16)), "composition: the gradients differ from rv_policy_loss_bf16's"
        assert bool(torch.isfinite(out["batch"]).all())
        arms = {"cross_entropy": ce, "dpo_three_launches": dpo, "dpo_pairs_only": pair_pass}
        times = {k: [] for k in arms}
        for rep in range(reps + 2):                      # two warm-up rounds
            for name, fn in arms.items():
                work.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append(e0.elapsed_time(e1))
        rec = dict(tool="dpo_bench", part="kernel", rows=rows, V=V, reps=reps, pairs=pairs, scored_rows=n, device=torch.cuda.get_device_name(0),
                   kernel_src=_src_hash())
        for name, ts in times.items():
            rec[name] = dict(ms_median=round(_median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), ms_all=[round(t, 4) for t in ts])
        rec["ce_spread_ms"] = round(max(times["cross_entropy"]) - min(times["cross_entropy"]), 4)
        rec["dpo_minus_ce_ms"] = round(_median(times["dpo_three_launches"]) - _median(times["cross_entropy"]), 4)
        rec["dpo_over_ce"] = round(_median(times["dpo_three_launches"]) / _median(times["cross_entropy"]), 3)
        recs.append(rec)
        del src, work, got
        torch.cuda.empty_cache()
    return recs


class _Pairs:
    """Tokenised pairs of random ids: 128 prompt tokens around one image, then the answer."""

    def __init__(self, n, V, side, answer_tokens):
        from radvlm_amd.llava.constants import IMAGE_TOKEN_INDEX
        rng = np.random.default_rng(0)
        self.items = []
        for i in range(n):
            prompt = rng.integers(1000, V - 1000, size=129).astype(np.int64)
            prompt[4] = IMAGE_TOKEN_INDEX
            item = dict(index=i, image=torch.from_numpy(rng.standard_normal((3, side, side)).astype(np.float32)), size=(side, side))
            for k in ("chosen", "rejected"):
                ans = rng.integers(1000, V - 1000, size=answer_tokens).astype(np.int64)
                item[f"{k}_input_ids"] = np.concatenate([prompt, ans])
                item[f"{k}_labels"] = np.concatenate([np.full(129, -100, dtype=np.int64), ans])
                item[f"{k}_attention_mask"] = np.ones(129 + answer_tokens, dtype=bool)
            self.items.append(item)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _collate(items):
    from radvlm_amd.llava.train.dpo_trainer import PAIR_KEYS
    out = {k: torch.from_numpy(np.stack([it[k] for it in items])) for k in PAIR_KEYS}
    out.update(images=[it["image"] for it in items], image_sizes=[it["size"] for it in items], indices=[it["index"] for it in items])
    return out


def trainer_step(a):
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    from radvlm_amd.llava.train.dpo_trainer import LLaVADPOTrainer
    geo = GEOMETRIES[a.geometry]
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in a.geometry else (LlavaConfig, LlavaLlamaForCausalLM)
    t0 = time.perf_counter()
    model = Model(Config(geometry=geo), device="cuda:0", init="fast", seed=0).train()
    ref = Model(Config(geometry=geo), device="cuda:0", init="fast", seed=0)
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    phases = {}

    def timed(obj, name, key):
        fn = getattr(obj, name)

        def wrapper(*args, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = fn(*args, **kw)
            torch.cuda.synchronize()
            phases[key] = phases.get(key, 0.0) + time.perf_counter() - t
            return r
        setattr(obj, name, wrapper)

    timed(ref, "sequence_logps", "reference_s")
    timed(model, "preference_loss", "policy_forward_s")
    timed(model.engine, "backward", "backward_s")
    timed(model.engine, "optimizer_step", "optimizer_s")
    data = _Pairs(2 * a.pairs, geo["lm"]["vocab"], geo["vision"]["image"], a.answer_tokens)
    args = SimpleNamespace(per_device_train_batch_size=a.pairs, gradient_accumulation_steps=1, max_steps=2, learning_rate=1e-6, weight_decay=0.0,
                           lr_scheduler_type="constant", seed=0, max_grad_norm=1.0, dataloader_num_workers=0, logging_steps=1, save_steps=0,
                           output_dir=None)
    trainer = LLaVADPOTrainer(model=model, ref_model=ref, args=args, train_dataset=data, data_collator=_collate)
    first = {}
    step = trainer._extra_log

    def after_step():            # the loop calls this once per logged step: keep the first step's phases apart
        if not first:
            first.update(phases)
            phases.clear()
        return step()
    trainer._extra_log = after_step
    state = trainer.train()
    rec = state["log_history"][-1]
    return [dict(tool="dpo_bench", part="trainer", geometry=a.geometry, pairs=a.pairs, sequences=2 * a.pairs, answer_tokens=a.answer_tokens,
                 prompt_positions=int(model.engine.P) + 128, init_s=round(t_init, 2), step_s=round(rec["step_time_s"], 3),
                 **{k: round(v, 3) for k, v in phases.items()}, first_step={k: round(v, 3) for k, v in first.items()},
                 loss=rec["loss"], dpo_loss=rec["dpo_loss"], sft_loss=rec["sft_loss"], grad_norm=rec["grad_norm"],
                 peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), device=torch.cuda.get_device_name(0), kernel_src=_src_hash())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "trainer"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--geometry", default="llava15_7b")
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--answer-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpo_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpo_bench measures on the GPU; none is visible")
    recs = kernel_ab(a.reps) if a.part == "kernel" else trainer_step(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

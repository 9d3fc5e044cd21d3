"""GRPO measurements: JSON lines appended to profiles/grpo_bench.jsonl.

  python tools/grpo_bench.py kernel  [--reps 20] [--importance-sampling-level sequence] [--out FILE]
  python tools/grpo_bench.py trainer [--geometry llava15_7b] [--prompts 8] [--generations 8] [--new-tokens 128] [--accum 4] [--lora]
                                     [--importance-sampling-level sequence] [--out FILE]

kernel   A/B of rv_cross_entropy (unchanged) against rv_policy_loss_bf16 on the same bf16 logits, in place, at [2048, 32000] and
         [2048, 152064].  Both are two sweeps of the row plus a handful of per-row loads.  The two bit anchors (logp == -loss_rows; the
         gradient at adv = 1, no old log-probs, beta = 0, gweight = c == the cross entropy's at inv_count = c) are asserted before any
         timing.  The arms alternate; every repetition restores the logits outside the timed window and is timed between device events;
         reported: the median of --reps, every repetition, and the CE arm's spread (max - min).  A second policy arm runs the full
         objective (old and reference log-probs, beta > 0).
         --importance-sampling-level sequence adds the GSPO arm at the same rows: the three launches of the engine's sequence branch --
         (A) rv_policy_loss_bf16 without dlogits, (B) rv_gspo_seqs_f64 on sequences of 128 scored tokens through row_idx, (C)
         rv_policy_loss_bf16 in place on the coefficients -- with the full objective, against policy_full's single sweep; its bit
         anchor (on-policy, the three launches leave the token level's gradients) is asserted before any timing.
trainer  One GRPOTrainer step at a full geometry with random weights: --prompts x --generations, prompts of 128 text tokens and one
         image (704 positions at llava15_7b), --new-tokens sampled tokens, num_iterations 2 so that the old-log-prob pass runs; a first
         step warms up, the second is reported, split into sampling / log-prob / update seconds.  --importance-sampling-level is
         passed to the trainer.
         --lora: the same step on a LoRA model (r 64, alpha 16, dropout 0.05) that samples from its live adapters
         (enable_adapter_decoding()), with beta 0.04 and no ref_model, so that the log-prob pass includes the reference taken under
         disable_adapter().
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


def kernel_ab(reps, level="token"):
    from radvlm_amd import lib, ops
    dev = torch.device("cuda:0")
    recs = []
    for rows, V in ((2048, 32000), (2048, 152064)):
        g = torch.Generator(device=dev).manual_seed(V)
        src = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
        labels = torch.randint(0, V, (rows,), device=dev, generator=g)
        labels[::17] = -100
        live = labels >= 0
        c = 1.0 / int(live.sum())
        ones = torch.ones(rows, device=dev)
        cw = torch.full((rows,), c, device=dev)
        adv = torch.randn(rows, device=dev, generator=g)
        work = src.clone()
        ce_rows = torch.empty(rows, device=dev)
        stats = torch.empty(5, rows, device=dev)

        def ce():
            lib.call("rv_cross_entropy", work, V, labels, ce_rows, work, V, rows, V, c)

        def policy(a=ones, old=None, ref=None, beta=0.0):
            lib.call("rv_policy_loss_bf16", work, V, labels, a, cw, cw, old, ref, 0.2, 0.28, beta, stats, work, V, rows, V)

        ce()
        want = work.clone()
        work.copy_(src)
        policy()
        torch.cuda.synchronize()
        assert torch.equal(work.view(torch.int16), want.view(torch.int16)), "SFT anchor: the gradients differ from rv_cross_entropy's"
        assert torch.equal(stats[0][live].view(torch.int32), (-ce_rows[live]).view(torch.int32)), "logp != -loss_rows"
        old = (stats[0] + 0.1 * torch.randn(rows, device=dev, generator=g)).contiguous()
        ref = (stats[0] - 0.05).contiguous()
        arms = {"cross_entropy": ce, "policy_sft_anchor": policy, "policy_full": lambda: policy(adv, old, ref, 0.04)}
        if level == "sequence":
            row_idx = torch.nonzero(live).flatten().to(torch.int32)
            n = int(row_idx.numel())
            seg = torch.arange(0, n + 128, 128, dtype=torch.int32, device=dev).clamp_(max=n)      # sequences of 128 scored tokens
            B = int(seg.numel()) - 1
            adv_seq = torch.randn(B, device=dev, generator=g)
            seq_of = torch.repeat_interleave(torch.arange(B, device=dev), (seg[1:] - seg[:-1]).long())
            zero, coef, kl, stats_c = torch.zeros(rows, device=dev), torch.zeros(rows, device=dev), torch.zeros(rows, device=dev), torch.empty_like(stats)

            def gspo(o=old, r=ref, beta=0.04):
                lib.call("rv_policy_loss_bf16", work, V, labels, zero, zero, zero, None, None, 0.0, 0.0, 0.0, stats, None, 0, rows, V)
                ops.gspo_seqs(stats[0], seg, row_idx, adv_seq, cw, cw, o, r, 0.2, 0.28, beta, coef, kl)
                lib.call("rv_policy_loss_bf16", work, V, labels, coef, ones, ones, None, None, 0.0, 0.0, 0.0, stats_c, work, V, rows, V)

            adv_rows = torch.zeros(rows, device=dev)
            adv_rows[row_idx.long()] = adv_seq[seq_of]
            work.copy_(src)
            policy(adv_rows)
            want_seq = work.clone()
            work.copy_(src)
            gspo(None, None, 0.0)
            torch.cuda.synchronize()
            assert torch.equal(work.view(torch.int16), want_seq.view(torch.int16)), "GSPO anchor: on-policy gradients differ from the token level's"
            del want_seq
            arms["gspo_three_launches"] = gspo
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
        nbytes = 3 * rows * V * 2                        # two reads and one write of the row
        rec = dict(tool="grpo_bench", part="kernel", rows=rows, V=V, reps=reps, bytes=nbytes, device=torch.cuda.get_device_name(0),
                   build=os.path.basename(os.environ.get("RADVLM_HIP_LIB", "default")), kernel_src=_src_hash())
        for name, ts in times.items():
            rec[name] = dict(ms_median=round(_median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4),
                             tb_per_s=round(nbytes / _median(ts) / 1e9, 3), ms_all=[round(t, 4) for t in ts])
        rec["ce_spread_ms"] = round(max(times["cross_entropy"]) - min(times["cross_entropy"]), 4)
        rec["policy_minus_ce_ms"] = round(_median(times["policy_sft_anchor"]) - _median(times["cross_entropy"]), 4)
        rec["policy_full_minus_ce_ms"] = round(_median(times["policy_full"]) - _median(times["cross_entropy"]), 4)
        if level == "sequence":
            rec["importance_sampling_level"], rec["sequences"] = level, B
            del rec["gspo_three_launches"]["tb_per_s"]      # `bytes` counts one in-place sweep, not the three launches
            rec["gspo_over_policy_full"] = round(_median(times["gspo_three_launches"]) / _median(times["policy_full"]), 4)
        recs.append(rec)
        del src, work, want
        torch.cuda.empty_cache()
    return recs


def trainer_step(a):
    from radvlm_amd.config import GEOMETRIES
    from radvlm_amd.llava.constants import IMAGE_TOKEN_INDEX
    from radvlm_amd.llava.model import LlavaConfig, LlavaLlamaForCausalLM, LlavaQwenConfig, LlavaQwenForCausalLM
    from radvlm_amd.llava.train.grpo_trainer import GRPOTrainer
    geo = GEOMETRIES[a.geometry]
    Config, Model = (LlavaQwenConfig, LlavaQwenForCausalLM) if "qwen" in a.geometry else (LlavaConfig, LlavaLlamaForCausalLM)
    t0 = time.perf_counter()
    lora = dict(r=64, alpha=16, dropout=0.05) if a.lora else None
    model = Model(Config(geometry=geo, lora=lora), device="cuda:0", init="fast", seed=0).train()
    if a.lora:
        model.enable_adapter_decoding()
    torch.cuda.synchronize()
    t_init = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    side, V = geo["vision"]["image"], geo["lm"]["vocab"]
    data = []
    for _ in range(2 * a.prompts):
        ids = rng.integers(1000, V - 1000, size=129).astype(np.int64)        # 128 text tokens around one image
        ids[4] = IMAGE_TOKEN_INDEX
        data.append(dict(prompt_ids=ids, images=torch.from_numpy(rng.standard_normal((3, side, side)).astype(np.float32)), image_sizes=(side, side)))
    reward = lambda completion_ids, **_: [float(np.mean([t % 2 == 0 for t in c])) if len(c) else 0.0 for c in completion_ids]
    args = SimpleNamespace(per_device_train_batch_size=a.prompts, num_generations=a.generations, max_completion_length=a.new_tokens, max_steps=2,
                           learning_rate=1e-6, weight_decay=0.0, lr_scheduler_type="constant", seed=0, num_iterations=2,
                           gradient_accumulation_steps=a.accum, max_grad_norm=1.0, beta=0.04 if a.lora else 0.0,
                           importance_sampling_level=a.importance_sampling_level)
    state = GRPOTrainer(model, args, data, reward).train()
    rec = state["log_history"][-1]
    return [dict(tool="grpo_bench", part="trainer", geometry=a.geometry, prompts=a.prompts, generations=a.generations, new_tokens=a.new_tokens,
                 prompt_positions=int(model.engine.P) + 128, micro_batches=a.accum, num_iterations=2, importance_sampling_level=a.importance_sampling_level, lora=lora, beta=args.beta, init_s=round(t_init, 2),
                 sampling_s=round(rec["time/sampling_s"], 3), scoring_s=round(rec["time/scoring_s"], 3), logps_s=round(rec["time/logps_s"], 3),
                 update_s=round(rec["time/update_s"], 3), mean_completion_length=rec["completions/mean_length"],
                 peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1), device=torch.cuda.get_device_name(0), kernel_src=_src_hash())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel", "trainer"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--geometry", default="llava15_7b")
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--generations", type=int, default=8)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--lora", action="store_true")
    ap.add_argument("--importance-sampling-level", default="token", choices=["token", "sequence"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grpo_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grpo_bench measures on the GPU; none is visible")
    recs = kernel_ab(a.reps, a.importance_sampling_level) if a.part == "kernel" else trainer_step(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""The NF4 frozen base (QLoRA) against the bf16 base on one box, interleaved.

  1. rv_nf4_dequant_bf16 alone on one decoder layer's seven matrices of the 7B and the 13B geometry (random codes and absmax: the time
     does not depend on the values), both modes, median of --reps launches, in GB/s of 0.5 B read + 2 B written per weight plus the
     absmax bytes;
  2. the llava15_7b LoRA step (r 64, bench.py's synthetic batch, S = 704) on two engines that hold the same weights, one with the bf16
     base (the behaviour before this format existed) and one with the NF4 base, in alternating blocks of --steps steps;
  3. base_weight_bytes and the peak device memory of each arm's blocks.

Nothing gates on the result: one JSON record per measurement is appended to --out.  RADVLM_HIP_LIB selects another build of the library
(a variant of csrc/nf4.hip); --tag names it in the records.  --toy-losses PATH writes twenty toy LoRA steps on the three bases;
--quant-error appends the reference's quantisation error on a seeded matrix (CPU arithmetic).

  python tools/qlora_bench.py [--batch 32] [--reps 20] [--steps 3] [--blocks 2] [--skip-step] [--tag kept] [--out profiles/qlora_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radvlm_amd import nf4 as N  # noqa: E402
from radvlm_amd import ops  # noqa: E402
from radvlm_amd.config import GEOMETRIES  # noqa: E402

STREAM_TBPS = 6.3          # the achievable HBM streaming rate of the microarchitecture guide the result is set against


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def dequant_alone(name, dq, reps):
    geo = {"vision": GEOMETRIES[name]["vision"], "lm": dict(GEOMETRIES[name]["lm"], layers=1)}
    plan = N.BasePlan(geo, dq)
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(2)
    codes = torch.randint(0, 256, (plan.code_bytes,), dtype=torch.uint8, device=dev, generator=g)
    kw = {}
    if dq:
        kw = dict(absmax_codes=torch.randint(0, 256, (plan.nblocks,), dtype=torch.uint8, device=dev, generator=g),
                  scale2=torch.rand(plan.nscale2, device=dev, generator=g) * 0.02, offset=torch.full((7,), 0.05, device=dev))
    else:
        kw = dict(absmax=torch.rand(plan.nblocks, device=dev, generator=g) * 0.1)
    tab, nch = plan.table(plan.names(0))
    tab_dev = torch.from_numpy(tab).to(dev)
    dst = torch.zeros(plan.scratch_numel, dtype=torch.bfloat16, device=dev)
    run = lambda: ops.nf4_dequant(codes, tab_dev, tab, nch, dst, **kw)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t = [_timed(run) for _ in range(reps)]
    w = plan.weights
    moved = 2 * w + plan.base_weight_bytes()
    med = statistics.median(t)
    return dict(mode="dequant_alone", geometry=name, double_quant=dq, weights=w, bytes_moved=moved, reps=reps, ms_median=med, ms_min=min(t),
                GBps=moved / med / 1e6, fraction_of_stream_rate=moved / med / 1e9 / STREAM_TBPS)


def toy_losses(path, steps=20):
    """Twenty LoRA steps (r 16, no adapter dropout) on the golden toy batch: a bf16 base against the NF4 base, plain and doubly quantised."""
    from radvlm_amd.engine import LlavaEngine
    g = np.load(os.path.join(ROOT, "tests", "golden", "toy_e2e.npz"))
    n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
    images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
    curves = {}
    for arm, dq in (("bf16", None), ("nf4", False), ("nf4_double_quant", True)):
        eng = LlavaEngine(GEOMETRIES["toy"], device="cuda:0", init="portable", seed=0, lora=dict(r=16, alpha=16, dropout=0.0))
        if dq is not None:
            eng.quantize_base_(double_quant=dq)
        curves[arm] = []
        for _ in range(steps):
            loss = eng.forward(g["input_ids"], g["attention_mask"], g["labels"], images)
            eng.backward()
            eng.optimizer_step(lr=2e-3, weight_decay=0.0, max_grad_norm=1.0)
            curves[arm].append(float(loss))
    rec = dict(geometry="toy", batch="toy_e2e", lora_r=16, lr=2e-3, weight_decay=0.0, max_grad_norm=1.0, **curves,
               max_abs_difference_nf4=float(np.abs(np.subtract(curves["nf4"], curves["bf16"])).max()),
               max_abs_difference_nf4_double_quant=float(np.abs(np.subtract(curves["nf4_double_quant"], curves["bf16"])).max()))
    with open(path, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec), flush=True)


def quant_error():
    """The reference's relative Frobenius error on a seeded bf16 N(0, 0.02) 4096 x 4096 matrix: CPU arithmetic, no GPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nf4_ref as R
    w = R.bf16_round((0.02 * np.random.RandomState(0).randn(4096 * 4096)).astype(np.float32))
    norm = np.linalg.norm(w.astype(np.float64))
    err = {("double_quant" if dq else "plain"): float(np.linalg.norm((R.roundtrip(w, dq) - w).astype(np.float64)) / norm) for dq in (False, True)}
    return dict(mode="quantisation_error", matrix="bf16 N(0, 0.02) 4096x4096, RandomState(0)", relative_frobenius=err)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quant-error", action="store_true", help="append the reference's quantisation error (CPU only) to --out and stop")
    ap.add_argument("--toy-losses", metavar="PATH", default=None, help="write the twenty-step toy curves to PATH and stop")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--double-quant", type=int, default=1)
    ap.add_argument("--skip-step", action="store_true", help="the dequant launch alone")
    ap.add_argument("--tag", default="kept")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qlora_bench.jsonl"))
    a = ap.parse_args()
    if a.toy_losses:
        return toy_losses(a.toy_losses)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(rec):
        rec = dict(rec, tag=a.tag, device=torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu")
        print(json.dumps(rec), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    if a.quant_error:
        return emit(quant_error())
    for name in ("llava15_7b", "llava15_13b"):
        for dq in (False, True):
            emit(dequant_alone(name, dq, a.reps))
    if a.skip_step:
        return

    import bench
    from radvlm_amd.engine import LlavaEngine
    geo = GEOMETRIES["llava15_7b"]
    dq = bool(a.double_quant)
    kw = dict(device="cuda:0", init="fast", seed=0, lora=dict(r=64, alpha=16, dropout=0.05))
    batches = [bench.synthetic_batch(geo, a.batch, seed=1234 + 1000 * k) for k in range(4)]

    def alone(eng):                                          # the peak of one step with this engine alone on the device
        for k in range(2):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            eng.forward(*batches[k])
            eng.backward()
            eng.optimizer_step(lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() / 2 ** 30

    first = LlavaEngine(geo, **kw)
    peak_alone = {"bf16": alone(first)}
    del first
    torch.cuda.empty_cache()
    engines = {"nf4": LlavaEngine(geo, **kw)}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    engines["nf4"].quantize_base_(double_quant=dq)
    torch.cuda.synchronize()
    act = dict(mode="quantize_base", geometry="llava15_7b", double_quant=dq, seconds=time.perf_counter() - t0,
               peak_GiB_during_the_act=torch.cuda.max_memory_allocated() / 2 ** 30,
               base_weight_bytes_bf16=N.bf16_matrix_bytes(geo), base_weight_bytes_nf4=engines["nf4"].base_weight_bytes(),
               scratch_bytes=engines["nf4"].nf4["plan"].scratch_bytes())
    emit(act)
    peak_alone["nf4"] = alone(engines["nf4"])
    engines["bf16"] = LlavaEngine(geo, **kw)           # the same seed: the same weights before quantisation, the parent's behaviour
    count = {k: 0 for k in engines}

    def step(arm):
        eng = engines[arm]
        b = batches[count[arm] % 4]
        count[arm] += 1
        loss = eng.forward(*b)
        eng.backward()
        eng.optimizer_step(lr=2e-5, weight_decay=0.0, max_grad_norm=1.0)
        return loss

    times, peak, losses = {k: [] for k in engines}, {}, {k: [] for k in engines}
    for block in range(a.blocks):
        for arm in ("bf16", "nf4"):
            step(arm)                                        # warm-up of the block
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                losses[arm].append(step(arm))
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / a.steps * 1e3)
            peak[arm] = torch.cuda.max_memory_allocated() / 2 ** 30
    S = 128 + (geo["vision"]["image"] // geo["vision"]["patch"]) ** 2
    emit(dict(mode="training_step", geometry="llava15_7b", lora_r=64, batch=a.batch, S=S, double_quant=dq, steps_per_block=a.steps, blocks=a.blocks,
              bf16_ms_per_step=times["bf16"], nf4_ms_per_step=times["nf4"], bf16_ms_median=statistics.median(times["bf16"]),
              nf4_ms_median=statistics.median(times["nf4"]), dequant_launches_per_step=2 * geo["lm"]["layers"],
              peak_GiB_alone_bf16=peak_alone["bf16"], peak_GiB_alone_nf4=peak_alone["nf4"],
              peak_GiB_both_engines_resident_bf16_arm=peak["bf16"], peak_GiB_both_engines_resident_nf4_arm=peak["nf4"],
              losses_bf16=[float(x) for x in losses["bf16"]], losses_nf4=[float(x) for x in losses["nf4"]]))


if __name__ == "__main__":
    main()

"""rv_adamw (fp32 moments) against rv_adamw8 (8-bit moments) on one box, interleaved.

  1. the optimizer alone over the 7B model's parameter groups (the engine's own launch lists at both widths), median of --reps per arm,
     arms alternating;
  2. the full training step at the headline shape (bench.py's synthetic batch, --batch pairs) through the engine at both widths, in
     alternating blocks of --steps steps; the state is converted in place between blocks, outside the timed region.

Nothing gates on the result: one JSON record per measurement is appended to --out.

  python tools/adam8_bench.py [--geometry llava15_7b] [--batch 32] [--reps 20] [--steps 3] [--blocks 2] [--out profiles/adam8_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radvlm_amd import ops  # noqa: E402
from radvlm_amd.config import GEOMETRIES  # noqa: E402
from radvlm_amd.engine import LlavaEngine  # noqa: E402

HYPER = dict(lr=2e-5, b1=0.9, b2=0.999, eps=1e-8)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", default="llava15_7b")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--skip-step", action="store_true", help="the optimizer alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam8_bench.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    geo = GEOMETRIES[a.geometry]
    eng = LlavaEngine(geo, device="cuda:0", init="fast", seed=0)
    eng.head_rows = eng.last_layer_rows = "labeled"
    n = eng.lm.numel
    g = torch.Generator(device=eng.device).manual_seed(1)
    for s in range(0, n, 1 << 28):                           # gradients of a plausible spread, without an fp32 copy of the whole buffer
        e = min(n, s + (1 << 28))
        eng.grads[s:e].copy_(torch.empty(e - s, device=eng.device).normal_(0, 1e-3, generator=g))
    eng.init_optimizer(state_bits=32)
    eng.opt_step = 1
    groups = eng.param_groups(HYPER["lr"], 0.0)
    for s, e, glr, gwd in groups:                            # a warm state: one real step
        ops.adamw(eng.lm.flat[s:e], eng.master[s:e], eng.grads[s:e], eng.m[s:e], eng.vv[s:e], glr, HYPER["b1"], HYPER["b2"], HYPER["eps"], gwd, 1)
    m32, v32 = eng.m, eng.vv
    bytes32 = eng.optimizer_state_bytes()
    eng.init_optimizer(state_bits=8)                         # quantises the warm state; m32 / v32 stay alive for the fp32 arm
    bytes8 = eng.optimizer_state_bytes()
    launches = {32: len(groups), 8: sum(len(eng._adamw8_runs(s, e)) for s, e, _, _ in groups)}
    n8 = sum(t["n"] for t in eng.plan8.tensors.values() if t["bits"] == 8)

    def arm32():
        for s, e, glr, gwd in groups:
            ops.adamw(eng.lm.flat[s:e], eng.master[s:e], eng.grads[s:e], m32[s:e], v32[s:e], glr, HYPER["b1"], HYPER["b2"], HYPER["eps"], gwd, 2)

    def arm8():
        for s, e, glr, gwd in groups:
            for run in eng._adamw8_runs(s, e):
                if run[0] == 8:
                    _, x, y, blk, nb, tab = run
                    ops.adamw8(eng.lm.flat[x:y], eng.master[x:y], eng.grads[x:y], eng.m8[blk * 256:(blk + nb) * 256],
                               eng.v8[blk * 256:(blk + nb) * 256], eng.am8[blk:blk + nb], eng.av8[blk:blk + nb], tab, nb, glr, HYPER["b1"],
                               HYPER["b2"], HYPER["eps"], gwd, 2)
                else:
                    _, x, y, pos = run
                    ops.adamw(eng.lm.flat[x:y], eng.master[x:y], eng.grads[x:y], eng.m[pos:pos + y - x], eng.vv[pos:pos + y - x], glr,
                              HYPER["b1"], HYPER["b2"], HYPER["eps"], gwd, 2)

    for fn in (arm32, arm8, arm32, arm8):
        fn()
    torch.cuda.synchronize()
    t = {32: [], 8: []}
    for _ in range(a.reps):
        t[32].append(_timed(arm32))
        t[8].append(_timed(arm8))
    rec = dict(mode="optimizer_alone", geometry=a.geometry, device=torch.cuda.get_device_name(0), parameters=n, parameters_8bit=n8,
               reps=a.reps, fp32_ms_median=statistics.median(t[32]), int8_ms_median=statistics.median(t[8]), fp32_ms_min=min(t[32]),
               int8_ms_min=min(t[8]), launches_fp32=launches[32], launches_int8=launches[8], moment_bytes_fp32=bytes32,
               moment_bytes_int8=bytes8, bytes_per_param_fp32=28.0, bytes_per_param_int8=(28.0 * (n - n8) + (16 + 16 / 256) * n8) / n)
    rec["fp32_TBps"] = rec["bytes_per_param_fp32"] * n / rec["fp32_ms_median"] / 1e9
    rec["int8_TBps"] = rec["bytes_per_param_int8"] * n / rec["int8_ms_median"] / 1e9
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    del m32, v32
    if a.skip_step:
        return

    import bench
    batches = [bench.synthetic_batch(geo, a.batch, seed=1234 + 1000 * k) for k in range(4)]
    count = [0]

    def step():
        b = batches[count[0] % 4]
        count[0] += 1
        eng.forward(*b)
        eng.backward()
        eng.optimizer_step(lr=HYPER["lr"], weight_decay=0.0, max_grad_norm=1.0)

    eng.opt_step = 1
    times = {8: [], 32: []}
    peak = {}
    for block in range(a.blocks):
        for bits in (8, 32):
            eng.init_optimizer(state_bits=bits)
            step()                                           # warm-up of the block (and of the allocator after the conversion)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            times[bits].append((time.perf_counter() - t0) / a.steps * 1e3)
            peak[bits] = torch.cuda.max_memory_allocated() / 2 ** 30
    rec = dict(mode="training_step", geometry=a.geometry, batch=a.batch, steps_per_block=a.steps, blocks=a.blocks,
               fp32_ms_per_step=times[32], int8_ms_per_step=times[8], fp32_ms_median=statistics.median(times[32]),
               int8_ms_median=statistics.median(times[8]), peak_GiB_fp32=peak[32], peak_GiB_int8=peak[8])
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

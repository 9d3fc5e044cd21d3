"""LoRA merge measurement (rv_lora_merge_bf16 over every adapted decoder linear): one JSON line per (geometry, W load policy).

  python tools/lora_merge_bench.py [--geos llava15_7b,llava15_13b,llava_ov_qwen2_7b] [--r 64] [--reps 5] [--out FILE]

A LoRA engine per geometry (random weights, init="fast"; the arithmetic does not depend on the values) and LlavaEngine.merge_lora_ over
its own adapters, which is what merge_and_unload() launches: seven matrices per layer, in place in the frozen base store.  Device time
between two events; the launches are queued behind a device-side sleep so that host enqueue time is not measured.  The W stream (26 GB
at 7B) exceeds every cache, so each repetition runs from cold caches for W.  Byte floor: one read and one write of every adapted W plus
the reads of A and B, at 6 TB/s.  Each W load / store policy (nontemporal, the kernel's own; default: RV_LORA_MERGE_NT=0) runs in a child process of its own,
one after the other, so the two are measured on the same box.  Records carry the kernel-source hash (radvlm_amd.build_id)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from radvlm_amd.config import GEOMETRIES  # noqa: E402
from radvlm_amd.params import LORA_TARGETS  # noqa: E402

FLOOR_BW = 6e12


def _src_hash():
    try:
        from radvlm_amd.build_id import kernel_source_sha256
        return kernel_source_sha256()
    except Exception:          # noqa: BLE001 -- the hash is a label, never a reason to lose a measurement
        return None


def _sleep():
    """~80 ms of device-side spinning: the host queues every launch of the merge before the first one starts."""
    try:
        torch.cuda._sleep(200_000_000)
    except (AttributeError, RuntimeError):
        pass


def run_child(geos, r, reps):
    from radvlm_amd.engine import LlavaEngine
    out = []
    for name in geos:
        eng = LlavaEngine(GEOMETRIES[name], device="cuda:0", init="fast", seed=0, lora=dict(r=r, alpha=16, dropout=0.0))
        pairs, nbytes = {}, 0
        for i in range(eng.l["layers"]):
            for t, _, _ in LORA_TARGETS:
                pre = f"model.layers.{i}.{t}"
                A, B = eng.lm.view(pre + ".lora_A.weight"), eng.lm.view(pre + ".lora_B.weight")
                pairs[pre] = (A, B)
                N, K = B.shape[0], A.shape[1]
                nbytes += 2 * (2 * N * K + r * (N + K))
        eng.merge_lora_(pairs, 0.25)                  # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            _sleep()
            e0.record()
            eng.merge_lora_(pairs, 0.25)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = sorted(times)[len(times) // 2]
        floor_ms = nbytes / FLOOR_BW * 1e3
        out.append(dict(tool="lora_merge_bench", geometry=name, r=r, nt=os.environ.get("RV_LORA_MERGE_NT", "1") != "0",
                        matrices=len(pairs), bytes=nbytes, ms_median=round(ms, 3), ms_all=[round(t, 3) for t in times],
                        tb_per_s=round(nbytes / ms / 1e9, 3), floor_ms_6tbps=round(floor_ms, 3), share_of_floor=round(floor_ms / ms, 3),
                        device=torch.cuda.get_device_name(0), kernel_src=_src_hash()))
        del eng, pairs
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geos", default="llava15_7b,llava15_13b,llava_ov_qwen2_7b")
    ap.add_argument("--r", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_merge_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    geos = a.geos.split(",")
    if a.child:
        for rec in run_child(geos, a.r, a.reps):
            print("RECORD " + json.dumps(rec), flush=True)
        return
    recs = []
    for nt in ("0", "1"):
        env = dict(os.environ, RV_LORA_MERGE_NT=nt)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--geos", a.geos, "--r", str(a.r), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True, timeout=900)
        sys.stderr.write(p.stderr[-2000:])
        if p.returncode != 0:
            raise SystemExit(f"child (RV_LORA_MERGE_NT={nt}) exited with {p.returncode}")
        recs += [json.loads(line[len("RECORD "):]) for line in p.stdout.splitlines() if line.startswith("RECORD ")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

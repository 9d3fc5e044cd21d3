"""Knowledge-distillation (GKD) measurements: JSON lines appended to profiles/gkd_bench.jsonl.

  python tools/gkd_bench.py kernel [--reps 20] [--out FILE]

kernel   rv_distill_loss_bf16 in place at [2048, 32000] and [1024, 152064], beta 0 (forward KL: two log-sum-exps and one sweep) and 0.5
         (generalised JSD: one sweep more), with rv_cross_entropy on the same student rows as context.  (The records of
         profiles/gkd_bench.jsonl with "_reread" / "_staged" arms are the A/B that decided against keeping both rows in LDS: that form
         was deleted afterwards)  The arms alternate inside every repetition; each run restores the logits outside the timed window and is timed between device events.  Reported: the
         median of --reps, min, max, every repetition, and bytes/s against the floor of 3 * rows * ld * 2 bytes (student and teacher
         read once, gradient written once; for the cross entropy 2 * rows * ld * 2).
"""
import argparse
import json
import os
import sys

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


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernel_ab(reps):
    from radvlm_amd import lib
    dev = torch.device("cuda:0")
    recs = []
    for rows, V in ((2048, 32000), (1024, 152064)):
        g = torch.Generator(device=dev).manual_seed(V)
        src = (torch.randn(rows, V, device=dev, generator=g) * 2).to(torch.bfloat16)
        teacher = (src.float() + torch.randn(rows, V, device=dev, generator=g)).to(torch.bfloat16)
        labels = torch.randint(0, V, (rows,), device=dev, generator=g)
        labels[::17] = -100
        cw = torch.full((rows,), 1.0 / int((labels >= 0).sum()), device=dev)
        work = src.clone()
        ce_rows = torch.empty(rows, device=dev)
        stats = torch.empty(4, rows, device=dev)

        def ce():
            lib.call("rv_cross_entropy", work, V, labels, ce_rows, work, V, rows, V, float(cw[0]))

        def distill(beta):
            lib.call("rv_distill_loss_bf16", work, V, teacher, V, None, labels, cw, cw, beta, 0.9, stats, work, V, rows, V)

        arms = {"cross_entropy": ce, "beta0": lambda: distill(0.0), "beta0.5": lambda: distill(0.5)}
        times = {k: [] for k in arms}
        for rep in range(reps + 2):                      # two warm-up rounds
            for name, fn in arms.items():
                work.copy_(src)
                ms, _ = _timed(fn)
                if rep >= 2:
                    times[name].append(ms)
        floor = 3 * rows * V * 2
        rec = dict(tool="gkd_bench", part="kernel", rows=rows, V=V, reps=reps, floor_bytes=floor, temperature=0.9,
                   device=torch.cuda.get_device_name(0), build=os.path.basename(os.environ.get("RADVLM_HIP_LIB", "default")), kernel_src=_src_hash())
        for name, ts in times.items():
            nbytes = floor if name != "cross_entropy" else 2 * rows * V * 2
            rec[name] = dict(us_median=round(1e3 * _median(ts), 1), us_min=round(1e3 * min(ts), 1), us_max=round(1e3 * max(ts), 1),
                             tb_per_s_of_floor=round(nbytes / _median(ts) / 1e9, 3), us_all=[round(1e3 * t, 1) for t in ts])
        recs.append(rec)
        del src, work, teacher
        torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernel"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gkd_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gkd_bench measures on the GPU; none is visible")
    recs = kernel_ab(a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in recs:
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

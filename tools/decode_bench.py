"""Decode measurement (greedy generation, KV cache): one JSON line per case.

  python tools/decode_bench.py [--geos llava15_7b,llava_ov_qwen2_7b] [--batches 1,8,32] [--prompt 704] [--new 128] [--out FILE]
  python tools/decode_bench.py --ab [--out FILE]     # rv_gemv_bf16 vs rv_gemm_nt_bf16 at M = 1, 4, 16, 32, interleaved on one box
  python tools/decode_bench.py --processors [--geos ..] [--batches 1,32] [--out FILE]
        # plain greedy argmax vs the logits processors (repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=new/2 with an EOS)
        # through rv_logits_process_argmax_f32, interleaved (plain, processors, plain, ...) on one engine

Per case: prefill ms, median decode ms / token after warm-up, tokens / s, weight + KV bytes per step and the implied HBM rate as a share
of the 8 TB/s peak.  Random-init weights (the arithmetic does not depend on the values); text-only prompts of --prompt tokens (the
anyres Qwen prompt: --prompt 7499).  Records carry the kernel-source hash (radvlm_amd.build_id)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radvlm_amd import ops  # noqa: E402
from radvlm_amd.config import GEOMETRIES  # noqa: E402
from radvlm_amd.engine import LlavaEngine  # noqa: E402

PEAK = 8e12


def _src_hash():
    try:
        from radvlm_amd.build_id import kernel_source_sha256
        return kernel_source_sha256()
    except Exception:          # noqa: BLE001 -- the hash is a label, never a reason to lose a measurement
        return None


def weight_bytes(eng):
    l = eng.l
    d, F, L, V = l["d"], l["ffn"], l["layers"], l["vocab"]
    per_layer = (d + 2 * eng.kvd) * d + d * d + 2 * F * d + d * F
    return 2 * (L * per_layer + V * d)


def case(geo, B, prompt, new, warm=8):
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache, logits = eng.prefill(ids, None, None, None, max_new_tokens=new)
    torch.cuda.synchronize()
    prefill_ms = (time.perf_counter() - t0) * 1e3
    tok = ops.argmax_rows(logits, eng.vocab)
    times = []
    for _ in range(new - 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        logits = eng.decode_step(cache, tok.to(torch.int32))
        tok = ops.argmax_rows(logits, eng.vocab)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    steady = times[warm:]
    ms = float(np.median(steady))
    kv_bytes = int(2 * eng.l["layers"] * 2 * eng.kvd * int(cache.lens.mean()) * B)
    wb = weight_bytes(eng)
    rate = (wb + kv_bytes) / (ms * 1e-3)
    del cache
    return dict(geo=geo, B=B, prompt=prompt, new_tokens=new, prefill_ms=round(prefill_ms, 2), decode_ms_per_step=round(ms, 3),
                decode_ms_p10=round(float(np.percentile(steady, 10)), 3), decode_ms_p90=round(float(np.percentile(steady, 90)), 3),
                steps_timed=len(steady), tokens_per_s=round(B * 1e3 / ms, 1), weight_bytes=wb, kv_bytes_per_step=kv_bytes,
                implied_TBps=round(rate / 1e12, 3), share_of_8TBps=round(rate / PEAK, 3), bound="HBM (weight stream)",
                gemv_max_m=eng.gemv_max_m, kernel_src=_src_hash())


def ab(reps=20):
    """rv_gemv_bf16 vs the tiled GEMM on the 7B decode shapes, interleaved (A, B, A, B ...) so that clock / thermal drift hits both."""
    out = []
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        d, F = l["d"], l["ffn"]
        kvd = l.get("kv_heads", l["heads"]) * (d // l["heads"])
        shapes = [("qkv", d + 2 * kvd, d), ("o", d, d), ("gu", 2 * F, d), ("down", d, F), ("lm_head", l["vocab"], d)]
        for name, N, K in shapes:
            w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
            flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
            for M in (1, 4, 16, 32):
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                dt = torch.float32 if name == "lm_head" else torch.bfloat16
                fns = {"gemv": lambda: ops.gemv(x, w, out_dtype=dt), "gemm": lambda: ops.gemm_nt(x, w, out_dtype=dt)}
                ts = {k: [] for k in fns}
                for k in fns:
                    fns[k]()
                for _ in range(reps):
                    for k, f in fns.items():
                        flush.zero_()             # cold weights, as in a decode step (the other layers' weights evicted them)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                g, m = float(np.median(ts["gemv"])), float(np.median(ts["gemm"]))
                out.append(dict(geo=geo, shape=name, N=N, K=K, M=M, gemv_us=round(g, 2), gemm_us=round(m, 2), speedup=round(m / g, 3),
                                gemv_TBps=round(2 * N * K / (g * 1e-6) / 1e12, 3), split=ops.gemv_split(N, K)))
            del w, flush
    return out


def _decode_loop(eng, ids, new, lp=None, warm=8):
    """Median decode step (decode_step + token choice) in ms; with `lp` (generation.LogitsProcessors) the token comes from
    rv_logits_process_argmax_f32 and is recorded in the device history, as greedy_generate does."""
    B = ids.shape[0]
    cache, logits = eng.prefill(ids, None, None, None, max_new_tokens=new)
    hist = torch.zeros(B, new, dtype=torch.int32, device=logits.device) if lp is not None else None

    def choose(lg, t):
        if lp is None:
            return ops.argmax_rows(lg, eng.vocab)
        tk = ops.logits_process_argmax(lg, eng.vocab, hist, t, lp.penalty, lp.ngram, *lp.device_args(t, lg.device))
        hist[:, t] = tk.to(torch.int32)
        return tk

    tok = choose(logits, 0)
    times = []
    for t in range(1, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        logits = eng.decode_step(cache, tok.to(torch.int32))
        tok = choose(logits, t)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    del cache
    return times[warm:]


def processors_ab(geo, B, prompt, new, reps=3):
    from radvlm_amd.generation import LogitsProcessors, parse_generate_kwargs
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
    cfg = parse_generate_kwargs(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=new // 2, eos_token_id=2))
    lp = LogitsProcessors(cfg, eng.vocab)
    ts = {"plain": [], "processors": []}
    _decode_loop(eng, ids, 16)                                      # warm-up of both paths
    _decode_loop(eng, ids, 16, lp)
    for _ in range(reps):
        ts["plain"] += _decode_loop(eng, ids, new)
        ts["processors"] += _decode_loop(eng, ids, new, lp)
    p, q = float(np.median(ts["plain"])), float(np.median(ts["processors"]))
    return dict(geo=geo, B=B, prompt=prompt, new_tokens=new, mode="processors_ab", processors="repetition_penalty=1.2,no_repeat_ngram_size=3,"
                f"min_new_tokens={new // 2},eos=2", plain_ms_per_step=round(p, 3), processors_ms_per_step=round(q, 3),
                delta_ms=round(q - p, 4), delta_share=round((q - p) / p, 4), steps_timed_each=len(ts["plain"]), reps=reps,
                kernel_src=_src_hash())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geos", default="llava15_7b,llava_ov_qwen2_7b")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt", type=int, default=704)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--processors", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.ab:
        recs = ab()
    elif a.processors:
        recs = [processors_ab(g, b, a.prompt, a.new) for g in a.geos.split(",") for b in map(int, a.batches.split(","))]
    else:
        recs = [case(g, b, a.prompt, a.new) for g in a.geos.split(",") for b in map(int, a.batches.split(","))]
    for r in recs:
        r["kernel_src"] = r.get("kernel_src") or _src_hash()
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Decode measurement (greedy generation, KV cache): one JSON line per case.

  python tools/decode_bench.py [--geos llava15_7b,llava_ov_qwen2_7b] [--batches 1,8,32] [--prompt 704] [--new 128] [--out FILE]
  python tools/decode_bench.py --ab [--out FILE]     # rv_gemv_bf16 vs rv_gemm_nt_bf16 at M = 1, 4, 16, 32, interleaved on one box
  python tools/decode_bench.py --continue [--geos ..] [--batches 1,8] [--reps 5] [--out FILE]
        # a two-turn conversation per config on one engine: turn 2 = turn 1's prompt + its 64 generated tokens + a 40-token follow-up;
        # time to first token of turn 2 through a GenerationCache (LlavaEngine.extend) vs a fresh full call, interleaved, and decode
        # ms / step after the continuation vs after a fresh prefill.  llava15_7b: one 336 px image; llava_ov_qwen2_7b: one anyres_max_9
        # image (10 tiles of 384 px, S = 7499)
  python tools/decode_bench.py --processors [--geos ..] [--batches 1,32] [--out FILE]
        # plain greedy argmax vs the logits processors (repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=new/2 with an EOS)
        # through rv_logits_process_argmax_f32, interleaved (plain, processors, plain, ...) on one engine
  python tools/decode_bench.py --batch-eval [--geos ..] [--requests 256] [--reps 3] [--out FILE]
        # an evaluation split: N requests of --prompt tokens, EOS disabled, budgets mixed (portable_rng in [32, 512]) or equal (256);
        # (a) generate_batch(max_batch_size=32), (b) static groups of 32 through generate() (a per-row criterion ends each row at its
        # budget), (c) generate() at B = 1 on the first 16 requests; interleaved, medians; useful tokens / s and the prefill share of
        # wall time; then the admission-threshold sweep (1, 4, 8, 16 free slots) and rv_logits_process_argmax_rows_f32 vs
        # rv_logits_process_argmax_f32 at 32 rows x vocab
  python tools/decode_bench.py --batch-kernel-ab [--geos ..]  # the kernel A/B of --batch-eval alone
  python tools/decode_bench.py --batch-trace [--geos ..]     # generate_batch with processors + logprobs, then generate() B = 32 with
        # the same processors: the workload of `rocprofv3 --kernel-trace --stats` for the two kernels side by side
  python tools/decode_bench.py --w8 [--geos ..] [--batches 1,8,32] [--out FILE]
        # int8 decoder weights: one engine per geometry, quantize_decoder_(), then the decode loop with engine.w8_decode False / True
        # interleaved three times (bf16 kernel on the dequantised weights vs rv_gemv_w8_bf16: same output bits); medians per arm, the
        # bf16 arm's spread, bytes per step and the implied HBM rate; plus how far the quantised model's logits and greedy tokens are
        # from the unquantised model's on the same prompt (a property of the scheme, reported, never gated)
  python tools/decode_bench.py --w8-shapes [--out FILE]   # per-shape kernel A/B: rv_gemv_bf16 on the dequantised weight vs
        # rv_gemv_w8_bf16, the 7B Llama and Qwen2-7B decoder shapes, M = 1, 4, 8, 16, 32, cold weights, interleaved
  python tools/decode_bench.py --w8-quality   # the toy goldens' models: logits distance and greedy-token agreement, int8 vs unquantised
  python tools/decode_bench.py --w4 | --w4-shapes | --w4-quality   # the same three for MXFP4 decoder weights (quantize_decoder_("mxfp4"),
        # rv_gemv_w4_bf16, engine.w4_decode); the int8 kernel / an int8 engine is timed in the same rounds, for information
  python tools/decode_bench.py --w8-trace [--geos llava15_7b]   # a B = 1 int8 decode run: the workload of `rocprofv3 --kernel-trace --stats`
  python tools/decode_bench.py --kv8 [--geos ..] [--batches 1,8,32] [--out FILE]
        # int8 KV cache: one engine per geometry, the decode loop on an int8-dtype cache with engine.kv8_decode False / True interleaved
        # three times after one untimed repetition of both (rv_attn_decode_bf16 on the dequantised bf16 rows vs rv_attn_decode_kv8_bf16
        # on the int8 rows: same output bits), then the same after quantize_decoder_(); medians per arm, the reference arm's spread and
        # the KV bytes per step of both arms
  python tools/decode_bench.py --kv8-shapes [--out FILE]   # kernel A/B of the two attention entries: the 7B and Qwen2-7B head shapes,
        # 704 and 7,603 keys, B = 1, 8, 32, cold cache, interleaved; torch.equal is asserted before timing
  python tools/decode_bench.py --kv8-quality   # the toy goldens' models: next-step logits distance and greedy-token agreement, int8
        # cache vs bf16 cache (measured and recorded, never gated)
  python tools/decode_bench.py --kv8-trace [--geos llava15_7b] [--batches 32]   # an int8-cache decode run: the workload of
        # `rocprofv3 --kernel-trace --stats`
  python tools/decode_bench.py --sample [--geos ..] [--batches 1,8,32] [--out FILE]
        # seeded sampling: (1) rv_sample_rows_f32 (the chat default T=0.2 top_k=50 top_p=0.7, and every warper on) vs
        # rv_logits_process_argmax_rows_f32 with logprobs (one read of the row) at 1 and 32 rows x 32,000 and 152,064, device time,
        # interleaved; (2) the decode step with the token drawn by the sampler vs the greedy argmax on one engine: one untimed
        # repetition, the two arms alternated three times, medians of medians, and the gate sampled <= greedy + the greedy arm's
        # spread + the cost of the launches sampling adds (10 with the chat default: one launch per sweep and one for the draw in
        # place of the argmax launch) at the step's enqueue rate, greedy step / DECODE_LAUNCHES
  python tools/decode_bench.py --beams [--geos ..] [--prompt 704] [--new 48] [--out FILE]
        # beam search: (a) ms per beam step (log-softmax, top-K, the one device-to-host copy, BeamState on the host, the ancestry table
        # upload, decode_step(beams=)) for num_beams 1, 3, 5 at B = 1 and 8, beside this build's plain decode step (decode_step + argmax)
        # at batch B * num_beams, the two arms alternated three times on one engine; (b) rv_attn_decode_beam_bf16 with an identity
        # table vs rv_attn_decode_bf16 on the same cache, device time, interleaved; (c) kv_cache_bytes of the B * num_beams rows, which
        # a per-step reorder of the cache (HF's reorder_cache) would read and write once per generated token
  python tools/decode_bench.py --lookup [--geos ..] [--prompt 704] [--new 128] [--out FILE]
        # prompt-lookup decoding: (a) generate() at B = 1 plain vs prompt_lookup_num_tokens = 3, 7, 15 on one engine, bf16 and then int8
        # weights, every arm run once untimed and then three times interleaved, ms per emitted token after the prompt pass (the call's
        # wall time less that of the same call with max_new_tokens=1), medians over the three; the drafter is injected: an oracle (the
        # plain run's own continuation: k + 1 tokens per step, the ceiling), one that is never right (the cost of a wasted verify
        # step, the floor) and the real PromptLookupDrafter on this random-weight model (labelled as such: it says nothing about a
        # trained checkpoint); the break-even acceptance the floor implies; (b) rv_attn_decode_verify_bf16 vs the same R rows through
        # rv_attn_decode_beam_bf16 (prefix_row 0, prefix_len L_max: the same bits) for R = 4, 8, 16, 32 at 704 and 7603 keys, device
        # time, interleaved, three medians per arm
  python tools/decode_bench.py --lookup-kernel-ab [--geos ..]   # (b) alone
  python tools/decode_bench.py --cfg [--geos ..] [--batches 1,8,16] [--prompt 704] [--new 128] [--out FILE]
        # classifier-free guidance: (1) rv_cfg_guide_rows_f32's two launch structures (pair: one workgroup per row pair; split: row
        # statistics, then an elementwise launch over many workgroups) and the unfused baseline (rv_log_softmax_rows_f32 twice, then
        # three torch elementwise kernels) at 32,000 and 152,064 columns, 1 and 16 rows, device time, median of 50, interleaved, on
        # rows just written (warm) and after a 1 GiB fill has evicted them (cold); (2) the decode step (decode_step + guide + argmax)
        # of a guided run of B requests -- 2 * B cache rows -- with a full-length and with a 1-token negative prompt, beside the plain
        # step at B and at 2 * B rows, on one engine: one untimed pass of every arm, then the arms alternated three times; median ms
        # per step per arm, the spread of the three medians, guided / plain(B), guided / plain(2B) and whether the guided step lies
        # below 2 x plain(B) -- HF's two forward passes -- by more than the plain arm's spread; the guide launch's share of the step
  python tools/decode_bench.py --cfg-kernel-ab   # (1) alone
  python tools/decode_bench.py --shared-shapes [--out FILE]   # kernel A/B of shared prompt prefixes: rv_attn_decode_bf16 vs
        # rv_attn_decode_shared_bf16 on one cache, the 7B and Qwen2-7B head shapes, 704 and 7,603 shared keys (each row 40 keys of
        # its own after them), B = 32 rows in groups of 2, 4, 8, 16, 32 that hold one prefix; the protocol of --kv8-shapes: cold
        # cache, interleaved, median of 20, torch.equal asserted before timing; the plain arm's p10 / p90 are its spread
  python tools/decode_bench.py --share-prefix [--geos ..] [--new 32] [--out FILE]
        # generate_batch end to end: 64 requests = 8 images x 8 questions of 24 - 40 tokens behind a 35-token system prompt and
        # the image (llava_ov_qwen2_7b: anyres_max_9, 10 tiles, 8 slots), image-major order, 32 slots, EOS disabled; arms: sharing off,
        # sharing on with shared_route "plain" and with "shared", one untimed pass of each and then interleaved three times; per
        # arm the median wall time with that run's time inside prefill / extend, tower runs (calls, images) and decode ms / step
  python tools/decode_bench.py --score-shapes [--out FILE]   # kernel A/B of scoring: rv_attn_extend_bf16 on the materialised cache
        # (every candidate's row holds a copy of the prompt's keys) vs rv_attn_extend_prefix_bf16 (one prompt row read in place), the 7B
        # and Qwen2-7B head shapes, a 704-position prompt with 2, 8, 32 candidates of 4 and of 64 tokens (3 / 63 rows each); the
        # protocol of --kv8-shapes: cold cache, interleaved, median of 20, torch.equal asserted before timing; the extend arm's
        # p10 / p90 are its spread; plus the bytes per candidate of the copy the prefix kernel avoids, over the layers
  python tools/decode_bench.py --kvpress-shapes [--out FILE]   # prompt cache compression's three kernels per layer: rv_kv_votes_f32,
        # rv_kv_select_i32, rv_kv_gather_bf16 on random q|k|v rows, the 7B and Qwen2-7B head shapes, 704 and 7,603 keys (budget
        # min(1024, keys / 2), window 32, pool 7), B = 1, 8, 32; the protocol of --kv8-shapes: cold cache, interleaved, median of 20
  python tools/decode_bench.py --kvpress [--geos ..] [--batches 1,8,32] [--prompt 7603] [--out FILE]
        # decode ms / step, cache bytes and prompt-pass ms with and without prompt_kv_budget=1024 at a 7,603-position prompt (one
        # untimed pass of both arms, then interleaved), after the toy goldens' quality figures (first decode step's logits, relative
        # L2, and the share of agreeing greedy tokens against the uncompressed call, at budgets of 1/2 and 1/4 of the prompt)
  python tools/decode_bench.py --score [--geos ..] [--reps 3] [--out FILE]
        # model.score() against the one-by-one route: the training forward on prompt + candidate with the candidate as labels,
        # reading the loss, once per candidate (the tower and the prompt's rows run every time); one image prompt of 704 spliced
        # positions (or the shortest the geometry's image allows), C = 2, 8, 32 candidates of 4 and of 64 tokens, one engine per
        # geometry, one untimed pass of both arms and then the arms alternated --reps times; wall ms per call, medians, the
        # one-by-one arm's spread (max - min) and whether score() is faster by more than that spread; the decoder rows of both arms
  python tools/decode_bench.py --dola-shapes [--out FILE]   # DoLa's kernel alone: rv_dola_contrast_rows_f32 against the unfused
        # composition (rv_log_softmax_rows_f32 twice, torch's exp / log / products, sum, argmax, masked subtraction) on the same rows,
        # 32,000 columns with 8 candidates and 152,064 with 7, rows 1, 8, 32; torch.equal asserted before timing; device time,
        # interleaved, median of 20, warm and after a 1 GiB fill; the unfused arm's p10 / p90 are its spread
  python tools/decode_bench.py --dola [--geos ..] [--batches 1,8,32] [--prompt 704] [--new 128] [--out FILE]
        # the decode step (decode_step + contrast + argmax) with dola_layers="high" beside the plain step on one engine: one untimed
        # pass of every arm, then the arms alternated three times; median ms per step per arm, the spread of the three medians, the
        # added ms per step, and the candidates' lm_head rows in a second launch against stacked with the mature rows into one
        # skinny launch where that keeps the mature rows' bits (LlavaEngine.tap_lm_head)
  python tools/decode_bench.py --constraint [--geos ..] [--batches 1,32] [--prompt 704] [--new 128] [--out FILE]
        # constrained decoding: (1) rv_constrain_rows_f32 alone at 32,000 and 152,064 columns, 1 and 32 rows, a state that allows one
        # id (the mask stores n - 1 columns) and one that allows every id (no store), each with and without the advance in front,
        # device time, median of 50, warm; (2) the decode step (decode_step + constrain + argmax) with a from_choices constraint of
        # 8 choices of --new tokens, so that every row stays live for the whole loop, beside the plain step on one engine: one untimed
        # pass of both arms, then the arms alternated three times; median ms per step per arm, the plain arm's spread, the added ms
  python tools/decode_bench.py --assistant [--geos llava15_7b] [--draft-layers 4] [--prompt 704] [--new 128] [--out profiles/assist_bench.jsonl]
        # assisted generation at B = 1 with a draft of the target's width and --draft-layers layers: the plain step, the draft step,
        # verify_step at R = k + 1 for k = 3, 5, 7, 15 and the accept kernel (alone, and with the sampler's warp of the R rows), wall ms,
        # medians; then greedy generate(assistant_model=) end to end with a drafter that runs the draft engine for real and proposes
        # scripted tokens, at acceptance 0, k // 2 and k of k: ms per token, tokens / s, speed-up over the plain call on the same box and
        # in the same run, and the break-even accepted drafts per round (random weights have no acceptance rate of their own)
  python tools/decode_bench.py --lora [--geos ..] [--batches 1,32] [--prompt 704] [--new 40] [--out FILE]
        # decoding on live LoRA adapters (r = 64): the decode step on merged weights, on the live adapters and on the live adapters
        # switched off, interleaved on one box; median and p10 / p90 of 20 samples per arm (a sample: the median step of one loop),
        # live / merged beside the adapters' share of the streamed weight bytes

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


def w8_shapes(reps=20):
    """rv_gemv_bf16 on the dequantised weight vs rv_gemv_w8_bf16 per decoder shape, interleaved, cold weights (as ab())."""
    out = []
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        d, F = l["d"], l["ffn"]
        kvd = l.get("kv_heads", l["heads"]) * (d // l["heads"])
        for name, N, K in [("qkv", d + 2 * kvd, d), ("o", d, d), ("gu", 2 * F, d), ("down", d, F)]:
            w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
            packed, scale = ops.quantize_rows_w8(w)
            flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
            for M in (1, 4, 8, 16, 32):
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                fns = {"bf16": lambda: ops.gemv(x, w), "w8": lambda: ops.gemv_w8(x, packed, scale, K)}
                assert torch.equal(fns["bf16"](), fns["w8"]())
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, f in fns.items():
                        flush.zero_()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                b, q = float(np.median(ts["bf16"])), float(np.median(ts["w8"]))
                out.append(dict(mode="w8", geo=geo, shape=name, N=N, K=K, M=M, bf16_us=round(b, 2), w8_us=round(q, 2), speedup=round(b / q, 3),
                                bf16_TBps=round(2 * N * K / (b * 1e-6) / 1e12, 3), w8_TBps=round((N * packed.shape[1] + 4 * N) / (q * 1e-6) / 1e12, 3),
                                split=ops.gemv_split(N, K), layout="16-byte interleaved step pairs",
                                build=os.path.basename(os.environ.get("RADVLM_HIP_LIB", "default")), kernel_src=_src_hash()))
            del w, packed, flush
    return out


def w8_weight_bytes(eng):
    """Weight bytes a decode step reads on the int8 route: packed rows + scales of the four decoder matrices, bf16 lm_head."""
    l = eng.l
    q = sum(p.numel() + 4 * s.numel() for layer in eng.w8 for p, s in layer.values())
    return int(q + 2 * l["vocab"] * l["d"])


def w8_ab(geo, batches, prompt, new, reps=3):
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    rng = np.random.default_rng(0)
    ids1 = rng.integers(0, eng.vocab, (1, prompt))

    def greedy(n):
        cache, logits = eng.prefill(ids1, None, None, None, max_new_tokens=n)
        first = logits[0].clone()
        toks = [ops.argmax_rows(logits, eng.vocab)]
        for _ in range(n - 1):
            toks.append(ops.argmax_rows(eng.decode_step(cache, toks[-1].to(torch.int32)), eng.vocab))
        return first, torch.cat(toks).cpu().numpy()

    lg0, tk0 = greedy(64)                                             # the unquantised model on the prompt of the timed runs
    eng.quantize_decoder_()
    lg1, tk1 = greedy(64)
    quality = dict(logits_rel_l2=round(float((lg1 - lg0).norm() / lg0.norm()), 5), greedy_tokens_agree=round(float((tk0 == tk1).mean()), 4),
                   first_disagreement=int(np.argmax(tk0 != tk1)) if (tk0 != tk1).any() else None, tokens=64)
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        ts = {False: [], True: []}
        for flag in (False, True):                                     # warm-up: one untimed repetition of both routes
            eng.w8_decode = flag
            _decode_loop(eng, ids, new)
        for _ in range(reps):
            for flag in (False, True):
                eng.w8_decode = flag
                ts[flag].append(float(np.median(_decode_loop(eng, ids, new))))
        eng.w8_decode = True
        b, q = float(np.median(ts[False])), float(np.median(ts[True]))
        kv = int(2 * eng.l["layers"] * 2 * eng.kvd * (prompt + new // 2) * B)
        wb, w8b = weight_bytes(eng), w8_weight_bytes(eng)
        recs.append(dict(geo=geo, mode="w8_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, bf16_ms_per_step=round(b, 3),
                         w8_ms_per_step=round(q, 3), bf16_ms_all=[round(x, 3) for x in ts[False]], w8_ms_all=[round(x, 3) for x in ts[True]],
                         bf16_spread_ms=round(max(ts[False]) - min(ts[False]), 3), delta_ms=round(b - q, 3), speedup=round(b / q, 3),
                         w8_faster_by_more_than_bf16_spread=bool(b - q > max(ts[False]) - min(ts[False])),
                         bf16_tokens_per_s=round(B * 1e3 / b, 1), w8_tokens_per_s=round(B * 1e3 / q, 1), bf16_weight_bytes=wb,
                         w8_weight_bytes=w8b, weight_bytes_ratio=round(w8b / wb, 3), kv_bytes_per_step=kv,
                         bf16_implied_TBps=round((wb + kv) / (b * 1e-3) / 1e12, 3), w8_implied_TBps=round((w8b + kv) / (q * 1e-3) / 1e12, 3),
                         quality_vs_unquantised=quality, kernel_src=_src_hash()))
    return recs


def w8_quality_toy(new=32, fmt="int8"):
    """How far int8 (or, fmt="mxfp4", 4-bit) decoder weights move the toy goldens' models (portable-init weights, the golden prompts with their images): relative
    L2 of the last prompt row's logits and the share of greedy tokens that agree with the unquantised model.  Reported, never gated."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    recs = []
    for geo, golden in (("toy", "toy_e2e"), ("toy_qwen", "toy_qwen_e2e")):
        g = np.load(os.path.join(root, golden + ".npz"))
        n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
        images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
        sizes = [tuple(x) for x in g["image_sizes"].tolist()]
        eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="portable", seed=0)

        def run():
            out = []
            for b in range(n):
                p = g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)
                cache, logits = eng.prefill(p[None], None, [images[b]], [sizes[b]], max_new_tokens=new)
                toks = [ops.argmax_rows(logits, eng.vocab)]
                for _ in range(new - 1):
                    toks.append(ops.argmax_rows(eng.decode_step(cache, toks[-1].to(torch.int32)), eng.vocab))
                out.append((logits[0].clone(), torch.cat(toks).cpu().numpy()))
            return out

        a = run()
        eng.quantize_decoder_(fmt)
        b = run()
        recs.append(dict(geo=geo, mode="w8_quality_toy" if fmt == "int8" else "w4_quality_toy", prompts=n, new_tokens=new,
                         logits_rel_l2=[round(float((y[0] - x[0]).norm() / x[0].norm()), 5) for x, y in zip(a, b)],
                         greedy_tokens_agree=[round(float((x[1] == y[1]).mean()), 4) for x, y in zip(a, b)]))
    return recs


def _timed_interleaved(fns, flush, reps):
    """Every function of `fns` timed `reps` times in turn (A, B, C, A, B, C ...) on cold weights; microseconds per call."""
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return ts


def w4_shapes(reps=20):
    """rv_gemv_bf16 on the MXFP4-quantised weight vs rv_gemv_w4_bf16 per decoder shape (the same output bits), interleaved, cold weights,
    as w8_shapes(); the int8 kernel on an int8 copy of the same weight is timed in the same rounds, for information."""
    out = []
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        d, F = l["d"], l["ffn"]
        kvd = l.get("kv_heads", l["heads"]) * (d // l["heads"])
        for name, N, K in [("qkv", d + 2 * kvd, d), ("o", d, d), ("gu", 2 * F, d), ("down", d, F)]:
            w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
            packed, scales = ops.quantize_rows_mxfp4(w)
            p8, s8 = ops.quantize_rows_w8(w.clone())
            flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
            for M in (1, 4, 8, 16, 32):
                x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
                fns = {"bf16": lambda: ops.gemv(x, w), "w4": lambda: ops.gemv_w4(x, packed, scales, K), "w8": lambda: ops.gemv_w8(x, p8, s8, K)}
                assert torch.equal(fns["bf16"](), fns["w4"]())
                fns["w8"]()
                ts = _timed_interleaved(fns, flush, reps)
                b, q, q8 = (float(np.median(ts[k])) for k in ("bf16", "w4", "w8"))
                spread = float(np.percentile(ts["bf16"], 75) - np.percentile(ts["bf16"], 25))
                out.append(dict(mode="w4", geo=geo, shape=name, N=N, K=K, M=M, bf16_us=round(b, 2), w4_us=round(q, 2), w8_us=round(q8, 2),
                                speedup=round(b / q, 3), speedup_vs_w8=round(q8 / q, 3), bf16_iqr_us=round(spread, 2),
                                bf16_min_us=round(min(ts["bf16"]), 2), bf16_max_us=round(max(ts["bf16"]), 2),
                                w4_faster_by_more_than_bf16_spread=bool(b - q > max(ts["bf16"]) - min(ts["bf16"])),
                                bf16_TBps=round(2 * N * K / (b * 1e-6) / 1e12, 3),
                                w4_TBps=round(N * (packed.shape[1] + scales.shape[1]) / (q * 1e-6) / 1e12, 3),
                                split=ops.gemv_split(N, K), layout="16-byte interleaved step quads + E8M0 bytes",
                                build=os.path.basename(os.environ.get("RADVLM_HIP_LIB", "default")), kernel_src=_src_hash()))
            del w, packed, scales, p8, s8, flush
    return out


def w4_weight_bytes(eng):
    """Weight bytes a decode step reads on the 4-bit route: nibble rows + scale bytes of the four decoder matrices, bf16 lm_head."""
    l = eng.l
    q = sum(p.numel() + s.numel() for layer in eng.w4 for p, s in layer.values())
    return int(q + 2 * l["vocab"] * l["d"])


def w4_ab(geo, batches, prompt, new, reps=3):
    """The --w8 protocol for MXFP4: the decode step with engine.w4_decode False / True, interleaved `reps` times; a second engine with
    int8 weights is timed in the same rounds (the int8 figure of the same box)."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    eng8 = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    ids1 = np.random.default_rng(0).integers(0, eng.vocab, (1, prompt))

    def greedy(e, n):
        cache, logits = e.prefill(ids1, None, None, None, max_new_tokens=n)
        first = logits[0].clone()
        toks = [ops.argmax_rows(logits, e.vocab)]
        for _ in range(n - 1):
            toks.append(ops.argmax_rows(e.decode_step(cache, toks[-1].to(torch.int32)), e.vocab))
        return first, torch.cat(toks).cpu().numpy()

    lg0, tk0 = greedy(eng, 64)                                        # the unquantised model on the prompt of the timed runs
    eng.quantize_decoder_("mxfp4")
    eng8.quantize_decoder_("int8")
    quality = {}
    for name, e in (("mxfp4", eng), ("int8", eng8)):
        lg1, tk1 = greedy(e, 64)
        quality[name] = dict(logits_rel_l2=round(float((lg1 - lg0).norm() / lg0.norm()), 5),
                             greedy_tokens_agree=round(float((tk0 == tk1).mean()), 4),
                             first_disagreement=int(np.argmax(tk0 != tk1)) if (tk0 != tk1).any() else None, tokens=64)
    arms = {"bf16": (eng, False), "w4": (eng, True), "w8": (eng8, True)}
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        ts = {k: [] for k in arms}

        def run(k):
            e, flag = arms[k]
            e.w4_decode = flag
            try:
                return float(np.median(_decode_loop(e, ids, new)))
            finally:
                e.w4_decode = True

        for k in arms:                                                 # warm-up: one untimed repetition of every arm
            run(k)
        for _ in range(reps):
            for k in arms:
                ts[k].append(run(k))
        b, q, q8 = (float(np.median(ts[k])) for k in ("bf16", "w4", "w8"))
        kv = int(2 * eng.l["layers"] * 2 * eng.kvd * (prompt + new // 2) * B)
        wb, w4b, w8b = weight_bytes(eng), w4_weight_bytes(eng), w8_weight_bytes(eng8)
        recs.append(dict(geo=geo, mode="w4_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, bf16_ms_per_step=round(b, 3),
                         w4_ms_per_step=round(q, 3), w8_ms_per_step=round(q8, 3), bf16_ms_all=[round(x, 3) for x in ts["bf16"]],
                         w4_ms_all=[round(x, 3) for x in ts["w4"]], w8_ms_all=[round(x, 3) for x in ts["w8"]],
                         bf16_spread_ms=round(max(ts["bf16"]) - min(ts["bf16"]), 3), delta_ms=round(b - q, 3), speedup=round(b / q, 3),
                         w4_faster_by_more_than_bf16_spread=bool(b - q > max(ts["bf16"]) - min(ts["bf16"])),
                         bf16_tokens_per_s=round(B * 1e3 / b, 1), w4_tokens_per_s=round(B * 1e3 / q, 1), w8_tokens_per_s=round(B * 1e3 / q8, 1),
                         bf16_weight_bytes=wb, w4_weight_bytes=w4b, w8_weight_bytes=w8b, weight_bytes_ratio=round(w4b / wb, 3),
                         kv_bytes_per_step=kv, bf16_implied_TBps=round((wb + kv) / (b * 1e-3) / 1e12, 3),
                         w4_implied_TBps=round((w4b + kv) / (q * 1e-3) / 1e12, 3), quality_vs_unquantised=quality, kernel_src=_src_hash()))
    return recs


def w8_trace(geo, prompt, new):
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    eng.quantize_decoder_()
    ids = np.random.default_rng(0).integers(0, eng.vocab, (1, prompt))
    ts = _decode_loop(eng, ids, new)
    torch.cuda.synchronize()
    return [dict(geo=geo, mode="w8_trace", B=1, prompt=prompt, new_tokens=new, w8_ms_per_step_under_trace=round(float(np.median(ts)), 3),
                 kernel_src=_src_hash())]


def _decode_loop(eng, ids, new, lp=None, warm=8, sm=None, kv_dtype=None, con=None, attn=None, press=None):
    """Median decode step (decode_step + token choice) in ms; with `lp` (generation.LogitsProcessors) the token comes from
    rv_logits_process_argmax_f32 and is recorded in the device history, as greedy_generate does; with `sm` (the sampling settings of
    parse_generate_kwargs) it is drawn by rv_sample_rows_f32, row b with seed sm.seed + b, as greedy_generate does.  kv_dtype: the
    cache's dtype (prefill's kv_dtype).  con (a constraints.TokenConstraint for every row): ops.constrain_rows advances and masks each
    step's rows before the token choice, as greedy_generate does (the host mirror of the states is not part of the loop).  attn
    (decode_step's attn_layers= / attn_mean= as a dict): every step also returns its attention maps, as generate(output_attentions=True)
    asks for them; they are dropped here.  press (prefill's compress=(N, w, k)): the loop runs on the compressed prompt cache."""
    B = ids.shape[0]
    cache, logits = eng.prefill(ids, None, None, None, max_new_tokens=new, **({} if kv_dtype is None else dict(kv_dtype=kv_dtype)),
                                **({} if press is None else dict(compress=press)))
    if con is not None:
        tabs = con.device_tables(logits.device)
        cstate = torch.full((B,), con.start, dtype=torch.int32, device=logits.device)
        ops.constrain_rows(logits, eng.vocab, cstate, tabs)
    hist = torch.zeros(B, new, dtype=torch.int32, device=logits.device) if lp is not None else None
    if sm is not None:
        seeds = torch.tensor([sm.seed + b for b in range(B)], dtype=torch.int64, device=logits.device)
        steps = torch.arange(new, dtype=torch.int32, device=logits.device)[:, None].expand(new, B).contiguous()
        ws = ops.sample_rows_workspace(B, logits.device)

    def choose(lg, t):
        if sm is not None:
            return ops.sample_rows(lg, eng.vocab, seeds, steps[t], sm.temperature, sm.top_k, sm.top_p, sm.min_p, ws=ws)
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
        logits = eng.decode_step(cache, tok.to(torch.int32)) if attn is None else eng.decode_step(cache, tok.to(torch.int32), **attn)[0]
        if con is not None:
            ops.constrain_rows(logits, eng.vocab, cstate, tabs, tok=tok)
        tok = choose(logits, t)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    del cache
    if con is not None:
        assert int((cstate < 0).sum()) == 0                        # every row stayed inside its choice for the whole loop
    return times[warm:]


def _long_choices(vocab, new, k=8, seed=0):
    """k answer choices of `new` tokens each over distinct ids, so that a row stays live for a whole loop of `new` steps: the first step
    allows k ids, every later one a single id, and the mask stores vocab - 1 columns of -inf per row and step."""
    from radvlm_amd.constraints import TokenConstraint
    ids = np.random.default_rng(seed).permutation(vocab)[:k * new + 1]
    return TokenConstraint.from_choices(ids[:k * new].reshape(k, new).tolist(), eos=[int(ids[-1])])


def constraint_ab(geo, batches, prompt, new, reps=3):
    """The decode step with a from_choices constraint (ops.constrain_rows before the argmax) beside the plain decode step on one
    engine, interleaved `reps` times as --kv8 does: one untimed pass of both arms, then the median step of every pass."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    con = _long_choices(eng.vocab, new)
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        arms = {"plain": lambda: _decode_loop(eng, ids, new), "constrained": lambda: _decode_loop(eng, ids, new, con=con)}
        for fn in arms.values():
            fn()
        ts = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ts[k].append(float(np.median(fn())))
        p, c = float(np.median(ts["plain"])), float(np.median(ts["constrained"]))
        spread = max(ts["plain"]) - min(ts["plain"])
        recs.append(dict(geo=geo, mode="constraint_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, vocab=eng.vocab, n_states=con.n_states,
                         n_edges=con.n_edges, plain_ms_per_step=round(p, 3), constrained_ms_per_step=round(c, 3),
                         plain_ms_all=[round(x, 3) for x in ts["plain"]], constrained_ms_all=[round(x, 3) for x in ts["constrained"]],
                         plain_spread_ms=round(spread, 3), added_ms=round(c - p, 3), constrained_over_plain=round(c / p, 4),
                         added_beyond_plain_spread=bool(c - p > spread)))
    return recs


def constraint_shapes(reps=50):
    """rv_constrain_rows_f32 alone at n = 32,000 and 152,064, rows 1 and 32: a state that allows one id (the mask stores n - 1
    columns), a state that allows every id (no store: the walk over n edges alone), each also with the advance (tok=) in front.
    Device time per call (events around it), median of `reps`, warm."""
    from radvlm_amd.constraints import TokenConstraint
    recs = []
    for n in (32000, 152064):
        every = {i: 0 for i in range(n)}
        con = TokenConstraint._from_edges([every, {n // 2: 1}])
        tabs = con.device_tables("cuda")
        for rows in (1, 32):
            x = torch.randn(rows, n, device="cuda")
            rec = dict(mode="constraint_kernel", kernel_form="whole-row bitmap", rows=rows, vocab=n, reps=reps, stored_bytes_one_id=4 * (n - 1) * rows)
            for name, s in (("one_id", 1), ("every_id", 0)):
                for adv in (False, True):
                    state = torch.full((rows,), s, dtype=torch.int32, device="cuda")
                    tok = torch.full((rows,), n // 2, dtype=torch.int64, device="cuda") if adv else None
                    us = []
                    for _ in range(reps + 5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        ops.constrain_rows(x, n, state, tabs, tok=tok)
                        e1.record()
                        e1.synchronize()
                        us.append(e0.elapsed_time(e1) * 1e3)
                    assert int(state[0]) == s                       # both states loop on n // 2
                    us = us[5:]
                    key = f"{name}{'_advance' if adv else ''}"
                    rec[f"{key}_us"] = round(float(np.median(us)), 2)
                    rec[f"{key}_p10_p90_us"] = [round(float(np.percentile(us, 10)), 2), round(float(np.percentile(us, 90)), 2)]
            recs.append(rec)
    return recs


def kv8_ab(geo, batches, prompt, new, reps=3):
    """The decode step on an int8-dtype cache, reference arm (dequantised bf16 rows, rv_attn_decode_bf16) vs int8 arm, bf16 weights and
    then int8 weights, on one engine."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    recs = []
    for weights in ("bf16", "int8"):
        if weights == "int8":
            eng.quantize_decoder_()
        for B in batches:
            ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
            ts = {False: [], True: []}
            for flag in (False, True):                                 # warm-up: one untimed repetition of both arms
                eng.kv8_decode = flag
                _decode_loop(eng, ids, new, kv_dtype="int8")
            for _ in range(reps):
                for flag in (False, True):
                    eng.kv8_decode = flag
                    ts[flag].append(float(np.median(_decode_loop(eng, ids, new, kv_dtype="int8"))))
            eng.kv8_decode = True
            b, q = float(np.median(ts[False])), float(np.median(ts[True]))
            keys = (prompt + new // 2) * B * eng.l["layers"]
            kv16, kv8 = int(keys * 4 * eng.kvd), int(keys * (2 * eng.kvd + 8 * eng.Hkv))
            wb = w8_weight_bytes(eng) if weights == "int8" else weight_bytes(eng)
            recs.append(dict(geo=geo, mode="kv8_ab", weights=weights, B=B, prompt=prompt, new_tokens=new, reps=reps, ref_ms_per_step=round(b, 3),
                             kv8_ms_per_step=round(q, 3), ref_ms_all=[round(x, 3) for x in ts[False]], kv8_ms_all=[round(x, 3) for x in ts[True]],
                             ref_spread_ms=round(max(ts[False]) - min(ts[False]), 3), delta_ms=round(b - q, 3), speedup=round(b / q, 3),
                             kv8_faster_by_more_than_ref_spread=bool(b - q > max(ts[False]) - min(ts[False])),
                             ref_tokens_per_s=round(B * 1e3 / b, 1), kv8_tokens_per_s=round(B * 1e3 / q, 1), weight_bytes=wb,
                             ref_kv_bytes_per_step=kv16, kv8_kv_bytes_per_step=kv8, kv_bytes_ratio=round(kv8 / kv16, 3),
                             ref_implied_TBps=round((wb + kv16) / (b * 1e-3) / 1e12, 3), kv8_implied_TBps=round((wb + kv8) / (q * 1e-3) / 1e12, 3),
                             kernel_src=_src_hash()))
    return recs


def kv8_shapes(reps=20, keys=(704, 7603), batches=(1, 8, 32)):
    """rv_attn_decode_bf16 on the dequantised cache vs rv_attn_decode_kv8_bf16 on the int8 cache per head shape, interleaved, cold cache."""
    out = []
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        H, hd = l["heads"], l["d"] // l["heads"]
        Hkv = l.get("kv_heads", H)
        kvd = Hkv * hd
        for n in keys:
            for B in batches:
                src = torch.randn(B * n, 2 * kvd, device="cuda", dtype=torch.bfloat16)
                q8 = torch.zeros(B, n, 2 * kvd, dtype=torch.int8, device="cuda")
                s = torch.ones(B, n, 2 * Hkv, dtype=torch.float32, device="cuda")
                deq = torch.zeros(B, n, 2 * kvd, dtype=torch.bfloat16, device="cuda")
                ops.kv_quantize_rows(src, torch.arange(B * n, dtype=torch.int64, device="cuda"), Hkv, hd, cache=(q8, s), xhat=deq)
                del src
                q = torch.randn(B, H * hd, device="cuda", dtype=torch.bfloat16)
                kv_len = torch.full((B,), n, dtype=torch.int32, device="cuda")
                fns = {"bf16": lambda: ops.attn_decode(q, deq, kv_len, H, Hkv, hd, kvd), "kv8": lambda: ops.attn_decode_kv8(q, (q8, s), kv_len, H, Hkv, hd, kvd)}
                assert torch.equal(fns["bf16"](), fns["kv8"]())
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, f in fns.items():
                        flush.zero_()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                b, k8 = float(np.median(ts["bf16"])), float(np.median(ts["kv8"]))
                by16, by8 = B * n * 4 * kvd, B * n * (2 * kvd + 8 * Hkv)
                out.append(dict(mode="kv8_kernel_ab", geo=geo, H=H, Hkv=Hkv, hd=hd, keys=n, B=B, bf16_us=round(b, 2), kv8_us=round(k8, 2),
                                speedup=round(b / k8, 3), bf16_TBps=round(by16 / (b * 1e-6) / 1e12, 3), kv8_TBps=round(by8 / (k8 * 1e-6) / 1e12, 3),
                                chunk=128, kernel_src=_src_hash()))
                del q8, s, deq
    return out


def kv8_quality_toy(new=32):
    """How far an int8 KV cache moves the toy goldens' models: relative L2 of the logits of the step after the last prompt row (the first
    that reads quantised rows; the prompt pass itself is unquantised) and the share of greedy tokens that agree with the bf16 cache.
    Reported, never gated."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    recs = []
    for geo, golden in (("toy", "toy_e2e"), ("toy_qwen", "toy_qwen_e2e")):
        g = np.load(os.path.join(root, golden + ".npz"))
        n = len([k for k in g.files if k.startswith("image") and k[5:].isdigit()])
        images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
        sizes = [tuple(x) for x in g["image_sizes"].tolist()]
        eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="portable", seed=0)

        def run(kv_dtype):
            out = []
            for b in range(n):
                p = g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)
                cache, logits = eng.prefill(p[None], None, [images[b]], [sizes[b]], max_new_tokens=new, kv_dtype=kv_dtype)
                toks, nxt = [ops.argmax_rows(logits, eng.vocab)], None
                for _ in range(new - 1):
                    logits = eng.decode_step(cache, toks[-1].to(torch.int32))
                    nxt = logits[0].clone() if nxt is None else nxt
                    toks.append(ops.argmax_rows(logits, eng.vocab))
                out.append((nxt, torch.cat(toks).cpu().numpy()))
            return out

        a, b = run("bf16"), run("int8")
        recs.append(dict(geo=geo, mode="kv8_quality_toy", prompts=n, new_tokens=new,
                         next_step_logits_rel_l2=[round(float((y[0] - x[0]).norm() / x[0].norm()), 5) for x, y in zip(a, b)],
                         greedy_tokens_agree=[round(float((x[1] == y[1]).mean()), 4) for x, y in zip(a, b)]))
    return recs


def kvpress_shapes(reps=20, keys=(704, 7603), batches=(1, 8, 32), w=32, k=7):
    """rv_kv_votes_f32, rv_kv_select_i32 and rv_kv_gather_bf16 per layer and head shape on random q|k|v rows: B prompts of `keys`
    positions, budget N = min(1024, keys // 2); interleaved, cold cache, median of `reps` (the protocol of kv8_shapes)."""
    out = []
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        H, hd = l["heads"], l["d"] // l["heads"]
        Hkv = l.get("kv_heads", H)
        d, kvd = H * hd, Hkv * hd
        for n in keys:
            N = min(1024, n // 2)
            for B in batches:
                qkv = torch.randn(B * n, d + 2 * kvd, device="cuda", dtype=torch.bfloat16)
                cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * n
                seq = torch.arange(B, dtype=torch.int32, device="cuda")
                cache = torch.zeros(B, N + 128, 2 * kvd, dtype=torch.bfloat16, device="cuda")
                votes = torch.empty(B, Hkv, n - w, dtype=torch.float32, device="cuda")
                keep = torch.empty(B, Hkv, N, dtype=torch.int32, device="cuda")
                fns = {"votes": lambda: ops.kv_votes(qkv, cu, H, Hkv, hd, w, n, out=votes),
                       "select": lambda: ops.kv_select(votes, cu, N, w, k, out=keep),
                       "gather": lambda: ops.kv_gather(qkv[:, d:], cu, keep, seq, cache, Hkv, hd)}
                for f in fns.values():                                      # warm-up, and select / gather read what votes / select wrote
                    f()
                ts = _timed_interleaved(fns, flush, reps)
                med = {a: float(np.median(v)) for a, v in ts.items()}
                out.append(dict(mode="kvpress_kernels", geo=geo, H=H, Hkv=Hkv, hd=hd, keys=n, B=B, budget=N, window=w, pool=k,
                                votes_us=round(med["votes"], 2), select_us=round(med["select"], 2), gather_us=round(med["gather"], 2),
                                total_us=round(sum(med.values()), 2),
                                votes_p10_p90_us=[round(float(np.percentile(ts["votes"], q)), 2) for q in (10, 90)], reps=reps,
                                kernel_src=_src_hash()))
                del qkv, cache, votes, keep
    return out


def kvpress_e2e(geo, batches, prompt=7603, new=40, N=1024, w=32, k=7, reps=2):
    """The decode step and the prompt pass with and without prompt_kv_budget=N at a `prompt`-position prompt on one engine (random token
    prompts): ms per step (the median step of every pass, passes interleaved after one untimed pass of both arms), the cache's bytes,
    and the prompt pass's time with the three kernels in its layer loop."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    press = (N, w, k)
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))

        def fill(arm):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cache, _ = eng.prefill(ids, None, None, None, max_new_tokens=new, **({} if arm is None else dict(compress=arm)))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, cache.nbytes()
        ts, pf, nb = {None: [], press: []}, {None: [], press: []}, {}
        for arm in (None, press):
            fill(arm)
        for _ in range(reps):
            for arm in (None, press):
                ms, nb[arm] = fill(arm)
                pf[arm].append(ms)
                ts[arm].append(float(np.median(_decode_loop(eng, ids, new, press=arm))))
        a, b = float(np.median(ts[None])), float(np.median(ts[press]))
        recs.append(dict(geo=geo, mode="kvpress_ab", B=B, prompt=prompt, new_tokens=new, budget=N, window=w, pool=k, reps=reps,
                         full_ms_per_step=round(a, 3), pressed_ms_per_step=round(b, 3), speedup=round(a / b, 3),
                         full_ms_all=[round(x, 3) for x in ts[None]], pressed_ms_all=[round(x, 3) for x in ts[press]],
                         full_cache_bytes=int(nb[None]), pressed_cache_bytes=int(nb[press]),
                         full_prefill_ms=round(float(np.median(pf[None])), 1), pressed_prefill_ms=round(float(np.median(pf[press])), 1),
                         added_prefill_ms=round(float(np.median(pf[press]) - np.median(pf[None])), 1), kernel_src=_src_hash()))
    return recs


def kvpress_quality_toy(new=32, w=8, k=3):
    """How far prompt_kv_budget moves the toy goldens' models, as kv8_quality_toy reports it: relative L2 of the logits of the first
    decode step (the first that reads the compact cache; the prompt pass itself is uncompressed) and the share of greedy tokens that
    agree with the uncompressed call, at budgets of a half and a quarter of each prompt.  Reported, never gated: random-init toys say
    nothing about a trained checkpoint."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    recs = []
    for geo, golden in (("toy", "toy_e2e"), ("toy_qwen", "toy_qwen_e2e")):
        g = np.load(os.path.join(root, golden + ".npz"))
        n = len([x for x in g.files if x.startswith("image") and x[5:].isdigit()])
        images = [torch.from_numpy(g[f"image{i}"]) for i in range(n)]
        sizes = [tuple(x) for x in g["image_sizes"].tolist()]
        eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="portable", seed=0)

        def run(frac):
            out = []
            for b in range(n):
                p = g["input_ids"][b][g["attention_mask"][b].astype(bool)].astype(np.int64)
                P = int(eng.plan(p[None], None, None, [images[b]], [sizes[b]])["lens"][0])
                kw = {} if frac is None else dict(compress=(max(w + 1, int(P * frac)), w, k))
                cache, logits = eng.prefill(p[None], None, [images[b]], [sizes[b]], max_new_tokens=new, **kw)
                toks, nxt = [ops.argmax_rows(logits, eng.vocab)], None
                for _ in range(new - 1):
                    logits = eng.decode_step(cache, toks[-1].to(torch.int32))
                    nxt = logits[0].clone() if nxt is None else nxt
                    toks.append(ops.argmax_rows(logits, eng.vocab))
                out.append((nxt, torch.cat(toks).cpu().numpy(), P))
            return out
        a = run(None)
        for frac in (0.5, 0.25):
            b = run(frac)
            recs.append(dict(geo=geo, mode="kvpress_quality_toy", prompts=n, new_tokens=new, window=w, pool=k, budget_fraction=frac,
                             prompt_positions=[x[2] for x in a],
                             next_step_logits_rel_l2=[round(float((y[0] - x[0]).norm() / x[0].norm()), 5) for x, y in zip(a, b)],
                             greedy_tokens_agree=[round(float((x[1] == y[1]).mean()), 4) for x, y in zip(a, b)]))
    return recs


def kv8_trace(geo, B, prompt, new):
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
    ts = _decode_loop(eng, ids, new, kv_dtype="int8")
    torch.cuda.synchronize()
    return [dict(geo=geo, mode="kv8_trace", B=B, prompt=prompt, new_tokens=new, kv8_ms_per_step_under_trace=round(float(np.median(ts)), 3),
                 kernel_src=_src_hash())]


def _beam_loop(eng, ids, nb, new, warm=8):
    """The steps of generation.beam_generate (no EOS id, so every step runs), each timed from the scores of the previous decode step to
    the synchronised end of the next one; returns the ms of the steps after `warm`."""
    from types import SimpleNamespace
    from radvlm_amd.generation import BeamState, advance_tail_src
    B, V, dev = ids.shape[0], eng.vocab, eng.device
    rows = B * nb
    lens = np.full(B, ids.shape[1], dtype=np.int64)
    st = BeamState(B, nb, V, new)
    cache = eng.new_kv_cache(rows, ids.shape[1] + new)
    roots = np.arange(B) * nb
    _, logits = eng.prefill(ids, None, None, None, max_new_tokens=new, cache=cache, slots=roots)
    cache.lens[:] = np.repeat(lens, nb)
    logits = logits.repeat_interleave(nb, dim=0)
    geo = SimpleNamespace(prefix_row=eng._dev(np.repeat(roots, nb).astype(np.int32)), prefix_len=eng._dev(np.repeat(lens, nb).astype(np.int32)),
                          tail_src=None, tail_cols=0)
    tail = np.zeros((rows, new), dtype=np.int32)
    ws = ops.beam_topk_workspace(B, nb, V, st.K, dev)
    times = []
    for t in range(new - 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.log_softmax_rows(logits, V)
        top = ops.beam_topk(logits, V, nb, eng._dev(st.running_scores.reshape(-1)), st.K, ws=ws).cpu()
        parent, tok = st.step(top[0].view(torch.float32).numpy(), top[1].numpy())
        tail = advance_tail_src(tail, (roots[:, None] + parent).reshape(-1), t)
        geo.tail_src, geo.tail_cols = eng._dev(tail), t + 1
        logits = eng.decode_step(cache, tok.reshape(-1), beams=geo)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    del cache
    return times[warm:]


def beams_step_ab(geo, prompt, new, reps=3):
    """(a) and (c): the beam step beside the plain decode step at the same number of rows, one engine per geometry."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    recs = []
    for B in (1, 8):
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        for nb in (1, 3, 5):
            wide = np.repeat(ids, nb, axis=0)                        # the plain arm: B * nb independent rows, each with its own prompt copy
            ts = {"plain": [], "beam": []}
            _decode_loop(eng, wide, 12)                              # one untimed pass of both arms
            _beam_loop(eng, ids, nb, 12)
            for _ in range(reps):
                ts["plain"].append(float(np.median(_decode_loop(eng, wide, new))))
                ts["beam"].append(float(np.median(_beam_loop(eng, ids, nb, new))))
            p, q = float(np.median(ts["plain"])), float(np.median(ts["beam"]))
            recs.append(dict(geo=geo, mode="beams_step", B=B, num_beams=nb, rows=B * nb, prompt=prompt, new_tokens=new, reps=reps,
                             plain_ms_per_step=round(p, 3), beam_ms_per_step=round(q, 3), plain_ms_all=[round(v, 3) for v in ts["plain"]],
                             beam_ms_all=[round(v, 3) for v in ts["beam"]], plain_spread_ms=round(max(ts["plain"]) - min(ts["plain"]), 3),
                             delta_ms=round(q - p, 3), delta_share=round((q - p) / p, 4),
                             kv_cache_bytes=eng.kv_cache_bytes(B * nb, prompt + new),
                             reorder_bytes_per_step_not_moved=2 * eng.kv_cache_bytes(B * nb, prompt + new // 2),
                             gemv_route=bool(B * nb <= eng.gemv_max_m), kernel_src=_src_hash()))
    return recs


def beams_kernel_ab(geo, prompt, new=48, reps=50):
    """(b): rv_attn_decode_beam_bf16 with an identity table (prefix in the row itself, every tail entry the row itself) against
    rv_attn_decode_bf16 on the same cache and queries; device time per launch pair, interleaved."""
    l = GEOMETRIES[geo]["lm"]
    H, Hkv = l["heads"], l.get("kv_heads", l["heads"])
    hd = l["d"] // H
    kvd = Hkv * hd
    recs = []
    for rows in (1, 3, 5, 8, 24, 40):
        L_max = prompt + new
        cache = (torch.randn(rows, L_max, 2 * kvd, device="cuda", dtype=torch.float32) * 0.5).to(torch.bfloat16)
        q = torch.randn(rows, H * hd, device="cuda", dtype=torch.bfloat16)
        kv_len = torch.full((rows,), prompt + new // 2, dtype=torch.int32, device="cuda")
        own = torch.arange(rows, dtype=torch.int32, device="cuda")
        plen = torch.full((rows,), prompt, dtype=torch.int32, device="cuda")
        tail = own[:, None].expand(rows, new).contiguous()
        fns = {"plain": lambda: ops.attn_decode(q, cache, kv_len, H, Hkv, hd, kvd),
               "beam": lambda: ops.attn_decode_beam(q, cache, kv_len, own, plen, tail, H, Hkv, hd, kvd)}
        assert torch.equal(fns["plain"](), fns["beam"]())
        ts = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3)
        a, b = float(np.median(ts["plain"])), float(np.median(ts["beam"]))
        recs.append(dict(geo=geo, mode="beams_kernel_ab", rows=rows, H=H, Hkv=Hkv, hd=hd, kv_len=prompt + new // 2, L_max=L_max, reps=reps,
                         plain_us=round(a, 2), beam_us=round(b, 2), plain_p10_p90=[round(float(np.percentile(ts["plain"], p)), 2) for p in (10, 90)],
                         beam_p10_p90=[round(float(np.percentile(ts["beam"], p)), 2) for p in (10, 90)], ratio=round(b / a, 3),
                         kernel_src=_src_hash()))
    return recs


class _ScriptDrafter:
    """Benchmark drafters: proposes the plain run's own next k tokens (right=True: every draft is accepted) or tokens that differ
    from them (right=False: none is)."""

    def __init__(self, ref, prompt_len, k, right, vocab):
        self.ref, self.P, self.k, self.right, self.V = np.asarray(ref, dtype=np.int64), prompt_len, k, right, vocab

    def propose(self, seq):
        t = len(seq) - self.P
        d = self.ref[t:t + self.k]
        return d if self.right else (d + 1) % self.V


def lookup_e2e(geo, prompt, new, reps=3, ks=(3, 7, 15)):
    """(a) of --lookup: one engine per geometry, bf16 weights and then quantize_decoder_()."""
    from radvlm_amd.generation import greedy_generate, parse_generate_kwargs
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    ids = np.random.default_rng(0).integers(0, eng.vocab, (1, prompt))
    recs = []

    def call(n, k=None, drafter=None):
        kw = dict(max_new_tokens=n, eos_token_id=None, return_dict_in_generate=True)
        if k is not None:
            kw["prompt_lookup_num_tokens"] = k
        cfg = parse_generate_kwargs(kw, lookup=True)
        cfg.drafter = drafter
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = greedy_generate(eng, ids, None, None, None, cfg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for weights in ("bf16", "int8"):
        if weights == "int8":
            eng.quantize_decoder_()
        _, plain = call(new)
        ref = plain.sequences[0].cpu().numpy()
        arms = {"prefill": lambda: call(1), "plain": lambda: call(new)}
        for k in ks:
            arms[f"oracle_k{k}"] = lambda k=k: call(new, k, _ScriptDrafter(ref, prompt, k, True, eng.vocab))
            arms[f"never_k{k}"] = lambda k=k: call(new, k, _ScriptDrafter(ref, prompt, k, False, eng.vocab))
            arms[f"real_k{k}"] = lambda k=k: call(new, k)
        ts, stats = {a: [] for a in arms}, {}
        for a, f in arms.items():                                      # one untimed repetition of every arm
            _, out = f()
            if a != "prefill":
                assert torch.equal(out.sequences, plain.sequences), a
            stats[a] = getattr(out, "lookup_stats", None)
        for _ in range(reps):
            for a, f in arms.items():
                ts[a].append(f()[0])
        pre = float(np.median(ts["prefill"]))
        per_tok = {a: [(v - pre) / (new - 1) for v in ts[a]] for a in arms if a != "prefill"}
        med = {a: float(np.median(v)) for a, v in per_tok.items()}
        spread = max(per_tok["plain"]) - min(per_tok["plain"])
        rec = dict(geo=geo, mode="lookup_e2e", weights=weights, B=1, prompt=prompt, new_tokens=new, reps=reps, prefill_ms=round(pre, 2),
                   plain_ms_per_token=round(med["plain"], 3), plain_ms_all=[round(v, 3) for v in per_tok["plain"]],
                   plain_spread_ms=round(spread, 3), arms={}, kernel_src=_src_hash())
        for k in ks:
            o, n, r = med[f"oracle_k{k}"], med[f"never_k{k}"], med[f"real_k{k}"]
            rec["arms"][f"k{k}"] = dict(
                oracle_ms_per_token=round(o, 3), oracle_ms_all=[round(v, 3) for v in per_tok[f"oracle_k{k}"]], oracle_stats=stats[f"oracle_k{k}"],
                oracle_speedup=round(med["plain"] / o, 3), oracle_faster_by_more_than_plain_spread=bool(med["plain"] - o > spread),
                never_ms_per_token=round(n, 3), never_ms_all=[round(v, 3) for v in per_tok[f"never_k{k}"]], never_stats=stats[f"never_k{k}"],
                wasted_step_cost_vs_plain=round(n / med["plain"], 3),
                # a step that accepts a drafts emits a + 1 tokens for the never-right step's time: even at a + 1 = never / plain
                break_even_accepted_per_step=round(max(n / med["plain"] - 1.0, 0.0), 3),
                break_even_acceptance_rate=round(max(n / med["plain"] - 1.0, 0.0) / k, 4),
                real_drafter_random_weights_ms_per_token=round(r, 3), real_drafter_random_weights_stats=stats[f"real_k{k}"])
        recs.append(rec)
    return recs


def _scripted_model_drafter(draft, k, cfg, new, prompt, ref, j):
    """An assist.ModelDrafter that runs the draft engine for real -- catch-up, k chained draft steps, the copy to the host -- and then
    proposes the plain run's next j tokens followed by wrong ones (the Scripted idea of tests/test_generate_lookup_gpu.py: random
    weights have no acceptance rate of their own).  Its bookkeeping is told that it fed the scripted tokens, so the next round's
    catch-up feeds what a real assistant with that acceptance would feed."""
    from radvlm_amd.assist import ModelDrafter

    class Scripted(ModelDrafter):
        def propose(self, seq):
            own = super().propose(seq)
            t = len(seq) - self.P
            out = np.array([(ref[t + i] if t + i < len(ref) else 0) if i < j else ((ref[t + i] if t + i < len(ref) else 0) + 1) % self.engine.vocab
                            for i in range(len(own))], dtype=np.int64)
            self.fed = self.fed[:t] + [int(v) for v in out[:max(len(own) - 1, 0)]]
            return out
    return Scripted(draft, k, cfg, new, prompt)


def assistant_bench(geo, prompt, new, reps=3, ks=(3, 5, 7, 15), draft_layers=4, warm=8):
    """--assistant: B = 1, a draft of the target's width with draft_layers decoder layers.  (1) step times on one box, wall ms with a
    synchronize around each step, medians after `warm` steps: the target's plain step (decode_step + argmax), the draft's step, the
    target's verify_step at R = k + 1, and the sampled round's extra launches (the sampler's warp of R rows + rv_spec_accept_rows_f32).
    (2) greedy generate(assistant_model=) end to end with the scripted drafter at acceptance 0, k // 2 and k of k: ms per token after
    the two prefills, tokens / s, speed-up over the plain call, and the break-even number of accepted drafts per round,
    never_ms_per_round / plain_ms_per_token - 1."""
    from types import SimpleNamespace
    from radvlm_amd.generation import greedy_generate, parse_generate_kwargs
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    dgeo = dict(GEOMETRIES[geo])
    dgeo["lm"] = dict(dgeo["lm"], layers=draft_layers)
    draft = LlavaEngine(dgeo, device="cuda:0", init="fast", seed=1)
    V = eng.vocab
    ids = np.random.default_rng(0).integers(0, V, (1, prompt))

    def timed(f, n):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[warm:]))

    # ---- (1) the steps
    steps = {}
    for name, e in (("plain_step_ms", eng), ("draft_step_ms", draft)):
        cache, logits = e.prefill(ids, None, None, None, max_new_tokens=new)
        tok = [ops.argmax_rows(logits, V)]

        def step(e=e, cache=cache, tok=tok):
            tok[0] = ops.argmax_rows(e.decode_step(cache, tok[0]), V)
        steps[name] = timed(step, new - 1)
        del cache
    cache, logits = eng.prefill(ids, None, None, None, max_new_tokens=new)
    seed1 = torch.tensor([7], dtype=torch.int64, device="cuda")
    for k in ks:
        R = k + 1
        feed = np.random.default_rng(k).integers(0, V, R)
        steps[f"verify_step_ms_k{k}"] = timed(lambda: eng.verify_step(cache, feed), warm + 20)       # lens is not advanced: every call is the same step
        p = eng.verify_step(cache, feed).clone()
        q = (p[:k] + 0.5 * torch.randn_like(p[:k])).contiguous()
        si = torch.arange(R, dtype=torch.int32, device="cuda")
        dr = torch.from_numpy(feed[:k].astype(np.int32)).cuda()
        sws, aws = ops.sample_rows_workspace(R, "cuda"), ops.spec_accept_workspace(1, R, "cuda")
        seedR = seed1.expand(R).contiguous()

        def accept():
            x = p.clone()
            ops.sample_rows(x, V, seedR, si, 0.8, 50, 0.9, 0.0, write_scores=True, ws=sws)
            ops.spec_accept_rows(x, q, dr, seed1, si[:1], V, ws=aws)
        steps[f"warp_and_accept_ms_k{k}"] = timed(accept, warm + 20)
        steps[f"accept_kernel_ms_k{k}"] = timed(lambda: ops.spec_accept_rows(p, q, dr, seed1, si[:1], V, ws=aws), warm + 20)
    del cache

    # ---- (2) end to end, greedy, scripted acceptance
    def call(n, k=None, j=0, ref=None):
        kw = dict(max_new_tokens=n, eos_token_id=None, return_dict_in_generate=True)
        if k is not None:
            kw.update(assistant_model=SimpleNamespace(engine=draft), num_assistant_tokens=k)
        cfg = parse_generate_kwargs(kw, lookup=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            if k is not None:
                cfg.drafter = _scripted_model_drafter(draft, k, cfg, n, prompt, ref, j)
                cfg.drafter.start(ids, None, None, None)
            out = greedy_generate(eng, ids, None, None, None, cfg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    _, plain = call(new)
    ref = plain.sequences[0].cpu().numpy().tolist()
    arms = {"prefill": lambda: call(1), "prefill_both": lambda: call(1, ks[0], 0, ref), "plain": lambda: call(new)}
    for k in ks:
        for j in (0, k // 2, k):
            arms[f"k{k}_a{j}"] = lambda k=k, j=j: call(new, k, j, ref)
    ts, stats = {a: [] for a in arms}, {}
    for a, f in arms.items():                                          # one untimed repetition of every arm
        _, out = f()
        if not a.startswith("prefill"):
            assert torch.equal(out.sequences, plain.sequences), a
        stats[a] = getattr(out, "assist_stats", None)
    for _ in range(reps):
        for a, f in arms.items():
            ts[a].append(f()[0])
    pre = {a: float(np.median(ts[a])) for a in ("prefill", "prefill_both")}
    per_tok = {a: [(v - pre["prefill" if a == "plain" else "prefill_both"]) / (new - 1) for v in ts[a]] for a in arms if not a.startswith("prefill")}
    med = {a: float(np.median(v)) for a, v in per_tok.items()}
    spread = max(per_tok["plain"]) - min(per_tok["plain"])
    rec = dict(geo=geo, mode="assistant_bench", B=1, prompt=prompt, new_tokens=new, reps=reps, draft_layers=draft_layers,
               target_layers=eng.l["layers"], prefill_ms=round(pre["prefill"], 2), prefill_both_ms=round(pre["prefill_both"], 2),
               steps={n: round(v, 3) for n, v in steps.items()}, plain_ms_per_token=round(med["plain"], 3),
               plain_tokens_per_s=round(1e3 / med["plain"], 1), plain_spread_ms=round(spread, 3), arms={}, kernel_src=_src_hash())
    for k in ks:
        cell = {}
        for j in (0, k // 2, k):
            m = med[f"k{k}_a{j}"]
            cell[f"accept_{j}_of_{k}"] = dict(ms_per_token=round(m, 3), tokens_per_s=round(1e3 / m, 1), speedup=round(med["plain"] / m, 3),
                                             ms_all=[round(v, 3) for v in per_tok[f"k{k}_a{j}"]], stats=stats[f"k{k}_a{j}"],
                                             differs_by_more_than_plain_spread=bool(abs(med["plain"] - m) > spread))
        never = med[f"k{k}_a0"]                                         # a never-right round emits one token: its time is the round's
        cell["break_even_accepted_per_round"] = round(max(never / med["plain"] - 1.0, 0.0), 3)
        cell["break_even_acceptance_rate"] = round(max(never / med["plain"] - 1.0, 0.0) / k, 4)
        rec["arms"][f"k{k}"] = cell
    return [rec]


def lookup_kernel_ab(geo, reps=40, rounds=3):
    """(b) of --lookup: the verify kernel against the beam kernel on the same rows, one sequence."""
    l = GEOMETRIES[geo]["lm"]
    H, Hkv = l["heads"], l.get("kv_heads", l["heads"])
    hd = l["d"] // H
    kvd = Hkv * hd
    recs = []
    for L in (704, 7603):
        L_max = L + 32
        cache = (torch.randn(1, L_max, 2 * kvd, device="cuda", dtype=torch.float32) * 0.5).to(torch.bfloat16)
        for R in (4, 8, 16, 32):
            q = torch.randn(R, H * hd, device="cuda", dtype=torch.bfloat16)
            kv0 = torch.tensor([L], dtype=torch.int32, device="cuda")
            kv_len = (L + torch.arange(R, device="cuda")).to(torch.int32)
            zero = torch.zeros(R, dtype=torch.int32, device="cuda")
            plen = torch.full((R,), L_max, dtype=torch.int32, device="cuda")
            fns = {"verify": lambda: ops.attn_decode_verify(q, cache, kv0, R, H, Hkv, hd, kvd),
                   "beam": lambda: ops.attn_decode_beam(q, cache, kv_len, zero, plen, None, H, Hkv, hd, kvd)}
            assert torch.equal(fns["verify"](), fns["beam"]())
            meds = {k: [] for k in fns}
            for _ in range(rounds):
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, f in fns.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                for k in fns:
                    meds[k].append(float(np.median(ts[k])))
            v, b = float(np.median(meds["verify"])), float(np.median(meds["beam"]))
            spread = max(meds["beam"]) - min(meds["beam"])
            recs.append(dict(geo=geo, mode="lookup_kernel_ab", R=R, H=H, Hkv=Hkv, hd=hd, kv_len0=L, L_max=L_max, reps=reps, rounds=rounds,
                             verify_us=round(v, 2), beam_us=round(b, 2), verify_us_all=[round(x, 2) for x in meds["verify"]],
                             beam_us_all=[round(x, 2) for x in meds["beam"]], beam_spread_us=round(spread, 2), ratio=round(v / b, 3),
                             verify_slower_by_more_than_beam_spread=bool(v - b > spread), kernel_src=_src_hash()))
    return recs


def cfg_kernel_ab(reps=50):
    """rv_cfg_guide_rows_f32 as one launch per row pair ("pair"), as statistics + elementwise launch ("split"), and the unfused
    baseline: two rv_log_softmax_rows_f32 calls and torch's three elementwise kernels.  Device time per call (events around it, so a
    gap between an arm's launches counts), median of `reps`, arms interleaved; every call starts from freshly copied raw rows, either
    still in the caches ("warm": what a decode step leaves) or evicted by a 1 GiB fill ("cold").  The three arms are checked to give
    the same bits before anything is timed."""
    recs = []
    g = 1.5
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    for n in (32000, 152064):
        for rows in (1, 16):
            rng = np.random.default_rng(n + rows)
            c0 = torch.from_numpy((rng.standard_normal((rows, n)) * 4).astype(np.float32)).cuda()
            u0 = torch.from_numpy((rng.standard_normal((rows, n)) * 4).astype(np.float32)).cuda()
            c, u = c0.clone(), u0.clone()
            ws = ops.cfg_guide_workspace(rows, "cuda")

            def unfused():
                ops.log_softmax_rows(c, n)
                ops.log_softmax_rows(u, n)
                c.sub_(u).mul_(g).add_(u)

            fns = {"pair": lambda: ops.cfg_guide_rows(c, u, n, g, route="pair"), "split": lambda: ops.cfg_guide_rows(c, u, n, g, ws=ws, route="split"),
                   "unfused": unfused}
            outs = {}
            for k, f in fns.items():
                c.copy_(c0), u.copy_(u0)
                f()
                outs[k] = c.clone()
            assert torch.equal(outs["pair"], outs["split"]) and torch.equal(outs["pair"], outs["unfused"])
            rec = dict(mode="cfg_kernel_ab", rows=rows, vocab=n, reps=reps, g=g)
            for temp in ("warm", "cold"):
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, f in fns.items():
                        c.copy_(c0), u.copy_(u0)
                        if temp == "cold":
                            flush.fill_(0.0)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                rec.update({f"{k}_{temp}_us": round(v, 2) for k, v in med.items()})
                rec.update({f"{k}_{temp}_p10_p90_us": [round(float(np.percentile(ts[k], 10)), 2), round(float(np.percentile(ts[k], 90)), 2)] for k in fns})
                rec[f"split_over_pair_{temp}"] = round(med["split"] / med["pair"], 3)
                rec[f"unfused_over_split_{temp}"] = round(med["unfused"] / med["split"], 3)
            recs.append(rec)
    return recs


def _guided_loop(eng, ids, nids, new, warm=8):
    """The decode step of guided generation as generation._guided_generate runs it: one cache of 2 * B rows, two prefills, then per
    step decode_step over all rows + ops.cfg_guide_rows + argmax.  Returns (step times in ms after warm-up, the guide launch's median
    device time in us on the last step's rows)."""
    B, V = ids.shape[0], eng.vocab
    L_max = max(ids.shape[1], nids.shape[1]) + new
    cache = eng.new_kv_cache(2 * B, L_max)
    _, c = eng.prefill(ids, None, None, None, cache=cache, slots=np.arange(B))
    _, u = eng.prefill(nids, None, None, None, cache=cache, slots=B + np.arange(B))
    ws = ops.cfg_guide_workspace(B, c.device)
    tok = ops.argmax_rows(ops.cfg_guide_rows(c, u, V, 1.5, ws=ws), V)
    times = []
    for _ in range(1, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        both = eng.decode_step(cache, torch.cat([tok, tok]).to(torch.int32))
        tok = ops.argmax_rows(ops.cfg_guide_rows(both[:B], both[B:], V, 1.5, ws=ws), V)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    raw = both.clone()
    gus = []
    for _ in range(50):
        both.copy_(raw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.cfg_guide_rows(both[:B], both[B:], V, 1.5, ws=ws)
        e1.record()
        e1.synchronize()
        gus.append(e0.elapsed_time(e1) * 1e3)
    del cache
    return times[warm:], float(np.median(gus))


def cfg_ab(geo, batches, prompt, new, reps=3):
    """Guided decode at B requests (full-length and 1-token negative prompts) beside the plain decode step at B and at 2 * B rows."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    recs = []
    for B in batches:
        rng = np.random.default_rng(0)
        ids, ids2 = rng.integers(0, eng.vocab, (B, prompt)), rng.integers(0, eng.vocab, (2 * B, prompt))
        neg_full, neg_one = rng.integers(0, eng.vocab, (B, prompt)), ids[:, -1:]
        guide_us = {}

        def guided(name, nids):
            ts, gu = _guided_loop(eng, ids, nids, new)
            guide_us.setdefault(name, []).append(gu)
            return ts

        arms = {"plain_B": lambda: _decode_loop(eng, ids, new), "plain_2B": lambda: _decode_loop(eng, ids2, new),
                "guided_full": lambda: guided("guided_full", neg_full), "guided_one": lambda: guided("guided_one", neg_one)}
        for f in arms.values():                                         # one untimed pass of every arm
            f()
        guide_us.clear()
        ts = {k: [] for k in arms}
        for _ in range(reps):
            for k, f in arms.items():
                ts[k].append(float(np.median(f())))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = {k: max(v) - min(v) for k, v in ts.items()}
        rec = dict(geo=geo, mode="cfg_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, vocab=eng.vocab, guide_route=ops.CFG_GUIDE_ROUTE)
        for k in arms:
            rec[f"{k}_ms_per_step"], rec[f"{k}_ms_all"], rec[f"{k}_spread_ms"] = round(med[k], 3), [round(x, 3) for x in ts[k]], round(spread[k], 3)
        for k in ("guided_full", "guided_one"):
            gu = float(np.median(guide_us[k]))
            rec[f"{k}_over_plain_B"] = round(med[k] / med["plain_B"], 3)
            rec[f"{k}_over_plain_2B"] = round(med[k] / med["plain_2B"], 3)
            rec[f"{k}_minus_plain_2B_ms"] = round(med[k] - med["plain_2B"], 3)
            rec[f"{k}_below_2x_plain_B_by_more_than_spread"] = bool(2 * med["plain_B"] - med[k] > spread["plain_B"])
            rec[f"{k}_guide_us"], rec[f"{k}_guide_share_of_step"] = round(gu, 2), round(gu * 1e-3 / med[k], 4)
        rec["two_forwards_ms"] = round(2 * med["plain_B"], 3)
        recs.append(rec)
    return recs


def _dola_inputs(n, nl, rows, seed=0):
    """The kernel tests' rows: f = 4 randn, candidate k = f + 0.25 * 2^(k/2) randn in a shuffled order."""
    g = torch.Generator().manual_seed(seed + n + 31 * nl + rows)
    f = 4 * torch.randn(rows, n, generator=g)
    order = torch.randperm(nl, generator=g).tolist()
    c = torch.stack([f + 0.25 * 2 ** (order[k] / 2) * torch.randn(rows, n, generator=g) for k in range(nl)])
    return f.cuda(), c.cuda()


def dola_shapes(reps=20):
    """rv_dola_contrast_rows_f32 (four launches: statistics, divergence pieces, select, contrast) against the unfused composition on
    the same rows: two rv_log_softmax_rows_f32 calls, then torch's exp / log / products, the sum, argmax and the masked subtraction.
    n = 32000 with 8 candidates and n = 152064 with 7, rows 1, 8, 32.  Device time per call (events around it), median of `reps`, arms
    interleaved, every call from freshly copied raw rows, warm and after a 1 GiB fill ("cold").  torch.equal of the contrasted rows is
    asserted before anything is timed.  The kernel has one launch structure, so there is no second arm of its own."""
    recs = []
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    log_rt = torch.tensor(ops.DOLA_LOG_RT, dtype=torch.float32, device="cuda")
    for n, nl in ((32000, 8), (152064, 7)):
        for rows in (1, 8, 32):
            f0, c0 = _dola_inputs(n, nl, rows)
            f, c = f0.clone(), c0.clone()
            ws = ops.dola_workspace(rows, nl, "cuda")
            ar = torch.arange(rows, device="cuda")

            def unfused():
                lf = ops.log_softmax_rows(f, n)
                lq = ops.log_softmax_rows(c.view(nl * rows, n), n).view(nl, rows, n)
                M = 0.5 * (lf.exp() + lq.exp())
                lm = M.log()
                J = torch.where(M > 0, M * ((lm - lf) + (lm - lq)), M).double().sum(-1)
                lb = lq[J.argmax(0), ar]
                thresh = lf.max(1, keepdim=True).values + log_rt
                f.copy_(torch.where(lf < thresh, torch.full_like(lf, float("-inf")), lf - lb))

            fns = {"fused": lambda: ops.dola_contrast_rows(f, c, n, ws=ws), "unfused": unfused}
            outs = {}
            for k, fn in fns.items():
                f.copy_(f0), c.copy_(c0)
                fn()
                outs[k] = f.clone()
            assert torch.equal(outs["fused"], outs["unfused"])
            rec = dict(mode="dola_kernel_ab", rows=rows, vocab=n, n_layers=nl, reps=reps)
            for temp in ("warm", "cold"):
                ts = {k: [] for k in fns}
                for _ in range(reps):
                    for k, fn in fns.items():
                        f.copy_(f0), c.copy_(c0)
                        if temp == "cold":
                            flush.fill_(0.0)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        ts[k].append(e0.elapsed_time(e1) * 1e3)
                med = {k: float(np.median(v)) for k, v in ts.items()}
                rec.update({f"{k}_{temp}_us": round(v, 2) for k, v in med.items()})
                rec.update({f"{k}_{temp}_p10_p90_us": [round(float(np.percentile(ts[k], 10)), 2), round(float(np.percentile(ts[k], 90)), 2)] for k in fns})
                rec[f"unfused_over_fused_{temp}"] = round(med["unfused"] / med["fused"], 3)
                spread = float(np.percentile(ts["unfused"], 90) - np.percentile(ts["unfused"], 10))
                rec[f"fused_faster_by_more_than_unfused_spread_{temp}"] = bool(med["unfused"] - med["fused"] > spread)
            recs.append(rec)
    return recs


def _dola_loop(eng, ids, new, layers, warm=8):
    """The decode step of generate(dola_layers=) as greedy_generate runs it: decode_step(tap_layers=) + ops.dola_contrast_rows + argmax.
    Returns (step times in ms after warm-up, the contrast call's median device time in us on the last step's rows)."""
    B, V = ids.shape[0], eng.vocab
    cache, f, c = eng.prefill(ids, None, None, None, max_new_tokens=new, tap_layers=layers)
    ws = ops.dola_workspace(B, len(layers), f.device)
    tok = ops.argmax_rows(ops.dola_contrast_rows(f, c, V, ws=ws)[0], V)
    times = []
    for _ in range(1, new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f, c = eng.decode_step(cache, tok.to(torch.int32), tap_layers=layers)
        tok = ops.argmax_rows(ops.dola_contrast_rows(f, c, V, ws=ws)[0], V)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    raw, us = f.clone(), []
    for _ in range(20):
        f.copy_(raw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.dola_contrast_rows(f, c, V, ws=ws)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    del cache
    return times[warm:], float(np.median(us))


def dola_ab(geo, batches, prompt, new, reps=3):
    """The decode step with dola_layers="high" beside the plain decode step, interleaved `reps` times as --kv8 does; the candidates'
    lm_head rows in a second launch ("second") and, where it keeps the mature rows' bits, stacked with them into one skinny launch
    ("stacked", LlavaEngine.tap_lm_head)."""
    from radvlm_amd.generation import resolve_dola_layers
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    layers = resolve_dola_layers("high", eng.l["layers"])
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        head = eng.W("lm_head.weight")
        max_m = eng.gemv_max_m_wide if head.shape[0] >= 65536 else eng.gemv_max_m
        stackable = B <= min(max_m, ops.GEMV_MAX_M) and (1 + len(layers)) * B <= ops.GEMV_MAX_M
        contrast_us = {}

        def dola(route):
            eng.tap_lm_head = route
            try:
                ts, us = _dola_loop(eng, ids, new, layers)
            finally:
                del eng.tap_lm_head
            contrast_us.setdefault(route, []).append(us)
            return ts

        arms = {"plain": lambda: _decode_loop(eng, ids, new), "dola_second": lambda: dola("second")}
        if stackable:
            arms["dola_stacked"] = lambda: dola("stacked")
        for fn in arms.values():                                        # one untimed pass of every arm
            fn()
        contrast_us.clear()
        ts = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():
                ts[k].append(float(np.median(fn())))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rec = dict(geo=geo, mode="dola_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, vocab=eng.vocab, dola_layers=list(layers),
                   stacked_applies=bool(stackable))
        for k in arms:
            rec[f"{k}_ms_per_step"], rec[f"{k}_ms_all"], rec[f"{k}_spread_ms"] = round(med[k], 3), [round(x, 3) for x in ts[k]], round(max(ts[k]) - min(ts[k]), 3)
        for k in arms:
            if k != "plain":
                us = float(np.median(contrast_us[k.split("_", 1)[1]]))
                rec[f"{k}_added_ms"], rec[f"{k}_over_plain"] = round(med[k] - med["plain"], 3), round(med[k] / med["plain"], 3)
                rec[f"{k}_contrast_us"] = round(us, 2)
        if stackable:
            rec["stacked_minus_second_ms"] = round(med["dola_stacked"] - med["dola_second"], 3)
            rec["stacked_faster_by_more_than_second_spread"] = bool(med["dola_second"] - med["dola_stacked"] > max(ts["dola_second"]) - min(ts["dola_second"]))
        recs.append(rec)
    return recs


def attentions_ab(geo, batches, prompt, new, reps=3):
    """The decode step that also returns its attention maps (decode_step(attn_layers=), what generate(output_attentions=True) runs)
    beside the plain decode step on one engine, interleaved `reps` times after one untimed pass of every arm: every layer and the
    last layer only, per head and as the head mean.  One record per batch size; nothing gates on it."""
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    L = eng.l["layers"]
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        arms = {"plain": None}
        for lname, layers in (("all", tuple(range(L))), ("last", (L - 1,))):
            for rname, mean in (("per_head", False), ("mean_heads", True)):
                arms[f"{lname}_{rname}"] = dict(attn_layers=layers, attn_mean=mean)
        for kw in arms.values():                                        # one untimed pass of every arm
            _decode_loop(eng, ids, min(new, 16), attn=kw, warm=0)
        ts = {k: [] for k in arms}
        for _ in range(reps):
            for k, kw in arms.items():
                ts[k].append(float(np.median(_decode_loop(eng, ids, new, attn=kw))))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        rec = dict(geo=geo, mode="attentions_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, layers=L, heads=eng.l["heads"],
                   kv_heads=eng.Hkv, head_dim=eng.hd)
        for k in arms:
            rec[f"{k}_ms_per_step"], rec[f"{k}_ms_all"], rec[f"{k}_spread_ms"] = round(med[k], 3), [round(x, 3) for x in ts[k]], round(max(ts[k]) - min(ts[k]), 3)
            if k != "plain":
                rec[f"{k}_added_ms"], rec[f"{k}_over_plain"] = round(med[k] - med["plain"], 3), round(med[k] / med["plain"], 3)
        recs.append(rec)
    return recs


def lora_weight_bytes(eng):
    """Bytes of the adapters a decode step streams: lora_A [r, in] and lora_B [out, r] of every layer's seven modules."""
    return 2 * sum(eng.lm.view(n).numel() for n in eng.lm.names() if ".lora_" in n)


def lora_ab(geo, batches, prompt, new, samples=20, r=64):
    """The decode step on (a) merged weights, (b) live adapters (engine.adapter_decoding: rv_lora_down_rows_bf16 + rv_gemv_lora_bf16 per
    fused projection) and (c) live adapters switched off (engine.adapters_off: the skinny route is rv_gemv_bf16 again), interleaved on
    one box: one untimed pass of every arm, then `samples` rounds of a, b, c; a sample is the median step of one decode loop.  The
    merged arm is a second engine of the same run after merge_lora(); (b) and (c) share one engine."""
    lora = dict(r=r, alpha=16, dropout=0.05)
    live = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0, lora=lora)
    merged = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0, lora=lora)
    for eng in (live, merged):
        for n in eng.lm.names():
            if n.endswith("lora_B.weight"):                             # peft starts B at zero; the time does not depend on the values
                eng.lm.view(n).normal_(0.0, 0.02)
    ad_bytes, wb = lora_weight_bytes(live), weight_bytes(live)
    merged.merge_lora()
    live.adapter_decoding = True
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, live.vocab, (B, prompt))

        def off():
            live.adapters_off = True
            try:
                return _decode_loop(live, ids, new)
            finally:
                live.adapters_off = False

        arms = {"merged": lambda: _decode_loop(merged, ids, new), "live": lambda: _decode_loop(live, ids, new), "off": off}
        for fn in arms.values():
            fn()
        ts = {k: [] for k in arms}
        for _ in range(samples):
            for k, fn in arms.items():
                ts[k].append(float(np.median(fn())))
        rec = dict(geo=geo, mode="lora_ab", B=B, r=r, prompt=prompt, new_tokens=new, samples=samples, weight_bytes=wb, adapter_bytes=ad_bytes,
                   adapter_over_weight_bytes=round(ad_bytes / wb, 4), entry_calls_per_layer=dict(merged=4, live=8, off=4),
                   build=os.path.basename(os.environ.get("RADVLM_HIP_LIB", "default")))
        for k in arms:
            rec[f"{k}_ms_per_step"] = round(float(np.median(ts[k])), 3)
            rec[f"{k}_ms_p10"], rec[f"{k}_ms_p90"] = round(float(np.percentile(ts[k], 10)), 3), round(float(np.percentile(ts[k], 90)), 3)
        rec["live_over_merged"] = round(rec["live_ms_per_step"] / rec["merged_ms_per_step"], 3)
        rec["off_over_merged"] = round(rec["off_ms_per_step"] / rec["merged_ms_per_step"], 3)
        recs.append(rec)
    return recs


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


SAMPLE_SETTINGS = {"chat_default": dict(temperature=0.2, top_k=50, top_p=0.7), "everything": dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05)}
SAMPLE_SWEEPS = 10                # sweeps of the row rv_sample_rows_f32 makes with top-k and top-p on: max, 4 + 4 radix passes, the tile sums
SAMPLE_LAUNCHES = SAMPLE_SWEEPS + 1   # one launch per sweep (8 workgroups share a row and meet at launch boundaries) and one for the draw
DECODE_LAUNCHES = 420             # kernel launches of one greedy decode step at 7B (from a kernel trace)


def sample_kernel_ab(reps=30):
    """rv_sample_rows_f32 vs rv_logits_process_argmax_rows_f32 with logprobs (no processor active: one read of the row) on the same
    rows; interleaved, device time per launch (median µs)."""
    from radvlm_amd.generation import parse_generate_kwargs
    recs = []
    for n in (32000, 152064):
        for rows in (1, 32):
            x = torch.from_numpy((np.random.default_rng(1).standard_normal((rows, n)) * 4).astype(np.float32)).cuda()
            info = torch.zeros(3, rows, dtype=torch.int32, device="cuda")
            seeds = torch.arange(rows, dtype=torch.int64, device="cuda")
            lpo = torch.empty(rows, dtype=torch.float32, device="cuda")
            ws = ops.sample_rows_workspace(rows, "cuda")
            fns = {"argmax_logprob": lambda: ops.logits_process_argmax_rows(x, n, None, info[0], info[1], info[2], logprob=lpo)}
            for name, kw in SAMPLE_SETTINGS.items():
                sm = parse_generate_kwargs(dict(do_sample=True, seed=0, **kw)).sampling
                fns[name] = (lambda sm=sm: ops.sample_rows(x, n, seeds, info[1], sm.temperature, sm.top_k, sm.top_p, sm.min_p, logprob=lpo, ws=ws))
            ts = {k: [] for k in fns}
            for f in fns.values():
                f()
            for _ in range(reps):
                for k, f in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    ts[k].append(e0.elapsed_time(e1) * 1e3)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            recs.append(dict(mode="sample_kernel_ab", rows=rows, vocab=n, reps=reps, sweeps=SAMPLE_SWEEPS, launches=SAMPLE_LAUNCHES,
                             **{k + "_us": round(v, 2) for k, v in med.items()},
                             **{"ratio_" + k: round(med[k] / med["argmax_logprob"], 2) for k in SAMPLE_SETTINGS}))
    return recs


def sample_ab(geo, batches, prompt, new, reps=3):
    """The decode step with the token drawn by rv_sample_rows_f32 (chat default) against the greedy argmax, on one engine."""
    from radvlm_amd.generation import parse_generate_kwargs
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    sm = parse_generate_kwargs(dict(do_sample=True, seed=0, **SAMPLE_SETTINGS["chat_default"])).sampling
    recs = []
    for B in batches:
        ids = np.random.default_rng(0).integers(0, eng.vocab, (B, prompt))
        ts = {"greedy": [], "sampled": []}
        for arm in ts:                                                 # one untimed repetition of both arms
            _decode_loop(eng, ids, new, sm=sm if arm == "sampled" else None)
        for _ in range(reps):
            for arm in ts:
                ts[arm].append(float(np.median(_decode_loop(eng, ids, new, sm=sm if arm == "sampled" else None))))
        g, q = float(np.median(ts["greedy"])), float(np.median(ts["sampled"]))
        spread = max(ts["greedy"]) - min(ts["greedy"])
        added = SAMPLE_LAUNCHES - 1                                    # the sampler's launches take the place of the argmax launch
        gate = spread + added * g / DECODE_LAUNCHES                    # the added launches at the step's enqueue rate
        recs.append(dict(geo=geo, mode="sample_ab", B=B, prompt=prompt, new_tokens=new, reps=reps, setting="chat_default",
                         greedy_ms_per_step=round(g, 3), sampled_ms_per_step=round(q, 3), greedy_ms_all=[round(v, 3) for v in ts["greedy"]],
                         sampled_ms_all=[round(v, 3) for v in ts["sampled"]], greedy_spread_ms=round(spread, 3), launches_added=added,
                         delta_ms=round(q - g, 3), gate_ms=round(gate, 3), gate_holds=bool(q - g <= gate), holds_on_spread_alone=bool(q - g <= spread),
                         kernel_src=_src_hash()))
    return recs


def shared_shapes(reps=20, keys=(704, 7603), groups=(2, 4, 8, 16, 32), B=32, own=40):
    """rv_attn_decode_bf16 vs rv_attn_decode_shared_bf16 per head shape: B rows in groups that hold one prefix of `keys` positions and
    `own` positions of their own, interleaved, cold cache."""
    from radvlm_amd.generation import shared_tiles
    out = []
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        H, hd = l["heads"], l["d"] // l["heads"]
        Hkv = l.get("kv_heads", H)
        kvd, rpt = Hkv * hd, ops.SHARED_TILE_COLS // (H // Hkv)
        for n in keys:
            L = n + own + 1
            cache = torch.randn(B, L, 2 * kvd, device="cuda", dtype=torch.bfloat16)
            q = torch.randn(B, H * hd, device="cuda", dtype=torch.bfloat16)
            kv_len = torch.full((B,), n + own, dtype=torch.int32, device="cuda")
            for gs in groups:
                for s in range(B):
                    if s % gs:
                        cache[s, :n] = cache[s - s % gs, :n]
                c0, tile = shared_tiles(np.arange(B), np.arange(B) // gs, np.full(B, n), rpt, 128, B)
                plan = ops.shared_tiles_upload(c0, tile, rpt, "cuda")
                fns = {"plain": lambda: ops.attn_decode(q, cache, kv_len, H, Hkv, hd, kvd),
                       "shared": lambda: ops.attn_decode_shared(q, cache, kv_len, plan.c0, plan.tile, H, Hkv, hd, kvd)}
                assert torch.equal(fns["plain"](), fns["shared"]())
                ts = _timed_interleaved(fns, flush, reps)
                pl, sh = float(np.median(ts["plain"])), float(np.median(ts["shared"]))
                p10, p90 = float(np.percentile(ts["plain"], 10)), float(np.percentile(ts["plain"], 90))
                out.append(dict(mode="shared_kernel_ab", geo=geo, H=H, Hkv=Hkv, hd=hd, shared_keys=n, keys=n + own, B=B, group=gs,
                                rows_per_tile=rpt, tiles=int((tile[:, 0] >= 0).sum()), c0=int(c0.max()), plain_us=round(pl, 2),
                                shared_us=round(sh, 2), shared_over_plain=round(sh / pl, 3), plain_p10_us=round(p10, 2),
                                plain_p90_us=round(p90, 2), shared_p10_us=round(float(np.percentile(ts["shared"], 10)), 2),
                                shared_p90_us=round(float(np.percentile(ts["shared"], 90)), 2),
                                shared_faster_by_more_than_plain_spread=bool(pl - sh > p90 - p10), reps=reps, chunk=128,
                                kernel_src=_src_hash()))
                print(f"# {geo} keys {n} group {gs}: plain {pl:.1f} us, shared {sh:.1f} us", file=sys.stderr, flush=True)
            del cache
    return out


def score_shapes(reps=20, prompt=704, cands=(2, 8, 32), lens=(4, 64)):
    """rv_attn_extend_bf16 on the materialised cache vs rv_attn_extend_prefix_bf16 per head shape: C candidates of n tokens (n - 1 rows
    each) after one prompt of `prompt` positions, interleaved, cold cache."""
    out = []
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for geo in ("llava15_7b", "llava_ov_qwen2_7b"):
        l = GEOMETRIES[geo]["lm"]
        H, hd, L = l["heads"], l["d"] // l["heads"], l["layers"]
        Hkv = l.get("kv_heads", H)
        kvd = Hkv * hd
        for n in lens:
            T = n - 1
            for C in cands:
                prefix = torch.randn(1, prompt, 2 * kvd, device="cuda", dtype=torch.bfloat16)
                tail = torch.randn(C, T, 2 * kvd, device="cuda", dtype=torch.bfloat16)
                mat = torch.cat([prefix.expand(C, -1, -1), tail], dim=1).contiguous()          # the copy share_prefix would make
                q = torch.randn(C * T, H * hd, device="cuda", dtype=torch.bfloat16)
                cu = torch.arange(C + 1, dtype=torch.int32, device="cuda") * T
                plen = torch.full((C,), prompt, dtype=torch.int32, device="cuda")
                prow = torch.zeros(C, dtype=torch.int32, device="cuda")
                fns = {"extend": lambda: ops.attn_extend(q, mat, cu, plen, H, Hkv, hd, kvd, T),
                       "prefix": lambda: ops.attn_extend_prefix(q, prefix, tail, cu, prow, plen, H, Hkv, hd, kvd, T)}
                assert torch.equal(fns["extend"](), fns["prefix"]())
                ts = _timed_interleaved(fns, flush, reps)
                ex, px = float(np.median(ts["extend"])), float(np.median(ts["prefix"]))
                p10, p90 = float(np.percentile(ts["extend"], 10)), float(np.percentile(ts["extend"], 90))
                out.append(dict(mode="score_kernel_ab", geo=geo, H=H, Hkv=Hkv, hd=hd, prompt=prompt, candidates=C, candidate_tokens=n,
                                rows=C * T, extend_us=round(ex, 2), prefix_us=round(px, 2), prefix_over_extend=round(px / ex, 3),
                                extend_p10_us=round(p10, 2), extend_p90_us=round(p90, 2),
                                prefix_p10_us=round(float(np.percentile(ts["prefix"], 10)), 2),
                                prefix_p90_us=round(float(np.percentile(ts["prefix"], 90)), 2),
                                prefix_faster_by_more_than_extend_spread=bool(ex - px > p90 - p10),
                                prefix_slower_by_more_than_extend_spread=bool(px - ex > p90 - p10),
                                copy_bytes_avoided_per_candidate=prompt * 2 * kvd * 2 * L, reps=reps, chunk=ops.EXTEND_CHUNK,
                                kernel_src=_src_hash()))
                print(f"# {geo} C {C} x {n} tokens: extend {ex:.1f} us, prefix {px:.1f} us", file=sys.stderr, flush=True)
                del prefix, tail, mat, q
    return out


def score_e2e(geo, reps=3, prompt=704, cands=(2, 8, 32), lens=(4, 64)):
    """--score: scoring.score() vs one training forward per (prompt + candidate), reading the loss."""
    from radvlm_amd import scoring
    g = GEOMETRIES[geo]
    eng = LlavaEngine(g, device="cuda:0", init="fast", seed=0)
    rng = np.random.default_rng(0)
    img = g["vision"]["image"]
    image = torch.randn(3, img, img, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    size = (img, img)
    probe = np.full(36, 5, dtype=np.int64)
    probe[35] = -200
    base = int(eng.plan(probe[None], None, None, [image], [size])["lens"][0])      # 35 tokens, then the image's rows
    ids = rng.integers(3, eng.vocab, size=36 + max(0, prompt - base), dtype=np.int64)
    ids[35] = -200
    P = int(eng.plan(ids[None], None, None, [image], [size])["lens"][0])
    recs = []
    for n in lens:
        for C in cands:
            cs = [rng.integers(3, eng.vocab, n).astype(np.int64) for _ in range(C)]

            def shared():
                return scoring.score(eng, [ids], [cs], images=[image], image_sizes=[size])

            def one_by_one():
                losses = []
                for c in cs:
                    full = np.concatenate([ids, c])[None]
                    labels = np.full(full.shape, -100, dtype=np.int64)
                    labels[0, ids.size:] = c
                    losses.append(eng.forward(full, np.ones(full.shape, dtype=bool), labels, [image], image_sizes=[size]))
                    eng.ctx = None
                return [float(v) for v in losses]

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, r

            with torch.no_grad():
                _, so = timed(shared)                                           # one untimed pass of both arms
                _, lo = timed(one_by_one)
                # the two routes score the same thing: mean token log-prob against the loss, within the bf16-logits CE's rounding
                gap = max(abs(-float(so.logprobs[0][c]) / n - lo[c]) for c in range(C))
                ts = {"score": [], "one_by_one": []}
                for _ in range(reps):
                    ts["score"].append(timed(shared)[0])
                    ts["one_by_one"].append(timed(one_by_one)[0])
            sm, om = float(np.median(ts["score"])), float(np.median(ts["one_by_one"]))
            spread = max(ts["one_by_one"]) - min(ts["one_by_one"])
            recs.append(dict(mode="score_e2e", geo=geo, prompt_positions=P, candidates=C, candidate_tokens=n, reps=reps,
                             score_ms=round(sm, 2), one_by_one_ms=round(om, 2), score_over_one_by_one=round(sm / om, 4),
                             score_ms_all=[round(v, 2) for v in ts["score"]], one_by_one_ms_all=[round(v, 2) for v in ts["one_by_one"]],
                             one_by_one_spread_ms=round(spread, 2), score_faster_by_more_than_one_by_one_spread=bool(om - sm > spread),
                             decoder_rows_score=P + C * (n - 1), decoder_rows_one_by_one=C * (P + n), tower_passes_score=1,
                             tower_passes_one_by_one=C, max_abs_mean_nll_gap=round(gap, 5), kernel_src=_src_hash()))
            print(f"# {geo} C {C} x {n} tokens: score {sm:.1f} ms, one by one {om:.1f} ms", file=sys.stderr, flush=True)
    return recs


class _ShareClock:
    """Wall time inside the engine's prompt passes (prefill, extend) and decode steps, and the tower's runs, synchronised around each
    call (the scheduler synchronises every step anyway).  prefill called from extend is not counted twice."""

    def __init__(self, eng):
        self.eng, self.depth = eng, 0
        self.reset()
        for name in ("prefill", "extend", "decode_step", "encode_images"):
            setattr(eng, name, self._wrap(name, getattr(eng, name)))

    def reset(self):
        self.prompt_ms, self.prefills, self.extends, self.steps, self.tower_calls, self.tower_images = 0.0, 0, 0, [], 0, 0

    def _wrap(self, name, fn):
        def timed(*a, **k):
            if name == "encode_images":
                self.tower_calls += 1
                self.tower_images += int(a[0].shape[0])
                return fn(*a, **k)
            if self.depth:
                return fn(*a, **k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.depth += 1
            try:
                r = fn(*a, **k)
            finally:
                self.depth -= 1
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if name == "decode_step":
                self.steps.append(ms)
            else:
                self.prompt_ms += ms
                self.prefills += name == "prefill"
                self.extends += name == "extend"
            return r
        return timed

    def close(self):
        for name in ("prefill", "extend", "decode_step", "encode_images"):
            delattr(self.eng, name)


def share_prefix_e2e(geo, new=32, reps=3, n_img=8, n_q=8):
    """--share-prefix: generate_batch over n_img images x n_q questions with sharing off, on (plain kernel) and on (shared kernel).
    32 slots; 8 for the anyres_max_9 prompts, the largest batch of 7.6k-position prompts the prompt pass has been run at (--continue)."""
    from radvlm_amd.generation import BatchScheduler, batch_requests, parse_batch_kwargs
    eng, ids, images, sizes = _conversation(geo, n_img)
    rng = np.random.default_rng(3)
    prompts, ims, szs = [], [], []
    for i in range(n_img):
        for _ in range(n_q):
            prompts.append(np.concatenate([ids[0, :36], rng.integers(3, eng.vocab, int(rng.integers(24, 41)))]))   # the system prompt, the image token
            ims.append(images[i])
            szs.append(sizes[i])
    clock = _ShareClock(eng)
    slots = 8 if eng.aspect.startswith("anyres") else 32
    arms = {"off": (False, None), "on_plain": (True, "plain"), "on_shared": (True, "shared")}

    def run(arm):
        share, route = arms[arm]
        cfg = parse_batch_kwargs(dict(max_new_tokens=new, eos_token_id=None, **(dict(share_prefix=True) if share else {})), len(prompts))
        clock.reset()
        eng.shared_route = route
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            sch = BatchScheduler(eng, batch_requests(prompts, ims, szs), cfg, slots)
            out = sch.run()
        finally:
            eng.shared_route = None
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return dict(wall_s=round(wall / 1e3, 3), prompt_pass_s=round(clock.prompt_ms / 1e3, 3), prefills=clock.prefills, extends=clock.extends,
                    tower_calls=clock.tower_calls, tower_images=clock.tower_images, decode_steps=len(clock.steps),
                    decode_ms_per_step=round(float(np.median(clock.steps)), 3), shares=sum(e[0] == "share" for e in sch.events),
                    tokens=sum(len(o.generated_tokens) for o in out.values())), [o.generated_tokens for o in out.values()]

    first = {arm: run(arm) for arm in arms}                           # untimed pass of every arm
    assert first["on_plain"][1] == first["on_shared"][1]              # the two routes: the same tokens
    runs = {arm: [] for arm in arms}
    for _ in range(reps):
        for arm in arms:
            runs[arm].append(run(arm)[0])
            print(f"# {geo} {arm}: {runs[arm][-1]}", file=sys.stderr, flush=True)
    clock.close()
    lens = eng.plan(prompts[0][None], None, None, [ims[0]], [szs[0]])["lens"]
    rec = dict(mode="share_prefix", geo=geo, requests=len(prompts), images=n_img, questions_per_image=n_q, prompt_positions=int(lens[0]),
               new_tokens=new, max_batch_size=slots, reps=reps, image_aspect_ratio=eng.aspect,
               tokens_equal_off_vs_on=sum(a == b for a, b in zip(first["off"][1], first["on_shared"][1])), kernel_src=_src_hash())
    for arm, rs in runs.items():
        wall = [r["wall_s"] for r in rs]
        rec[arm] = dict(rs[int(np.argsort(wall)[len(wall) // 2])], wall_s_all=wall)
    rec["wall_on_shared_over_off"] = round(rec["on_shared"]["wall_s"] / rec["off"]["wall_s"], 3)
    rec["wall_on_plain_over_off"] = round(rec["on_plain"]["wall_s"] / rec["off"]["wall_s"], 3)
    return [rec]


def _conversation(geo, B, seed=0):
    """Engine + turn-1 batch of the --continue configs: ids as bench.py's synthetic batch (129 ids, the image token at 35)."""
    g = GEOMETRIES[geo]
    kw = {}
    if geo == "llava_ov_qwen2_7b":
        kw = dict(merge_type="spatial_unpad", image_aspect_ratio="anyres_max_9", image_grid_pinpoints="(1x1),...,(6x6)")
    eng = LlavaEngine(g, device="cuda:0", init="fast", seed=0, **kw)
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, eng.vocab, size=(B, 129), dtype=np.int64)
    ids[:, 35] = -200
    gen = torch.Generator().manual_seed(seed)
    img = g["vision"]["image"]
    if kw:
        images = [torch.randn(10, 3, img, img, generator=gen).to(torch.bfloat16) for _ in range(B)]
        sizes = [(1024, 1024)] * B
    else:
        images = [torch.randn(3, img, img, generator=gen).to(torch.bfloat16) for _ in range(B)]
        sizes = [(img, img)] * B
    return eng, ids, images, sizes


def _snapshot(gc):
    from radvlm_amd.engine import KVCache
    kv = gc.kv
    return (KVCache([t.clone() for t in kv.layers], kv.lens, kv.L_max), [r.copy() for r in gc.records], list(gc.images),
            gc.weights_version, gc._next_uid)


def _restore(gc, snap):
    from radvlm_amd.engine import KVCache
    kv, recs, imgs, ver, uid = snap
    gc.kv = KVCache([t.clone() for t in kv.layers], kv.lens, kv.L_max)
    gc.records, gc.images, gc.weights_version, gc._next_uid = [r.copy() for r in recs], list(imgs), ver, uid


def continue_case(geo, B, reps=5, turn1_new=64, follow=40, new=64, warm=8):
    from radvlm_amd.generation import GenerationCache, greedy_generate, parse_generate_kwargs, position_records, reuse_lengths
    eng, ids1, images, sizes = _conversation(geo, B)
    gc = GenerationCache()
    t1 = greedy_generate(eng, ids1, None, images, sizes, parse_generate_kwargs(dict(max_new_tokens=turn1_new, past_key_values=gc)))
    ids2 = np.concatenate([ids1, t1.cpu().numpy(), np.random.default_rng(1).integers(3, eng.vocab, (B, follow))], axis=1)
    snap = _snapshot(gc)
    first = lambda cache: parse_generate_kwargs(dict(max_new_tokens=1, **({} if cache is None else dict(past_key_values=cache))))

    def ttft(cached):
        if cached:
            _restore(gc, snap)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        greedy_generate(eng, ids2, None, images, sizes, first(gc if cached else None))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    ttft(True), ttft(False)                                           # warm-up of both paths
    ts = {"cached": [], "fresh": []}
    for _ in range(reps):
        ts["cached"].append(ttft(True))
        ts["fresh"].append(ttft(False))
    # decode after the continuation (K|V of turn 1 from the decode path, extend rows) vs after a fresh prefill of the turn-2 prompt
    plan = eng.plan(ids2, None, None, images, sizes)
    _restore(gc, snap)
    reuse = reuse_lengths(gc.records, position_records(plan, gc._image_uids(images, sizes)))
    steps = {}
    for mode in ("fresh", "cached"):
        if mode == "cached":
            _restore(gc, snap)
            cache, logits = eng.extend(gc.kv, ids2, None, images, sizes, reuse=reuse, max_new_tokens=new, plan=plan)
        else:
            cache, logits = eng.prefill(ids2, None, images, sizes, max_new_tokens=new)
        tok = ops.argmax_rows(logits, eng.vocab)
        times = []
        for _ in range(new - 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logits = eng.decode_step(cache, tok.to(torch.int32))
            tok = ops.argmax_rows(logits, eng.vocab)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        steps[mode] = float(np.median(times[warm:]))
        del cache
    gc.reset()
    lens = plan["lens"].astype(np.int64)
    c, f = float(np.median(ts["cached"])), float(np.median(ts["fresh"]))
    return dict(geo=geo, B=B, mode="continue", prompt_turn1=int(lens.max()) - turn1_new - follow, turn1_new_tokens=turn1_new,
                follow_up_tokens=follow, prompt_turn2=int(lens.max()), reused_per_row=reuse.tolist()[:1] + ([] if B == 1 else ["..."]),
                new_rows_total=int((lens - reuse).sum()), ttft_cached_ms=round(c, 2), ttft_fresh_ms=round(f, 2), ttft_speedup=round(f / c, 2),
                ttft_cached_all=[round(x, 2) for x in ts["cached"]], ttft_fresh_all=[round(x, 2) for x in ts["fresh"]], reps=reps,
                decode_ms_per_step_after_continue=round(steps["cached"], 3), decode_ms_per_step_plain=round(steps["fresh"], 3),
                extend_kv_floor_bytes_per_layer=int(lens.sum() * 2 * eng.kvd * 2), kernel_src=_src_hash())


class _PrefillClock:
    """Wall time spent in engine.prefill (synchronised around each call; the schedulers synchronise every step anyway)."""

    def __init__(self, eng):
        self.eng, self.ms, self.calls = eng, 0.0, 0
        self._pf = eng.prefill

        def pf(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = self._pf(*a, **k)
            torch.cuda.synchronize()
            self.ms += (time.perf_counter() - t0) * 1e3
            self.calls += 1
            return r

        eng.prefill = pf

    def reset(self):
        self.ms, self.calls = 0.0, 0

    def close(self):
        del self.eng.prefill


def _eval_requests(eng, n, prompt, workload):
    from radvlm_amd import portable_rng
    ids = np.random.default_rng(0).integers(0, eng.vocab, (n, prompt))
    if workload == "mixed":
        budgets = portable_rng.integers(0, portable_rng.name_tag("batch_eval_budgets"), (n,), 32, 513).tolist()
    else:
        budgets = [256] * n
    return [ids[i] for i in range(n)], [int(b) for b in budgets]


def _arm(eng, clock, arm, prompts, budgets, admit=None):
    """One timed run of an arm -> (wall ms, useful tokens, prefill ms, prefills)."""
    from radvlm_amd.generation import BatchScheduler, batch_requests, greedy_generate, parse_batch_kwargs, parse_generate_kwargs
    clock.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if arm == "a":
        cfg = parse_batch_kwargs(dict(max_new_tokens=budgets, eos_token_id=None), len(prompts))
        out = BatchScheduler(eng, batch_requests(prompts), cfg, 32, admit_free=admit).run()
        useful = sum(len(o.generated_tokens) for o in out.values())
    elif arm == "b":                        # static groups of 32 through generate(), each to its group's largest budget
        useful = 0
        for g0 in range(0, len(prompts), 32):
            bud = budgets[g0:g0 + 32]
            crit = lambda ids, s, bud=bud: torch.tensor([ids.shape[1] >= b for b in bud])
            cfg = parse_generate_kwargs(dict(max_new_tokens=max(bud), eos_token_id=None, stopping_criteria=[crit]))
            seq = greedy_generate(eng, np.stack(prompts[g0:g0 + 32]), None, None, None, cfg)
            useful += sum(min(b, seq.shape[1]) for b in bud)
    else:                                   # generate() at B = 1 on the first 16 requests
        useful = 0
        for p, b in zip(prompts[:16], budgets[:16]):
            seq = greedy_generate(eng, p[None], None, None, None, parse_generate_kwargs(dict(max_new_tokens=b, eos_token_id=None)))
            useful += seq.shape[1]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, useful, clock.ms, clock.calls


def _kernel_ab(n, rows=32, t=64, reps=50):
    """rv_logits_process_argmax_rows_f32 (without / with logprobs) vs rv_logits_process_argmax_f32 at `rows` x n (the vocabulary), every
    row at step t, the processors of --processors; interleaved, device time per launch (median µs)."""
    from radvlm_amd.generation import LogitsProcessors, parse_generate_kwargs
    cfg = parse_generate_kwargs(dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=2 * t, eos_token_id=2))
    lp = LogitsProcessors(cfg, n)
    rng = np.random.default_rng(1)
    x0 = torch.from_numpy((rng.standard_normal((rows, n)) * 4).astype(np.float32)).cuda()
    hist = torch.from_numpy(rng.integers(0, n, (rows, 2 * t)).astype(np.int32)).cuda()
    info = torch.from_numpy(np.stack([np.arange(rows), np.full(rows, t), np.full(rows, lp.min_new)]).astype(np.int32)).cuda()
    i32 = lambda ids: torch.tensor(ids, dtype=torch.int32, device="cuda") if ids else None
    bans = (i32(sorted(set(lp.suppress) | set(lp.one))), i32(lp.begin), i32(lp.eos))
    lpo = torch.empty(rows, dtype=torch.float32, device="cuda")
    x = x0.clone()
    fns = {"uniform": lambda: ops.logits_process_argmax(x, n, hist, t, lp.penalty, lp.ngram, *lp.device_args(t, x.device)),
           "rows": lambda: ops.logits_process_argmax_rows(x, n, hist, info[0], info[1], info[2], lp.penalty, lp.ngram, *bans),
           "rows_logprob": lambda: ops.logits_process_argmax_rows(x, n, hist, info[0], info[1], info[2], lp.penalty, lp.ngram, *bans,
                                                                  logprob=lpo)}
    ts = {k: [] for k in fns}
    for f in fns.values():
        f()
    for _ in range(reps):
        for k, f in fns.items():
            x.copy_(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return dict(rows=rows, vocab=n, t=t, uniform_us=round(med["uniform"], 2), rows_us=round(med["rows"], 2),
                rows_logprob_us=round(med["rows_logprob"], 2), ratio_rows=round(med["rows"] / med["uniform"], 3),
                ratio_rows_logprob=round(med["rows_logprob"] / med["uniform"], 3), reps=reps)


def batch_eval(geo, n=256, prompt=704, reps=3, sweep=(1, 4, 8, 16)):
    """--batch-eval: N requests of `prompt` tokens, EOS disabled, budgets mixed (portable_rng in [32, 512]) or equal (256); arms (a)
    generate_batch(max_batch_size=32), (b) static groups of 32 through generate(), (c) generate() at B = 1 on the first 16 requests;
    interleaved, `reps` reps, medians.  Then the admission-threshold sweep on mixed (one run each) and the kernel A/B."""
    from radvlm_amd.generation import ADMIT_FREE_SLOTS
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    clock = _PrefillClock(eng)
    recs = []
    work = {w: _eval_requests(eng, n, prompt, w) for w in ("mixed", "equal")}
    _arm(eng, clock, "a", work["equal"][0][:8], [8] * 8)            # warm-up of both paths
    _arm(eng, clock, "b", work["equal"][0][:8], [8] * 8)
    for w, (prompts, budgets) in work.items():
        runs = {k: [] for k in "abc"}
        for _ in range(reps):
            for arm in "abc":
                runs[arm].append(_arm(eng, clock, arm, prompts, budgets))
                print(f"# {geo} {w} arm {arm}: {runs[arm][-1][0] / 1e3:.2f} s", file=sys.stderr, flush=True)
        rec = dict(geo=geo, mode="generate_batch", workload=w, requests=n, prompt=prompt, budget_sum=int(sum(budgets)),
                   budget_mean=round(float(np.mean(budgets)), 1), budget_max=int(max(budgets)), max_batch_size=32,
                   admit_free_slots=ADMIT_FREE_SLOTS, reps=reps)
        for arm, rs in runs.items():
            wall = [r[0] for r in rs]
            i = int(np.argsort(wall)[len(wall) // 2])
            ms, useful, pms, pcalls = rs[i]
            rec[arm] = dict(wall_s=round(ms / 1e3, 3), useful_tokens=useful, tokens_per_s=round(useful * 1e3 / ms, 1),
                            prefill_share=round(pms / ms, 4), prefills=pcalls, wall_s_all=[round(r[0] / 1e3, 3) for r in rs])
        rec["a_over_b"] = round(rec["a"]["tokens_per_s"] / rec["b"]["tokens_per_s"], 3)
        rec["c_note"] = "arm c: generate() at B = 1 over the first 16 requests only, tokens/s as measured on those"
        recs.append(rec)
    prompts, budgets = work["mixed"]
    sweep_rec = dict(geo=geo, mode="generate_batch_sweep", workload="mixed", requests=n, prompt=prompt, max_batch_size=32, runs=[])
    for thr in sweep:
        ms, useful, pms, pcalls = _arm(eng, clock, "a", prompts, budgets, admit=thr)
        print(f"# {geo} sweep {thr}: {ms / 1e3:.2f} s", file=sys.stderr, flush=True)
        sweep_rec["runs"].append(dict(admit_free_slots=thr, wall_s=round(ms / 1e3, 3), tokens_per_s=round(useful * 1e3 / ms, 1),
                                      prefill_share=round(pms / ms, 4), prefills=pcalls))
    recs.append(sweep_rec)
    clock.close()
    recs.append(dict(geo=geo, mode="generate_batch_kernel_ab", **_kernel_ab(eng.vocab)))
    for r in recs:
        r["kernel_src"] = _src_hash()
    return recs


def batch_trace(geo, n=48):
    """--batch-trace (run under rocprofv3 --kernel-trace --stats): generate_batch with processors and logprobs (rows at different
    steps: rv_logits_process_argmax_rows_f32 at 32 rows), then generate() at B = 32 with the same processors
    (rv_logits_process_argmax_f32 at 32 rows) on the same engine and vocabulary."""
    from radvlm_amd.generation import generate_batch, greedy_generate, parse_batch_kwargs, parse_generate_kwargs
    eng = LlavaEngine(GEOMETRIES[geo], device="cuda:0", init="fast", seed=0)
    prompts, _ = _eval_requests(eng, n, 704, "mixed")
    budgets = np.random.default_rng(2).integers(16, 65, n).tolist()
    proc = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8, eos_token_id=2)
    out = generate_batch(eng, prompts, None, None, parse_batch_kwargs(dict(max_new_tokens=budgets, **proc), n), max_batch_size=32,
                         return_logprobs=True)
    greedy_generate(eng, np.stack(prompts[:32]), None, None, None, parse_generate_kwargs(dict(max_new_tokens=64, **proc)))
    torch.cuda.synchronize()
    return [dict(geo=geo, mode="generate_batch_trace", requests=n, generated=sum(len(o.generated_tokens) for o in out.values()),
                 kernel_src=_src_hash())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geos", default="llava15_7b,llava_ov_qwen2_7b")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--prompt", type=int, default=704)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--processors", action="store_true")
    ap.add_argument("--continue", dest="cont", action="store_true")
    ap.add_argument("--batch-eval", action="store_true")
    ap.add_argument("--batch-trace", action="store_true")
    ap.add_argument("--batch-kernel-ab", action="store_true")
    ap.add_argument("--w8", action="store_true")
    ap.add_argument("--w8-shapes", action="store_true")
    ap.add_argument("--w8-trace", action="store_true")
    ap.add_argument("--w8-quality", action="store_true")
    ap.add_argument("--w4", action="store_true")
    ap.add_argument("--w4-shapes", action="store_true")
    ap.add_argument("--w4-quality", action="store_true")
    ap.add_argument("--kv8", action="store_true")
    ap.add_argument("--kv8-shapes", action="store_true")
    ap.add_argument("--kv8-quality", action="store_true")
    ap.add_argument("--kv8-trace", action="store_true")
    ap.add_argument("--kvpress", action="store_true")
    ap.add_argument("--kvpress-shapes", action="store_true")
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--beams", action="store_true")
    ap.add_argument("--lookup", action="store_true")
    ap.add_argument("--lookup-kernel-ab", action="store_true")
    ap.add_argument("--assistant", action="store_true")
    ap.add_argument("--draft-layers", type=int, default=4)
    ap.add_argument("--cfg", action="store_true")
    ap.add_argument("--cfg-kernel-ab", action="store_true")
    ap.add_argument("--dola", action="store_true")
    ap.add_argument("--dola-shapes", action="store_true")
    ap.add_argument("--attentions", action="store_true")
    ap.add_argument("--constraint", action="store_true")
    ap.add_argument("--lora", action="store_true")
    ap.add_argument("--shared-shapes", action="store_true")
    ap.add_argument("--share-prefix", action="store_true")
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--score-shapes", action="store_true")
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.ab:
        recs = ab()
    elif a.w8_shapes:
        recs = w8_shapes()
    elif a.w8:
        recs = [r for g in a.geos.split(",") for r in w8_ab(g, list(map(int, a.batches.split(","))), a.prompt, a.new)]
    elif a.w8_quality:
        recs = w8_quality_toy()
    elif a.w8_trace:
        recs = [r for g in a.geos.split(",") for r in w8_trace(g, a.prompt, a.new)]
    elif a.w4_shapes:
        recs = w4_shapes()
    elif a.w4:
        recs = [r for g in a.geos.split(",") for r in w4_ab(g, list(map(int, a.batches.split(","))), a.prompt, a.new)]
    elif a.w4_quality:
        recs = w8_quality_toy(fmt="mxfp4")
    elif a.kv8_shapes:
        recs = kv8_shapes()
    elif a.kv8:
        recs = [r for g in a.geos.split(",") for r in kv8_ab(g, list(map(int, a.batches.split(","))), a.prompt, a.new)]
    elif a.kv8_quality:
        recs = kv8_quality_toy()
    elif a.kv8_trace:
        recs = [r for g in a.geos.split(",") for r in kv8_trace(g, int(a.batches.split(",")[-1]), a.prompt, a.new)]
    elif a.kvpress_shapes:
        recs = kvpress_shapes()
    elif a.kvpress:
        prompt = a.prompt if a.prompt != ap.get_default("prompt") else 7603
        new = a.new if a.new != ap.get_default("new") else 40
        recs = kvpress_quality_toy() + [r for g in a.geos.split(",") for r in kvpress_e2e(g, list(map(int, a.batches.split(","))), prompt, new,
                                                                                       reps=min(a.reps, 2))]
    elif a.sample:
        recs = sample_kernel_ab() + [r for g in a.geos.split(",") for r in sample_ab(g, list(map(int, a.batches.split(","))), a.prompt, a.new)]
    elif a.beams:
        new = a.new if a.new != ap.get_default("new") else 48
        recs = [r for g in a.geos.split(",") for r in beams_kernel_ab(g, a.prompt, new) + beams_step_ab(g, a.prompt, new, reps=min(a.reps, 3))]
    elif a.assistant:
        geos = a.geos if a.geos != ap.get_default("geos") else "llava15_7b"
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "assist_bench.jsonl")
        recs = [r for g in geos.split(",") for r in assistant_bench(g, a.prompt, a.new, reps=min(a.reps, 3), draft_layers=a.draft_layers)]
    elif a.lookup_kernel_ab:
        recs = [r for g in a.geos.split(",") for r in lookup_kernel_ab(g)]
    elif a.lookup:
        recs = [r for g in a.geos.split(",") for r in lookup_kernel_ab(g) + lookup_e2e(g, a.prompt, a.new, reps=min(a.reps, 3))]
    elif a.cfg_kernel_ab:
        recs = cfg_kernel_ab()
    elif a.dola_shapes:
        recs = dola_shapes()
    elif a.dola:
        recs = [r for g in a.geos.split(",") for r in dola_ab(g, list(map(int, a.batches.split(","))), a.prompt, a.new, reps=min(a.reps, 3))]
    elif a.attentions:
        batches = a.batches if a.batches != ap.get_default("batches") else "1,32"
        recs = [r for g in a.geos.split(",") for r in attentions_ab(g, list(map(int, batches.split(","))), a.prompt, a.new, reps=min(a.reps, 3))]
    elif a.lora:
        batches = a.batches if a.batches != ap.get_default("batches") else "1,32"
        new = a.new if a.new != ap.get_default("new") else 40
        recs = [r for g in a.geos.split(",") for r in lora_ab(g, list(map(int, batches.split(","))), a.prompt, new)]
    elif a.constraint:
        batches = a.batches if a.batches != ap.get_default("batches") else "1,32"
        recs = constraint_shapes() + [r for g in a.geos.split(",") for r in constraint_ab(g, list(map(int, batches.split(","))), a.prompt, a.new,
                                                                                          reps=min(a.reps, 3))]
    elif a.shared_shapes:
        recs = shared_shapes()
    elif a.score_shapes:
        recs = score_shapes()
    elif a.score:
        recs = [r for g in a.geos.split(",") for r in score_e2e(g, reps=min(a.reps, 3))]
    elif a.share_prefix:
        new = a.new if a.new != ap.get_default("new") else 32
        recs = [r for g in a.geos.split(",") for r in share_prefix_e2e(g, new=new, reps=min(a.reps, 3))]
    elif a.cfg:
        batches = a.batches if a.batches != ap.get_default("batches") else "1,8,16"
        recs = cfg_kernel_ab() + [r for g in a.geos.split(",") for r in cfg_ab(g, list(map(int, batches.split(","))), a.prompt, a.new)]
    elif a.batch_eval:
        recs = [r for g in a.geos.split(",") for r in batch_eval(g, n=a.requests, prompt=a.prompt, reps=min(a.reps, 3))]
    elif a.batch_kernel_ab:
        recs = [dict(geo=g, mode="generate_batch_kernel_ab", **_kernel_ab(GEOMETRIES[g]["lm"]["vocab"])) for g in a.geos.split(",")]
    elif a.batch_trace:
        recs = [r for g in a.geos.split(",") for r in batch_trace(g)]
    elif a.cont:
        batches = a.batches if a.batches != ap.get_default("batches") else "1,8"
        recs = [continue_case(g, b, reps=a.reps) for g in a.geos.split(",") for b in map(int, batches.split(","))]
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

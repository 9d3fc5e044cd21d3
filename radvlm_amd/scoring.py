"""model.score(): log-likelihoods of candidate answers after one prompt pass.

The host side, pure numpy and checkable without a GPU: request validation, grouping of the prompts into prefill groups (equal prompts
prefilled once), packing of a group's candidates into launches, the index arrays of a launch (LlavaEngine.score_tails reads them), the
memory check and the assembly of the result in input order.  The device side is LlavaEngine.score_tails: a candidate of n tokens after
a prompt of P spliced positions runs its tokens t_0 .. t_{n-2} at positions P .. P + n - 2 against the prompt's cached keys, read in
place (rv_attn_extend_prefix_bf16), and together with the prompt's last-row logits these give all n predictions."""
from types import SimpleNamespace

import numpy as np
import torch

SCORE_ROW_BUDGET = 4096          # decoder rows of one launch (the activations of a launch are a few hundred KiB per row at 7B)
LAUNCH_MAX_SEQ_TILES = 65535     # rv_attn_extend_prefix_bf16: sequences * query tiles per launch (gridDim.z)
LOGITS_BYTES_CAP = 256 << 20     # the fp32 logits of one lm_head slice


class ScoreOutput(SimpleNamespace):
    """score()'s result, per prompt i and candidate c: .token_logprobs[i][c] fp32 [len(candidate)], log_softmax(raw logits)[token] at
    every candidate position; .logprobs[i] float64 [C_i], each candidate's sum (added in fp64 in token order); .is_greedy[i] bool [C_i],
    true when every token is its row's argmax (lm-evaluation-harness's loglikelihood pair)."""

    def best(self, length_normalized=False):
        """LongTensor [N]: per prompt the index of the candidate with the highest sum, or with the highest mean per token; ties go to
        the lower index."""
        out = []
        for lp, toks in zip(self.logprobs, self.token_logprobs):
            v = lp.numpy().astype(np.float64)
            if length_normalized:
                v = v / np.array([t.numel() for t in toks], dtype=np.float64)
            out.append(int(np.argmax(v)))                     # the first of equal maxima
        return torch.tensor(out, dtype=torch.int64)


def sum_in_order(x):
    """The fp64 sum of a sequence, added left to right."""
    s = np.float64(0.0)
    for v in np.asarray(x, dtype=np.float64).reshape(-1):
        s = s + v
    return float(s)


def check_candidates(candidates, n, vocab):
    """candidates of score(), normalised: a list of n lists of int64 arrays.  ValueError for a list of another length, an empty list, an
    empty or non-1-D candidate and ids outside [0, vocab) (image placeholders included: candidates are text)."""
    if not isinstance(candidates, (list, tuple)):
        raise ValueError(f"`candidates` must be a list of {n} lists of token-id sequences, one list per prompt")
    if len(candidates) != n:
        raise ValueError(f"`candidates` has {len(candidates)} entries for {n} prompts")
    out = []
    for i, cs in enumerate(candidates):
        if not isinstance(cs, (list, tuple)) or len(cs) == 0:
            raise ValueError(f"prompt {i}: `candidates[{i}]` must be a non-empty list of token-id sequences")
        row = []
        for c, t in enumerate(cs):
            a = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
            if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"prompt {i}, candidate {c}: a candidate is a non-empty 1-D sequence of token ids, got shape {a.shape}, "
                                 f"dtype {a.dtype}")
            a = a.astype(np.int64)
            if (a < 0).any() or (a >= vocab).any():
                raise ValueError(f"prompt {i}, candidate {c}: token ids must lie in [0, {vocab}) (candidates are text: no image tokens)")
            row.append(a)
        out.append(row)
    return out


def plan_groups(records, max_batch_size):
    """Prefill groups: the prompts in input order, max_batch_size at a time; within a group prompts with equal position records (equal
    ids and image rows of bit-identical pixels and sizes: generation.position_records) are prefilled once.  Returns a list of
    SimpleNamespace(requests: the group's prompt indices, leaders: the distinct prompts to prefill (indices, first occurrence),
    row: {prompt index: its leader's place in `leaders`})."""
    if isinstance(max_batch_size, bool) or not isinstance(max_batch_size, (int, np.integer)) or max_batch_size < 1:
        raise ValueError(f"max_batch_size must be an int >= 1, got {max_batch_size!r}")
    groups = []
    for g0 in range(0, len(records), int(max_batch_size)):
        reqs = list(range(g0, min(g0 + int(max_batch_size), len(records))))
        leaders, row = [], {}
        for i in reqs:
            hit = next((k for k, j in enumerate(leaders) if len(records[j]) == len(records[i]) and
                        np.array_equal(records[j], records[i])), None)
            if hit is None:
                hit = len(leaders)
                leaders.append(i)
            row[i] = hit
        groups.append(SimpleNamespace(requests=reqs, leaders=leaders, row=row))
    return groups


def query_tile(G):
    """Query rows per workgroup of rv_attn_extend_prefix_bf16 for G q heads per kv head (csrc/score.hip xt_qs)."""
    return 16 * (1 if G >= 4 else 4 // G)


def pack_launches(lengths, G, row_budget=SCORE_ROW_BUDGET, max_seq_tiles=LAUNCH_MAX_SEQ_TILES):
    """A group's candidates (token counts `lengths`, in order) cut into consecutive launches: a launch's rows sum(len - 1) stay within
    row_budget (a candidate longer than the budget gets a launch of its own) and its sequences * ceil(max(len - 1) / query_tile(G))
    within the kernel's grid limit.  Returns a list of lists of candidate indices."""
    if row_budget < 1:
        raise ValueError(f"row_budget must be >= 1, got {row_budget}")
    qt = query_tile(G)
    launches, cur, rows, mq = [], [], 0, 0
    for c, n in enumerate(lengths):
        r = int(n) - 1
        mq2 = max(mq, r)
        tiles = max(1, -(-mq2 // qt))
        if cur and (rows + r > row_budget or (len(cur) + 1) * tiles > max_seq_tiles):
            launches.append(cur)
            cur, rows, mq2 = [], 0, r
        cur.append(c)
        rows += r
        mq = mq2
    if cur:
        launches.append(cur)
    return launches


def launch_arrays(prefix_row, prefix_len, tails):
    """The index arrays of one score_tails launch.  Candidate k (tokens tails[k], n_k >= 1 of them) continues prompt row prefix_row[k]
    of prefix_len[k] spliced positions and runs n_k - 1 rows: its tokens t_0 .. t_{n-2} at positions P .. P + n - 2, whose targets are
    t_1 .. t_{n-1}; t_0 is scored from the prompt's last-row logits (row src_row[k] = prefix_row[k] of the prefill logits).
    cu_q int32 [C + 1]; tokens / positions / targets int32 [M]; tail_rows int64 [M], row k * T_max + i of the flattened tail cache;
    first_targets / src_row / prefix_row / prefix_len int32 [C]; T_max = max_q = the longest run (0: nothing runs); the flat result holds
    candidate k's tokens at offsets[k] .. offsets[k + 1]: first_out int64 [C] and row_out int64 [M] say where each value goes."""
    C = len(tails)
    prefix_row = np.asarray(prefix_row, dtype=np.int64).reshape(-1)
    prefix_len = np.asarray(prefix_len, dtype=np.int64).reshape(-1)
    if prefix_row.shape[0] != C or prefix_len.shape[0] != C:
        raise ValueError(f"{C} candidates need {C} prefix rows and lengths")
    n = np.array([len(t) for t in tails], dtype=np.int64)
    if C == 0 or (n < 1).any():
        raise ValueError("a launch needs at least one candidate and every candidate at least one token")
    runs = n - 1
    T_max = int(runs.max())
    cu_q = np.concatenate([[0], np.cumsum(runs)]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    tk = [np.asarray(t, dtype=np.int64) for t in tails]
    return SimpleNamespace(
        C=C, M=int(runs.sum()), T_max=T_max, max_q=T_max, cu_q=cu_q, offsets=offsets,
        tokens=cat([t[:-1] for t in tk], np.int32),
        targets=cat([t[1:] for t in tk], np.int32),
        positions=cat([prefix_len[k] + np.arange(runs[k]) for k in range(C)], np.int32),
        tail_rows=cat([k * T_max + np.arange(runs[k]) for k in range(C)], np.int64),
        first_targets=np.array([t[0] for t in tk], dtype=np.int32),
        src_row=prefix_row.astype(np.int32), prefix_row=prefix_row.astype(np.int32), prefix_len=prefix_len.astype(np.int32),
        first_out=offsets[:-1].copy(),
        row_out=cat([offsets[k] + 1 + np.arange(runs[k]) for k in range(C)], np.int64))


def tail_cache_bytes(layers, kvd, n_cand, T_max):
    """Bytes of a launch's tail cache: per layer a bf16 [n_cand, T_max, 2 * kvd] tensor.  No copy of a prompt is part of it."""
    return int(layers) * int(n_cand) * int(T_max) * 2 * int(kvd) * 2


def plan_group(prefix_len, cand_row, tails, G, layers, kvd, row_budget=SCORE_ROW_BUDGET):
    """One prefill group's scoring plan.  prefix_len: the spliced length of each prefilled prompt row; cand_row[k]: the row candidate k
    continues; tails: the candidates' tokens, in the order their results are wanted.  Returns SimpleNamespace(launches: a list of
    (candidate indices, launch_arrays), prefix_rows, P_max, prefix_positions = prefix_rows * P_max (what the prefix cache holds: one row
    per distinct prompt, however many candidates), tail_cache_bytes: the largest launch's, rows: the decoder rows of all launches)."""
    prefix_len = np.asarray(prefix_len, dtype=np.int64).reshape(-1)
    cand_row = np.asarray(cand_row, dtype=np.int64).reshape(-1)
    if len(tails) != cand_row.shape[0] or (cand_row < 0).any() or (cand_row >= prefix_len.shape[0]).any():
        raise ValueError("every candidate needs the index of a prefilled prompt row")
    launches = []
    for cands in pack_launches([len(t) for t in tails], G, row_budget):
        launches.append((cands, launch_arrays(cand_row[cands], prefix_len[cand_row[cands]], [tails[c] for c in cands])))
    return SimpleNamespace(launches=launches, prefix_rows=int(prefix_len.shape[0]), P_max=int(prefix_len.max()),
                           prefix_positions=int(prefix_len.shape[0]) * int(prefix_len.max()),
                           tail_cache_bytes=max(tail_cache_bytes(layers, kvd, a.C, a.T_max) for _, a in launches),
                           rows=sum(a.M for _, a in launches))


def check_memory(need, free, prefix_rows, P_max):
    """The error of a group that does not fit, naming max_batch_size as BatchScheduler._run does."""
    if free is not None and need > free:
        raise ValueError(f"score: the prompt cache of {prefix_rows} rows x {P_max} positions and the candidates' tail cache need {need} "
                         f"bytes, but only {free} bytes of device memory are free: lower max_batch_size")


def assemble(n_cands, pieces):
    """Results in input order.  n_cands[i]: candidates of prompt i; pieces: (prompt i, candidate c, fp32 log-probs, int64 argmax ids,
    int64 tokens) in any order, each (i, c) exactly once.  Returns a ScoreOutput."""
    tl = [[None] * n for n in n_cands]
    gr = [[None] * n for n in n_cands]
    for i, c, lp, am, tok in pieces:
        if tl[i][c] is not None:
            raise ValueError(f"prompt {i}, candidate {c} was scored twice")
        tl[i][c] = torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32).copy())
        gr[i][c] = bool(np.array_equal(np.asarray(am, dtype=np.int64), np.asarray(tok, dtype=np.int64)))
    if any(t is None for row in tl for t in row):
        raise ValueError("a candidate was not scored")
    return ScoreOutput(token_logprobs=tl,
                       logprobs=[torch.tensor([sum_in_order(t.numpy()) for t in row], dtype=torch.float64) for row in tl],
                       is_greedy=[torch.tensor(row, dtype=torch.bool) for row in gr])


def score(engine, inputs, candidates, images=None, image_sizes=None, max_batch_size=32):
    """model.score() on an engine: see LlavaLlamaForCausalLM.score."""
    from .generation import BatchScheduler, batch_requests, position_records
    engine._check_generation()
    reqs = batch_requests(inputs, images, image_sizes)
    cands = check_candidates(candidates, len(reqs), engine.vocab)
    held, records = [], []                                    # one uid table per call: (pixels, image_size) of every distinct image
    for r in reqs:
        pl = engine.plan(r.ids[None], None, None, r.images, r.sizes)
        records.append(position_records(pl, BatchScheduler._image_uids(held, r))[0])
    del held
    G, L = engine.l["heads"] // engine.Hkv, engine.l["layers"]
    pieces = []
    for grp in plan_groups(records, max_batch_size):
        # image requests first: in a batch the splice gives a text-only prompt a (dummy) image slot, which must not shift later images
        order = sorted(range(len(grp.leaders)), key=lambda j: not reqs[grp.leaders[j]].images)
        place = {j: k for k, j in enumerate(order)}           # leader j sits in row place[j] of the prefill batch
        rq = [reqs[grp.leaders[j]] for j in order]
        owner = [(i, c) for i in grp.requests for c in range(len(cands[i]))]
        plan = plan_group([len(records[grp.leaders[j]]) for j in order], [place[grp.row[i]] for i, _ in owner],
                          [cands[i][c] for i, c in owner], G, L, engine.kvd)
        check_memory(engine.kv_cache_bytes(plan.prefix_rows, plan.P_max) + plan.tail_cache_bytes, engine.free_device_bytes(),
                     plan.prefix_rows, plan.P_max)
        T = max(r.ids.size for r in rq)
        ids = np.zeros((len(rq), T), dtype=np.int64)
        am = np.zeros((len(rq), T), dtype=bool)
        for b, r in enumerate(rq):
            ids[b, :r.ids.size], am[b, :r.ids.size] = r.ids, True
        imgs = [im for r in rq for im in r.images]
        sizes = [s for r in rq for s in (r.sizes or [])] if any(r.sizes is not None for r in rq) else None
        prefix, logits = engine.prefill(ids, am, imgs or None, sizes)
        for idx, arr in plan.launches:
            lp, amax = engine.score_tails(prefix, arr.prefix_row, [cands[owner[k][0]][owner[k][1]] for k in idx], logits, arrays=arr)
            lp, amax = lp.cpu().numpy(), amax.cpu().numpy()
            for j, k in enumerate(idx):
                i, c = owner[k]
                a, b = int(arr.offsets[j]), int(arr.offsets[j + 1])
                pieces.append((i, c, lp[a:b], amax[a:b], cands[i][c]))
        del prefix, logits
    return assemble([len(c) for c in cands], pieces)

"""Assisted generation's draft side (generate(assistant_model=m, num_assistant_tokens=k); HF: AssistedCandidateGenerator): a second
engine with a KV cache of its own proposes up to k tokens per round behind generation._lookup_loop's drafter hook, and the model
verifies them in one verify_step.  Greedy, the result is bit for bit the plain call's.  Sampled (do_sample=True, seed=), the round is
speculative sampling (ops.spec_accept_rows): reproducible for a given (seed, assistant, k) and distributed as the plain call, but not
token-identical to it -- the uniforms are spent differently.  Streams of one seed: 0 the target's resample / bonus draw, 1 the accept
tests, 2 the draft model's own draws."""
import numpy as np
import torch

DRAFT_TAG = 2


def check_assistant(engine, draft):
    """ValueError naming what differs when the draft engine cannot stand in for `engine`'s drafts: another vocabulary size, or a
    vision input (tower kind, image and patch size, merge type, aspect ratio, grid pinpoints) that would not take the same images /
    image_sizes.  The decoder geometry and the weight format are free.  Host only."""
    if int(draft.vocab) != int(engine.vocab):
        raise ValueError(f"assistant_model: its vocabulary holds {int(draft.vocab)} ids, the model's {int(engine.vocab)}: a draft model "
                         f"has to share the tokenizer")
    mine = dict(tower=engine.v.get("kind"), image=engine.v["image"], patch=engine.v["patch"], mm_patch_merge_type=engine.merge_type,
                image_aspect_ratio=engine.aspect, image_grid_pinpoints=engine.pinpoints)
    its = dict(tower=draft.v.get("kind"), image=draft.v["image"], patch=draft.v["patch"], mm_patch_merge_type=draft.merge_type,
               image_aspect_ratio=draft.aspect, image_grid_pinpoints=draft.pinpoints)
    diff = [f"{k} {its[k]!r} vs {mine[k]!r}" for k in mine if str(its[k]) != str(mine[k])]
    if diff:
        raise ValueError(f"assistant_model: it does not take the model's images / image_sizes ({'; '.join(diff)})")


class ModelDrafter:
    """The drafter of an assisted call: propose(seq) as generation.PromptLookupDrafter, on a B = 1 KVCache of the draft engine.
    start() prefills the cache with the call's prompt and images.  Every propose() first brings the cache up to the emitted tokens:
    `fed` are the tokens the cache holds behind the prompt, the emitted ones it agrees with are kept by setting cache.lens back (a
    rejected draft's K|V rows stay past lens as stale rows), and the rest -- the last draft and the token after it following a fully
    accepted round, else the one token that replaced a rejected draft -- go through verify_step, or decode_step when it is one token.
    Then up to k token choices, each from the step before it: the call's logits processors on the draft's own history (the emitted
    tokens, then its drafts) and the argmax, or the call's warpers and a draw with the seed's stream 2, whose warped row is kept as
    q_rows[i] for the accept kernel.  A choice is fed to the next decode_step as the device tensor it is; the drafts come to the host
    in one copy at the end.  A draft row the sampler cannot draw (a NaN in the draft model's scores) ends the draft before it: the round
    verifies what came before and the target draws that position itself.  No more than budget - emitted - 1 tokens are drafted, which is what the accept loop could still use.
    The engine's training state is not touched: prefill, decode_step and verify_step are the generation steps."""

    def __init__(self, engine, k, cfg, budget, prompt_tokens, prompt_len=0, seed=None):
        from .generation import LogitsProcessors
        self.engine, self.k, self.T, self.P = engine, int(k), int(budget), int(prompt_tokens)
        self.sm, self.seed = cfg.sampling, seed
        self.lp = LogitsProcessors(cfg, engine.vocab, prompt_len)
        self.cache, self.base, self.fed, self.q_rows = None, 0, [], None

    def start(self, ids, am, images, image_sizes):
        eng, dev = self.engine, self.engine.device
        self.cache, _ = eng.prefill(ids, am, images, image_sizes, max_new_tokens=self.T + 1)
        self.base, self.fed = int(self.cache.lens[0]), []
        self.hist = torch.zeros(1, self.T + 1, dtype=torch.int32, device=dev) if self.lp.active else None
        self.bans = self.lp.rows_device_args(dev) if self.lp.active else None
        if self.sm is not None:
            from . import ops
            self.q_rows = torch.empty(self.k, eng.vocab, dtype=torch.float32, device=dev)
            self.seed_dev = torch.tensor([self.seed], dtype=torch.int64, device=dev)
            self.ws = ops.sample_rows_workspace(1, dev)

    def _catch_up(self, emitted):
        """Feed what the cache lacks of `emitted`; returns the logits row after its last token."""
        eng, cache = self.engine, self.cache
        keep = 0
        while keep < min(len(self.fed), len(emitted) - 1) and self.fed[keep] == emitted[keep]:
            keep += 1
        cache.lens[:] = self.base + keep
        while True:
            chunk = emitted[keep:keep + 32]
            if len(chunk) == 1:
                logits = eng.decode_step(cache, np.asarray(chunk))
            else:
                logits = eng.verify_step(cache, np.asarray(chunk))[len(chunk) - 1:]
                cache.lens += len(chunk)
            keep += len(chunk)
            if keep == len(emitted):
                self.fed = list(emitted)
                return logits

    def propose(self, seq):
        from . import ops
        eng, sm, lp, V = self.engine, self.sm, self.lp, self.engine.vocab
        emitted = [int(v) for v in np.asarray(seq).reshape(-1)[self.P:]]
        t = len(emitted)
        n = min(self.k, self.T - t - 1)
        if n <= 0 or t == 0:
            return np.zeros(0, dtype=np.int64)
        logits = self._catch_up(emitted)
        if lp.active or sm is not None:
            # one upload: slot, step and EOS minimum of every draft row, then the emitted tokens
            info = eng._dev(np.concatenate([np.zeros(n), t + np.arange(n), np.full(n, lp.min_new), emitted]).astype(np.int32))
            steps = info[n:2 * n]
            if lp.active:
                self.hist[0, :t] = info[3 * n:]
        drafts, raw = [], []
        for i in range(n):
            if i:
                logits = eng.decode_step(self.cache, drafts[-1])
            if lp.active:
                nxt = ops.logits_process_argmax_rows(logits, V, self.hist, info[i:i + 1], steps[i:i + 1], info[2 * n + i:2 * n + i + 1],
                                                     lp.penalty, lp.ngram, *self.bans)
            elif sm is None:
                nxt = ops.argmax_rows(logits, V)
            if sm is not None:
                nxt = ops.sample_rows(logits, V, self.seed_dev, steps[i:i + 1], sm.temperature, sm.top_k, sm.top_p, sm.min_p,
                                      write_scores=True, ws=self.ws, tag=DRAFT_TAG)
                self.q_rows[i].copy_(logits[0, :V])
                raw.append(nxt.clone())
                nxt.clamp_(min=0)          # a row the sampler could not draw (-1): id 0 is fed so that the chain stays on the device
            if lp.active:
                self.hist[0, t + i] = nxt[0]
            drafts.append(nxt)
        out = torch.cat(raw if sm is not None else drafts).cpu().numpy().astype(np.int64)
        # the cache holds the emitted tokens and every draft but the last (id 0 where the sampler marked -1).  A draft of -1 stays -1
        # in what is returned: the accept loop's clamp_draft cuts the draft before it, so the round verifies the drafts before that
        # row and falls back to the target's own draw there; the draft model's unusable row is never tested
        self.fed = emitted + [max(int(v), 0) for v in out[:n - 1]]
        return out

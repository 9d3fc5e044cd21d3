"""CPU tests of generate_batch(share_prefix=True)'s host side (radvlm_amd/generation.py): the matching rule (best_source and the
scheduler's per-call image uids), the two-phase admission driven by the fake engine and host picker of tests/test_generate_batch_host.py,
the tile table (shared_tiles against a brute-force restatement, check_shared_tiles), the refusals, and the declarations of
rv_attn_decode_shared_bf16."""
import os

import numpy as np
import pytest
import torch

from test_generate_batch_host import IMG_ROWS, V, FakeEngine, HostPicker, alone
from radvlm_amd.generation import (SHARE_MIN_PREFIX, SHARED_TILE_COLS, BatchScheduler, batch_requests, best_source, check_shared_tiles,
                                   parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs, shared_tiles)
from radvlm_amd.splice import IMAGE_TOKEN_INDEX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 128
SYS = (np.arange(140) * 7 % V).astype(np.int64)               # a "system prompt" longer than one decode chunk


class ShareEngine(FakeEngine):
    """FakeEngine with what share_prefix reaches: a plan that position_records can read, extend(..., slots=, reuse=) and
    decode_step(shared=).  extend REFUSES a row whose first `reuse` positions are not the request's own: a copy from a row that does
    not hold the prefix fails the test there, and a wrong copy that slipped through would change the tokens (logits_of reads every
    position)."""
    shared_rows_per_tile = 16

    def __init__(self, free=None):
        super().__init__(free)
        self.extends, self.plans = [], []

    def plan(self, ids, am, labels, images, sizes):
        ids = np.asarray(ids)
        assert ids.shape[0] == 1
        idx, k = [], 0
        for v in ids[0]:
            if v == IMAGE_TOKEN_INDEX:
                idx += [-(2 + k * IMG_ROWS + j) for j in range(IMG_ROWS)]
                k += 1
            else:
                idx.append(int(v))
        n, nfr = len(idx), k * IMG_ROWS
        return dict(lens=np.array([n]), S=n, idx=np.array(idx, dtype=np.int64), attention_mask=np.ones((1, n), dtype=bool), n_feat_rows=nfr,
                    image_rows=[(i * IMG_ROWS, (i + 1) * IMG_ROWS, nfr, nfr) for i in range(k)])

    def extend(self, cache, ids, am, images, sizes, reuse=None, slots=None):
        imgs, k, rows = list(images or []), 0, []
        for b in range(ids.shape[0]):
            p = ids[b][am[b]]
            n_img = int((p == IMAGE_TOKEN_INDEX).sum())
            seq = self._splice(p, imgs[k:k + n_img])
            k += n_img
            s, r = slots[b], int(reuse[b])
            assert SHARE_MIN_PREFIX <= r <= len(seq) - 1 and cache.lens[s] == r
            assert cache.layers[0][s, :r].tolist() == seq[:r], f"slot {s} does not hold the {r} shared positions"
            cache.layers[0][s, r:len(seq)] = seq[r:]
            cache.lens[s] = len(seq)
            rows.append(self.logits_of(seq))
        self.extends.append((tuple(slots), [int(r) for r in reuse]))
        return cache, torch.stack(rows)

    def shared_plan(self, c0, tile):
        check_shared_tiles(c0, tile, self.shared_rows_per_tile)
        return (c0.copy(), tile.copy())

    def decode_step(self, cache, tokens, **kw):
        assert set(kw) <= {"shared"}
        self.plans.append(kw.get("shared") if "shared" in kw else "plain")
        return super().decode_step(cache, tokens)


def _img(i):
    return torch.full((3, 4, 4), float(i))


def _req(image, question, sys=SYS):
    """An image first (None: text only), the system prompt, then the question's tokens."""
    head = [] if image is None else [IMAGE_TOKEN_INDEX]
    return np.array(head + list(sys) + list(question), dtype=np.int64)


def _sched(prompts, images, slots, admit=None, image_sizes=None, **kw):
    cfg = parse_batch_kwargs(dict(kw), len(prompts))
    eng = ShareEngine()
    sch = BatchScheduler(eng, batch_requests(prompts, images, image_sizes), cfg, slots, return_logprobs=True, admit_free=admit, picker=HostPicker(cfg))
    return sch, eng, cfg


def _spliced(eng, prompts, images):
    return [eng._splice(p, [] if im is None else [im]) for p, im in zip(prompts, images)]


def _lcp(a, b):
    k = 0
    while k < min(len(a), len(b)) and a[k] == b[k]:
        k += 1
    return k


# ------------------------------------------------------------------------------------------------ matching
def test_best_source_rule_and_caps():
    base = np.arange(300)
    other = np.concatenate([base[:200], base[200:] + 1000])
    assert best_source(base, [(3, other)]) == (3, 200)
    assert best_source(base, [(3, base)]) == (3, 299)                             # capped at len_request - 1
    assert best_source(base, [(3, base[:150])]) == (3, 150)                       # capped at the source's prompt length
    assert best_source(base[:150], [(3, base)]) == (3, 149)
    assert best_source(base, [(5, other), (2, base[:250]), (4, base[:250])]) == (2, 250)       # the longest P, then the lowest slot
    assert best_source(base, [(1, other), (0, base[:100])]) == (1, 200)
    assert best_source(base, []) == (-1, 0)
    assert best_source(base, [(0, base + 1)]) == (-1, 0)


def test_threshold_is_one_decode_chunk():
    assert SHARE_MIN_PREFIX == CHUNK
    from radvlm_amd.engine import KVCache
    assert KVCache.chunk == SHARE_MIN_PREFIX
    a = np.arange(400)
    for p, shares in ((127, False), (128, True)):
        b = np.concatenate([a[:p], a[p:] + 1000])
        assert best_source(b, [(0, a)]) == ((0, p) if shares else (-1, 0))
    # through the scheduler: a 127-position common prefix is two prefills, a 128-position one a prefill and an extend
    for n_sys, shares in ((127 - IMG_ROWS, False), (128 - IMG_ROWS, True)):
        ps = [_req(0, [1, 2, 3], SYS[:n_sys]), _req(0, [4, 5], SYS[:n_sys])]
        sch, eng, _ = _sched(ps, [_img(0)] * 2, 2, share_prefix=True, max_new_tokens=3)
        sch.run()
        assert len(eng.extends) == int(shares)
        assert [e for e in sch.events if e[0] == "share"] == ([("share", 1, 1, 0, 128)] if shares else [])


def test_same_image_other_size_does_not_match():
    ps = [_req(0, [1, 2, 3]), _req(0, [4, 5, 6]), _req(0, [7, 8])]
    sch, eng, _ = _sched(ps, [_img(0)] * 3, 3, image_sizes=[(4, 4), (4, 5), (4, 4)], share_prefix=True, max_new_tokens=2)
    assert best_source(sch.records[1], [(0, sch.records[0])]) == (-1, 0)
    assert best_source(sch.records[2], [(0, sch.records[0])]) == (0, IMG_ROWS + len(SYS))
    sch.run()
    assert [e for e in sch.events if e[0] == "share"] == [("share", 2, 2, 0, IMG_ROWS + len(SYS))]
    # equal content in two tensors is one image; other pixels are another
    sch, _, _ = _sched(ps[:2], [_img(0), _img(0).clone()], 2, share_prefix=True, max_new_tokens=2)
    assert best_source(sch.records[1], [(0, sch.records[0])])[1] == IMG_ROWS + len(SYS)
    sch, _, _ = _sched(ps[:2], [_img(0), _img(1)], 2, share_prefix=True, max_new_tokens=2)
    assert best_source(sch.records[1], [(0, sch.records[0])]) == (-1, 0)


def test_source_may_be_a_follower_whose_row_holds_the_prefix():
    # A leads and finishes after one token; B (copied from A) keeps decoding; C is admitted into A's slot and copies from B's row
    ps = [_req(0, [1, 2]), _req(0, [3, 4, 5]), _req(0, [3, 4, 6, 7])]
    ims = [_img(0)] * 3
    sch, eng, cfg = _sched(ps, ims, 2, share_prefix=True, max_new_tokens=[1, 8, 3])
    out = sch.run()
    sp = _spliced(eng, ps, ims)
    shares = [e for e in sch.events if e[0] == "share"]
    assert shares == [("share", 1, 1, 0, _lcp(sp[1], sp[0])), ("share", 2, 0, 1, _lcp(sp[2], sp[1]))]
    assert shares[1][4] == IMG_ROWS + len(SYS) + 2                                 # B's own question tokens too: B's row holds them
    assert eng.prefills == [((0,), [V])] and [e[0] for e in eng.extends] == [(1,), (0,)]
    for i, b in enumerate([1, 8, 3]):
        assert out[f"req_{i}"].generated_tokens == alone(eng, ps[i], [ims[i]], b, cfg)


def test_slot_refilled_in_the_same_admission_is_no_source():
    # A (image 0) and X (image 1) finish together; then D (image 2) refills A's slot while C (image 0) is admitted beside it: slot 0's
    # stale rows still hold A's prompt, but C must not copy them
    ps = [_req(0, [1, 2]), _req(1, [1, 2]), _req(2, [5]), _req(0, [3, 4])]
    ims = [_img(0), _img(1), _img(2), _img(0)]
    sch, eng, cfg = _sched(ps, ims, 2, share_prefix=True, max_new_tokens=[1, 1, 3, 3])
    out = sch.run()
    assert [e for e in sch.events if e[0] == "share"] == [] and eng.extends == []
    assert [p[0] for p in eng.prefills] == [(0, 1), (0, 1)]
    # when the refilling request itself holds the prefix, it is the source, as a leader of this admission, with ITS records
    ps[2], ims[2] = _req(0, [3, 9]), _img(0)
    sch, eng, cfg = _sched(ps, ims, 2, share_prefix=True, max_new_tokens=[1, 1, 3, 3])
    out = sch.run()
    assert [e for e in sch.events if e[0] == "share"] == [("share", 3, 1, 0, IMG_ROWS + len(SYS) + 1)]
    assert [p[0] for p in eng.prefills] == [(0, 1), (0,)] and eng.extends == [((1,), [IMG_ROWS + len(SYS) + 1])]
    for i, b in enumerate([1, 1, 3, 3]):
        assert out[f"req_{i}"].generated_tokens == alone(eng, ps[i], [ims[i]], b, cfg)


# ------------------------------------------------------------------------------------------------ schedule
def _grid(n_img=3, n_q=4, seed=0):
    rng = np.random.default_rng(seed)
    ps, ims = [], []
    for i in range(n_img):
        for _ in range(n_q):
            ps.append(_req(i, rng.integers(0, V, int(rng.integers(2, 7)))))
            ims.append(_img(i))
    return ps, ims


def test_leaders_prefilled_followers_extended():
    ps, ims = _grid()
    sch, eng, cfg = _sched(ps, ims, 4, admit=4, share_prefix=True, max_new_tokens=5)
    out = sch.run()
    sp = _spliced(eng, ps, ims)
    assert [e for e in sch.events if e[0] == "admit"] == [("admit", (0, 1, 2, 3), (0, 1, 2, 3)), ("admit", (4, 5, 6, 7), (0, 1, 2, 3)),
                                                          ("admit", (8, 9, 10, 11), (0, 1, 2, 3))]
    assert eng.prefills == [((0,), [V])] * 3                                       # one leader per image, alone in its prefill
    shares = [e for e in sch.events if e[0] == "share"]
    assert [(q, s) for _, q, s, _, _ in shares] == [(q, q % 4) for q in range(12) if q % 4]
    for _, q, s, src, p in shares:
        # the longest common prefix over the sources there were: the image's leader in slot 0 (ties go to the lowest slot)
        assert src == 0 and p == min(_lcp(sp[q], sp[q - q % 4]), len(sp[q]) - 1) and p >= IMG_ROWS + len(SYS)
    assert [e[0] for e in eng.extends] == [(1, 2, 3)] * 3 and [e[1] for e in eng.extends] == [[s[4] for s in shares[k:k + 3]] for k in (0, 3, 6)]
    k = sch.events.index(shares[0])
    assert sch.events[k - 1][0] == "admit" and sch.events[k + 3][0] == "decode"     # right after the "admit" entry
    for i in range(12):
        assert out[f"req_{i}"].generated_tokens == alone(eng, ps[i], [ims[i]], 5, cfg)
    # every decode step got the table of its active set: one tile of the four slots, one whole shared chunk
    assert all(p != "plain" for p in eng.plans)
    for c0, tile in eng.plans:
        assert c0.tolist() == [1] * 4 and tile[0, :4].tolist() == [0, 1, 2, 3] and (tile[1:] == -1).all() and (tile[0, 4:] == -1).all()


def test_followers_retile_when_the_leader_finishes_and_its_slot_is_refilled():
    ps, ims = _grid(n_img=1, n_q=4)
    ps.append(_req(7, [1, 2, 3]))                                                  # another image: refills the leader's slot
    ims.append(_img(7))
    sch, eng, cfg = _sched(ps, ims, 4, admit=1, share_prefix=True, max_new_tokens=[2, 7, 7, 7, 4])
    out = sch.run()
    fin = [e for e in sch.events if e[0] == "finish"]
    assert fin[0] == ("finish", 0, 0, 2) and ("admit", (4,), (0,)) in sch.events
    tables = [(c0.tolist(), tile[:, :4].tolist()) for c0, tile in (p for p in eng.plans if p != "plain")]
    none = [-1] * 4
    assert tables[0] == ([1] * 4, [[0, 1, 2, 3], none, none, none])               # the leader decodes once (its budget is 2)
    assert tables[1] == ([0, 1, 1, 1], [none, [1, 2, 3, -1], none, none])          # then the followers tile among themselves,
    assert all(t == tables[1] for t in tables[1:])                                 # also beside the other image's request in slot 0
    assert len(tables) == 6 and "plain" not in eng.plans
    for i, b in enumerate([2, 7, 7, 7, 4]):
        assert out[f"req_{i}"].generated_tokens == alone(eng, ps[i], [ims[i]], b, cfg)


def test_nothing_in_common_is_the_plain_run():
    ps = [_req(i if i % 3 else None, [i, i + 1, i + 2], SYS[i:i + 20] + i) for i in range(7)]
    ims = [_img(i) if i % 3 else None for i in range(7)]
    runs = []
    for kw in ({}, dict(share_prefix=False), dict(share_prefix=True)):
        sch, eng, cfg = _sched(ps, ims, 3, max_new_tokens=[3, 5, 2, 6, 4, 1, 5], **kw)
        out = sch.run()
        runs.append((sch.events, {k: (v.generated_tokens, v.logprobs) for k, v in out.items()}, eng.prefills, eng.plans, eng.extends))
    assert runs[0] == runs[1] == runs[2]
    assert runs[2][4] == [] and set(runs[2][3]) == {"plain"}                       # decode_step was never given shared=


# ------------------------------------------------------------------------------------------------ tables
def _tiles_brute(active, lineage, P, rpt, chunk, S):
    c0 = np.zeros(S, dtype=np.int32)
    tile = np.full((S, SHARED_TILE_COLS), -1, dtype=np.int32)
    act = set(int(s) for s in active)
    for s in range(S):
        if s not in act or lineage[s] < 0:
            continue
        mates = [u for u in range(S) if u in act and lineage[u] == lineage[s]]
        k = mates.index(s) // rpt
        mine = mates[k * rpt:(k + 1) * rpt]
        c = min(P[u] for u in mine) // chunk
        if len(mine) >= 2 and c > 0:
            c0[s] = c
            if mine[0] == s:
                tile[s, :len(mine)] = mine
    return c0, tile


@pytest.mark.parametrize("rpt", [2, 4, 16])
def test_shared_tiles_against_brute_force(rpt):
    rng = np.random.default_rng(rpt)
    seen_tiles = 0
    for _ in range(200):
        S = int(rng.integers(1, 40))
        lineage = rng.integers(-1, 4, S)
        P = np.where(lineage >= 0, rng.choice([70, 96, 128, 200, 256, 300, 700], S), 0)
        active = np.flatnonzero(rng.random(S) < 0.7)
        c0, tile = shared_tiles(active, lineage, P, rpt, 32 if rpt == 4 else 128, S)
        rc0, rtile = _tiles_brute(active, lineage, P, rpt, 32 if rpt == 4 else 128, S)
        assert c0.dtype == np.int32 and tile.dtype == np.int32 and tile.shape == (S, SHARED_TILE_COLS)
        assert np.array_equal(c0, rc0) and np.array_equal(tile, rtile)
        check_shared_tiles(c0, tile, rpt)
        idle = np.setdiff1d(np.arange(S), active)
        assert (c0[idle] == 0).all() and (tile[idle] == -1).all() and (c0[lineage < 0] == 0).all()
        seen_tiles += int((tile[:, 0] >= 0).sum())
    assert seen_tiles > 100


def test_check_shared_tiles_rejects():
    lineage, P = np.zeros(6, dtype=np.int64), np.full(6, 300)
    c0, tile = shared_tiles(np.arange(6), lineage, P, 4, 128, 6)
    assert c0.tolist() == [2] * 6 and tile[0, :4].tolist() == [0, 1, 2, 3] and tile[4, :3].tolist() == [4, 5, -1]
    check_shared_tiles(c0, tile, 4)

    def bad(edit, rpt=4, match="shared tiles"):
        c, t = c0.copy(), tile.copy()
        edit(c, t)
        with pytest.raises(ValueError, match=match):
            check_shared_tiles(c, t, rpt)

    bad(lambda c, t: t.__setitem__((0, 1), 6), match="outside")                    # an entry >= S
    bad(lambda c, t: t.__setitem__((0, 1), -2), match="outside")                   # an entry < -1
    bad(lambda c, t: t.__setitem__((1, slice(0, 2)), [0, 1]), match="leader comes first")      # a non-leader listed first
    bad(lambda c, t: c.__setitem__(2, 1), match="one shared chunk count")          # unequal c0 within a tile
    bad(lambda c, t: c.__setitem__(slice(0, 4), 0), match="one shared chunk count")            # a listed tile without a shared chunk
    bad(lambda c, t: t.__setitem__((4, 2), 3), match="exactly one")                # a row in two tiles
    bad(lambda c, t: t.__setitem__((0, slice(0, 4)), [0, 1, -1, 3]))               # -1 inside a list
    bad(lambda c, t: t.__setitem__((4, slice(0, 3)), -1), match="exactly one")     # rows with c0 > 0 that no tile lists
    bad(lambda c, t: c.__setitem__(5, -1), match="negative")
    bad(lambda c, t: None, rpt=2)                                                  # a tile of more rows than the kernel reads
    with pytest.raises(ValueError):
        check_shared_tiles(c0, tile[:, :8], 4)
    with pytest.raises(ValueError):
        check_shared_tiles(c0[:5], tile, 4)


# ------------------------------------------------------------------------------------------------ refusals and types
def test_refusals_and_types():
    assert parse_batch_kwargs({}, 2).share_prefix is False
    assert parse_batch_kwargs(dict(share_prefix=False), 2).share_prefix is False
    assert parse_batch_kwargs(dict(share_prefix=True, do_sample=True, seed=3), 2).share_prefix is True
    assert parse_batch_kwargs(dict(share_prefix=False, kv_cache_dtype="int8", guidance_scale=2.0), 2).share_prefix is False
    with pytest.raises(NotImplementedError, match="int8"):
        parse_batch_kwargs(dict(share_prefix=True, kv_cache_dtype="int8"), 2)
    with pytest.raises(NotImplementedError, match="guidance_scale"):
        parse_batch_kwargs(dict(share_prefix=True, guidance_scale=2.0), 2)
    for v in (1, 0, "yes", None, [True]):
        with pytest.raises(ValueError, match="share_prefix"):
            parse_batch_kwargs(dict(share_prefix=v), 2)
    with pytest.raises(TypeError, match="share_prefix"):
        parse_generate_kwargs(dict(share_prefix=True))
    with pytest.raises(TypeError, match="share_prefix"):
        parse_generate_kwargs(dict(share_prefix=True), lookup=True)
    with pytest.raises(TypeError, match="share_prefix"):
        parse_beam_kwargs(dict(share_prefix=True, num_beams=2))


def test_entry_point_is_declared_and_built():
    from radvlm_amd import lib, ops
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert "prefix" in build.split('SRCS="')[1].split('"')[0].split() and '$(printf "$OBJ/%s.res " $SRCS)' in build
    assert len(lib.SIGNATURES["rv_attn_decode_shared_bf16"][1]) == 21
    assert callable(ops.attn_decode_shared) and ops.SHARED_TILE_COLS == SHARED_TILE_COLS == 16


def test_route_table():
    """shared_route None: the measured table (one q head per kv head, from 3 rows in a tile or 2,313 shared keys on); forced arms."""
    from types import SimpleNamespace
    from radvlm_amd.engine import KVCache, LlavaEngine
    eng = LlavaEngine.__new__(LlavaEngine)                                         # the lookup alone: no device, no weights
    cache = SimpleNamespace(chunk=KVCache.chunk)

    def plan(rows, c0):
        tile = np.full((rows + 1, 16), -1, dtype=np.int32)
        tile[0, :rows] = np.arange(rows)
        return SimpleNamespace(tile_host=tile, c0_host=np.array([c0] * rows + [0], dtype=np.int32))

    eng.l, eng.Hkv = dict(heads=32), 32
    assert [eng._use_shared(plan(r, c), cache) for r, c in ((2, 5), (2, 18), (2, 19), (3, 1), (16, 59))] == [False, False, True, True, True]
    eng.l, eng.Hkv = dict(heads=28), 4
    assert not any(eng._use_shared(plan(r, c), cache) for r, c in ((2, 5), (2, 59)))
    eng.l, eng.Hkv = dict(heads=8), 4                                              # an unmeasured group size: plain
    assert not eng._use_shared(plan(8, 59), cache)
    eng.shared_route = "shared"
    assert eng._use_shared(plan(2, 1), cache)
    eng.shared_route = "plain"
    eng.l, eng.Hkv = dict(heads=32), 32
    assert not eng._use_shared(plan(16, 59), cache)
    eng.shared_route = "neither"
    with pytest.raises(ValueError):
        eng._use_shared(plan(16, 59), cache)

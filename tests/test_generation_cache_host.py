"""CPU tests of the conversation KV cache's host side (generate(past_key_values=GenerationCache())): keyword validation, the position
records of a splice plan, the prefix-matching rule, the growth size and the C-ABI declaration of the extend attention kernel."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from radvlm_amd.engine import LlavaEngine
from radvlm_amd.generation import (NEWLINE_RECORD, GenerationCache, grown_length, parse_generate_kwargs, position_records,
                                   reuse_lengths)
from radvlm_amd.splice import IMAGE_TOKEN_INDEX as IMG


def _planner(merge_type="flat", padding_side="right", side=2):
    """The fields LlavaEngine.plan reads, for a tower of side x side patches (no device, no weights)."""
    return SimpleNamespace(P=side * side, side=side, merge_type=merge_type, aspect="square", pinpoints=None, v={"image": 28},
                           max_len=None, padding_side=padding_side)


def _plan(rows, n_images, padding_side="right", merge_type="flat"):
    T = max(len(r) for r in rows)
    ids = np.zeros((len(rows), T), dtype=np.int64)
    am = np.zeros((len(rows), T), dtype=bool)
    for b, r in enumerate(rows):
        sl = slice(T - len(r), T) if padding_side == "left" else slice(0, len(r))
        ids[b, sl], am[b, sl] = r, True
    images = [torch.zeros(3, 28, 28) for _ in range(n_images)]
    return LlavaEngine.plan(_planner(merge_type, padding_side), ids, am, None, images, [(28, 28)] * n_images)


def test_extend_symbol_declared_and_bound():
    from radvlm_amd import lib
    assert "rv_attn_extend_bf16" in lib.SIGNATURES


def test_past_key_values_keyword_validation():
    c = GenerationCache()
    assert parse_generate_kwargs(dict(past_key_values=c)).past_key_values is c
    assert parse_generate_kwargs({}).past_key_values is None
    assert parse_generate_kwargs(dict(past_key_values=c, use_cache=True)).past_key_values is c
    with pytest.raises(TypeError, match="GenerationCache"):
        parse_generate_kwargs(dict(past_key_values=((torch.zeros(1), torch.zeros(1)),)))
    with pytest.raises(TypeError, match="GenerationCache"):
        parse_generate_kwargs(dict(past_key_values=object()))
    with pytest.raises(ValueError, match="use_cache"):
        parse_generate_kwargs(dict(past_key_values=c, use_cache=False))


def test_empty_cache_surface():
    c = GenerationCache()
    assert c.get_seq_length() == 0 and c.batch_size is None
    c.crop(5)                                          # no-op when empty
    assert c.get_seq_length() == 0


def test_records_of_tokens_and_image_rows():
    p = _plan([[5, 6, IMG, 7]], 1)                     # 2x2 patches: 4 image rows
    (r,) = position_records(p, [3])
    assert r.tolist()[:2] == [5, 6] and r.tolist()[-1] == 7 and r.size == 7
    img = r[2:6]
    assert (img < 0).all() and len(set(img.tolist())) == 4
    (r2,) = position_records(p, [4])                   # another image: same tokens, other image rows
    assert (r2[:2] == r[:2]).all() and (r2[2:6] != r[2:6]).all() and r2[6] == r[6]


def test_records_mark_image_newline():
    p = _plan([[5, IMG, 7]], 1, merge_type="spatial_unpad")
    (r,) = position_records(p, [0])
    assert NEWLINE_RECORD in r.tolist()


def test_reuse_rule_tokens_and_cap():
    a = np.array([1, 2, 3, 4, 5])
    assert reuse_lengths([a], [np.array([1, 2, 3, 4, 5, 6, 7])]).tolist() == [5]     # cached prefix fully reused
    assert reuse_lengths([a], [np.array([1, 2, 9, 4, 5, 6])]).tolist() == [2]        # rewritten history: the true common prefix
    assert reuse_lengths([a], [a.copy()]).tolist() == [4]                            # the same prompt: the last position is recomputed
    assert reuse_lengths([a], [np.array([1, 2, 3])]).tolist() == [2]                 # a shorter prompt: len - 1
    assert reuse_lengths([a], [np.array([7, 2, 3])]).tolist() == [0]
    assert reuse_lengths([a], [np.array([1])]).tolist() == [0]


def test_reuse_rule_image_rows():
    p1 = _plan([[5, 6, IMG, 7]], 1)
    old = position_records(p1, [0])
    p2 = _plan([[5, 6, IMG, 7, 8, 9]], 1)
    assert reuse_lengths(old, position_records(p2, [0])).tolist() == [7]             # the image and the text after it
    assert reuse_lengths(old, position_records(p2, [1])).tolist() == [2]             # a changed image: only the text before it
    p3 = _plan([[5, 4, IMG, 7, 8]], 1)
    assert reuse_lengths(old, position_records(p3, [0])).tolist() == [1]


def test_reuse_rule_rows_differ_and_padding_side():
    for side in ("right", "left"):
        old = position_records(_plan([[1, 2, 3, 4], [1, 2]], 0, padding_side=side), [])
        new = position_records(_plan([[1, 2, 3, 4, 5, 6], [1, 9, 9, 9, 9]], 0, padding_side=side), [])
        assert [x.tolist() for x in new] == [[1, 2, 3, 4, 5, 6], [1, 9, 9, 9, 9]]     # valid positions only, whatever the side
        assert reuse_lengths(old, new).tolist() == [4, 1]


def test_reuse_rule_two_images_in_a_batch():
    p = _plan([[5, IMG, 6], [7, IMG, 8]], 2)
    old = position_records(p, [0, 1])
    assert reuse_lengths(old, position_records(p, [0, 2])).tolist() == [5, 1]        # row 1's image changed


def test_crop_keeps_records_and_lengths_together():
    from radvlm_amd.engine import KVCache
    c = GenerationCache()
    c.kv = KVCache([torch.zeros(2, 8, 4)], [6, 3], 8)
    c.records = [np.arange(6), np.arange(3)]
    assert c.get_seq_length() == 6 and c.batch_size == 2
    c.crop(4)
    assert c.kv.lens.tolist() == [4, 3] and [len(r) for r in c.records] == [4, 3]
    c.crop(-1)
    assert c.kv.lens.tolist() == [3, 3] and [len(r) for r in c.records] == [3, 3]


def test_bind_checks_engine_batch_and_weights_version():
    from radvlm_amd.engine import KVCache
    e1, e2 = SimpleNamespace(weights_version=0), SimpleNamespace(weights_version=0)
    c = GenerationCache()
    c._bind(e1, 2)
    c.kv, c.records, c.weights_version = KVCache([torch.zeros(2, 8, 4)], [3, 3], 8), [np.arange(3)] * 2, 0
    with pytest.raises(ValueError, match="another model"):
        c._bind(e2, 2)
    with pytest.raises(ValueError, match="sequences"):
        c._bind(e1, 3)
    c._bind(e1, 2)
    assert c.get_seq_length() == 3
    e1.weights_version = 1                             # the weights changed since: the cache is emptied
    c._bind(e1, 2)
    assert c.get_seq_length() == 0 and c.kv is None


def test_image_identity_is_bitwise():
    c = GenerationCache()
    a = torch.randn(3, 4, 4)
    uids = c._image_uids([a], [(4, 4)])
    c.images = [(uids[0], a.clone(), (4, 4))]
    assert c._image_uids([a.clone()], [(4, 4)]) == uids
    assert c._image_uids([a.clone()], [(4, 5)]) != uids                             # another image_size
    b = a.clone()
    b[0, 0, 0] = torch.nextafter(b[0, 0, 0], torch.tensor(1e9))
    assert c._image_uids([b], [(4, 4)]) != uids                                      # one ulp differs
    assert c._image_uids([a.to(torch.float64)], [(4, 4)]) != uids                    # another dtype


def test_growth_size():
    assert grown_length(300, 300) == 300
    assert grown_length(300, 120) == 300
    assert grown_length(300, 301) == 512
    assert grown_length(1000, 7600) == 7680
    assert grown_length(256, 257) % 256 == 0

"""CPU tests of generate()'s host side: keyword validation, the token budget, EOS / pad / stopping-criteria bookkeeping of the greedy loop,
and the C-ABI declarations of the decode kernels."""
import os

import numpy as np
import pytest
import torch

from radvlm_amd.generation import GreedyState, new_token_budget, parse_generate_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_SYMBOLS = ("rv_gemv_bf16", "rv_gemv_split", "rv_attn_decode_bf16", "rv_kv_append_bf16", "rv_argmax_rows_f32")


def test_decode_symbols_declared_and_bound():
    from radvlm_amd import lib
    assert set(DECODE_SYMBOLS) <= set(lib.SIGNATURES)


def test_gemv_split_depends_on_weight_shape_only():
    """The split-K factor of the skinny GEMM is a function of (N, K): a row's reduction order never depends on the batch."""
    from radvlm_amd import lib, ops
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    lib.load()
    assert ops.gemv_split(32000, 4096) >= 1
    for N, K in ((4096, 4096), (3584, 18944), (4608, 3584), (256, 448)):
        s = ops.gemv_split(N, K)
        assert s >= 1 and (K + 31) // 32 >= s * 8, (N, K, s)


def test_kwargs_validation():
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(do_sample=True))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(num_beams=4))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(streamer=object()))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs(dict(inputs_embeds=torch.zeros(1, 2, 8)))
    with pytest.raises(NotImplementedError):
        parse_generate_kwargs({}, lora=True)
    with pytest.raises(TypeError):
        parse_generate_kwargs(dict(no_such_option=1))
    with pytest.raises(TypeError):
        parse_generate_kwargs(dict(stopping_criteria=[3]))
    c = parse_generate_kwargs(dict(do_sample=False, num_beams=1, temperature=0.2, top_p=None, use_cache=True, max_new_tokens=7))
    assert c.max_new_tokens == 7 and c.eos == [] and c.pad == 0
    assert parse_generate_kwargs(dict(eos_token_id=2)).pad == 2                   # pad defaults to the first EOS
    assert parse_generate_kwargs(dict(eos_token_id=[5, 2], pad_token_id=0)).eos == [5, 2]
    assert parse_generate_kwargs({}, config_eos=9).eos == [9]


def test_token_budget():
    mk = lambda **k: parse_generate_kwargs(k)
    assert new_token_budget(mk(), 100) == 20
    assert new_token_budget(mk(max_new_tokens=5, max_length=3), 100) == 5
    assert new_token_budget(mk(max_length=120), 100) == 20            # inputs_embeds generation: max_length counts the prompt
    assert new_token_budget(mk(max_length=50), 100) == 0


def test_eos_rows_are_padded_after_finishing():
    st = GreedyState(3, parse_generate_kwargs(dict(eos_token_id=[7, 8], pad_token_id=0)))
    assert list(st.step(np.array([7, 1, 2]))) == [7, 1, 2]
    assert list(st.unfinished) == [False, True, True]
    assert list(st.step(np.array([5, 8, 3]))) == [0, 8, 3]
    assert list(st.unfinished) == [False, False, True] and not st.all_done
    assert list(st.step(torch.tensor([4, 4, 8]))) == [0, 0, 8]
    assert st.all_done
    assert st.sequences().tolist() == [[7, 0, 0], [1, 8, 0], [2, 3, 8]]


def test_without_eos_nothing_is_padded():
    st = GreedyState(2, parse_generate_kwargs(dict(pad_token_id=0)))
    st.step(np.array([7, 1]))
    st.step(np.array([7, 1]))
    assert st.sequences().tolist() == [[7, 7], [1, 1]] and not st.all_done


def test_stopping_criteria_bool_and_per_row():
    calls = []

    def keyword(ids, scores):             # the radiology eval's form: (ids, scores) -> bool
        calls.append(ids.shape)
        return bool((ids[:, -1] == 42).all())

    st = GreedyState(2, parse_generate_kwargs(dict(stopping_criteria=[keyword])))
    st.step(np.array([42, 1]), scores=torch.zeros(2, 10))
    assert not st.all_done
    st.step(np.array([42, 42]), scores=torch.zeros(2, 10))
    assert st.all_done and calls == [(2, 1), (2, 2)]
    st = GreedyState(2, parse_generate_kwargs(dict(stopping_criteria=[lambda i, s: torch.tensor([True, False])], eos_token_id=3,
                                                   pad_token_id=9)))
    st.step(np.array([1, 1]))
    assert list(st.unfinished) == [False, True]
    assert list(st.step(np.array([1, 1]))) == [9, 1]

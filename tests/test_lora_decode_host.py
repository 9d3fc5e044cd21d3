"""Host tests of live-adapter decoding: the C ABI of csrc/lora_decode.hip and of gemv.hip's adapter entry as declared, bound and exported, the K split of the
down-projection (a host function), and the generation parsers' refusal, which now names the switch as well."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rv_lora_down_rows_bf16", "rv_gemv_lora_bf16")


def test_symbols_declared_bound_and_exported():
    from radvlm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "radvlm_hip.h")).read()
    dll = lib.load()
    for s in SYMBOLS:
        assert s in lib.SIGNATURES, s
        assert getattr(dll, s) is not None
    assert "int rv_lora_down_split(int r, int K);" in hdr and "rv_lora_down_split" in lib.SIGNATURES
    assert "lora_decode" in open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read().split('SRCS="')[1].split('"')[0].split()


def test_down_split_is_a_function_of_k_that_keeps_two_steps_per_wave():
    from radvlm_amd import ops
    for r in (8, 40, 64):
        assert [ops.lora_down_split(r, K) for K in (40, 96, 512, 1024, 2048, 4096, 11008, 18944)] == [1, 1, 2, 4, 8, 16, 32, 32]
    for K in range(8, 20000, 1208):
        split, steps = ops.lora_down_split(64, K), (K + 31) // 32
        assert split == 1 or steps // (4 * split) >= 2


def test_parsers_keep_refusing_and_name_the_switch():
    from radvlm_amd.generation import parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs
    for parse in (lambda: parse_generate_kwargs(dict(max_new_tokens=2), lora=True), lambda: parse_batch_kwargs(dict(max_new_tokens=2), 1, lora=True),
                  lambda: parse_beam_kwargs(dict(max_new_tokens=2, num_beams=2), lora=True)):
        with pytest.raises(NotImplementedError, match="merge_and_unload") as e:
            parse()
        assert "enable_adapter_decoding" in str(e.value)
    parse_generate_kwargs(dict(max_new_tokens=2), lora=False)

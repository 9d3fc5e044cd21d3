"""CPU tests of what the seven split-KV cache attention entry points share: every source includes csrc/attn_split.h and none restates
the combine, and the ops wrappers check a caller's `out` before they reach the library."""
import os
import re

import pytest
import torch

from radvlm_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("decode", "beam", "kvq", "lookup", "prefix", "extend", "score")


def test_sources_share_the_header_and_restate_no_combine():
    csrc = os.path.join(ROOT, "radvlm_amd", "csrc")
    hdr = open(os.path.join(csrc, "attn_split.h")).read()
    assert len(re.findall(r"void (\w*_combine_kernel)\(", hdr)) == 1 and "attn_split_launch(" in hdr and "split_merge(" in hdr
    for name in SOURCES:
        src = open(os.path.join(csrc, name + ".hip")).read()
        assert '#include "attn_split.h"' in src and "attn_split_launch(" in src, name          # the launcher and the combine are shared,
        assert not re.search(r"void \w*_combine_kernel\(", src), name                         # not restated
    for name, body in (("decode", "attn_decode_body<"), ("beam", "attn_decode_body<"), ("lookup", "attn_decode_nq_body<"),
                       ("prefix", "attn_decode_nq_body<"), ("extend", "attn_extend_body<"), ("score", "attn_extend_body<")):
        assert body in open(os.path.join(csrc, name + ".hip")).read(), name
    for name in ("decode", "beam", "score"):                                                  # one torch.argmax tie rule, in common.h
        src = open(os.path.join(csrc, name + ".hip")).read()
        assert "am_better(" in src and not re.search(r"bool \w+_better\(", src), name
    assert len(re.findall(r"bool am_better\(", open(os.path.join(csrc, "common.h")).read())) == 1


@pytest.mark.parametrize("wrapper", ["attn_decode", "attn_decode_kv8", "attn_decode_beam"])
def test_wrappers_check_a_passed_out_before_any_library_call(wrapper, monkeypatch):
    """CPU tensors stand in for device ones (the device / dtype assertion is stubbed out): a right-shaped `out` reaches lib.call once, a
    wrong-shaped or column-strided one raises AssertionError first."""
    calls = []
    monkeypatch.setattr(ops, "_chk", lambda t, dtype=None: t)
    monkeypatch.setattr(lib, "call", lambda name, *args: calls.append(name))
    B, L_max, H, Hkv, hd = 2, 64, 4, 2, 64
    q = torch.zeros(B, H * hd, dtype=torch.bfloat16)
    kv_len = torch.tensor([3, 64], dtype=torch.int32)
    cache = torch.zeros(B, L_max, 2 * Hkv * hd, dtype=torch.bfloat16)

    def run(out):
        if wrapper == "attn_decode":
            return ops.attn_decode(q, cache, kv_len, H, Hkv, hd, Hkv * hd, out=out)
        if wrapper == "attn_decode_kv8":
            c8 = (cache.to(torch.int8), torch.ones(B, L_max, 2 * Hkv))
            return ops.attn_decode_kv8(q, c8, kv_len, H, Hkv, hd, Hkv * hd, out=out)
        own = torch.tensor([0, 1], dtype=torch.int32)
        return ops.attn_decode_beam(q, cache, kv_len, own, kv_len, None, H, Hkv, hd, Hkv * hd, out=out)

    good = torch.zeros(B, H * hd, dtype=torch.bfloat16)
    assert run(good) is good and run(None).shape == (B, H * hd) and len(calls) == 2
    for bad in (torch.zeros(B, H * hd - 8, dtype=torch.bfloat16), torch.zeros(B + 1, H * hd, dtype=torch.bfloat16),
                torch.zeros(B, 2 * H * hd, dtype=torch.bfloat16)[:, ::2]):
        with pytest.raises(AssertionError):
            run(bad)
    assert len(calls) == 2

"""GPU tests of radvlm_amd/csrc/nf4.hip, all exact: rv_nf4_quantize_bf16 against tests/nf4_ref.py bit for bit on codes and absmax (its own
CPU checks: tests/test_nf4_host.py), rv_nf4_dequant_bf16 against it bit for bit in both modes -- a three-tensor table with non-adjacent
destinations against three one-tensor launches -- and the second level's codes against rv_adam8_quantize_f32.  Every buffer carries a
sentinel behind (and between the tensors of a table) what a kernel may write."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nf4_ref as R

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
_INT = {BF16: torch.int16, F32: torch.int32, U8: torch.uint8}
_SENT = {BF16: 0x7fc5, F32: 0x7fc5a5a5, U8: 0xAB}


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _sent(shape, dtype=BF16, device="cuda"):
    return torch.full(tuple(shape), _SENT[dtype], dtype=_INT[dtype], device=device).view(dtype)


def _same(got, want, what):
    g, w = got.contiguous().view(_INT[got.dtype]).cpu(), want.contiguous().view(_INT[want.dtype]).cpu()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bool(bad.any()):
        i = int(bad.reshape(-1).int().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ; first at {i}: got {int(g.reshape(-1)[i]) & 0xffffffff:#x}, "
                             f"want {int(w.reshape(-1)[i]) & 0xffffffff:#x}")


def _bf16(x):
    """bf16-exact fp32 numpy -> bf16 tensor on the device, through the bit patterns."""
    return torch.from_numpy(R.bf16_bits(x).view(np.int16)).cuda().view(BF16)


def _bits(u16, device="cpu"):
    return torch.from_numpy(np.asarray(u16, np.uint16).view(np.int16)).to(device).view(BF16)


# ------------------------------------------------------------------------------------------------ quantise
def test_quantize_matches_the_reference_bit_for_bit():
    ops = _ops()
    for name, x in R.host_inputs().items():
        n, nb, nc = x.size, R.nblocks(x.size), (x.size + 1) // 2
        codes, absmax = _sent((nc + 5,), U8), _sent((nb + 1,), F32)
        ops.nf4_quantize(_bf16(x), codes, absmax)
        wc, wa = R.quantize(x)
        want_c, want_a = _sent((nc + 5,), U8, "cpu"), _sent((nb + 1,), F32, "cpu")
        want_c[:nc], want_a[:nb] = torch.from_numpy(wc), torch.from_numpy(wa)
        _same(codes, want_c, f"{name}: codes")            # the sentinel bytes behind the last code and absmax entry are untouched
        _same(absmax, want_a, f"{name}: absmax")


# ------------------------------------------------------------------------------------------------ dequantise
LENS = (320, 65, 16447)


def _store(dq):
    """Three tensors in one set of buffers (16-byte aligned starts, gaps of sentinel between them) and their reference dequantisation."""
    r = np.random.RandomState(5)
    xs = [R.bf16_round((0.02 * r.randn(n)).astype(np.float32)) for n in LENS]
    xs[2][64 * 200:64 * 201] = 0.0                                          # an all-zero block inside the long tensor
    code0, blk0, s20 = [], [], []
    c = b = s = 0
    for x in xs:
        c, b, s = (c + 15) // 16 * 16 + 16, (b + 15) // 16 * 16 + 16, (s + 3) // 4 * 4 + 4
        code0.append(c), blk0.append(b), s20.append(s)
        c, b, s = c + (x.size + 1) // 2, b + R.nblocks(x.size), s + (R.nblocks(x.size) + 255) // 256
    codes = _sent((c + 16,), U8, "cpu")
    absmax, acodes, scale2 = _sent((b + 4,), F32, "cpu"), _sent((b + 16,), U8, "cpu"), _sent((s + 4,), F32, "cpu")
    offset = torch.zeros(3, dtype=F32)
    want = []
    for k, x in enumerate(xs):
        packed, am = R.quantize(x)
        codes[code0[k]:code0[k] + packed.size] = torch.from_numpy(packed)
        absmax[blk0[k]:blk0[k] + am.size] = torch.from_numpy(am)
        c2, sc2, off = R.double_quantize(am)
        acodes[blk0[k]:blk0[k] + c2.size] = torch.from_numpy(c2)
        scale2[s20[k]:s20[k] + sc2.size] = torch.from_numpy(sc2)
        offset[k] = float(off)
        want.append(R.dequantize(packed, R.effective_absmax(c2, sc2, off) if dq else am, x.size))
    dev = dict(codes=codes.cuda())
    if dq:
        dev.update(absmax_codes=acodes.cuda(), scale2=scale2.cuda(), offset=offset.cuda())
    else:
        dev.update(absmax=absmax.cuda())
    return xs, code0, blk0, s20, dev, want


def _table(ks, code0, blk0, s20, dst0):
    n = np.array([LENS[k] for k in ks], np.int64)
    nch = (n + 2047) // 2048
    tab = np.array([np.cumsum(nch) - nch, [code0[k] for k in ks], [blk0[k] for k in ks], n, dst0, [s20[k] for k in ks]], np.int64)
    return tab, int(nch.sum())


@pytest.mark.parametrize("dq", [False, True])
def test_dequant_table_matches_the_reference_and_three_single_launches(dq):
    ops = _ops()
    xs, code0, blk0, s20, dev, want = _store(dq)
    assert 16447 > 8 * 2048 and 16447 % 2048 and 16447 % 8                    # full vector chunks, then a short, odd tail
    # non-adjacent destinations: 16-byte aligned, 2-byte aligned only (the masked narrow form on whole chunks), 16-byte aligned
    dst0 = [8, 8 + 320 + 35, 8 + 320 + 35 + 65 + 28]
    total = dst0[2] + LENS[2] + 9
    assert dst0[1] % 8 and not dst0[2] % 8

    def launch(ks, out):
        tab, nch = _table(ks, code0, blk0, s20, [dst0[k] for k in ks])
        kw = dict(dev)
        if dq:
            kw["offset"] = dev["offset"][ks[0]:ks[0] + len(ks)].contiguous()
        ops.nf4_dequant(kw.pop("codes"), torch.from_numpy(tab).cuda(), tab, nch, out, **kw)

    out = _sent((total,))
    launch([0, 1, 2], out)
    ref = _sent((total,), device="cpu")
    for k in range(3):
        ref[dst0[k]:dst0[k] + LENS[k]] = _bits(want[k])
    _same(out, ref, f"dq={dq}: table launch against the reference (and the sentinel outside the tensors)")
    single = _sent((total,))
    for k in range(3):
        launch([k], single)
    _same(single, ref, f"dq={dq}: three one-tensor launches")
    again = _sent((total,))
    launch([0, 1, 2], again)
    _same(again, out, f"dq={dq}: a second launch")
    if dq:                                                                   # double quantisation changes the weights, and only through absmax
        plain = _store(False)[5]
        assert any(not np.array_equal(a, b) for a, b in zip(plain, want))


def test_second_level_codes_are_the_8bit_optimizer_quantisers():
    """absmax - offset through rv_adam8_quantize_f32(kind 0) gives the reference's second-level codes and scales, on the absmax the
    quantise kernel wrote; 257 blocks: a short last second-level block."""
    ops = _ops()
    from radvlm_amd import nf4 as N
    x = R.host_inputs()[f"n{64 * 256 + 63}"]
    _, am = ops.nf4_quantize(_bf16(x))
    host = am.cpu().numpy()
    assert host.size == 257 and np.array_equal(host.view(np.uint32), R.quantize(x)[1].view(np.uint32))
    off = N.absmax_offset(host)
    c2, sc2, want_off = R.double_quantize(host)
    assert off.view(np.uint32) == want_off.view(np.uint32)
    codes, scale2 = ops.adam8_quantize(torch.from_numpy((host - off).astype(np.float32)).cuda(), 0)
    _same(codes, torch.from_numpy(c2), "second-level codes")
    _same(scale2, torch.from_numpy(sc2), "second-level scales")

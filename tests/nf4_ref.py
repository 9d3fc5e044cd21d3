"""numpy definition of the NF4 frozen decoder base (rv_nf4_quantize_bf16, rv_nf4_dequant_bf16; radvlm_amd/csrc/nf4.hip).

Block-wise 4-bit NormalFloat quantisation with optional double quantisation after Dettmers et al., "QLoRA: Efficient Finetuning of
Quantized LLMs", restated here and pinned by this file.  bitsandbytes is not importable where this project is built and tested: nothing
here is compared against its files or its kernels, and its serialised layouts are not read or written.

  table      TABLE below, sixteen fp32 values, ascending, code 0 .. 15 (t[7] = 0, the ends are -1 and 1).
  block      64 consecutive elements of ONE named weight tensor in row-major order, counted from its first element; the last block may
             be short; one fp32 absmax = max |x| per block.
  quantise   s = absmax, or 1 for an all-zero block;  a = fp32(x) / s in IEEE fp32;  mid[i] = fp32((float64(t[i]) + float64(t[i+1])) / 2);
             code = number of midpoints strictly below a.  This midpoint rule is the definition (it is not "nearest level in float64").
  packing    two codes per byte, element 2j in the high nibble, element 2j + 1 in the low one; an odd length leaves the last low nibble 0.
  dequantise bf16_rne(fp32(t[code] * absmax)): one fp32 multiply, one rounding to bf16 (ties to even).
  double quantisation, per tensor:
             offset = fp32(S / nblocks), S the float64 sum of the tensor's absmax values taken LEFT TO RIGHT, block 0 first, one
             float64 addition per block (absmax_offset());  r = fp32(absmax - offset) element by element;  r is quantised by the signed
             dynamic 8-bit scheme of tests/adam8_ref.py (256 values per second-level block, one fp32 scale2 = max |r| each);
             the EFFECTIVE absmax of a block is fp32(fp32(table8[c] * scale2) + offset), and dequantisation uses that value -- double
             quantisation changes the model's weights, by exactly this much.

Non-finite weights are outside the contract.  The committed device table is radvlm_amd/csrc/nf4_codebook.h.
"""
import numpy as np

import adam8_ref

BLOCK = 64
BLOCK2 = adam8_ref.BLOCK
F32 = np.float32

TABLE = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
                  -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                  0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], np.float64).astype(F32)
MID = ((TABLE[:-1].astype(np.float64) + TABLE[1:].astype(np.float64)) / 2.0).astype(F32)


def bf16_bits(x):
    """fp32 -> the uint16 bit patterns of bf16, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x))


def nblocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def codes_of(x):
    """fp32 [n] (bf16-exact or not) -> (codes uint8 [n], one per element, absmax fp32 [nblocks(n)])."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    codes = np.empty(x.size, np.uint8)
    absmax = np.empty(nblocks(x.size), F32)
    for b in range(absmax.size):
        xb = x[b * BLOCK:(b + 1) * BLOCK]
        am = F32(np.max(np.abs(xb)))
        absmax[b] = am
        a = (xb / (am if am != 0 else F32(1.0))).astype(F32)              # IEEE fp32 division
        codes[b * BLOCK:(b + 1) * BLOCK] = np.searchsorted(MID, a, side="left")
    return codes, absmax


def pack(codes):
    """uint8 codes [n] -> bytes [ceil(n / 2)], element 2j high, 2j + 1 low; an odd n leaves the last low nibble 0."""
    c = np.asarray(codes, np.uint8).reshape(-1)
    if c.size & 1:
        c = np.concatenate([c, np.zeros(1, np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)


def unpack(packed, n):
    p = np.asarray(packed, np.uint8).reshape(-1)
    c = np.empty(p.size * 2, np.uint8)
    c[0::2], c[1::2] = p >> 4, p & 15
    return c[:n]


def quantize(x):
    """fp32 [n] -> (packed bytes [ceil(n / 2)], absmax fp32 [nblocks(n)])."""
    codes, absmax = codes_of(x)
    return pack(codes), absmax


def absmax_offset(absmax):
    """fp32(mean) with the float64 sum taken left to right, block 0 first."""
    s = 0.0                                                                 # a Python float is a float64
    for v in np.asarray(absmax, F32).tolist():
        s += v
    return F32(s / len(absmax))


def double_quantize(absmax):
    """absmax fp32 [nb] of ONE tensor -> (codes2 uint8 [nb], scale2 fp32 [ceil(nb / 256)], offset fp32)."""
    absmax = np.asarray(absmax, F32)
    off = absmax_offset(absmax)
    codes2, scale2 = adam8_ref.quantize((absmax - off).astype(F32), adam8_ref.SIGNED)
    return codes2, scale2, off


def effective_absmax(codes2, scale2, off):
    return (adam8_ref.dequantize(codes2, scale2, adam8_ref.SIGNED) + F32(off)).astype(F32)


def dequantize(packed, absmax, n):
    """-> uint16 bf16 bit patterns [n]; absmax is the plain or the effective one."""
    c = unpack(packed, n)
    am = np.repeat(np.asarray(absmax, F32), BLOCK)[:n]
    return bf16_bits((TABLE[c] * am).astype(F32))


def roundtrip(x, double_quant=False):
    """fp32 [n] -> the dequantised weights as fp32 (bf16-exact)."""
    packed, absmax = quantize(x)
    if double_quant:
        absmax = effective_absmax(*double_quantize(absmax))
    return bf16_to_f32(dequantize(packed, absmax, np.asarray(x).size))


LENGTHS = (1, 2, 63, 64, 65, 127, 129, 16385)


def host_inputs():
    """name -> fp32 vector of bf16-exact values: the inputs shared by tests/test_nf4_host.py and tests/test_nf4_kernels_gpu.py."""
    r = np.random.RandomState(11)
    out = {}
    for n in LENGTHS + (64 * 256 + 63,):                                   # the last: a short last second-level block
        out[f"n{n}"] = bf16_round((0.02 * r.randn(n)).astype(F32))
    z = bf16_round((0.02 * r.randn(4 * BLOCK)).astype(F32))
    z[BLOCK:2 * BLOCK] = 0.0                                                # an all-zero block
    z[2 * BLOCK:3 * BLOCK] = 0.0
    z[2 * BLOCK + 17] = F32(-0.375)                                         # a block of one value
    out["zero_and_single"] = z
    e = bf16_round((0.01 * r.randn(4 * BLOCK)).astype(F32))
    e[0], e[BLOCK - 1] = F32(0.5), F32(-0.5)                                # +-max at either end of a block
    e[BLOCK], e[2 * BLOCK - 1] = F32(-0.25), F32(0.25)
    e[3 * BLOCK - 1] = F32(2.0)
    e[3 * BLOCK] = F32(-2.0)
    out["max_at_ends"] = e
    m = np.concatenate([np.nextafter(MID, F32(-np.inf)), MID, np.nextafter(MID, F32(np.inf))])
    m = bf16_round(m[np.abs(m) < 1])                                        # bf16 neighbours of the midpoints, absmax 1 per block
    blocks = [np.concatenate([[F32(1.0)], m[i:i + BLOCK - 1]]) for i in range(0, m.size, BLOCK - 1)]
    out["near_midpoints"] = np.concatenate(blocks).astype(F32)
    return out

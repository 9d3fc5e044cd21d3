"""numpy restatement of the MXFP4 weight quantisation (include/radvlm_hip.h, rv_quantize_rows_mxfp4_bf16): OCP Microscaling FP4, E2M1
elements with one E8M0 power-of-two scale per block of 32 consecutive k, uint32 arithmetic throughout.  For a bf16 row w of K entries,
per block (the last block is shorter when K % 32 != 0; only its existing entries count):

    amax = max |w| over the block
    e    = floor(log2(amax)) - 2      (the fp32 exponent field of amax minus 2; e = 0 for an all-zero block)
    a    = |w| / 2^e                  (exact in fp32)
    code = nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0..7), ties to the EVEN code, a > 6 saturates to code 7
    W^   = sign(w) * value[code] * 2^e   (exactly a bf16 number; a zero result is +0.0: nibble 0, never "-0")
    nibble = sign << 3 | code ;  scale byte = e + 127 (E8M0)

This is the OCP MX v1.0 scale rule (floor, saturating).  bf16 values travel as uint16 bit patterns.  Block maxima outside
[2^-120, 2^120] and non-finite weights are outside the contract."""
import numpy as np

from w8_ref import bf16_bits_to_f32, f32_to_bf16_bits  # noqa: F401  (re-exported: one bf16 rounding restatement for both formats)

VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)
# midpoints between neighbouring values; a tie goes to the even code, so the odd-to-even midpoints are closed from below
_MID = np.array([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], np.float32)
_INCLUSIVE = np.array([False, True, False, True, False, True, False])      # a >= mid counts where the upper code is even


def steps(K):
    return (K + 31) // 32


def quantize_rows(w_bits):
    """w_bits: uint16 [N, K] bf16 bit patterns -> (nibbles uint8 [N, K], scale bytes uint8 [N, steps(K)], W^ uint16 [N, K])."""
    w_bits = np.asarray(w_bits, np.uint16)
    N, K = w_bits.shape
    ks = steps(K)
    full = np.zeros((N, ks * 32), np.uint16)
    full[:, :K] = w_bits
    u = full.astype(np.uint32) << np.uint32(16)
    mag = (u & np.uint32(0x7FFFFFFF)).reshape(N, ks, 32)                    # fp32 bits of |w|: ordered as the values are
    amax = mag.max(axis=2)
    sb = np.where(amax > 0, ((amax >> np.uint32(23)) & np.uint32(0xFF)) - np.uint32(2), np.uint32(127)).astype(np.uint32)
    inv = ((np.uint32(254) - sb) << np.uint32(23)).view(np.float32)         # 2^-e
    a = mag.view(np.float32) * inv[:, :, None]
    code = np.zeros(a.shape, np.uint32)
    for mid, inc in zip(_MID, _INCLUSIVE):
        code += (a >= mid) if inc else (a > mid)
    sign = (u >> np.uint32(31)).reshape(N, ks, 32)
    nib = np.where(code > 0, (sign << np.uint32(3)) | code, np.uint32(0))
    # bf16 bits of value[code] * 2^e: code >= 2 is (exponent, mantissa) = (code >> 1, code & 1) with bias 1; code 1 is 2^(e - 1)
    field = np.where(code == 1, np.uint32(0), code << np.uint32(6)) + ((sb[:, :, None] - np.uint32(1)) << np.uint32(7))
    what = np.where(code > 0, field | (sign << np.uint32(15)), np.uint32(0))
    return (nib.reshape(N, ks * 32)[:, :K].astype(np.uint8), sb.astype(np.uint8),
            what.reshape(N, ks * 32)[:, :K].astype(np.uint16))


def dequantize(nib, sb):
    """fp32 values of (nibbles [N, K], scale bytes [N, steps(K)]) by VALUES[code] * 2^e in floating point (an independent route to W^)."""
    N, K = nib.shape
    e = np.repeat(sb.astype(np.int32) - 127, 32, axis=1)[:, :K]
    v = VALUES[nib & 7] * np.where(nib & 8, np.float32(-1.0), np.float32(1.0))
    return np.ldexp(v, e).astype(np.float32)


def packed_row_bytes(K):
    """Bytes of a packed nibble row: 64 per quad of 32-deep K steps."""
    return (steps(K) + 3) // 4 * 64


def scale_row_bytes(K):
    """Bytes of a scale row: one per K step, padded to whole quads."""
    return (steps(K) + 3) // 4 * 4


def pack_rows(nib, sb):
    """The packed layout the two kernels share: per quad j of 32-deep K steps 64 bytes; lane group g (k = 8 g .. 8 g + 7 of a step) owns
    bytes 16 g .. 16 g + 15: 4 bytes per step u = 0..3 of the quad, weight i of the group in bits 4 i .. 4 i + 3 of that little-endian
    dword (byte i // 2, low nibble for even i).  Padding past K: nibble 0, scale byte 127.  -> (packed uint8, scales uint8)."""
    N, K = nib.shape
    quads = (steps(K) + 3) // 4
    full = np.zeros((N, quads * 128), np.uint8)
    full[:, :K] = nib
    b = full[:, 0::2] | (full[:, 1::2] << 4)                                # [N, quads * 64]: byte = k // 2 within the row
    packed = np.ascontiguousarray(b.reshape(N, quads, 4, 4, 4).transpose(0, 1, 3, 2, 4)).reshape(N, quads * 64)   # (u, g, byte) -> (g, u, byte)
    scales = np.full((N, quads * 4), 127, np.uint8)
    scales[:, :steps(K)] = sb
    return packed, scales


def unpack_rows(packed, scales, K):
    N, ldp = packed.shape
    quads = ldp // 64
    b = np.ascontiguousarray(packed.reshape(N, quads, 4, 4, 4).transpose(0, 1, 3, 2, 4)).reshape(N, quads * 64)
    nib = np.empty((N, quads * 128), np.uint8)
    nib[:, 0::2] = b & 15
    nib[:, 1::2] = b >> 4
    return nib[:, :K], scales[:, :steps(K)]

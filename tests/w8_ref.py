"""numpy restatement of the row-wise int8 weight quantisation (include/radvlm_hip.h, rv_quantize_rows_w8_bf16), fp32 throughout and
uint32 arithmetic for the bf16 rounding.  For a bf16 row w of K entries:

    amax = max |w|
    s    = amax / 127                                (IEEE fp32 division; s = 1 for an all-zero row)
    q    = clamp(rint(float(w) / s), -127, 127)      (IEEE division, round half to even)
    W^   = bf16_rne(float(q) * s)                    (one fp32 multiply, one round-to-nearest-even to bf16)

bf16 values travel as uint16 bit patterns.  Non-finite weights are outside the contract."""
import numpy as np


def bf16_bits_to_f32(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(x):
    """Round-to-nearest-even of finite fp32 values to bf16, as bit patterns (uint16)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    return (r >> np.uint32(16)).astype(np.uint16)


def quantize_rows(w_bits):
    """w_bits: uint16 [N, K] bf16 bit patterns -> (q int8 [N, K], s fp32 [N], W^ uint16 [N, K])."""
    w = bf16_bits_to_f32(w_bits)
    amax = np.abs(w).max(axis=1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(amax > 0, amax / np.float32(127.0), np.float32(1.0)).astype(np.float32)
        q = np.clip(np.rint(w / s[:, None]), np.float32(-127.0), np.float32(127.0)).astype(np.float32)
    what = f32_to_bf16_bits(q * s[:, None])
    return q.astype(np.int8), s, what


def packed_row_bytes(K):
    """Bytes of a packed row: 64 per pair of 32-deep K steps."""
    return ((K + 31) // 32 + 1) // 2 * 64


def pack_rows(q):
    """The packed layout the two kernels share: per pair j of 32-deep K steps 64 bytes, lane group g (k = 8 g .. 8 g + 7 of a step) owns
    bytes 16 g .. 16 g + 15: its 8 weights of step 2 j, then its 8 of step 2 j + 1.  Zero padding past K."""
    N, K = q.shape
    ks = (K + 31) // 32
    pairs = (ks + 1) // 2
    full = np.zeros((N, pairs * 64), np.int8)
    full[:, :K] = q
    return np.ascontiguousarray(full.reshape(N, pairs, 2, 4, 8).transpose(0, 1, 3, 2, 4)).reshape(N, pairs * 64)


def unpack_rows(packed, K):
    N, ldp = packed.shape
    pairs = ldp // 64
    return np.ascontiguousarray(packed.reshape(N, pairs, 4, 2, 8).transpose(0, 1, 3, 2, 4)).reshape(N, pairs * 64)[:, :K]

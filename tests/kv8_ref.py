"""numpy restatement of the int8 KV cache quantisation (include/radvlm_hip.h, rv_kv_quantize_rows_bf16): the rule of tests/w8_ref.py
applied per group, a group being the hd values of one kv head of K, or of V, at one cached position.  A K|V row holds 2 * Hkv groups:
K of kv head g at columns g * hd, V at Hkv * hd + g * hd.  bf16 values travel as uint16 bit patterns."""
import numpy as np

import w8_ref


def quantize_kv_rows(kv_bits, Hkv, hd):
    """kv_bits: uint16 [M, 2 * Hkv * hd] bf16 bit patterns of M K|V rows -> (q int8 [M, 2 * Hkv * hd] in the same columns,
    s fp32 [M, 2 * Hkv] with column g the scale of K head g and column Hkv + g that of V head g, x^ uint16 [M, 2 * Hkv * hd])."""
    kv_bits = np.asarray(kv_bits)
    M, width = kv_bits.shape
    assert width == 2 * Hkv * hd
    q, s, xhat = w8_ref.quantize_rows(kv_bits.reshape(M * 2 * Hkv, hd))
    return q.reshape(M, width), s.reshape(M, 2 * Hkv), xhat.reshape(M, width)

"""Thin typed wrappers over the C ABI (radvlm_amd.lib): shape checks on the host, then one kernel launch.

Names follow the reference's operators.  No op here has a torch fallback.
"""
import math

import numpy as np
import torch

from . import lib
from .lib import ACT_GELU, ACT_GELU_TANH, ACT_NONE, ACT_QUICK_GELU  # noqa: F401

BF16 = torch.bfloat16


def _chk(t, dtype=BF16):
    assert t.is_cuda and t.dtype == dtype, (t.device, t.dtype)
    return t


def round_up(x, m):
    return (x + m - 1) // m * m


_WS = {}


def default_workspace(device):
    """128 MiB fp32 scratch per device for the GEMM's split-K / tail-split modes (stream-ordered reuse)."""
    key = (device.type, device.index)
    if key not in _WS:
        _WS[key] = torch.empty(32 << 20, dtype=torch.float32, device=device)
    return _WS[key]


def gemm_nt(a, b, out=None, bias=None, residual=None, act=ACT_NONE, out_dtype=BF16):
    """out[M,N] = act(a[M,K] @ b[N,K]^T + bias) + residual.  a, b: 2-D bf16 views with unit inner stride."""
    return gemm(a, b, out=out, bias=bias, residual=residual, act=act, out_dtype=out_dtype)


def _gemm_nt_direct(a, b, out=None, bias=None, residual=None, act=ACT_NONE, out_dtype=BF16):
    """rv_gemm_nt_bf16 entry point (no scratch: plain tiles only); kept for ABI coverage in the tests."""
    _chk(a), _chk(b)
    M, K = a.shape
    N, K2 = b.shape
    assert K == K2 and a.stride(1) == 1 and b.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype in (BF16, torch.float32)
    if bias is not None:
        _chk(bias)
        assert bias.numel() == N and bias.is_contiguous()
    res_f32 = 0
    ldr = 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
        res_f32 = int(residual.dtype == torch.float32)
        ldr = residual.stride(0)
    lib.call("rv_gemm_nt_bf16", a, a.stride(0), b, b.stride(0), out, out.stride(0), bias, residual, ldr, M, N, K, act,
             int(out.dtype == torch.float32), res_f32, lib.zeros16(a.device))
    return out


def gemm(a, b, ta=False, tb=False, out=None, bias=None, residual=None, act=ACT_NONE, out_dtype=BF16, alpha=1.0, a2=None, b2=None,
         workspace=None):
    """out[M,N] = act(op(a) @ op(b)^T + bias) + residual with a stored [K,M] if ta else [M,K], b stored [K,N] if tb else [N,K]."""
    _chk(a), _chk(b)
    assert a.stride(1) == 1 and b.stride(1) == 1
    (K, M) = a.shape if ta else a.shape[::-1]
    (K2, N) = b.shape if tb else b.shape[::-1]
    assert K == K2, (a.shape, b.shape, ta, tb)
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype in (BF16, torch.float32)
    res_f32, ldr = 0, 0
    if residual is not None:
        assert residual.shape == (M, N) and residual.stride(1) == 1
        res_f32, ldr = int(residual.dtype == torch.float32), residual.stride(0)
    if bias is not None:
        assert bias.numel() == N and bias.is_contiguous()
    if workspace is None:
        workspace = default_workspace(a.device)
    # fused second operand pair (a2 like a, b2 like b, contraction K2) and/or split-K scratch
    K2 = 0
    if a2 is not None:
        _chk(a2), _chk(b2)
        assert a2.stride(1) == 1 and b2.stride(1) == 1
        (K2, M2) = a2.shape if ta else a2.shape[::-1]
        (K2b, N2) = b2.shape if tb else b2.shape[::-1]
        assert M2 == M and N2 == N and K2 == K2b
    ws_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    lib.call("rv_gemm_bf16_ex", a, a.stride(0), b, b.stride(0), out, out.stride(0), bias, residual, ldr, M, N, K, int(ta), int(tb),
             float(alpha), act, int(out.dtype == torch.float32), res_f32, a2, a2.stride(0) if a2 is not None else 0, b2,
             b2.stride(0) if b2 is not None else 0, K2, workspace, ws_bytes, lib.zeros16(a.device))
    return out


def gemm_rope(a, b, cos_sin, S, rope_heads, hd, bias=None, positions=None, out=None):
    """out[M,N] = rope(a[M,K] @ b[N,K]^T + bias): rotary embedding applied to the first rope_heads heads (q then k) in the epilogue."""
    _chk(a), _chk(b)
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and a.stride(1) == 1 and b.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=a.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype == BF16
    ws = default_workspace(a.device)
    lib.call("rv_gemm_rope_bf16", a, a.stride(0), b, b.stride(0), out, out.stride(0), bias, M, N, K, cos_sin, positions, S, rope_heads, hd,
             ws, ws.numel() * ws.element_size(), lib.zeros16(a.device))
    return out


def gemm_swiglu_fwd(a, wgu, F, gu=None, act=None):
    """(gu [M,2F], act [M,F]) = (a @ wgu^T, silu(gate) * up) in one launch; wgu = stacked [gate; up] rows [2F, K]."""
    _chk(a), _chk(wgu)
    M, K = a.shape
    assert wgu.shape == (2 * F, K) and a.stride(1) == 1 and wgu.stride(1) == 1
    gu = torch.empty(M, 2 * F, dtype=BF16, device=a.device) if gu is None else gu
    act = torch.empty(M, F, dtype=BF16, device=a.device) if act is None else act
    ws = default_workspace(a.device)
    lib.call("rv_gemm_swiglu_fwd_bf16", a, a.stride(0), wgu, wgu.stride(0), gu, gu.stride(0), act, act.stride(0), M, F, K,
             ws, ws.numel() * ws.element_size(), lib.zeros16(a.device))
    return gu, act


def gemm_swiglu_bwd(dy, wd, gu, F, dgu=None):
    """dgu [M,2F] = swiglu'(gu) * (dy [M,d] @ wd [d,F]): down_proj's input gradient with the activation backward in the epilogue."""
    _chk(dy), _chk(wd), _chk(gu)
    M, K = dy.shape
    assert wd.shape == (K, F) and gu.shape == (M, 2 * F) and dy.stride(1) == 1 and wd.stride(1) == 1 and gu.stride(1) == 1
    dgu = torch.empty_like(gu) if dgu is None else dgu
    ws = default_workspace(dy.device)
    # d(act) as a tensor exists only in the unfused fallback (small shapes): allocate it there, not for the 7B step
    small = M * F <= (1 << 24)
    scratch = torch.empty(M, F, dtype=BF16, device=dy.device) if small else None
    try:
        lib.call("rv_gemm_swiglu_bwd_bf16", dy, dy.stride(0), wd, wd.stride(0), gu, gu.stride(0), dgu, dgu.stride(0), scratch,
                 F if small else 0, M, F, K, ws, ws.numel() * ws.element_size(), lib.zeros16(dy.device))
    except lib.RadvlmHipError:
        if small:
            raise
        scratch = torch.empty(M, F, dtype=BF16, device=dy.device)     # a large shape that still took the fallback (forced kernel choice)
        lib.call("rv_gemm_swiglu_bwd_bf16", dy, dy.stride(0), wd, wd.stride(0), gu, gu.stride(0), dgu, dgu.stride(0), scratch, F, M, F, K,
                 ws, ws.numel() * ws.element_size(), lib.zeros16(dy.device))
    return dgu


def transpose(x, r_pad=None, out=None):
    """x [R,C] (unit inner stride) -> [C, r_pad] with zero padding."""
    _chk(x)
    R, C = x.shape
    r_pad = r_pad or round_up(R, 8)
    if out is None:
        out = torch.empty(C, r_pad, dtype=BF16, device=x.device)
    assert out.shape == (C, r_pad) and out.stride(1) == 1 and x.stride(1) == 1
    lib.call("rv_transpose_bf16", x, x.stride(0), 0, 0, out, out.stride(0), 0, 0, R, C, r_pad, 1, 1, 0)
    return out


def transpose_heads(x, B, S, H, hd, s_pad, out=None, perm32=True, cu=None):
    """x: token-major view [(b*S+s), H*hd] (row stride ld) -> [B,H,hd,s_pad] (zero padded along s).
    perm32 (what the attention kernels expect): the sequence axis is stored in MFMA contraction order per group of 32.
    cu (int32 [B+1], packed batches): sample b owns rows [cu[b], cu[b+1]) of x; S = the longest sample."""
    _chk(x)
    assert x.shape[1] == H * hd and x.stride(1) == 1 and (cu is not None or x.shape[0] == B * S)
    if out is None:
        out = torch.empty(B, H, hd, s_pad, dtype=BF16, device=x.device)
    ld = x.stride(0)
    if cu is not None:
        lib.call("rv_transpose_bf16_varlen", x, ld, cu, hd, out, s_pad, H * hd * s_pad, hd * s_pad, S, hd, s_pad, B, H, int(perm32))
    else:
        lib.call("rv_transpose_bf16", x, ld, S * ld, hd, out, s_pad, H * hd * s_pad, hd * s_pad, S, hd, s_pad, B, H, int(perm32))
    return out


def rmsnorm_fwd(x, w, eps=1e-5, y=None, rstd=None):
    _chk(x), _chk(w)
    rows, d = x.shape
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if rstd is None else rstd
    lib.call("rv_rmsnorm_fwd", x, w, y, rstd, rows, d, eps)
    return y, rstd


def rmsnorm_bwd(dy, x, w, rstd, dx=None, dx_add=False, dw=None, dw_accumulate=False):
    rows, d = x.shape
    assert dy.is_contiguous() and x.is_contiguous()
    nblk = min(rows, 1024)
    part = torch.empty(nblk, d, dtype=torch.float32, device=x.device)
    if dx is None:
        dx = torch.empty_like(x)
        dx_add = False
    lib.call("rv_rmsnorm_bwd", dy, x, w, rstd, dx, int(dx_add), part, nblk, rows, d)
    if dw is None:
        dw = torch.empty(d, dtype=BF16, device=x.device)
        dw_accumulate = False
    lib.call("rv_colsum_f32", part, nblk, d, dw, int(dw_accumulate))
    return dx, dw


def layernorm_fwd(x, w, b, eps=1e-5, y=None, save_stats=False):
    rows, d = x.shape
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if save_stats else None
    lib.call("rv_layernorm_fwd", x, w, b, y, stats, rows, d, eps)
    return (y, stats) if save_stats else y


def layernorm_bwd(dy, x, w, stats, dw, db, dx=None, dx_add=False, accumulate=False):
    """dx (+)= LN'(dy); dw/db (bf16 [d] views) (+)= parameter gradients."""
    rows, d = x.shape
    assert dy.is_contiguous() and x.is_contiguous()
    nblk = min(rows, 512)
    part = torch.empty(nblk, 2 * d, dtype=torch.float32, device=x.device)
    if dx is None:
        dx = torch.empty_like(x)
        dx_add = False
    lib.call("rv_layernorm_bwd", dy, x, w, stats, dx, int(dx_add), part, nblk, rows, d)
    wb = torch.empty(2 * d, dtype=BF16, device=x.device)
    lib.call("rv_colsum_f32", part, nblk, 2 * d, wb, 0)
    if accumulate:
        lib.call("rv_add_bf16", dw, wb[:d], dw, d)
        lib.call("rv_add_bf16", db, wb[d:], db, d)
    else:
        dw.copy_(wb[:d])
        db.copy_(wb[d:])
    return dx


def quick_gelu_fwd(x, y=None):
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    lib.call("rv_quick_gelu_fwd", x, y, x.numel())
    return y


def quick_gelu_bwd(dy, x, dx=None):
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x) if dx is None else dx
    lib.call("rv_quick_gelu_bwd", dy, x, dx, x.numel())
    return dx


def gelu_tanh_fwd(x, y=None):
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    lib.call("rv_gelu_tanh_fwd", x, y, x.numel())
    return y


def gelu_tanh_bwd(dy, x, dx=None):
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x) if dx is None else dx
    lib.call("rv_gelu_tanh_bwd", dy, x, dx, x.numel())
    return dx


def bias_grad(dy, out=None, accumulate=False):
    """db[c] = sum_r dy[r, c]."""
    rows, cols = dy.shape
    nblk = min(rows, 256)
    part = torch.empty(nblk, cols, dtype=torch.float32, device=dy.device)
    lib.call("rv_colsum_partial_bf16", dy, dy.stride(0), rows, cols, part, nblk)
    if out is None:
        out = torch.empty(cols, dtype=BF16, device=dy.device)
        accumulate = False
    lib.call("rv_colsum_f32", part, nblk, cols, out, int(accumulate))
    return out


def rope_table(S, hd, theta=10000.0, device="cuda", round_bf16=True):
    """fp32 [S, hd/2, 2] (cos, sin); computed like LlamaRotaryEmbedding.forward (modeling_llama.py:123-139):
    fp32 trig, then rounded through bf16 like the reference's ``.to(dtype=x.dtype)``."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    fr = torch.outer(torch.arange(S, dtype=torch.float32), inv)
    cs = torch.stack((fr.cos(), fr.sin()), dim=-1)
    if round_bf16:
        cs = cs.to(BF16).float()
    return cs.contiguous().to(device)


def rope_inplace(x, cos_sin, S, heads, hd, nsec, direction=1, positions=None):
    """positions (int32 [rows], packed batches): explicit position of every token row; default row % S."""
    rows = x.shape[0]
    if positions is not None:
        lib.call("rv_rope_inplace_pos", x, x.stride(0), cos_sin, positions, rows, heads, hd, nsec, direction)
    else:
        lib.call("rv_rope_inplace", x, x.stride(0), cos_sin, rows, S, heads, hd, nsec, direction)
    return x


def attn_fwd(q, k, vT, B, S, H, hd, s_pad, causal, lens=None, scale=None, out=None, lse=None, kv_heads=None, cu=None, v=None):
    """q, k: token-major [(B*S), H*hd] / [(B*S), kv_heads*hd] views; vT [B,kv_heads,hd,s_pad], or (head_dim 128) v = the
    token-major value view like k with vT=None: no transposed copy.  Returns (out [(B*S), H*hd], lse fp32 [B,H,s_pad])."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    Hkv = kv_heads or H
    if out is None:
        out = torch.empty(q.shape[0], H * hd, dtype=BF16, device=q.device)
    if lse is None:
        lse = torch.zeros(B, H, s_pad, dtype=torch.float32, device=q.device)
    if v is not None:
        assert vT is None and hd == 128
        lib.call("rv_attn_fwd_nat", q, q.stride(0), k, k.stride(0), v, v.stride(0), out, out.stride(0), lse, lens, cu, B, H, Hkv, S, s_pad, hd,
                 int(causal), scale, lib.zeros16(q.device))
        return out, lse
    lib.call("rv_attn_fwd_gqa", q, q.stride(0), k, k.stride(0), vT, out, out.stride(0), lse, lens, cu, B, H, Hkv, S, s_pad, hd,
             int(causal), scale, lib.zeros16(q.device))
    return out, lse


def attn_bwd(q, k, v, o, dout, lse, B, S, H, hd, s_pad, causal, lens=None, scale=None, dq=None, dk=None, dv=None,
             kv_heads=None, use_workspace=True, cu=None, rope=None, natural=True, delta=None):
    """rope = (cos_sin table, positions or None): dq / dk are returned as gradients of the un-rotated q / k (the rotary embedding's
    adjoint runs in the epilogues)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    dev = q.device
    Hkv = kv_heads or H
    rows = q.shape[0]                       # B*S, or the packed row count cu[B]
    if hd == 128 and natural:
        delta = torch.zeros(B, H, s_pad, dtype=torch.float32, device=dev) if delta is None else delta
        dq = torch.empty(rows, H * hd, dtype=BF16, device=dev) if dq is None else dq
        dk = torch.empty(rows, Hkv * hd, dtype=BF16, device=dev) if dk is None else dk
        dv = torch.empty(rows, Hkv * hd, dtype=BF16, device=dev) if dv is None else dv
        ws = torch.empty(2 * rows * H * hd, dtype=BF16, device=dev) if (Hkv != H and use_workspace) else None
        lib.call("rv_attn_bwd_nat", q, q.stride(0), k, k.stride(0), v, v.stride(0), o, o.stride(0), dout, dout.stride(0), lse, delta,
                 dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0), lens, cu, rows if cu is not None else 0, B, H, Hkv, S, s_pad, hd,
                 int(causal), scale, ws, ws.numel() * ws.element_size() if ws is not None else 0,
                 rope[0] if rope else None, rope[1] if rope else None, lib.zeros16(dev))
        return dq, dk, dv
    qT = transpose_heads(q, B, S, H, hd, s_pad, cu=cu)
    kT = transpose_heads(k, B, S, Hkv, hd, s_pad, cu=cu)
    doT = transpose_heads(dout, B, S, H, hd, s_pad, cu=cu)
    delta = torch.zeros(B, H, s_pad, dtype=torch.float32, device=dev) if delta is None else delta
    dq = torch.empty(rows, H * hd, dtype=BF16, device=dev) if dq is None else dq
    dk = torch.empty(rows, Hkv * hd, dtype=BF16, device=dev) if dk is None else dk
    dv = torch.empty(rows, Hkv * hd, dtype=BF16, device=dev) if dv is None else dv
    # per-query-head dK/dV partials for the small-grid grouped-query case (the C side decides whether to use it)
    ws = torch.empty(2 * rows * H * hd, dtype=BF16, device=dev) if (Hkv != H and use_workspace) else None
    lib.call("rv_attn_bwd_gqa_rope", q, q.stride(0), k, k.stride(0), v, v.stride(0), o, o.stride(0), dout, dout.stride(0), qT, kT, doT,
             lse, delta, dq, dq.stride(0), dk, dk.stride(0), dv, dv.stride(0), lens, cu, rows if cu is not None else 0, B, H, Hkv, S,
             s_pad, hd, int(causal), scale,
             ws, ws.numel() * ws.element_size() if ws is not None else 0, rope[0] if rope else None, rope[1] if rope else None, lib.zeros16(dev))
    return dq, dk, dv


def swiglu_fwd(gu, F, act=None):
    rows = gu.shape[0]
    if act is None:
        act = torch.empty(rows, F, dtype=BF16, device=gu.device)
    lib.call("rv_swiglu_fwd", gu, gu.stride(0), act, act.stride(0), rows, F)
    return act


def swiglu_bwd(dact, gu, F, dgu=None):
    rows = gu.shape[0]
    dgu = torch.empty_like(gu) if dgu is None else dgu
    lib.call("rv_swiglu_bwd", dact, dact.stride(0), gu, gu.stride(0), dgu, dgu.stride(0), rows, F)
    return dgu


def dropout(x, p, seed, y=None):
    """Inverted dropout with a regenerable counter-based mask (same (p, seed) in backward)."""
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    lib.call("rv_dropout_bf16", x, y, x.numel(), float(p), int(seed))
    return y


def lora_down(x, a, alpha, p, seed, out=None):
    """t[M, r] = alpha * dropout_p(x) @ a^T with the mask of dropout(x, p, seed), in one pass over x (x contiguous [M, K], K % 64 == 0,
    r <= 64); other shapes take the two-launch sequence."""
    M, K = x.shape
    r = a.shape[0]
    # rv_lora_down_bf16 takes 16-byte vector accesses: base pointers 16-byte aligned, adapter rows a multiple of 8 elements apart
    if not ((x.is_contiguous() or (p <= 0 and x.stride(1) == 1 and x.stride(0) % 8 == 0)) and K % 64 == 0 and r <= 64 and r % 4 == 0 and a.stride(1) == 1
            and x.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0 and a.stride(0) % 8 == 0):
        return gemm(dropout(x.contiguous(), p, seed) if p > 0 else x, a, alpha=alpha, out=out)
    if out is None:
        out = torch.empty(M, r, dtype=BF16, device=x.device)
    lib.call("rv_lora_down_bf16", x, x.stride(0), a, a.stride(0), out, out.stride(0), M, r, K, float(alpha), float(p), int(seed), lib.zeros16(x.device))
    return out


def lora_a_grad(dt, x, ga, p, seed, accumulate, workspace):
    """ga[r, K] (+)= dt[M, r]^T @ dropout(x, p, seed)[M, K] in one pass over x, the mask re-created in registers (rv_lora_a_grad_bf16: x contiguous,
    r <= 64, r % 8 == 0, K % 8 == 0); other shapes take the two-launch sequence (dropout kernel, split-K weight-gradient GEMM)."""
    M, K = x.shape
    r = dt.shape[1]
    ok = (x.is_contiguous() and dt.stride(1) == 1 and dt.stride(0) % 8 == 0 and ga.stride(1) == 1 and r <= 64 and r % 8 == 0 and K % 8 == 0
          and x.data_ptr() % 16 == 0 and dt.data_ptr() % 16 == 0 and workspace is not None and workspace.numel() * workspace.element_size() >= r * K * 4)
    if not ok:
        return gemm(dt, dropout(x.contiguous(), p, seed) if p > 0 else x, ta=True, tb=True, out=ga, residual=ga if accumulate else None, workspace=workspace)
    lib.call("rv_lora_a_grad_bf16", dt, dt.stride(0), x, x.stride(0), ga, ga.stride(0), M, r, K, float(p), int(seed), int(bool(accumulate)),
             workspace, workspace.numel() * workspace.element_size())
    return ga


def gemm_dropout_add(a, b, y, p, seed, tb=True, alpha=1.0, accumulate=True):
    """y (+)= dropout(alpha * a @ op(b)) with the mask of dropout(., p, seed) over y's elements, applied in the GEMM epilogue (the product is
    never stored unmasked).  a [M, K], b [K, N] (tb) or [N, K]; y [M, N] contiguous rows."""
    _chk(a), _chk(b), _chk(y)
    M, K = a.shape
    N = b.shape[1] if tb else b.shape[0]
    assert y.shape == (M, N) and (b.shape[0] if tb else b.shape[1]) == K and a.stride(1) == 1 and b.stride(1) == 1 and y.stride(1) == 1
    if p <= 0 or N % 8 or y.stride(0) != N or y.data_ptr() % 16:       # the mask indexes y as M * N contiguous elements, 16-byte accesses
        t = gemm(a, b, tb=tb, alpha=alpha)
        return dropout_add(t, y, p, seed) if p > 0 else y.add_(t) if accumulate else y.copy_(t)
    lib.call("rv_gemm_dropout_add_bf16", a, a.stride(0), b, b.stride(0), y, y.stride(0), M, N, K, int(tb), float(alpha), float(p), int(seed),
             int(accumulate), lib.zeros16(a.device))
    return y


def dropout_add(x, y, p, seed):
    """y += dropout(x) (same regenerable mask as dropout(x, p, seed)), one pass."""
    assert x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    lib.call("rv_dropout_add_bf16", x, y, x.numel(), float(p), int(seed))
    return y


def gelu_fwd(x, y=None):
    assert x.is_contiguous()
    y = torch.empty_like(x) if y is None else y
    lib.call("rv_gelu_fwd", x, y, x.numel())
    return y


def gelu_bwd(dy, x, dx=None):
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x) if dx is None else dx
    lib.call("rv_gelu_bwd", dy, x, dx, x.numel())
    return dx


def cross_entropy(logits, labels_shifted, V, inv_count, grad_inplace=True):
    """Returns (loss scalar fp32 tensor [1], loss_rows). If grad_inplace, logits are overwritten by dlogits."""
    rows = logits.shape[0]
    loss_rows = torch.empty(rows, dtype=torch.float32, device=logits.device)
    dl = logits if grad_inplace else None
    lib.call("rv_cross_entropy", logits, logits.stride(0), labels_shifted, loss_rows, dl, logits.stride(0) if grad_inplace else 0,
             rows, V, inv_count)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    lib.call("rv_sum_f32", loss_rows, rows, inv_count, loss)
    return loss, loss_rows


POLICY_STATS = ("logp", "loss", "wloss", "kl", "clip")       # the planes of rv_policy_loss_bf16's stats buffer, in order


def policy_loss(logits, labels_shifted, V, adv, weight, gscale=1.0, old_logp=None, ref_logp=None, eps_low=0.2, eps_high=0.2, beta=0.0,
                dlogits="inplace"):
    """The GRPO token loss on bf16 logits rows (rv_policy_loss_bf16).  adv, weight: per-row host or device floats; the loss value is
    weighted by fp32(weight), the gradient by fp32(weight * gscale) formed in double -- the engine's `inv * gscale` convention.
    dlogits: "inplace" (the logits buffer is overwritten), a bf16 buffer, or None (statistics only).
    Returns (loss fp32 [1] = sum of weight * loss, stats fp32 [5, rows] in POLICY_STATS order)."""
    _chk(logits)
    rows, dev = logits.shape[0], logits.device
    f32 = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous()
    w64 = torch.as_tensor(weight).detach().to("cpu", torch.float64)
    assert w64.numel() == rows and labels_shifted.numel() == rows and labels_shifted.dtype == torch.int64
    adv, old_logp, ref_logp = f32(adv), f32(old_logp), f32(ref_logp)
    assert adv.numel() == rows and all(t is None or t.numel() == rows for t in (old_logp, ref_logp))
    lweight, gweight = f32(w64.to(torch.float32)), f32((w64 * float(gscale)).to(torch.float32))
    dl = logits if isinstance(dlogits, str) else dlogits
    assert not isinstance(dlogits, str) or dlogits == "inplace"
    stats = torch.empty(len(POLICY_STATS), rows, dtype=torch.float32, device=dev)
    lib.call("rv_policy_loss_bf16", logits, logits.stride(0), labels_shifted, adv, lweight, gweight, old_logp, ref_logp, float(eps_low),
             float(eps_high), float(beta), stats, dl, dl.stride(0) if dl is not None else 0, rows, V)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lib.call("rv_sum_f32", stats[2], rows, 1.0, loss)
    return loss, stats


DISTILL_STATS = ("jsd", "wloss", "kl_teacher", "kl_student")       # the planes of rv_distill_loss_bf16's stats buffer, in order


def distill_loss(logits, teacher, labels_shifted, V, weight, gscale=1.0, beta=0.5, temperature=1.0, teacher_row=None, dlogits="inplace"):
    """The generalised JSD between bf16 student rows `logits` and bf16 teacher rows `teacher` (rv_distill_loss_bf16; beta 0 / 1: forward /
    reverse KL).  labels_shifted only marks the scored rows (a label outside [0, V): ignored).  weight: per-row host or device floats;
    the loss value is weighted by fp32(weight), the gradient by fp32(weight * gscale) formed in double -- policy_loss's convention.
    teacher_row: int32 [rows] student row -> teacher row (-1: none) or None (row r <-> row r).
    dlogits: "inplace" (the logits buffer is overwritten), a bf16 buffer, or None (statistics only).
    Returns (loss fp32 [1] = sum of weight * jsd, stats fp32 [4, rows] in DISTILL_STATS order)."""
    _chk(logits), _chk(teacher)
    rows, dev = logits.shape[0], logits.device
    w64 = torch.as_tensor(weight).detach().to("cpu", torch.float64)
    assert w64.numel() == rows and labels_shifted.numel() == rows and labels_shifted.dtype == torch.int64
    assert teacher_row is None or (teacher_row.dtype == torch.int32 and teacher_row.numel() == rows)
    assert teacher_row is not None or teacher.shape[0] >= rows          # the map's entries are the caller's to keep inside the teacher
    lweight, gweight = w64.to(torch.float32).to(dev).contiguous(), (w64 * float(gscale)).to(torch.float32).to(dev).contiguous()
    dl = logits if isinstance(dlogits, str) else dlogits
    assert not isinstance(dlogits, str) or dlogits == "inplace"
    stats = torch.empty(len(DISTILL_STATS), rows, dtype=torch.float32, device=dev)
    lib.call("rv_distill_loss_bf16", logits, logits.stride(0), teacher, teacher.stride(0), teacher_row, labels_shifted, lweight, gweight,
             float(beta), float(temperature), stats, dl, dl.stride(0) if dl is not None else 0, rows, V)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lib.call("rv_sum_f32", stats[1], rows, 1.0, loss)
    return loss, stats


def seq_logp_sums(logp, seg_off, row_idx=None):
    """fp64 [B] sums of the scored tokens' log-probs of every sequence, in the fixed order include/radvlm_hip.h documents
    (rv_seq_logp_sums_f64).  logp fp32 rows; seg_off int32 [B + 1] in scored order; row_idx int32 (scored token -> row) or None."""
    assert logp.dtype == torch.float32 and logp.is_contiguous() and seg_off.dtype == torch.int32
    assert row_idx is None or row_idx.dtype == torch.int32
    B = seg_off.numel() - 1
    sums = torch.empty(B, dtype=torch.float64, device=logp.device)
    lib.call("rv_seq_logp_sums_f64", logp, seg_off, row_idx, sums, B, logp.numel())
    return sums


DPO_PLANES = ("pi_chosen", "pi_rejected", "h", "loss", "reward_chosen", "reward_rejected", "sum_chosen")     # rv_dpo_pairs_f64's planes, in order
DPO_BATCH = ("loss", "dpo_loss", "sft_loss")
DPO_LOSS_TYPES = ("sigmoid", "hinge", "ipo")


def dpo_pairs(logp, seg_off, row_idx, rho, loss_type, beta, label_smoothing, alpha_over_P, gamma_over_Nc, coef):
    """The pairwise DPO terms and the per-token gradient coefficients (rv_dpo_pairs_f64).  seg_off int32 [2P + 1]; rho fp64 [2P] or
    None; coef fp32 [rows], written at the scored rows only.  Returns (planes fp64 [7, P] in DPO_PLANES order, batch fp64 [3])."""
    assert logp.dtype == torch.float32 and logp.is_contiguous() and coef.dtype == torch.float32 and coef.numel() == logp.numel()
    assert seg_off.dtype == torch.int32 and seg_off.numel() % 2 == 1 and (row_idx is None or row_idx.dtype == torch.int32)
    P = (seg_off.numel() - 1) // 2
    assert rho is None or (rho.dtype == torch.float64 and rho.numel() == 2 * P)
    planes = torch.empty(len(DPO_PLANES), P, dtype=torch.float64, device=logp.device)
    batch = torch.empty(len(DPO_BATCH), dtype=torch.float64, device=logp.device)
    lib.call("rv_dpo_pairs_f64", logp, seg_off, row_idx, rho, P, DPO_LOSS_TYPES.index(loss_type), float(beta), float(label_smoothing),
             float(alpha_over_P), float(gamma_over_Nc), planes, batch, coef, logp.numel())
    return planes, batch


GSPO_PLANES = ("logratio", "ratio", "loss", "clip", "wkl")      # rv_gspo_seqs_f64's planes, in order
GSPO_BATCH = ("loss", "kl_loss")


def gspo_seqs(logp, seg_off, row_idx, adv_seq, lweight, gweight, old_logp, ref_logp, eps_low, eps_high, beta, coef, kl):
    """GRPO's sequence-level clipped ratio and the per-token gradient coefficients (rv_gspo_seqs_f64).  logp, lweight, gweight, old_logp
    (or None), ref_logp (None unless beta > 0): fp32 [rows]; seg_off int32 [B + 1]; row_idx int32 or None; adv_seq fp32 [B]; coef and kl
    fp32 [rows], written at the scored rows only.  Returns (planes fp64 [5, B] in GSPO_PLANES order, batch fp64 [2] in GSPO_BATCH order)."""
    rows = logp.numel()
    for t in (logp, adv_seq, lweight, gweight, coef, kl, old_logp, ref_logp):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert all(t is None or t.numel() == rows for t in (lweight, gweight, coef, kl, old_logp, ref_logp))
    assert seg_off.dtype == torch.int32 and (row_idx is None or row_idx.dtype == torch.int32)
    B = seg_off.numel() - 1
    assert adv_seq.numel() == B
    planes = torch.empty(len(GSPO_PLANES), B, dtype=torch.float64, device=logp.device)
    batch = torch.empty(len(GSPO_BATCH), dtype=torch.float64, device=logp.device)
    lib.call("rv_gspo_seqs_f64", logp, seg_off, row_idx, adv_seq, lweight, gweight, old_logp, ref_logp, float(eps_low), float(eps_high),
             float(beta), planes, batch, coef, kl, B, rows)
    return planes, batch


def gather_rows(idx, d, table_a, table_b=None, out=None):
    rows = idx.numel()
    assert idx.dtype == torch.int32
    if out is None:
        out = torch.empty(rows, d, dtype=BF16, device=idx.device)
    lib.call("rv_gather_rows", out, out.stride(0), table_a, table_a.stride(0) if table_a is not None else 0, table_b,
             table_b.stride(0) if table_b is not None else 0, idx, rows, d)
    return out


def segment_sum_rows(src, seg_off, pos, out_row, out):
    nseg = out_row.numel()
    if nseg == 0:
        return out
    lib.call("rv_segment_sum_rows", src, src.stride(0), seg_off, pos, out_row, nseg, out, out.stride(0), src.shape[1])
    return out


def weighted_segment_sum_rows(src, seg_off, pos, w, out_row, out):
    """out[out_row[s]] = sum_{j in segment s} w[j] * src[pos[j]]  (bilinear taps / their adjoint)."""
    nseg = out_row.numel()
    if nseg == 0:
        return out
    lib.call("rv_weighted_segment_sum_rows", src, src.stride(0), seg_off, pos, w, out_row, nseg, out, out.stride(0), src.shape[1])
    return out


def max4_rows_fwd(src, idx4, out_row, out):
    """out[out_row[s]] = max over the four rows src[idx4[s]]; returns the per-element winning slot (uint8 [n, d])."""
    n, d = out_row.numel(), src.shape[1]
    which = torch.empty(n, d, dtype=torch.uint8, device=src.device)
    lib.call("rv_max4_rows_fwd", src, src.stride(0), idx4, out_row, n, out, out.stride(0), which, d)
    return which


def max4_rows_bwd(dout, idx4, dout_row, which, dsrc):
    lib.call("rv_max4_rows_bwd", dout, dout.stride(0), idx4, dout_row, dout_row.numel(), which, dsrc, dsrc.stride(0), dout.shape[1])
    return dsrc


def add_pos_rows(x, pos, n, P):
    """x [n*P, d] += pos [P, d] broadcast over images, in place."""
    assert x.is_contiguous() and pos.is_contiguous() and x.shape[0] == n * P and pos.shape[0] == P
    lib.call("rv_add_pos_rows", x, pos, n, P, x.shape[1])
    return x


def normalize_tiles_u8(img, tile, mean, std, mode=0, factor=1.0 / 255, gh=1, gw=1):
    """uint8 device canvases [n, gh*tile, gw*tile, 3] -> normalised bf16 tiles [n*gh*gw, 3, tile, tile] (host processors' fp32 arithmetic:
    mode 0 = CLIPImageProcessor, 1 = SigLipImageProcessor)."""
    import ctypes
    assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.shape[1:] == (gh * tile, gw * tile, 3), img.shape
    n = img.shape[0]
    out = torch.empty(n * gh * gw, 3, tile, tile, dtype=BF16, device=img.device)
    m3, s3 = (ctypes.c_float * 3)(*[float(x) for x in mean]), (ctypes.c_float * 3)(*[float(x) for x in std])
    lib.call("rv_normalize_tiles_u8", img, out, n, gh, gw, tile, int(mode), float(factor), m3, s3)
    return out


def im2col_patches(pix, p, kp):
    n, c, H, W = pix.shape
    assert c == 3 and pix.is_contiguous()
    _chk(pix)
    out = torch.empty(n * (H // p) * (W // p), kp, dtype=BF16, device=pix.device)
    lib.call("rv_im2col_patches", pix, out, n, H, W, p, kp)
    return out


def clip_embed(patch_out, cls, pos, n, P, d):
    out = torch.empty(n * (P + 1), d, dtype=BF16, device=patch_out.device)
    lib.call("rv_clip_embed", patch_out, cls, pos, out, n, P, d)
    return out


def adamw(p, master, g, m, v, lr, b1, b2, eps, wd, step, gscale=None):
    n = p.numel()
    lib.call("rv_adamw", p, master, g, m, v, n, lr, b1, b2, eps, wd, 1.0 - b1 ** step, 1.0 - b2 ** step, gscale)


def adam8_quantize(x, kind, codes=None, absmax=None):
    """fp32 tensor -> (uint8 codes [n], fp32 absmax [ceil(n / 256)]) of the 8-bit AdamW state; kind 0 = exp_avg, 1 = exp_avg_sq."""
    n = x.numel()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and n > 0
    codes = torch.empty(n, dtype=torch.uint8, device=x.device) if codes is None else codes
    absmax = torch.empty((n + 255) // 256, dtype=torch.float32, device=x.device) if absmax is None else absmax
    assert codes.dtype == torch.uint8 and codes.numel() >= n and absmax.dtype == torch.float32 and absmax.numel() >= (n + 255) // 256
    lib.call("rv_adam8_quantize_f32", x, n, codes, absmax, int(kind))
    return codes, absmax


def adam8_dequantize(codes, absmax, n, kind, out=None):
    assert codes.is_cuda and codes.dtype == torch.uint8 and codes.numel() >= n and absmax.dtype == torch.float32
    assert absmax.numel() >= (n + 255) // 256 and n > 0
    out = torch.empty(n, dtype=torch.float32, device=codes.device) if out is None else out
    assert out.dtype == torch.float32 and out.numel() >= n and out.is_contiguous()
    lib.call("rv_adam8_dequantize_f32", codes, absmax, n, int(kind), out)
    return out


def nf4_quantize(x, codes=None, absmax=None):
    """bf16 tensor -> (packed NF4 codes uint8 [ceil(n / 2)], fp32 absmax [ceil(n / 64)]) of the frozen QLoRA base (csrc/nf4.hip)."""
    n = x.numel()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and n > 0
    codes = torch.empty((n + 1) // 2, dtype=torch.uint8, device=x.device) if codes is None else codes
    absmax = torch.empty((n + 63) // 64, dtype=torch.float32, device=x.device) if absmax is None else absmax
    assert codes.dtype == torch.uint8 and codes.numel() >= (n + 1) // 2 and codes.is_contiguous()
    assert absmax.dtype == torch.float32 and absmax.numel() >= (n + 63) // 64 and absmax.is_contiguous()
    lib.call("rv_nf4_quantize_bf16", x, n, codes, absmax)
    return codes, absmax


def nf4_dequant(codes, table, host_table, nchunks, dst, absmax=None, absmax_codes=None, scale2=None, offset=None):
    """rv_nf4_dequant_bf16: one launch writes every tensor of `table` (device int64 [6, T], nf4.BasePlan.table) into the bf16 buffer
    `dst`.  absmax: the plain mode; absmax_codes + scale2 + offset (one per tensor of the table): double quantisation.  host_table is
    the same table on the host: every range the kernel will touch is checked against the buffers here, the kernel trusts the table."""
    T = int(host_table.shape[1])
    assert table.dtype == torch.int64 and tuple(table.shape) == (6, T) and table.is_contiguous() and table.is_cuda
    assert codes.dtype == torch.uint8 and dst.dtype == torch.bfloat16 and dst.is_contiguous() and codes.is_contiguous()
    dq = absmax is None
    if dq:
        assert absmax_codes.dtype == torch.uint8 and scale2.dtype == torch.float32 and offset.dtype == torch.float32 and offset.numel() >= T
    else:
        assert absmax.dtype == torch.float32 and absmax_codes is None and scale2 is None and offset is None
    chunk0, code0, blk0, n, dst0, s20 = (host_table[k] for k in range(6))
    nch = (n + 2047) // 2048
    assert n.min() > 0 and chunk0[0] == 0 and (chunk0[1:] == (chunk0 + nch)[:-1]).all() and int((chunk0 + nch)[-1]) == int(nchunks)
    nb = (n + 63) // 64
    assert min(code0.min(), blk0.min(), dst0.min(), s20.min()) >= 0
    assert int((code0 + (n + 1) // 2).max()) <= codes.numel() and int((dst0 + n).max()) <= dst.numel()
    assert int((blk0 + nb).max()) <= (absmax_codes if dq else absmax).numel()
    assert not dq or int((s20 + (nb + 255) // 256).max()) <= scale2.numel()
    lib.call("rv_nf4_dequant_bf16", codes, absmax, absmax_codes, scale2, offset, table, T, int(nchunks), dst)
    return dst


def adamw8(p, master, g, codes_m, codes_v, absmax_m, absmax_v, table, nblocks, lr, b1, b2, eps, wd, step, gscale=None):
    """rv_adamw8 on one slice: `table` is the device int64 [3, T] block table of optim8.StatePlan.block_table, the code buffers hold
    nblocks * 256 bytes and the absmax buffers nblocks floats (checked here: the kernel trusts them)."""
    assert table.dtype == torch.int64 and table.dim() == 2 and table.shape[0] == 3 and table.is_contiguous()
    assert min(codes_m.numel(), codes_v.numel()) >= nblocks * 256 and min(absmax_m.numel(), absmax_v.numel()) >= nblocks
    assert codes_m.dtype == codes_v.dtype == torch.uint8 and absmax_m.dtype == absmax_v.dtype == torch.float32
    assert p.numel() == master.numel() == g.numel()
    lib.call("rv_adamw8", p, master, g, codes_m, codes_v, absmax_m, absmax_v, table, int(table.shape[1]), int(nblocks), lr, b1, b2, eps,
             wd, 1.0 - b1 ** step, 1.0 - b2 ** step, gscale)


def grad_norm_clip_coef(g, max_norm):
    """Returns fp32[2] device tensor: (global grad norm, clip coefficient) with no host sync."""
    nblk = 1024
    part = torch.empty(nblk, dtype=torch.float32, device=g.device)
    lib.call("rv_sumsq_partial_bf16", g, g.numel(), part, nblk)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    lib.call("rv_clip_coef", part, nblk, max_norm, out)
    return out


def to_bf16(x):
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    lib.call("rv_cast_f32_to_bf16", x.contiguous(), out, x.numel())
    return out


def to_f32(x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    lib.call("rv_cast_bf16_to_f32", x.contiguous(), out, x.numel())
    return out


# ------------------------------------------------------------------------------------------------ decode (generate)
GEMV_MAX_M = 32


def gemv_split(N, K):
    """K slices rv_gemv_bf16 uses for an [N, K] weight (a function of the weight shape alone)."""
    return int(lib.load().rv_gemv_split(int(N), int(K)))


def _gemv_args(x, N, K, out, bias, residual, out_dtype, workspace):
    """What gemv, gemv_w8 and gemv_w4 share once each has checked its own [N, K] weight operand: the checks of x, out (allocated when
    None), bias and residual, and the default workspace.  Returns (M, out, ldr, workspace, its bytes)."""
    _chk(x)
    M, Kx = x.shape
    assert 1 <= M <= GEMV_MAX_M and Kx == K and x.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=x.device)
    assert out.shape == (M, N) and out.stride(1) == 1 and out.dtype in (BF16, torch.float32)
    if bias is not None:
        _chk(bias)
        assert bias.numel() == N and bias.is_contiguous()
    ldr = 0
    if residual is not None:
        _chk(residual)
        assert residual.shape == (M, N) and residual.stride(1) == 1
        ldr = residual.stride(0)
    if workspace is None:
        workspace = default_workspace(x.device)
    return M, out, ldr, workspace, workspace.numel() * workspace.element_size()


def gemv(x, w, out=None, bias=None, residual=None, out_dtype=BF16, workspace=None):
    """out[M,N] = x[M,K] @ w[N,K]^T (+ bias) (+ residual) for M <= 32 rows (decode): rv_gemv_bf16, weights streamed once.
    Row r of the result is bit-identical for every M."""
    _chk(w)
    N, K = w.shape
    assert w.stride(1) == 1
    M, out, ldr, ws, ws_bytes = _gemv_args(x, N, K, out, bias, residual, out_dtype, workspace)
    lib.call("rv_gemv_bf16", x, x.stride(0), w, w.stride(0), out, out.stride(0), bias, residual, ldr, M, N, K,
             int(out.dtype == torch.float32), ws, ws_bytes)
    return out


def _quantize_rows_args(w):
    """The input checks quantize_rows_w8 and quantize_rows_mxfp4 share; returns (N, K)."""
    _chk(w)
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    assert K % 8 == 0 and w.stride(0) % 8 == 0
    return N, K


def w8_row_bytes(K):
    """Bytes of one packed int8 row for K input features: 64 per pair of 32-deep K steps (a function of K alone, no library call)."""
    return ((int(K) + 31) // 32 + 1) // 2 * 64


def quantize_rows_w8(w):
    """Row-wise int8 quantisation of a bf16 [N, K] weight IN PLACE (rv_quantize_rows_w8_bf16): s = max|row| / 127 (1 for a zero row),
    q = clamp(rint(w / s), -127, 127), w <- bf16(float(q) * s).  w may be a row-major view with a row stride (the fused q|k|v and
    gate|up views).  Returns (packed int8 [N, w8_row_bytes(K)] in gemv_w8's private layout, scale fp32 [N]).  Quantising the result
    again rounds again: call it once per weight.  Non-finite weights are outside the contract."""
    N, K = _quantize_rows_args(w)
    packed = torch.empty(N, w8_row_bytes(K), dtype=torch.int8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    lib.call("rv_quantize_rows_w8_bf16", w, w.stride(0), packed, packed.stride(0), scale, N, K)
    return packed, scale


def gemv_w8(x, packed, scale, K, out=None, bias=None, residual=None, out_dtype=BF16, workspace=None):
    """gemv() with the weight given as quantize_rows_w8's (packed, scale) of a [N, K] weight: rv_gemv_w8_bf16, half the weight bytes,
    bit-identical to gemv(x, w) on the dequantised weight quantize_rows_w8 left in place."""
    _chk(packed, torch.int8), _chk(scale, torch.float32)
    N = packed.shape[0]
    assert packed.is_contiguous() and packed.shape[1] == w8_row_bytes(K) and scale.numel() == N and scale.is_contiguous()
    M, out, ldr, ws, ws_bytes = _gemv_args(x, N, K, out, bias, residual, out_dtype, workspace)
    lib.call("rv_gemv_w8_bf16", x, x.stride(0), packed, packed.stride(0), scale, out, out.stride(0), bias, residual, ldr, M, N, K,
             int(out.dtype == torch.float32), ws, ws_bytes)
    return out


def w4_row_bytes(K):
    """Bytes of one packed MXFP4 nibble row for K input features: 64 per four 32-deep K steps (a function of K alone, no library call)."""
    return ((int(K) + 31) // 32 + 3) // 4 * 64


def w4_scale_row_bytes(K):
    """Bytes of one MXFP4 scale row for K input features: one E8M0 byte per 32-deep K step, padded to whole quads of steps."""
    return ((int(K) + 31) // 32 + 3) // 4 * 4


def quantize_rows_mxfp4(w):
    """MXFP4 quantisation of a bf16 [N, K] weight IN PLACE (rv_quantize_rows_mxfp4_bf16): per block of 32 consecutive k one power-of-two
    scale 2^e, e = floor(log2(max|block|)) - 2, and per weight the nearest E2M1 value of |w| / 2^e (ties to the even code, saturating);
    w <- sign * value * 2^e, exactly a bf16 number.  w may be a row-major view with a row stride (the fused q|k|v and gate|up views).
    Returns (packed uint8 [N, w4_row_bytes(K)] in gemv_w4's private layout, scales uint8 [N, w4_scale_row_bytes(K)]).  Lossy (about
    12 % relative Frobenius error on Gaussian rows).  Block maxima outside [2^-120, 2^120] and non-finite weights are outside the
    contract."""
    N, K = _quantize_rows_args(w)
    packed = torch.empty(N, w4_row_bytes(K), dtype=torch.uint8, device=w.device)
    scales = torch.empty(N, w4_scale_row_bytes(K), dtype=torch.uint8, device=w.device)
    lib.call("rv_quantize_rows_mxfp4_bf16", w, w.stride(0), packed, packed.stride(0), scales, scales.stride(0), N, K)
    return packed, scales


def gemv_w4(x, packed, scales, K, out=None, bias=None, residual=None, out_dtype=BF16, workspace=None):
    """gemv() with the weight given as quantize_rows_mxfp4's (packed, scales) of a [N, K] weight: rv_gemv_w4_bf16, 0.27x the weight
    bytes, bit-identical to gemv(x, w) on the quantised weight quantize_rows_mxfp4 left in place."""
    _chk(packed, torch.uint8), _chk(scales, torch.uint8)
    N = packed.shape[0]
    assert packed.is_contiguous() and packed.shape[1] == w4_row_bytes(K)
    assert scales.is_contiguous() and scales.shape == (N, w4_scale_row_bytes(K))
    M, out, ldr, ws, ws_bytes = _gemv_args(x, N, K, out, bias, residual, out_dtype, workspace)
    lib.call("rv_gemv_w4_bf16", x, x.stride(0), packed, packed.stride(0), scales, scales.stride(0), out, out.stride(0), bias, residual, ldr,
             M, N, K, int(out.dtype == torch.float32), ws, ws_bytes)
    return out


LORA_DECODE_MAX_MODS = 3


def lora_down_split(r, K):
    """K slices rv_lora_down_rows_bf16 uses for adapters of rank r over K input features (a function of (r, K) alone)."""
    return int(lib.load().rv_lora_down_split(int(r), int(K)))


def lora_down_rows(x, adapters, scale, out=None, workspace=None):
    """t[M, j*r:(j+1)*r] = bf16(scale * x[M,K] @ adapters[j][r,K]^T) for the 1..3 lora_A matrices that share the input x, M <= 32 rows
    (decode): rv_lora_down_rows_bf16, one call for a fused projection's adapters, K split over workgroups.  Row m of the result is
    bit-identical for every M."""
    _chk(x)
    M, K = x.shape
    n, r = len(adapters), adapters[0].shape[0]
    assert 1 <= n <= LORA_DECODE_MAX_MODS and x.stride(1) == 1
    lda = adapters[0].stride(0)
    for a in adapters:
        _chk(a)
        assert a.shape == (r, K) and a.stride(1) == 1 and a.stride(0) == lda
    if out is None:
        out = torch.empty(M, n * r, dtype=BF16, device=x.device)
    assert out.shape == (M, n * r) and out.stride(1) == 1 and out.dtype == BF16
    ws = default_workspace(x.device) if workspace is None else workspace
    ptrs = list(adapters) + [None] * (LORA_DECODE_MAX_MODS - n)
    lib.call("rv_lora_down_rows_bf16", x, x.stride(0), ptrs[0], ptrs[1], ptrs[2], lda, n, out, out.stride(0), M, r, K, float(scale), ws,
             ws.numel() * ws.element_size())
    return out


def gemv_lora(x, w, t, mods, out=None, bias=None, residual=None, workspace=None):
    """out[M,N] = x[M,K] @ w[N,K]^T + sum_j t[:, toff_j:toff_j+r] @ B_j^T on columns [c0_j, c1_j) (+ bias) (+ residual), bf16, M <= 32
    rows (decode): rv_gemv_lora_bf16.  mods: 1..3 entries (c0, c1, toff, B_j [c1 - c0, r]), ascending and disjoint, boundaries multiples
    of 64 (c1 may be N).  With every B_j zero the result is gemv(x, w, ...)'s, bit for bit; row m is bit-identical for every M."""
    _chk(w), _chk(t)
    N, K = w.shape
    n = len(mods)
    assert w.stride(1) == 1 and t.stride(1) == 1 and 1 <= n <= LORA_DECODE_MAX_MODS
    r, ldb = mods[0][3].shape[1], mods[0][3].stride(0)
    flat = []
    for c0, c1, toff, b in mods:
        _chk(b)
        assert b.shape == (c1 - c0, r) and b.stride(1) == 1 and b.stride(0) == ldb
        flat += [b, int(c0), int(c1), int(toff)]
    flat += [None, 0, 0, 0] * (LORA_DECODE_MAX_MODS - n)
    M, out, ldr, ws, ws_bytes = _gemv_args(x, N, K, out, bias, residual, BF16, workspace)
    assert out.dtype == BF16 and t.shape[0] == M
    lib.call("rv_gemv_lora_bf16", x, x.stride(0), w, w.stride(0), t, t.stride(0), r, n, *flat, ldb, out, out.stride(0), bias, residual, ldr,
             M, N, K, ws, ws_bytes)
    return out


def _attn_split_args(q, rows, H, hd, keys, out, chunk, scale):
    """What the seven split-KV attention wrappers share (csrc/attn_split.h's launcher checks the same on its side): the default scale,
    `out` (bf16 [rows, H*hd], allocated unless passed in, rows of unit stride) and the fp32 partial buffer for ceil(keys / chunk)
    chunks of every (row, head).  Returns (out, part, part_bytes, scale)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    if out is None:
        out = torch.empty(rows, H * hd, dtype=BF16, device=q.device)
    assert out.shape == (rows, H * hd) and out.stride(1) == 1
    nch = (keys + chunk - 1) // chunk
    part = torch.empty(rows * H * nch * (hd + 2), dtype=torch.float32, device=q.device)
    return out, part, part.numel() * 4, float(scale)


def attn_decode(q, cache, kv_len, H, Hkv, hd, v_off, out=None, chunk=128, scale=None):
    """One query row per (sequence, q head) against the cached keys [0, kv_len[b]): q [B, H*hd] rows; cache bf16 [B, L_max, width]
    with K of kv head g at columns g*hd and V at v_off + g*hd; kv_len int32 [B] (device).  Returns bf16 [B, H*hd]."""
    _chk(q), _chk(cache), _chk(kv_len, torch.int32)
    B, L_max, width = cache.shape
    assert q.shape == (B, H * hd) and q.stride(1) == 1 and cache.is_contiguous() and kv_len.numel() == B and kv_len.is_contiguous()
    out, part, part_bytes, scale = _attn_split_args(q, B, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_decode_bf16", q, q.stride(0), cache, width, L_max * width, v_off, kv_len, L_max, out, out.stride(0), part,
             part_bytes, B, H, Hkv, hd, chunk, scale)
    return out


def attn_decode_probs(q, cache, kv_len, H, Hkv, hd, L_out, per_head=True, mean=False, scale=None, out=None, mean_out=None):
    """The attention probabilities attn_decode's softmax never writes out (rv_attn_decode_probs_f32): q, cache, kv_len as in attn_decode
    (the cache's rows may be strided: a layer's K|V view; V is not read), L_out <= L_max columns.  Returns (probs, mean): fp32
    [B, H, L_out] softmax(scale * q K^T) over each row's keys [0, min(kv_len[b], L_out)) when per_head, and fp32 [B, L_out], its mean
    over the heads in head order, when mean; None for the one not asked for.  Columns at or past a row's key count are 0.
    out / mean_out: write into these instead (fp32 [B, H, >= L_out] with rows packed per sequence / [B, >= L_out], unit column
    stride; columns >= L_out are left as they are); they turn per_head / mean on."""
    _chk(q), _chk(cache), _chk(kv_len, torch.int32)
    B, L_max, width = cache.shape
    L_out = int(L_out)
    per_head, mean = per_head or out is not None, mean or mean_out is not None
    assert q.shape == (B, H * hd) and q.stride(1) == 1 and cache.stride(2) == 1 and kv_len.numel() == B and kv_len.is_contiguous()
    assert (per_head or mean) and 1 <= L_out <= L_max
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    if per_head and out is None:
        out = torch.empty(B, H, L_out, dtype=torch.float32, device=q.device)
    if mean and mean_out is None:
        mean_out = torch.empty(B, L_out, dtype=torch.float32, device=q.device)
    if out is not None:
        _chk(out, torch.float32)
        assert out.shape[:2] == (B, H) and out.shape[2] >= L_out and out.stride(2) == 1 and (B == 1 or out.stride(0) == H * out.stride(1))
    if mean_out is not None:
        _chk(mean_out, torch.float32)
        assert mean_out.shape[0] == B and mean_out.shape[1] >= L_out and mean_out.stride(1) == 1
    ws_bytes = lib.load().rv_attn_decode_probs_ws_bytes(B, H, L_out)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=q.device)
    lib.call("rv_attn_decode_probs_f32", q, q.stride(0), cache, cache.stride(1), cache.stride(0), kv_len, L_max, L_out, out,
             out.stride(1) if out is not None else 0, mean_out, mean_out.stride(0) if mean_out is not None else 0, ws, ws_bytes, B, H, Hkv,
             hd, float(scale))
    return (out[:, :, :L_out] if out is not None else None), (mean_out[:, :L_out] if mean_out is not None else None)


KVPRESS_MAX_WINDOW = 64   # observation window rows (rv_kv_votes_f32)
KVPRESS_MAX_POOL = 63     # pooling width, odd (rv_kv_select_i32)


def kv_votes(qkv, cu, H, Hkv, hd, w, max_P, flags=None, scale=None, out=None):
    """SnapKV votes (rv_kv_votes_f32): qkv the packed post-RoPE bf16 [M, >= (H + Hkv) * hd] q|k|v rows of a prompt pass (q head h at
    columns h*hd, K of kv head g at H*hd + g*hd), cu int32 [B + 1] (device), sequence b's last w rows its observation window.  Returns
    fp32 [B, Hkv, max_P - w]: column j < P_b - w is the attention the window's rows of the kv head's query heads pay to prefix key j
    (each row's causal softmax, summed); other columns and the rows of sequences with flags[b] == 0 (int32 [B], device) or
    P_b <= w are left as they are (out: write into this tensor; a new one is torch.empty)."""
    _chk(qkv), _chk(cu, torch.int32)
    B = cu.numel() - 1
    w, max_P = int(w), int(max_P)
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.shape[1] >= (H + Hkv) * hd and cu.is_contiguous() and B >= 1
    if flags is not None:
        _chk(flags, torch.int32)
        assert flags.numel() == B and flags.is_contiguous()
    if out is None:
        out = torch.empty(B, Hkv, max(max_P - w, 1), dtype=torch.float32, device=qkv.device)
    _chk(out, torch.float32)
    assert out.shape[:2] == (B, Hkv) and out.is_contiguous()
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    ws_bytes = lib.load().rv_kv_votes_ws_bytes(B, H, Hkv, w, max_P)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.float32, device=qkv.device)
    lib.call("rv_kv_votes_f32", qkv, qkv.stride(0), qkv[:, H * hd:], qkv.stride(0), cu, flags, max_P, out, out.shape[2], ws, ws_bytes, B, H,
             Hkv, hd, w, float(scale))
    return out


def kv_select(votes, cu, N, w, k, flags=None, out=None):
    """SnapKV selection (rv_kv_select_i32): votes fp32 [B, Hkv, ld_v] (non-negative), cu int32 [B + 1].  Returns int32 [B, Hkv, N]: per
    sequence with P_b > N and kv head, the N - w prefix positions with the largest max-pooled vote (width k, ties to the lower
    position) in ascending order, then the w window positions.  Rows of other sequences (and of flags[b] == 0) are left as they are."""
    _chk(votes, torch.float32), _chk(cu, torch.int32)
    B, Hkv, ld_v = votes.shape
    assert votes.is_contiguous() and cu.numel() == B + 1 and cu.is_contiguous()
    if flags is not None:
        _chk(flags, torch.int32)
        assert flags.numel() == B and flags.is_contiguous()
    if out is None:
        out = torch.empty(B, Hkv, int(N), dtype=torch.int32, device=votes.device)
    _chk(out, torch.int32)
    assert out.shape == (B, Hkv, int(N)) and out.is_contiguous()
    ws_bytes = lib.load().rv_kv_select_ws_bytes(B, Hkv, ld_v)
    ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=votes.device)
    lib.call("rv_kv_select_i32", votes, ld_v, cu, flags, out, ws, ws_bytes, B, Hkv, int(N), int(w), int(k))
    return out


def kv_gather(kv, cu, keep, seq, cache, Hkv, hd, flags=None):
    """SnapKV gather (rv_kv_gather_bf16): kv the packed bf16 K|V rows [M, 2 * Hkv * hd] of a prompt pass (a column view of the q|k|v
    product), keep int32 [B, Hkv, N] from kv_select, seq int32 [B] the sequences' rows of cache bf16 [rows, L_max, 2 * Hkv * hd].
    Slot s of every sequence with P_b > N takes, per kv head, the K|V of prompt position keep[b, g, s]; nothing else is written."""
    _chk(kv), _chk(cache), _chk(cu, torch.int32), _chk(keep, torch.int32), _chk(seq, torch.int32)
    B, _, N = keep.shape
    rows, L_max, width = cache.shape
    kvd = Hkv * hd
    assert kv.stride(1) == 1 and kv.shape[1] == 2 * kvd and width == 2 * kvd and cache.is_contiguous() and keep.is_contiguous()
    assert keep.shape[1] == Hkv and cu.numel() == B + 1 and seq.numel() == B and cu.is_contiguous() and seq.is_contiguous()
    if flags is not None:
        _chk(flags, torch.int32)
        assert flags.numel() == B and flags.is_contiguous()
    lib.call("rv_kv_gather_bf16", kv, kv.stride(0), kvd, cu, flags, keep, seq, cache, width, L_max, rows, B, Hkv, hd, N)
    return cache


EXTEND_CHUNK = 256        # keys per extend-attention workgroup: fixed, so a row's result never depends on the batch around it


def attn_extend(q, cache, cu_q, r, H, Hkv, hd, v_off, max_q, out=None, chunk=EXTEND_CHUNK, scale=None):
    """Causal attention of new query rows against a KV cache (rv_attn_extend_bf16): q [M, H*hd] rows, sequence b's rows
    cu_q[b] .. cu_q[b+1] - 1 at positions r[b] + i, their own K|V already in cache (bf16 [B, L_max, width], K of kv head g at columns
    g*hd, V at v_off + g*hd); cu_q (B + 1) / r (B) int32 device arrays, max_q >= every sequence's row count.  Returns bf16 [M, H*hd]."""
    _chk(q), _chk(cache), _chk(cu_q, torch.int32), _chk(r, torch.int32)
    B, L_max, width = cache.shape
    M = q.shape[0]
    assert q.shape == (M, H * hd) and q.stride(1) == 1 and cache.is_contiguous() and cu_q.numel() == B + 1 and r.numel() == B
    assert cu_q.is_contiguous() and r.is_contiguous() and 1 <= max_q <= M
    out, part, part_bytes, scale = _attn_split_args(q, M, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_extend_bf16", q, q.stride(0), cache, width, L_max * width, v_off, cu_q, r, L_max, out, out.stride(0), part,
             part_bytes, B, M, int(max_q), H, Hkv, hd, chunk, scale)
    return out


def attn_extend_prefix(q, prefix, tail, cu_q, prefix_row, prefix_len, H, Hkv, hd, v_off, max_q, out=None, chunk=EXTEND_CHUNK, scale=None):
    """attn_extend with two key sources (rv_attn_extend_prefix_bf16): sequence b's query rows cu_q[b] .. cu_q[b+1] - 1 sit at positions
    prefix_len[b] + i; keys below prefix_len[b] are read in place from row prefix_row[b] of `prefix` (bf16 [P_rows, P_max, width], e.g. a
    prefilled KV cache shared by many candidates), the rest from row b of `tail` (bf16 [B, T_max, width], the sequence's own rows, already
    written).  cu_q (B + 1) / prefix_row / prefix_len (B) int32 device arrays, 1 <= max_q <= T_max.  Bit-identical to attn_extend on the
    materialised cache at the same chunk.  Returns bf16 [M, H*hd]."""
    _chk(q), _chk(prefix), _chk(tail), _chk(cu_q, torch.int32), _chk(prefix_row, torch.int32), _chk(prefix_len, torch.int32)
    assert prefix.dim() == 3 and tail.dim() == 3 and prefix.is_contiguous() and tail.is_contiguous()
    P_rows, P_max, width = prefix.shape
    B, T_max, tw = tail.shape
    M = q.shape[0]
    assert tw == width and q.shape == (M, H * hd) and q.stride(1) == 1 and cu_q.numel() == B + 1
    assert prefix_row.numel() == B and prefix_len.numel() == B
    assert cu_q.is_contiguous() and prefix_row.is_contiguous() and prefix_len.is_contiguous() and 1 <= max_q <= M
    out, part, part_bytes, scale = _attn_split_args(q, M, H, hd, P_max + T_max, out, chunk, scale)
    lib.call("rv_attn_extend_prefix_bf16", q, q.stride(0), prefix, width, P_max * width, P_rows, P_max, tail, width, T_max * width, T_max,
             v_off, cu_q, prefix_row, prefix_len, out, out.stride(0), part, part_bytes, B, M, int(max_q), H, Hkv, hd, chunk,
             scale)
    return out


def token_logprob_rows(x, n, target, src_row=None, want_argmax=True):
    """(logprob fp32 [rows], argmax int64 [rows] or None) of rv_token_logprob_rows_f32: output row r reads row src_row[r] (r when
    src_row is None) of the fp32 logits x, first n columns, and gets log_softmax_rows' bits at column target[r] (int32 [rows] device;
    negative: 0.0, >= n: NaN) and the row's argmax (argmax_rows' rule).  x is not modified."""
    _chk(x, torch.float32), _chk(target, torch.int32)
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    rows = target.numel()
    assert rows >= 1 and target.is_contiguous()
    if src_row is not None:
        _chk(src_row, torch.int32)
        assert src_row.numel() == rows and src_row.is_contiguous()
    else:
        assert rows <= x.shape[0]
    logprob = torch.empty(rows, dtype=torch.float32, device=x.device)
    argmax = torch.empty(rows, dtype=torch.int64, device=x.device) if want_argmax else None
    lib.call("rv_token_logprob_rows_f32", x, x.stride(0), x.shape[0], int(n), src_row, target, rows, logprob, argmax)
    return logprob, argmax


def kv_append(src, cache, pos):
    """cache[b, pos[b], :] = src[b, :] (src [B, width] bf16 rows, e.g. the k|v columns of the qkv product; pos int32 [B] device)."""
    _chk(src), _chk(cache), _chk(pos, torch.int32)
    B, L_max, width = cache.shape
    assert src.shape == (B, width) and src.stride(1) == 1 and cache.is_contiguous() and pos.numel() == B and pos.is_contiguous()
    lib.call("rv_kv_append_bf16", src, src.stride(0), cache, width, L_max * width, pos, L_max, B, width)
    return cache


def _kvq_targets(src, cache, xhat, Hkv, hd):
    """Checks shared by kv_quantize_rows and kv_append_q8: cache is (q8 int8 [B, L_max, 2*kvd], s fp32 [B, L_max, 2*Hkv]) or None,
    xhat a bf16 [B, L_max, 2*kvd] cache or None.  Returns (q8, ld_q, s, ld_s, xhat, ld_x, B, L_max)."""
    width = 2 * Hkv * hd
    _chk(src)
    assert src.dim() == 2 and src.shape[1] == width and src.stride(1) == 1
    assert cache is not None or xhat is not None, "nothing to write: pass the int8 cache, the bf16 output or both"
    q8 = s = None
    shape = None
    if cache is not None:
        q8, s = cache
        _chk(q8, torch.int8), _chk(s, torch.float32)
        assert q8.dim() == 3 and q8.shape[2] == width and q8.is_contiguous()
        assert s.shape == (q8.shape[0], q8.shape[1], 2 * Hkv) and s.is_contiguous()
        shape = q8.shape[:2]
    if xhat is not None:
        _chk(xhat)
        assert xhat.dim() == 3 and xhat.shape[2] == width and xhat.is_contiguous() and (shape is None or xhat.shape[:2] == shape)
        shape = xhat.shape[:2]
    return q8, width, s, 2 * Hkv, xhat, width, int(shape[0]), int(shape[1])


def kv_quantize_rows(src, rows, Hkv, hd, cache=None, xhat=None):
    """Quantises the bf16 K|V rows src [M, 2*Hkv*hd] (a column view of the q|k|v product is fine) per (row, kv head, K / V) group --
    s = max|x| / 127 (1 for a zero group), q = clamp(rint(x / s), -127, 127) -- into the flat cache rows `rows` (int64 [M] device,
    b * L_max + position; rows outside the cache are skipped) of cache = (q8 int8 [B, L_max, 2*kvd], s fp32 [B, L_max, 2*Hkv]), and /
    or writes the dequantised bf16(float(q) * s) to the same rows of the bf16 cache `xhat` (rv_kv_quantize_rows_bf16)."""
    q8, ld_q, s, ld_s, xh, ld_x, B, L_max = _kvq_targets(src, cache, xhat, Hkv, hd)
    _chk(rows, torch.int64)
    M = src.shape[0]
    assert rows.numel() == M and rows.is_contiguous()
    lib.call("rv_kv_quantize_rows_bf16", src, src.stride(0), q8, ld_q, s, ld_s, xh, ld_x, rows, B * L_max, M, Hkv, hd)


def kv_append_q8(src, pos, Hkv, hd, cache=None, xhat=None):
    """kv_quantize_rows addressed like kv_append: row b of src [B, 2*Hkv*hd] goes to position pos[b] (int32 [B] device) of sequence b;
    a position outside the cache is skipped (rv_kv_append_q8_bf16)."""
    q8, ld_q, s, ld_s, xh, ld_x, B, L_max = _kvq_targets(src, cache, xhat, Hkv, hd)
    _chk(pos, torch.int32)
    assert src.shape[0] == B and pos.numel() == B and pos.is_contiguous()
    lib.call("rv_kv_append_q8_bf16", src, src.stride(0), q8, ld_q, s, ld_s, xh, ld_x, pos, L_max, B, Hkv, hd)


def attn_decode_kv8(q, cache, kv_len, H, Hkv, hd, v_off, out=None, chunk=128, scale=None):
    """attn_decode() over an int8 cache = (q8 int8 [B, L_max, width], s fp32 [B, L_max, 2*Hkv]): rv_attn_decode_kv8_bf16, bit-identical
    to attn_decode on (q8.float() * s.repeat_interleave(hd, -1)).to(bfloat16) at the same chunk.  K of kv head g at columns g*hd of q8
    and column g of s, V at v_off + g*hd and Hkv + g."""
    q8, s = cache
    _chk(q), _chk(q8, torch.int8), _chk(s, torch.float32), _chk(kv_len, torch.int32)
    B, L_max, width = q8.shape
    assert q.shape == (B, H * hd) and q.stride(1) == 1 and q8.is_contiguous() and kv_len.numel() == B and kv_len.is_contiguous()
    assert s.shape == (B, L_max, 2 * Hkv) and s.is_contiguous()
    out, part, part_bytes, scale = _attn_split_args(q, B, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_decode_kv8_bf16", q, q.stride(0), q8, width, L_max * width, v_off, s, 2 * Hkv, L_max * 2 * Hkv, Hkv, kv_len, L_max,
             out, out.stride(0), part, part_bytes, B, H, Hkv, hd, chunk, scale)
    return out


def argmax_rows(x, n, out=None):
    """int64 [rows]: torch.argmax of each fp32 row over its first n columns (lowest index on ties)."""
    _chk(x, torch.float32)
    rows = x.shape[0]
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= x.shape[1]
    out = torch.empty(rows, dtype=torch.int64, device=x.device) if out is None else out
    lib.call("rv_argmax_rows_f32", x, x.stride(0), rows, int(n), out)
    return out


LOGITS_PROCESS_MAX_N = 262144


def logits_process_argmax(x, n, hist, t, rep_penalty=1.0, ngram=0, ban=None, bad_tok=None, bad_off=None, out=None):
    """Greedy logits processors + argmax (rv_logits_process_argmax_f32): processes fp32 rows x[:, :n] IN PLACE -- repetition penalty on
    the distinct tokens of hist[:, :t], n-gram bans, multi-token bad words (CSR bad_tok / bad_off int32, bad_off of n_bad + 1 entries),
    -inf on the ids of `ban` (int32, shared by every row) -- and returns the int64 argmax of each processed row.  hist: int32 [rows, >= t]
    (the tokens generated so far), may be None when t == 0."""
    _chk(x, torch.float32)
    rows = x.shape[0]
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    ld_hist = 0
    if t > 0:
        _chk(hist, torch.int32)
        assert hist.dim() == 2 and hist.shape[0] == rows and hist.shape[1] >= t and hist.stride(1) == 1
        ld_hist = hist.stride(0)
    for a in (ban, bad_tok, bad_off):
        if a is not None:
            _chk(a, torch.int32)
            assert a.is_contiguous()
    n_bad = 0 if bad_off is None else bad_off.numel() - 1
    assert n_bad <= 0 or bad_tok is not None
    out = torch.empty(rows, dtype=torch.int64, device=x.device) if out is None else out
    lib.call("rv_logits_process_argmax_f32", x, x.stride(0), rows, int(n), hist if t > 0 else None, ld_hist, int(t), float(rep_penalty),
             int(ngram), ban, 0 if ban is None else ban.numel(), bad_tok, bad_off, max(n_bad, 0), out)
    return out


def logits_process_argmax_rows(x, n, hist, slot, t, min_new, rep_penalty=1.0, ngram=0, ban_always=None, ban_begin=None, ban_eos=None,
                               bad_tok=None, bad_off=None, out=None, logprob=None):
    """logits_process_argmax for rows at different steps (rv_logits_process_argmax_rows_f32): row r is at step t[r] with EOS minimum
    min_new[r] and reads its history from hist[slot[r], :t[r]] (slot, t, min_new: int32 [rows]; hist: int32 [slots, cols] or None).
    ban_always on every row, ban_begin where t[r] == 0, ban_eos where t[r] < min_new[r].  Processes x[:, :n] IN PLACE and returns the
    int64 argmax of each processed row; with `logprob` (fp32 [rows]) also writes the log-softmax of the processed row at that token."""
    _chk(x, torch.float32)
    rows = x.shape[0]
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    for a in (slot, t, min_new):
        _chk(a, torch.int32)
        assert a.dim() == 1 and a.numel() == rows and a.stride(0) == 1
    hist_rows = hist_cols = ld_hist = 0
    if hist is not None:
        _chk(hist, torch.int32)
        assert hist.dim() == 2 and hist.stride(1) == 1
        hist_rows, hist_cols, ld_hist = hist.shape[0], hist.shape[1], hist.stride(0)
    for a in (ban_always, ban_begin, ban_eos, bad_tok, bad_off):
        if a is not None:
            _chk(a, torch.int32)
            assert a.is_contiguous()
    n_bad = 0 if bad_off is None else bad_off.numel() - 1
    assert n_bad <= 0 or bad_tok is not None
    if logprob is not None:
        _chk(logprob, torch.float32)
        assert logprob.numel() == rows and logprob.is_contiguous()
    out = torch.empty(rows, dtype=torch.int64, device=x.device) if out is None else out
    cnt = lambda a: 0 if a is None else a.numel()
    lib.call("rv_logits_process_argmax_rows_f32", x, x.stride(0), rows, int(n), hist, ld_hist, hist_rows, hist_cols, slot, t, min_new,
             float(rep_penalty), int(ngram), ban_always, cnt(ban_always), ban_begin, cnt(ban_begin), ban_eos, cnt(ban_eos), bad_tok, bad_off,
             max(n_bad, 0), out, logprob)
    return out


def sample_rows_workspace(rows, device):
    """Scratch for sample_rows on up to `rows` rows (int64, never zeroed).  One per generation loop: calls that share it must run on one stream."""
    return torch.empty(lib.load().rv_sample_ws_bytes(int(rows)) // 8, dtype=torch.int64, device=device)


def sample_rows(x, n, seed, t, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, write_scores=False, out=None, logprob=None, ws=None, tag=0):
    """Seeded sampling (rv_sample_rows_f32): one token per fp32 row x[r, :n] after HF's warpers temperature -> top-k -> top-p -> min-p,
    drawn with the counter-based uniform of (seed[r], t[r]) (seed: int64 [rows] holding the uint64 bits, t: int32 [rows]).  write_scores:
    x[:, :n] becomes the warped scores (-inf where removed), else x is only read.  Returns int64 [rows]; -1 marks a row that cannot be
    sampled (NaN, +inf or no finite entry).  logprob (fp32 [rows]): log q of the drawn token.  ws: sample_rows_workspace(>= rows), allocated
    here when not given.  tag: another stream of the same seed (rv_sample_rows_tagged_f32; 0 is the plain entry point)."""
    _chk(x, torch.float32)
    rows = x.shape[0]
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    _chk(seed, torch.int64), _chk(t, torch.int32)
    for a in (seed, t):
        assert a.dim() == 1 and a.numel() == rows and a.stride(0) == 1
    if logprob is not None:
        _chk(logprob, torch.float32)
        assert logprob.numel() == rows and logprob.is_contiguous()
    out = torch.empty(rows, dtype=torch.int64, device=x.device) if out is None else out
    ws = sample_rows_workspace(rows, x.device) if ws is None else ws
    _chk(ws, torch.int64)
    assert ws.is_contiguous() and ws.numel() * 8 >= lib.load().rv_sample_ws_bytes(rows)
    args = (float(temperature), int(top_k or 0), float(top_p), float(min_p), 1 if write_scores else 0, out, logprob, ws, ws.numel() * 8)
    if tag:
        lib.call("rv_sample_rows_tagged_f32", x, x.stride(0), rows, int(n), seed, t, int(tag), *args)
    else:
        lib.call("rv_sample_rows_f32", x, x.stride(0), rows, int(n), seed, t, *args)
    return out


SPEC_MAX_R = 32               # rows per group of spec_accept_rows: up to 31 drafts and the row after them


def spec_accept_workspace(groups, R, device):
    """Scratch for spec_accept_rows on up to `groups` groups of R rows (int64, never zeroed)."""
    return torch.empty(max(lib.load().rv_spec_ws_bytes(int(groups), int(R)) // 8, 1), dtype=torch.int64, device=device)


def spec_accept_rows(p, q, draft, seed, t0, n, ws=None):
    """Speculative sampling's accept / resample step (rv_spec_accept_rows_f32).  p: fp32 [groups * R, >= n], the target's warped score
    rows; q: fp32 [groups * (R - 1), >= n], the draft's (None when R == 1); draft: int32 [groups, R - 1]; seed: int64 [groups] holding
    the uint64 bits; t0: int32 [groups], the step of each group's row 0.  Returns (n_accept int32 [groups], token int64 [groups],
    logprob fp32 [groups]): the drafts accepted, the token drawn after them (-1: an unusable row) and its log-probability under the
    target's row."""
    _chk(p, torch.float32), _chk(seed, torch.int64), _chk(t0, torch.int32)
    groups = seed.numel()
    assert p.dim() == 2 and p.stride(1) == 1 and groups > 0 and p.shape[0] % groups == 0 and 0 < n <= min(p.shape[1], LOGITS_PROCESS_MAX_N)
    R = p.shape[0] // groups
    assert 1 <= R <= SPEC_MAX_R and seed.is_contiguous() and t0.is_contiguous() and t0.numel() == groups
    ld_q = 0
    if R > 1:
        _chk(q, torch.float32), _chk(draft, torch.int32)
        assert q.dim() == 2 and q.stride(1) == 1 and q.shape[0] == groups * (R - 1) and q.shape[1] >= n
        assert draft.is_contiguous() and draft.numel() == groups * (R - 1)
        ld_q = q.stride(0)
    else:
        q = draft = None
    ws = spec_accept_workspace(groups, R, p.device) if ws is None else ws
    _chk(ws, torch.int64)
    assert ws.is_contiguous() and ws.numel() * 8 >= lib.load().rv_spec_ws_bytes(groups, R)
    n_accept = torch.empty(groups, dtype=torch.int32, device=p.device)
    token = torch.empty(groups, dtype=torch.int64, device=p.device)
    logprob = torch.empty(groups, dtype=torch.float32, device=p.device)
    lib.call("rv_spec_accept_rows_f32", p, p.stride(0), q, ld_q, draft, seed, t0, groups, R, int(n), n_accept, token, logprob, ws,
             ws.numel() * 8)
    return n_accept, token, logprob


def attn_decode_beam(q, cache, kv_len, prefix_row, prefix_len, tail_src, H, Hkv, hd, v_off, tail_cols=None, out=None, chunk=128, scale=None):
    """attn_decode for beams that share cache rows (rv_attn_decode_beam_bf16): query row r reads key position j from cache row
    prefix_row[r] while j < prefix_len[r], else from tail_src[r, j - prefix_len[r]] (int32 device tensors: [rows], [rows], [rows, >=
    tail_cols]; tail_src None or tail_cols 0: no tail).  q [rows, H*hd]; cache bf16 [cache_rows, L_max, width]; kv_len int32 [rows].
    Bit-identical to attn_decode on the gathered cache.  Returns bf16 [rows, H*hd]."""
    _chk(q), _chk(cache), _chk(kv_len, torch.int32), _chk(prefix_row, torch.int32), _chk(prefix_len, torch.int32)
    cache_rows, L_max, width = cache.shape
    rows = q.shape[0]
    assert q.shape == (rows, H * hd) and q.stride(1) == 1 and cache.is_contiguous()
    for a in (kv_len, prefix_row, prefix_len):
        assert a.dim() == 1 and a.numel() == rows and a.is_contiguous()
    ld_t = 0
    if tail_src is None:
        tail_cols = 0
    else:
        _chk(tail_src, torch.int32)
        assert tail_src.dim() == 2 and tail_src.shape[0] == rows and tail_src.stride(1) == 1
        tail_cols = tail_src.shape[1] if tail_cols is None else int(tail_cols)
        assert 0 <= tail_cols <= tail_src.shape[1]
        ld_t = tail_src.stride(0)
    out, part, part_bytes, scale = _attn_split_args(q, rows, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_decode_beam_bf16", q, q.stride(0), cache, width, L_max * width, v_off, kv_len, L_max, prefix_row, prefix_len,
             tail_src if tail_cols else None, ld_t, tail_cols, cache_rows, out, out.stride(0), part, part_bytes, rows, H, Hkv, hd, chunk,
             scale)
    return out


VERIFY_MAX_R = 32         # query rows per sequence of attn_decode_verify (rv_attn_decode_verify_bf16)


def attn_decode_verify(q, cache, kv_len0, R, H, Hkv, hd, v_off, out=None, chunk=128, scale=None):
    """attn_decode for R consecutive query rows per sequence (rv_attn_decode_verify_bf16): q [B * R, H*hd] rows, row b * R + i attends
    the keys [0, min(kv_len0[b] + i, L_max)) of cache row b (bf16 [B, L_max, width], as attn_decode); kv_len0 int32 [B] (device).  Each
    K / V fragment is read once for a group of rows.  Every row is bit-identical to attn_decode on that row alone with
    kv_len = kv_len0[b] + i.  Returns bf16 [B * R, H*hd]."""
    _chk(q), _chk(cache), _chk(kv_len0, torch.int32)
    B, L_max, width = cache.shape
    R = int(R)
    assert q.shape == (B * R, H * hd) and q.stride(1) == 1 and cache.is_contiguous() and kv_len0.numel() == B and kv_len0.is_contiguous()
    out, part, part_bytes, scale = _attn_split_args(q, B * R, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_decode_verify_bf16", q, q.stride(0), cache, width, L_max * width, v_off, kv_len0, L_max, out, out.stride(0), part,
             part_bytes, B, R, H, Hkv, hd, chunk, scale)
    return out


SHARED_TILE_COLS = 16     # columns of attn_decode_shared's tile table: 16 / G rows of them are read (rv_attn_decode_shared_bf16)


def shared_tiles_upload(c0, tile, rows_per_tile, device):
    """The device copies of a shared-prefix tile table (generation.shared_tiles: c0 int32 [S], tile int32 [S, 16]), validated by
    generation.check_shared_tiles first (ValueError for a table attn_decode_shared must not see).  Returns a namespace with .c0 / .tile
    (device int32) and .c0_host / .tile_host: what decode_step(shared=) and attn_decode_shared take, uploaded once per change of the
    active set, not per step."""
    from types import SimpleNamespace
    from .generation import check_shared_tiles
    c0 = np.ascontiguousarray(c0, dtype=np.int32)
    tile = np.ascontiguousarray(tile, dtype=np.int32)
    check_shared_tiles(c0, tile, rows_per_tile)
    return SimpleNamespace(c0=torch.from_numpy(c0).to(device), tile=torch.from_numpy(tile).to(device), c0_host=c0, tile_host=tile,
                           rows_per_tile=int(rows_per_tile))


def attn_decode_shared(q, cache, kv_len, c0, tile, H, Hkv, hd, v_off, out=None, chunk=128, scale=None):
    """attn_decode for rows grouped in tiles that hold equal K|V at their first c0 * chunk positions (rv_attn_decode_shared_bf16): c0
    int32 [B] and tile int32 [B, 16] device tensors from shared_tiles_upload (a table for 16 // (H // Hkv) rows per tile); a tile's
    shared chunks are read once, from its first row.  Bit-identical to attn_decode on the same cache when the tiles' rows really hold
    equal K|V there and at least c0 * chunk keys each.  Returns bf16 [B, H*hd]."""
    _chk(q), _chk(cache), _chk(kv_len, torch.int32), _chk(c0, torch.int32), _chk(tile, torch.int32)
    B, L_max, width = cache.shape
    assert q.shape == (B, H * hd) and q.stride(1) == 1 and cache.is_contiguous() and kv_len.numel() == B and kv_len.is_contiguous()
    assert c0.shape == (B,) and c0.is_contiguous() and tile.shape == (B, SHARED_TILE_COLS) and tile.is_contiguous()
    out, part, part_bytes, scale = _attn_split_args(q, B, H, hd, L_max, out, chunk, scale)
    lib.call("rv_attn_decode_shared_bf16", q, q.stride(0), cache, width, L_max * width, v_off, kv_len, c0, tile, L_max, out, out.stride(0),
             part, part_bytes, B, H, Hkv, hd, chunk, scale)
    return out


def log_softmax_rows(x, n):
    """In place: x[r, :n] <- log_softmax(x[r, :n]) for every fp32 row (rv_log_softmax_rows_f32); columns >= n are not touched."""
    _chk(x, torch.float32)
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    lib.call("rv_log_softmax_rows_f32", x, x.stride(0), x.shape[0], int(n))
    return x


# rv_cfg_guide_rows_f32's launch structure: "split" (row statistics, then an elementwise launch over many workgroups) or "pair" (one
# launch, one workgroup per row pair).  The two give the same bits; DESIGN.md 5b "Classifier-free guidance" holds their A/B.
CFG_GUIDE_ROUTE = "split"


def cfg_guide_workspace(rows, device):
    """Scratch for cfg_guide_rows' two-launch form at up to `rows` rows (fp32, never zeroed); calls that share it run on one stream."""
    return torch.empty(max(lib.load().rv_cfg_guide_ws_bytes(int(rows)) // 4, 1), dtype=torch.float32, device=device)


def cfg_guide_rows(c, u, n, g, ws=None, route=None):
    """Classifier-free guidance in place (rv_cfg_guide_rows_f32): c[r, :n] <- g * (log_softmax(c[r, :n]) - log_softmax(u[r, :n])) +
    log_softmax(u[r, :n]) for every fp32 row pair, the log-softmax values being log_softmax_rows' bits and the three operations rounded
    separately in that order (HF's expression).  u is only read; columns >= n of both are not touched; c and u must not overlap.
    route: None (CFG_GUIDE_ROUTE), "split" or "pair"; ws: cfg_guide_workspace(>= rows) for "split" (allocated when missing).  Returns c."""
    _chk(c, torch.float32), _chk(u, torch.float32)
    rows = c.shape[0]
    assert c.dim() == 2 and u.dim() == 2 and u.shape[0] == rows and rows >= 1 and c.stride(1) == 1 and u.stride(1) == 1
    assert 0 < n <= min(c.shape[1], u.shape[1], LOGITS_PROCESS_MAX_N)
    route = CFG_GUIDE_ROUTE if route is None else route
    assert route in ("split", "pair")
    if route == "pair":
        ws, ws_bytes = None, 0
    else:
        ws = cfg_guide_workspace(rows, c.device) if ws is None else ws
        _chk(ws, torch.float32)
        assert ws.is_contiguous() and ws.numel() * 4 >= lib.load().rv_cfg_guide_ws_bytes(rows)
        ws_bytes = ws.numel() * 4
    lib.call("rv_cfg_guide_rows_f32", c, c.stride(0), u, u.stride(0), rows, int(n), float(g), ws, ws_bytes)
    return c


DOLA_MAX_LAYERS = 16      # candidate layers per call (rv_dola_contrast_rows_f32)
DOLA_RELATIVE_TOP = 0.1   # HF's relative_top, fixed
DOLA_LOG_RT = float(np.float32(math.log(DOLA_RELATIVE_TOP)))        # fl32(ln relative_top): the float64 logarithm, rounded once


def dola_workspace(rows, n_layers, device):
    """Scratch for dola_contrast_rows at up to `rows` rows and `n_layers` candidates (fp64, never zeroed); calls that share it run on one
    stream."""
    return torch.empty(max(lib.load().rv_dola_ws_bytes(int(rows), int(n_layers)) // 8, 1), dtype=torch.float64, device=device)


def dola_contrast_rows(f, c, n, ws=None, want_jsd=False):
    """DoLa's layer choice, relative-top filter and contrast in place (rv_dola_contrast_rows_f32).  f: fp32 [rows, >= n], the last
    layer's raw logits; c: fp32 [n_layers, rows, >= n], the candidate layers' raw logits (only read, not overlapping f).  Per row the
    candidate with the largest Jensen-Shannon divergence from f's distribution is chosen (ties: the lower index; n_layers == 1: that
    one, no divergence computed) and f[r, :n] <- log_softmax(f) - log_softmax(c[chosen]) where log_softmax(f) >= max + ln 0.1, -inf
    elsewhere, on log_softmax_rows' bits with one rounding.  Columns >= n are not touched.  ws: dola_workspace(>= rows, n_layers)
    (allocated when missing).  Returns (f, chosen int32 [rows]) and with want_jsd also the divergences fp32 [rows, n_layers]."""
    _chk(f, torch.float32), _chk(c, torch.float32)
    assert f.dim() == 2 and c.dim() == 3 and f.stride(1) == 1 and c.stride(2) == 1
    rows, nl = f.shape[0], c.shape[0]
    assert rows >= 1 and c.shape[1] == rows and 1 <= nl <= DOLA_MAX_LAYERS
    assert 0 < n <= min(f.shape[1], c.shape[2], LOGITS_PROCESS_MAX_N)
    need = lib.load().rv_dola_ws_bytes(rows, nl)
    ws = dola_workspace(rows, nl, f.device) if ws is None else ws
    _chk(ws, torch.float64)
    assert ws.is_contiguous() and ws.numel() * 8 >= need
    chosen = torch.empty(rows, dtype=torch.int32, device=f.device)
    jsd = torch.empty(rows, nl, dtype=torch.float32, device=f.device) if want_jsd else None
    lib.call("rv_dola_contrast_rows_f32", f, f.stride(0), c, c.stride(1), c.stride(0), rows, nl, int(n), DOLA_LOG_RT, chosen, jsd, ws,
             ws.numel() * 8)
    return (f, chosen, jsd) if want_jsd else (f, chosen)


CONSTRAIN_TILE = 1024     # columns per sweep step of rv_constrain_rows_f32's workgroup (csrc/constrain.hip: CR_SWEEP)


def constrain_rows(x, n, state, tables, tok=None, slot=None):
    """Constrained decoding's advance and mask in place (rv_constrain_rows_f32).  x: fp32 [rows, >= n], a step's raw logits; state:
    int32 [state_rows], one automaton state per row, or per cache slot with slot= (int32 [rows], distinct: row r uses state[slot[r]]);
    tables: (edge_off int32 [n_states + 1], edge_tok int32 [n_edges], edge_next int32 [n_edges]) on the device
    (constraints.TokenConstraint.device_tables).  tok (int64 [rows], the token chosen from each row's previous step): a live state
    first takes that token's edge (-2 when it has none) and is written back; None: the states are used as they are.  Then a free row
    (-1) is not accessed, a dead row (-2, or a number outside [0, n_states)) becomes -inf, and a live row gets -inf on every column of
    [0, n) its state does not allow, the allowed columns keeping their bits.  Columns >= n are not touched.  Returns x."""
    _chk(x, torch.float32), _chk(state, torch.int32)
    off, etok, enext = tables
    for a in (off, etok, enext):
        _chk(a, torch.int32)
        assert a.dim() == 1 and a.is_contiguous()
    rows, n_states, n_edges = x.shape[0], off.numel() - 1, etok.numel()
    assert x.dim() == 2 and x.stride(1) == 1 and rows >= 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    assert n_states >= 1 and n_edges >= 1 and enext.numel() == n_edges
    assert state.dim() == 1 and state.is_contiguous() and state.numel() >= 1
    if slot is None:
        assert rows <= state.numel()
    else:
        _chk(slot, torch.int32)
        assert slot.dim() == 1 and slot.numel() == rows and slot.is_contiguous()
    if tok is not None:
        _chk(tok, torch.int64)
        assert tok.dim() == 1 and tok.numel() == rows and tok.is_contiguous()
    lib.call("rv_constrain_rows_f32", x, x.stride(0), rows, int(n), state, state.numel(), slot, tok, off, etok, enext, n_states, n_edges)
    return x


BEAM_MAX = 16             # beams per prompt (rv_beam_topk_f32)
BEAM_TOPK_MAX = 64        # candidates kept per prompt and step


def beam_topk_workspace(groups, nb, n, K, device):
    """Scratch for beam_topk at these sizes (int64, never zeroed); calls that share it must run on one stream."""
    return torch.empty(max(lib.load().rv_beam_topk_ws_bytes(int(groups), int(nb), int(n), int(K)) // 8, 1), dtype=torch.int64, device=device)


def beam_topk(x, n, nb, score, K, out=None, ws=None):
    """The K best of each prompt's nb * n candidates x[g * nb + r, i] + score[g * nb + r] (rv_beam_topk_f32): x fp32 [groups * nb, >= n],
    score fp32 [groups * nb].  Returns one int32 tensor [2, groups, K]: [0] holds the fp32 values' bits (view(torch.float32)), [1] the
    flat indices r * n + i; value descending, then index ascending.  One tensor, so one copy brings both to the host."""
    _chk(x, torch.float32), _chk(score, torch.float32)
    rows = x.shape[0]
    assert x.dim() == 2 and x.stride(1) == 1 and 0 < n <= min(x.shape[1], LOGITS_PROCESS_MAX_N)
    assert 1 <= nb <= BEAM_MAX and rows % nb == 0 and score.numel() == rows and score.is_contiguous()
    groups = rows // nb
    assert 1 <= K <= min(BEAM_TOPK_MAX, nb * n)
    out = torch.empty(2, groups, K, dtype=torch.int32, device=x.device) if out is None else out
    _chk(out, torch.int32)
    assert tuple(out.shape) == (2, groups, K) and out.is_contiguous()
    ws = beam_topk_workspace(groups, nb, n, K, x.device) if ws is None else ws
    _chk(ws, torch.int64)
    assert ws.is_contiguous() and ws.numel() * 8 >= lib.load().rv_beam_topk_ws_bytes(groups, nb, int(n), int(K))
    lib.call("rv_beam_topk_f32", x, x.stride(0), groups, int(nb), int(n), score, int(K), out[0], out[1], ws, ws.numel() * 8)
    return out


def lora_merge(w, A, B, scale):
    """In place: w[N,K] <- bf16(w + scale * B[N,r] @ A[r,K]) (rv_lora_merge_bf16: fp32 sum in a fixed order, one rounding).  w may be a
    row slice of a fused store (any row stride); r <= 256.  Returns w."""
    _chk(w), _chk(A), _chk(B)
    N, K = w.shape
    r = A.shape[0]
    assert A.dim() == 2 and B.dim() == 2 and A.shape[1] == K and tuple(B.shape) == (N, r), (tuple(w.shape), tuple(A.shape), tuple(B.shape))
    assert w.stride(1) == 1 and A.stride(1) == 1 and B.stride(1) == 1
    lib.call("rv_lora_merge_bf16", w, w.stride(0), B, B.stride(0), A, A.stride(0), N, K, r, float(scale))
    return w

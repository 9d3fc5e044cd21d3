"""GPU tests of the live-adapter decode kernels : rv_lora_down_rows_bf16 (radvlm_amd/csrc/lora_decode.hip) and rv_gemv_lora_bf16 (gemv.hip).
P1  with B = 0 the fused kernel gives rv_gemv_bf16's bits;  P2  a row's bits do not depend on M (both kernels);
P3  both against a float64 product of the bf16 inputs, test_gemv_matches_fp32_matmul's gate;  P4  bad arguments launch nothing.
The shapes are the smallest at which each mechanism can go wrong:
  N    K     r   modules                         what it exercises
  192  96    8   three, one per 64-column block  three K steps over four waves leave wave 0 -- the adapter's wave -- empty; partial adapter step
  72   40    40  one                             ragged last column block, K % 32 != 0, one full and one partial adapter step, bias and residual
  64   512   16  one                             gemv_split = 2
  128  1024  64  two                             gemv_split = 4, residual
  128  2048  64  two                             gemv_split = 8, residual
(rv_gemv_split doubles while every wave keeps two K steps: 64 steps / (4 waves * 2) = 8 at K = 2048, 4 at K = 1024.)"""
import pytest
import torch

from test_decode_kernels_gpu import _bf16_ulp

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
MS = (1, 3, 16, 17, 32)
# (N, K, r, module column ranges, bias, residual, rv_gemv_split(N, K))
SHAPES = [(192, 96, 8, ((0, 64), (64, 128), (128, 192)), False, False, 1),
          (72, 40, 40, ((0, 72),), True, True, 1),
          (64, 512, 16, ((0, 64),), False, False, 2),
          (128, 1024, 64, ((0, 64), (64, 128)), False, True, 4),
          (128, 2048, 64, ((0, 64), (64, 128)), False, True, 8)]
IDS = [f"N{s[0]}-K{s[1]}-r{s[2]}" for s in SHAPES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _case(N, K, r, cols, has_bias, has_res, zero_b=False):
    """bf16 host tensors of one shape: x [32, K], w [N, K], t [32, n r], the modules' B_j, bias, residual."""
    g = torch.Generator().manual_seed(N * 7 + K + r)
    x = torch.randn(32, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    t = torch.randn(32, len(cols) * r, generator=g).to(BF16)
    bs = [(torch.zeros(c1 - c0, r) if zero_b else torch.randn(c1 - c0, r, generator=g) * 0.05).to(BF16) for c0, c1 in cols]
    bias = (torch.randn(N, generator=g) * 0.02).to(BF16) if has_bias else None
    res = torch.randn(32, N, generator=g).to(BF16) if has_res else None
    return x, w, t, bs, bias, res


def _mods(cols, r, bs):
    return [(c0, c1, j * r, b) for j, ((c0, c1), b) in enumerate(zip(cols, bs))]


def _dev(*ts):
    return [None if t is None else ([u.cuda() for u in t] if isinstance(t, list) else t.cuda()) for t in ts]


@pytest.mark.parametrize("N,K,r,cols,has_bias,has_res,split", SHAPES, ids=IDS)
def test_zero_b_gives_the_bits_of_gemv(N, K, r, cols, has_bias, has_res, split):
    """P1."""
    _need_gpu()
    from radvlm_amd import ops
    assert ops.gemv_split(N, K) == split
    x, w, t, bs, bias, res = _dev(*_case(N, K, r, cols, has_bias, has_res, zero_b=True))
    assert float(t.float().abs().max()) > 0
    for M in MS:
        rm = None if res is None else res[:M]
        y = ops.gemv_lora(x[:M], w, t[:M], _mods(cols, r, bs), bias=bias, residual=rm)
        assert torch.equal(y, ops.gemv(x[:M], w, bias=bias, residual=rm)), M


@pytest.mark.parametrize("N,K,r,cols,has_bias,has_res,split", SHAPES, ids=IDS)
def test_rows_do_not_depend_on_m(N, K, r, cols, has_bias, has_res, split):
    """P2, both kernels: every row of an M-row launch against its one-row launch."""
    _need_gpu()
    from radvlm_amd import ops
    x, w, t, bs, bias, res = _dev(*_case(N, K, r, cols, has_bias, has_res))
    g = torch.Generator().manual_seed(K + r)
    adapters = [(torch.randn(r, K, generator=g) * 0.05).to(BF16).cuda() for _ in range(3)]
    mods = _mods(cols, r, bs)
    one_y = [ops.gemv_lora(x[m:m + 1], w, t[m:m + 1], mods, bias=bias, residual=None if res is None else res[m:m + 1])[0] for m in range(32)]
    one_t = {n: [ops.lora_down_rows(x[m:m + 1], adapters[:n], 2.0)[0] for m in range(32)] for n in (1, 2, 3)}
    for M in MS:
        y = ops.gemv_lora(x[:M], w, t[:M], mods, bias=bias, residual=None if res is None else res[:M])
        for m in range(M):
            assert torch.equal(y[m], one_y[m]), ("gemv_lora", M, m)
        for n in (1, 2, 3):
            tt = ops.lora_down_rows(x[:M], adapters[:n], 2.0)
            for m in range(M):
                assert torch.equal(tt[m], one_t[n][m]), ("lora_down_rows", n, M, m)


@pytest.mark.parametrize("N,K,r,cols,has_bias,has_res,split", SHAPES, ids=IDS)
def test_gemv_lora_matches_float64(N, K, r, cols, has_bias, has_res, split):
    """P3, fused kernel: |y - ref| <= ulp_bf16(ref) + 1e-5 (sum |x||w| + sum |t||b|); T is a given bf16 input."""
    _need_gpu()
    from radvlm_amd import ops
    assert ops.gemv_split(N, K) == split
    host = _case(N, K, r, cols, has_bias, has_res)
    x, w, t, bs, bias, res = host
    xd, wd, td, bd, biasd, resd = _dev(*host)
    ref = x.double() @ w.double().t()
    scale = x.double().abs() @ w.double().abs().t()
    for j, ((c0, c1), b) in enumerate(zip(cols, bs)):
        tj = t[:, j * r:(j + 1) * r].double()
        ref[:, c0:c1] += tj @ b.double().t()
        scale[:, c0:c1] += tj.abs() @ b.double().abs().t()
    ref = ref + (bias.double() if bias is not None else 0.0) + (res.double() if res is not None else 0.0)
    worst = 0.0
    for M in MS:
        y = ops.gemv_lora(xd[:M], wd, td[:M], _mods(cols, r, bd), bias=biasd, residual=None if resd is None else resd[:M]).double().cpu()
        err, ulp = (y - ref[:M]).abs(), _bf16_ulp(ref[:M])
        worst = max(worst, float((err / ulp).max()))
        assert float((err - (ulp + 1e-5 * scale[:M])).max()) <= 0, (M, float((err / ulp).max()))
    from conftest import record_measurement
    record_measurement("gemv_lora_bf16", N=N, K=K, r=r, modules=len(cols), split=split, max_err_in_ulps=worst)


@pytest.mark.parametrize("N,K,r,cols,has_bias,has_res,split", SHAPES, ids=IDS)
def test_lora_down_rows_matches_float64(N, K, r, cols, has_bias, has_res, split):
    """P3, down kernel at the same (K, r) with 1, 2 and 3 modules: |t - ref| <= ulp_bf16(ref) + 1e-5 |scale| sum |x||a|."""
    _need_gpu()
    from radvlm_amd import ops
    g = torch.Generator().manual_seed(K * 3 + r)
    x = torch.randn(32, K, generator=g).to(BF16)
    adapters = [(torch.randn(r, K, generator=g) * 0.05).to(BF16) for _ in range(3)]
    s = 16.0 / r
    xd, ad = x.cuda(), [a.cuda() for a in adapters]
    worst = 0.0
    for n in (1, 2, 3):
        a = torch.cat(adapters[:n], 0).double()
        ref = s * (x.double() @ a.t())
        scale = abs(s) * (x.double().abs() @ a.abs().t())
        for M in MS:
            t = ops.lora_down_rows(xd[:M], ad[:n], s)
            assert t.shape == (M, n * r)
            err, ulp = (t.double().cpu() - ref[:M]).abs(), _bf16_ulp(ref[:M])
            worst = max(worst, float((err / ulp).max()))
            assert float((err - (ulp + 1e-5 * scale[:M])).max()) <= 0, (n, M, float((err / ulp).max()))
    from conftest import record_measurement
    record_measurement("lora_down_rows_bf16", K=K, r=r, split=ops.lora_down_split(r, K), max_err_in_ulps=worst)


def test_bad_arguments_launch_nothing():
    """P4: RV_ERR_ARG, and the output keeps the value it had."""
    _need_gpu()
    from radvlm_amd import lib, ops
    dev = "cuda"
    K, N = 512, 128
    buf = torch.randn(33 * K + 8, device=dev).to(BF16)
    x = buf[:33 * K].view(33, K)
    w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
    ws = ops.default_workspace(torch.device(dev))
    wsb = ws.numel() * 4
    assert ops.gemv_split(N, K) > 1 and ops.lora_down_split(16, K) > 1

    def fused(M=4, r=16, c=(0, 64, 64, 128), xx=None, workspace=ws, ws_bytes=wsb, tt=None, b_off=0):
        t = torch.randn(33, 2 * 72, device=dev).to(BF16) if tt is None else tt
        bb = torch.randn(64 * 72 + 8, device=dev).to(BF16)
        b = bb[b_off:b_off + 64 * r].view(64, r)
        y = torch.full((33, N), 7.0, dtype=BF16, device=dev)
        xx = x if xx is None else xx
        with pytest.raises(lib.RadvlmHipError, match="code -1"):
            lib.call("rv_gemv_lora_bf16", xx, xx.stride(0), w, K, t, t.stride(0), r, 2, b, c[0], c[1], 0, b, c[2], c[3], r, None, 0, 0, 0, r,
                     y, N, None, None, 0, M, N, K, workspace, ws_bytes)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())

    def down(M=4, r=16, xx=None, workspace=ws, ws_bytes=wsb, a_off=0):
        aa = torch.randn(72 * K + 8, device=dev).to(BF16)
        a = aa[a_off:a_off + r * K].view(r, K)
        t = torch.full((33, 2 * r), 7.0, dtype=BF16, device=dev)
        xx = x if xx is None else xx
        with pytest.raises(lib.RadvlmHipError, match="code -1"):
            lib.call("rv_lora_down_rows_bf16", xx, xx.stride(0), a, a, None, K, 2, t, 2 * r, M, r, K, 1.0, workspace, ws_bytes)
        torch.cuda.synchronize()
        assert bool((t == 7.0).all())

    misaligned_x = buf[4:4 + 32 * K].view(32, K)                     # 8 bytes off a 16-byte boundary
    fused(c=(0, 32, 32, 128))                                        # a module boundary that is no multiple of 64
    fused(c=(0, 64, 96, 128))
    for kernel in (fused, down):
        kernel(r=12)
        kernel(r=72)
        kernel(M=33)
        kernel(M=4, xx=misaligned_x)
        kernel(workspace=None, ws_bytes=0)                           # split > 1 needs the workspace
        kernel(ws_bytes=64)
    fused(b_off=4)
    down(a_off=4)
    # and the same calls with good arguments succeed
    t = torch.randn(4, 32, device=dev).to(BF16)
    b = torch.zeros(64, 16, dtype=BF16, device=dev)
    y = ops.gemv_lora(x[:4], w, t, [(0, 64, 0, b), (64, 128, 16, b)])
    assert torch.equal(y, ops.gemv(x[:4], w))

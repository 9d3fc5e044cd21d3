"""GPU tests of rv_cfg_guide_rows_f32 on bare rows: bit-exact against rv_log_softmax_rows_f32 composed with the three separately
rounded operations (tests/cfg_ref.py, pinned to HF's processor by tests/test_cfg_host.py), both launch structures, guard columns and
strides, launch independence, the derived error bound against a float64 run of HF's processor, and the argument refusals."""
import numpy as np
import pytest
import torch

import cfg_ref
from cfg_ref import G_LIST, bits, combine

pytestmark = pytest.mark.gpu
ROUTES = ("split", "pair")
GUARD_C, GUARD_U = 5, 11


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _lsm(x, n):
    """rv_log_softmax_rows_f32 on a copy."""
    from radvlm_amd import ops
    return ops.log_softmax_rows(x[:, :n].clone(), n)


def _setup(c, u):
    """c, u numpy [rows, n] -> device tensors with different leading dimensions, guard columns, and u a slice of a taller tensor."""
    rows, n = c.shape
    cd = torch.full((rows, n + GUARD_C), 123.25, dtype=torch.float32, device="cuda")
    ud = torch.full((rows + 3, n + GUARD_U), -77.5, dtype=torch.float32, device="cuda")
    cd[:, :n] = torch.from_numpy(c).cuda()
    ud[2:2 + rows, :n] = torch.from_numpy(u).cuda()
    return cd, ud, ud[2:2 + rows]


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 32000, 152064])
@pytest.mark.parametrize("rows", [1, 3, 32])
def test_bit_exact_composition(n, rows):
    _need_gpu()
    from radvlm_amd import ops
    rng = np.random.default_rng(1000 * rows + n)
    for kind in ("flat", "peaked"):
        c, u = cfg_ref.logits_rows(rng, rows, n, kind), cfg_ref.logits_rows(rng, rows, n, kind)
        cd, ud, uv = _setup(c, u)
        u_before = ud.clone()
        lc, lu = _lsm(cd, n), _lsm(uv, n)
        lc_h, lu_h = lc.cpu().numpy(), lu.cpu().numpy()
        for g in G_LIST:
            want = (lc - lu).mul_(float(g)).add_(lu)                    # the same three torch operations, on the device
            if n <= 32000:
                assert np.array_equal(bits(want.cpu().numpy()), bits(combine(lc_h, lu_h, g))), (kind, g)
            for route in ROUTES:
                x = cd.clone()
                out = ops.cfg_guide_rows(x[:, :n], uv[:, :n], n, g, route=route)
                assert out.data_ptr() == x.data_ptr()
                assert torch.equal(x[:, :n].view(torch.int32), want.view(torch.int32)), (kind, g, route)
                assert torch.equal(x[:, n:], cd[:, n:])                # c's guard columns keep their bits
                assert torch.equal(ud.view(torch.int32), u_before.view(torch.int32))       # u, its guard columns and the rows around it


def test_contraction_is_visible():
    """g = 1/3 on random rows: fl(g * d) needs rounding almost everywhere, so a kernel that contracted g * d + lu into one fma would
    differ from HF's two roundings; the kernel equals the two-rounding result and differs from the one-rounding one."""
    _need_gpu()
    from radvlm_amd import ops
    rng = np.random.default_rng(7)
    n = 32000
    c, u = cfg_ref.logits_rows(rng, 2, n, "flat"), cfg_ref.logits_rows(rng, 2, n, "flat")
    cd, ud = torch.from_numpy(c).cuda(), torch.from_numpy(u).cuda()
    lc, lu = _lsm(cd, n).cpu().numpy(), _lsm(ud, n).cpu().numpy()
    d = lc - lu
    fma = (np.float64(np.float32(1 / 3)) * d.astype(np.float64) + lu.astype(np.float64)).astype(np.float32)
    two = combine(lc, lu, 1 / 3)
    assert not np.array_equal(bits(fma), bits(two))
    for route in ROUTES:
        got = ops.cfg_guide_rows(cd.clone(), ud, n, 1 / 3, route=route).cpu().numpy()
        assert np.array_equal(bits(got), bits(two)) and not np.array_equal(bits(got), bits(fma))


@pytest.mark.parametrize("n", [257, 32000])
def test_equal_rows_give_the_log_softmax(n):
    _need_gpu()
    from radvlm_amd import ops
    rng = np.random.default_rng(n)
    for kind in ("flat", "peaked"):
        c = torch.from_numpy(cfg_ref.logits_rows(rng, 3, n, kind)).cuda()
        want = _lsm(c, n)
        for g in G_LIST + (1, 1e6, -1e6):
            for route in ROUTES:
                assert torch.equal(ops.cfg_guide_rows(c.clone(), c.clone(), n, g, route=route), want), (kind, g, route)


@pytest.mark.parametrize("n", [1000, 152064])
def test_row_bits_do_not_depend_on_the_launch(n):
    _need_gpu()
    from radvlm_amd import ops
    rng = np.random.default_rng(n + 1)
    c = torch.from_numpy(cfg_ref.logits_rows(rng, 32, n, "peaked")).cuda()
    u = torch.from_numpy(cfg_ref.logits_rows(rng, 32, n, "flat")).cuda()
    full = {route: ops.cfg_guide_rows(c.clone(), u, n, 1.5, route=route) for route in ROUTES}
    assert torch.equal(full["split"].view(torch.int32), full["pair"].view(torch.int32))
    for r in (0, 13, 31):
        for route in ROUTES:
            one = ops.cfg_guide_rows(c[r:r + 1].clone(), u[r:r + 1], n, 1.5, route=route)
            assert torch.equal(one[0].view(torch.int32), full[route][r].view(torch.int32)), (r, route)
    # other rows holding something else do not change a row either
    c2, u2 = c.clone(), u.clone()
    c2[1:] = 0.0
    u2[1:] = 5.0
    assert torch.equal(ops.cfg_guide_rows(c2, u2, n, 1.5)[0].view(torch.int32), full["split"][0].view(torch.int32))


@pytest.mark.parametrize("n", [1000, 32000, 152064])
def test_within_the_derived_bound_of_float64(n):
    """|kernel - float64 HF| <= the bound csrc/cfg.hip derives (cfg_ref.error_bound), per entry.  The float64 run of HF's processor uses
    the caller's g unrounded, so the rounding of g to fp32 is part of what is measured."""
    _need_gpu()
    import torch as _t
    from conftest import record_measurement
    from radvlm_amd import ops
    rng = np.random.default_rng(n + 2)
    rows = 4
    worst = {}
    for kind in ("flat", "peaked"):
        c, u = cfg_ref.logits_rows(rng, rows, n, kind), cfg_ref.logits_rows(rng, rows, n, kind)
        c[0, :] = 0.0                                                   # a flat row: log(1 / n)
        u[1, 3] = 60.0                                                  # a peaked unconditional row
        cd, ud = torch.from_numpy(c).cuda(), torch.from_numpy(u).cuda()
        lc64, lu64 = cfg_ref.log_softmax64(c), cfg_ref.log_softmax64(u)
        for g in G_LIST:
            got = ops.cfg_guide_rows(cd.clone(), ud, n, g).cpu().numpy().astype(np.float64)
            ref = cfg_ref.hf_guided(c, u, g, _t.float64).numpy()
            bound = cfg_ref.error_bound(lc64, lu64, g, n)
            ratio = float((np.abs(got - ref) / bound).max())
            worst[f"{kind}_g{g:.3g}"] = ratio
            print(f"cfg_guide n={n} {kind} g={g:.4g}: worst |err| / bound = {ratio:.4f}, max |err| = {float(np.abs(got - ref).max()):.3e}")
    record_measurement("cfg_guide", n=n, worst_ratio_to_bound=max(worst.values()), **worst)
    assert max(worst.values()) <= 1.0, worst


def test_bad_arguments_are_refused():
    _need_gpu()
    from radvlm_amd import lib, ops
    c = torch.zeros(2, 64, device="cuda")
    u = torch.zeros(2, 64, device="cuda")
    ws = ops.cfg_guide_workspace(2, "cuda")
    good = lambda: [c, 64, u, 64, 2, 64, 1.5, ws, ws.numel() * 4]
    lib.call("rv_cfg_guide_rows_f32", *good())
    for i, v in ((5, 0), (5, -1), (5, ops.LOGITS_PROCESS_MAX_N + 1), (4, 0), (4, -3), (1, 63), (3, 63), (0, None), (2, None), (8, 31), (8, 0)):
        args = good()
        args[i] = v
        with pytest.raises(lib.RadvlmHipError):
            lib.call("rv_cfg_guide_rows_f32", *args)
    lib.call("rv_cfg_guide_rows_f32", c, 64, u, 64, 2, 64, 1.5, None, 0)            # no scratch: the one-launch form
    assert lib.load().rv_cfg_guide_ws_bytes(0) == 0 and lib.load().rv_cfg_guide_ws_bytes(3) == 48
    torch.cuda.synchronize()

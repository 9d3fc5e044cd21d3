"""GPU tests of radvlm_amd/csrc/adam8.hip, all exact: rv_adam8_quantize_f32 / rv_adam8_dequantize_f32 against tests/adam8_ref.py bit for
bit (its own CPU checks: tests/test_adam8_host.py), and the fused rv_adamw8 against the GPU composition dequantise -> rv_adamw -> quantise
per tensor, bit for bit on the parameter, the master copy, both code arrays and both absmax arrays.  Every buffer carries a sentinel
behind (and, between the tensors of a slice, inside) what a kernel may write."""
import numpy as np
import pytest
import torch

import adam8_ref as R

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


def _inputs(kind):
    out = dict(R.host_inputs(kind))
    r = np.random.RandomState(11 + kind)
    for n in (1, 255, 256, 257, 1027):
        x = (r.randn(n) * np.exp(2 * r.randn(n))).astype(np.float32)
        out[f"n{n}_random"] = x * x if kind == R.UNSIGNED else x
    return out


# ------------------------------------------------------------------------------------------------ quantise / dequantise
@pytest.mark.parametrize("kind", [R.SIGNED, R.UNSIGNED])
def test_quantize_and_dequantize_match_the_reference_bit_for_bit(kind):
    ops = _ops()
    for name, x in _inputs(kind).items():
        n, nb = x.size, R.nblocks(x.size)
        codes, absmax = _sent((n + 5,), U8), _sent((nb + 1,), F32)
        ops.adam8_quantize(torch.from_numpy(x).cuda(), kind, codes, absmax)
        wc, wa = R.quantize(x, kind)
        want_c, want_a = _sent((n + 5,), U8, "cpu"), _sent((nb + 1,), F32, "cpu")
        want_c[:n], want_a[:nb] = torch.from_numpy(wc), torch.from_numpy(wa)
        _same(codes, want_c, f"{name}: codes")
        _same(absmax, want_a, f"{name}: absmax")
        out = _sent((n + 1,), F32)
        ops.adam8_dequantize(codes, absmax, n, kind, out)
        want = _sent((n + 1,), F32, "cpu")
        want[:n] = torch.from_numpy(R.dequantize(wc, wa, kind))
        _same(out, want, f"{name}: dequantised")


@pytest.mark.parametrize("kind", [R.SIGNED, R.UNSIGNED])
def test_dequantize_every_code(kind):
    ops = _ops()
    codes = np.concatenate([np.arange(256), np.arange(255, -1, -1), [3]]).astype(np.uint8)
    absmax = np.array([1.0, 3.0, 2.0 ** -40], np.float32)
    out = _sent((codes.size + 1,), F32)
    ops.adam8_dequantize(torch.from_numpy(codes).cuda(), torch.from_numpy(absmax).cuda(), codes.size, kind, out)
    want = _sent((codes.size + 1,), F32, "cpu")
    want[:codes.size] = torch.from_numpy(R.dequantize(codes, absmax, kind))
    _same(out, want, "every code")


# ------------------------------------------------------------------------------------------------ the fused step
TABLES = {"one_1027": ((0, 1027),), "three_restarting": ((0, 300), (301, 5), (310, 4099))}     # (start, length): 301 and 310 are not 4-aligned
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


class _Slice:
    """One parameter-group slice with sentinels in the gaps between its tensors and behind it, and its 8-bit state."""

    def __init__(self, tensors, seed):
        self.tensors = tensors
        self.N = tensors[-1][0] + tensors[-1][1]
        nb = [R.nblocks(n) for _, n in tensors]
        self.first = [int(x) for x in np.cumsum([0] + nb[:-1])]
        self.nblocks = int(sum(nb))
        self.table = torch.tensor([[s for s, _ in tensors], [n for _, n in tensors], self.first], dtype=torch.int64).cuda()
        g = torch.Generator().manual_seed(seed)
        self.p, self.master = _sent((self.N + 8,), BF16), _sent((self.N + 8,), F32)
        for s, n in tensors:
            w = torch.randn(n, generator=g) * 0.05
            self.master[s:s + n] = w.cuda()
            self.p[s:s + n] = w.to(BF16).cuda()
        self.cm, self.cv = _sent((self.nblocks * 256 + 4,), U8), _sent((self.nblocks * 256 + 4,), U8)
        self.am, self.av = _sent((self.nblocks + 1,), F32), _sent((self.nblocks + 1,), F32)
        self.set_state(lambda n: torch.zeros(n), lambda n: torch.zeros(n))

    def set_state(self, fm, fv):
        """Quantise fm(n) / fv(n) (CPU fp32) into the state with the reference."""
        for (s, n), fb in zip(self.tensors, self.first):
            for kind, f, codes, absmax in ((0, fm, self.cm, self.am), (1, fv, self.cv, self.av)):
                c, a = R.quantize(f(n).numpy(), kind)
                codes[fb * 256:fb * 256 + n] = torch.from_numpy(c).cuda()
                absmax[fb:fb + a.size] = torch.from_numpy(a).cuda()

    def buffers(self):
        return dict(p=self.p, master=self.master, codes_m=self.cm, codes_v=self.cv, absmax_m=self.am, absmax_v=self.av)

    def clone(self):
        import copy
        c = copy.copy(self)
        c.p, c.master, c.cm, c.cv, c.am, c.av = (t.clone() for t in (self.p, self.master, self.cm, self.cv, self.am, self.av))
        return c

    def fused(self, ops, g, wd, step, gscale):
        ops.adamw8(self.p[:self.N], self.master[:self.N], g[:self.N], self.cm, self.cv, self.am, self.av, self.table, self.nblocks,
                   HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step, gscale=gscale)

    def composed(self, ops, g, wd, step, gscale):
        """Per tensor: dequantise, rv_adamw on aligned copies (its body and tail round alike, so the regrouping changes nothing), quantise."""
        for (s, n), fb in zip(self.tensors, self.first):
            cm, cv = self.cm[fb * 256:fb * 256 + n].clone(), self.cv[fb * 256:fb * 256 + n].clone()
            am, av = self.am[fb:fb + R.nblocks(n)].clone(), self.av[fb:fb + R.nblocks(n)].clone()
            m, v = ops.adam8_dequantize(cm, am, n, 0), ops.adam8_dequantize(cv, av, n, 1)
            p, master, gg = self.p[s:s + n].clone(), self.master[s:s + n].clone(), g[s:s + n].clone()
            ops.adamw(p, master, gg, m, v, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step, gscale=gscale)
            self.p[s:s + n], self.master[s:s + n] = p, master
            ops.adam8_quantize(m, 0, cm, am)
            ops.adam8_quantize(v, 1, cv, av)
            self.cm[fb * 256:fb * 256 + n], self.cv[fb * 256:fb * 256 + n] = cm, cv
            self.am[fb:fb + R.nblocks(n)], self.av[fb:fb + R.nblocks(n)] = am, av


def _grads(N, seed):
    g = torch.Generator().manual_seed(seed)
    return {"ordinary": (torch.randn(N + 8, generator=g) * torch.exp(2 * torch.randn(N + 8, generator=g)) * 1e-2).to(BF16).cuda(),
            "zero": torch.zeros(N + 8, dtype=BF16).cuda(), "2^-40": torch.full((N + 8,), 2.0 ** -40, dtype=BF16).cuda()}


def _states(sl, ops, seed):
    """fresh: the codes of 0 and absmax 0, step 1.  warm: one composed step later, step 2.  late: moments over a wide range, step 5000."""
    g = torch.Generator().manual_seed(seed)
    yield "fresh", sl.clone(), 1
    warm = sl.clone()
    warm.composed(ops, _grads(sl.N, seed + 1)["ordinary"], 0.0, 1, None)
    yield "warm", warm, 2
    late = sl.clone()
    late.set_state(lambda n: torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g)) * 1e-3,
                   lambda n: (torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g)) * 1e-3) ** 2)
    yield "late", late, 5000


@pytest.mark.parametrize("table", sorted(TABLES))
def test_adamw8_equals_dequantize_adamw_quantize(table):
    ops = _ops()
    sl = _Slice(TABLES[table], seed=5)
    grads = _grads(sl.N, 21)
    coef = torch.tensor([0.37], dtype=F32).cuda()
    cases = 0
    for sname, state, step in _states(sl, ops, 9):
        for gname, g in grads.items():
            for wd in (0.0, 0.1):
                for gscale in (None, coef):
                    a, b = state.clone(), state.clone()
                    a.fused(ops, g, wd, step, gscale)
                    b.composed(ops, g, wd, step, gscale)
                    for key, got in a.buffers().items():
                        _same(got, b.buffers()[key], f"{table} {sname} grad {gname} wd {wd} gscale {gscale is not None}: {key}")
                    if gname == "ordinary":              # the step did something: the comparison is not of two untouched buffers
                        assert not torch.equal(a.master[:300].view(torch.int32), state.master[:300].view(torch.int32))
                        assert not torch.equal(a.cm[:300], state.cm[:300])
                    cases += 1
    assert cases == 36


def test_zero_gradient_on_a_fresh_state_moves_nothing():
    ops = _ops()
    sl = _Slice(TABLES["three_restarting"], seed=6)
    before = sl.clone()
    sl.fused(ops, torch.zeros(sl.N + 8, dtype=BF16).cuda(), 0.0, 1, None)
    for key, got in sl.buffers().items():
        _same(got, before.buffers()[key], key)
    for (s, n), fb in zip(sl.tensors, sl.first):
        assert bool((sl.cm[fb * 256:fb * 256 + n] == 127).all()) and bool((sl.cv[fb * 256:fb * 256 + n] == 0).all())


def test_argument_errors_are_refused_before_launch():
    _ops()
    from radvlm_amd import lib
    sl = _Slice(TABLES["one_1027"], seed=7)
    before = sl.clone()
    g = torch.zeros(sl.N + 8, dtype=BF16).cuda()
    x = torch.ones(300, dtype=F32).cuda()
    codes, absmax = _sent((300,), U8), _sent((2,), F32)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, None)
    good = (sl.p, sl.master, g, sl.cm, sl.cv, sl.am, sl.av, sl.table, 1, sl.nblocks)
    bad_calls = [("rv_adam8_quantize_f32", (x, 0, codes, absmax, 0)), ("rv_adam8_quantize_f32", (x, 300, codes, absmax, 2)),
                 ("rv_adam8_quantize_f32", (None, 300, codes, absmax, 0)), ("rv_adam8_dequantize_f32", (codes, absmax, 300, -1, x)),
                 ("rv_adam8_dequantize_f32", (codes, None, 300, 0, x)), ("rv_adam8_dequantize_f32", (codes, absmax, 0, 0, x))]
    for i, repl in ((0, None), (1, sl.master[1:]), (2, g[1:]), (3, None), (5, None), (7, None), (8, 0), (9, 0), (3, sl.cm[1:])):
        args = list(good)
        args[i] = repl
        bad_calls.append(("rv_adamw8", tuple(args) + hyper))
    for name, args in bad_calls:
        with pytest.raises(lib.RadvlmHipError):
            lib.call(name, *args)
    torch.cuda.synchronize()
    for key, got in sl.buffers().items():
        _same(got, before.buffers()[key], key)
    assert bool((codes == 0xAB).all())

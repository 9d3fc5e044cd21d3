"""GPU tests of the decode kernels at the shapes, strides and key counts where they can go wrong (radvlm_amd/csrc/gemv.hip, decode.hip, extend.hip):
ragged K / N / M of the skinny GEMM and its int8 twin with exact integer products, needle rows that pin every key position of the
decode attention, leading dimensions other than the packed ones with guard columns, the cache append's skips and widths, the argmax's
NaN / inf / signed-zero conventions, and the argument checks.  References and input builders: tests/decode_ref.py (its own CPU checks:
tests/test_decode_ref_host.py).  Layouts the ops wrappers refuse go through the C ABI (radvlm_amd.lib.call)."""
import functools
import math

import pytest
import torch

from decode_ref import BF16, attn_decode_ref, bf16_ulp, gemv_ref, integer_operands, needle_cache

pytestmark = pytest.mark.gpu


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


def _call(name, *args):
    from radvlm_amd import lib
    lib.call(name, *args)


def _bits(t):
    """The tensor's bit patterns as integers, on the CPU (NaN sentinels compare equal to themselves this way)."""
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _sentinel(shape, dtype, device="cuda"):
    """A buffer of one NaN bit pattern (bf16 0x7fc5 / fp32 0x7fc5a5a5): a kernel cannot produce it by accident, and a read of it poisons the result."""
    if dtype == BF16:
        return torch.full(shape, 0x7fc5, dtype=torch.int16, device=device).view(BF16)
    return torch.full(shape, 0x7fc5a5a5, dtype=torch.int32, device=device).view(torch.float32)


# ------------------------------------------------------------------------------------------------ skinny GEMM
GEMV_NS = (1, 15, 16, 17, 63, 64, 65, 200)
GEMV_KS = (8, 24, 32, 40, 72, 264, 520, 1000, 2056)
GEMV_MS = (1, 15, 16, 17, 31, 32)


def _gemv_w8(ops, x, pk, K, **kw):
    return ops.gemv_w8(x, pk[0], pk[1], K, **kw)


@pytest.mark.parametrize("K", GEMV_KS)
def test_gemv_exact_integer_products(K):
    """Integer operands: every fp32 partial sum is exact, so the kernel's output is known to the bit whatever its K split, and a K group,
    a row or a column dropped, doubled or permuted shows.  Both epilogues (split 1: in the kernel; split > 1: the combine launch)."""
    ops = _ops()
    for N in GEMV_NS:
        split = ops.gemv_split(N, K)
        if K in (520, 2056):
            assert split > 1, (N, K, split)
        if K <= 264:
            assert split == 1, (N, K, split)
        x, w, bias, res = integer_operands(32, N, K, seed=1000 * N + K)
        ref0, ref1 = gemv_ref(x, w), gemv_ref(x, w, bias, res)
        assert float(ref1.abs().max()) <= 12344
        xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), res.cuda()
        # the int8 twin: quantising changes the integers (s = 3 / 127), so it is held to the bf16 kernel on the dequantised weight, bit
        # for bit, and that to the float64 product of the dequantised weight within the bound of test_gemv_matches_fp32_matmul
        wq = wd.clone()
        pk = ops.quantize_rows_w8(wq)
        wq_c = wq.cpu()
        refq = gemv_ref(x, wq_c, bias, res)
        boundq = bf16_ulp(refq) + 1e-5 * (x.double().abs() @ wq_c.double().abs().t())
        for M in GEMV_MS:
            y = ops.gemv(xd[:M], wd, out_dtype=torch.float32).cpu()
            assert torch.equal(y.double(), ref0[:M]), (N, K, M, "fp32")
            y = ops.gemv(xd[:M], wd, bias=bd, residual=rd[:M], out_dtype=torch.float32).cpu()
            assert torch.equal(y.double(), ref1[:M]), (N, K, M, "fp32 + bias + residual")
            y = ops.gemv(xd[:M], wd).cpu()
            assert torch.equal(y, ref0[:M].to(BF16)), (N, K, M, "bf16")
            y = ops.gemv(xd[:M], wd, bias=bd, residual=rd[:M]).cpu()
            assert torch.equal(y, ref1[:M].to(BF16)), (N, K, M, "bf16 + bias + residual")
            for dt in (BF16, torch.float32):
                a = ops.gemv(xd[:M], wq, bias=bd, residual=rd[:M], out_dtype=dt)
                b = _gemv_w8(ops, xd[:M], pk, K, bias=bd, residual=rd[:M], out_dtype=dt)
                assert _same_bits(a, b), (N, K, M, dt, "w8 against bf16 on the dequantised weight")
            assert _same_bits(ops.gemv(xd[:M], wq), _gemv_w8(ops, xd[:M], pk, K)), (N, K, M, "w8 against bf16, no bias")
            a16 = ops.gemv(xd[:M], wq, bias=bd, residual=rd[:M]).double().cpu()
            assert float(((a16 - refq[:M]).abs() - boundq[:M]).max()) <= 0, (N, K, M, "dequantised weight against float64")


@pytest.mark.parametrize("K", GEMV_KS)
def test_gemv_random_data_at_ragged_shapes(K):
    """Random data at the same shapes, the bound of test_gemv_matches_fp32_matmul against float64: within one bf16 ulp of the result plus
    1e-5 sum|x||w| (bf16 out), 1e-5 sum|x||w| (fp32 out)."""
    ops = _ops()
    worst = 0.0
    for N in GEMV_NS:
        g = torch.Generator().manual_seed(N * 7 + K)
        x = torch.randn(32, K, generator=g).to(BF16)
        w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
        bias = (torch.randn(N, generator=g) * 0.02).to(BF16)
        res = torch.randn(32, N, generator=g).to(BF16)
        xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), res.cuda()
        scale = x.double().abs() @ w.double().abs().t()
        ref0, ref1 = gemv_ref(x, w), gemv_ref(x, w, bias, res)
        for M in GEMV_MS:
            y = ops.gemv(xd[:M], wd, bias=bd, residual=rd[:M], out_dtype=torch.float32).double().cpu()
            err = ((y - ref1[:M]).abs() / scale[:M].clamp_min(1e-30)).max()
            assert float(err) <= 1e-5, (N, K, M, "fp32", float(err))
            for ref, kw in ((ref0, {}), (ref1, dict(bias=bd, residual=rd[:M]))):
                y = ops.gemv(xd[:M], wd, **kw).double().cpu()
                r = ref[:M]
                worst = max(worst, float(((y - r).abs() / bf16_ulp(r)).max()))
                over = (y - r).abs() - (bf16_ulp(r) + 1e-5 * scale[:M])
                assert float(over.max()) <= 0, (N, K, M, bool(kw), float(over.max()))
    from conftest import record_measurement
    record_measurement("gemv_edges", K=K, max_err_in_ulps=worst)


STRIDE_SHAPES = ((65, 40), (200, 520), (17, 2056))          # split 1, 2 and 8


@pytest.mark.parametrize("N,K", STRIDE_SHAPES)
@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "fp32"])
def test_gemv_leading_dimensions_and_guard_columns(N, K, dt):
    """x, out and residual as column slices of wider buffers, w as wide[:, :K] of an [N, K + 64] store: the same bits as the contiguous call,
    and not one element of the wide output outside the slice written."""
    ops = _ops()
    assert (ops.gemv_split(N, K) > 1) == (K >= 520)
    g = torch.Generator().manual_seed(N + K)
    for M in (1, 17, 32):
        x = torch.randn(M, K, generator=g).to(BF16).cuda()
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).cuda()
        bias = torch.randn(N, generator=g).to(BF16).cuda()
        res = torch.randn(M, N, generator=g).to(BF16).cuda()
        xw = _sentinel((M, K + 24), BF16)
        xw[:, 8:8 + K] = x
        ww = _sentinel((N, K + 64), BF16)
        ww[:, :K] = w
        rw = _sentinel((M, N + 9), BF16)
        rw[:, 5:5 + N] = res
        pk = ops.quantize_rows_w8(w.clone())                      # the packed int8 rows have one layout: x, out and residual are strided

        def run(name, xx, wx, **kw):
            return ops.gemv(xx, wx, **kw) if name == "bf16" else _gemv_w8(ops, xx, pk, K, **kw)

        for name in ("bf16", "w8"):
            want = run(name, x, w, bias=bias, residual=res, out_dtype=dt)
            assert not torch.isnan(want).any()
            ow = _sentinel((M, N + 11), dt)
            before = _bits(ow)
            run(name, xw[:, 8:8 + K], ww[:, :K], bias=bias, residual=rw[:, 5:5 + N], out=ow[:, 3:3 + N])
            assert _same_bits(ow[:, 3:3 + N], want), (name, M)
            after = _bits(ow)
            assert torch.equal(after[:, :3], before[:, :3]) and torch.equal(after[:, 3 + N:], before[:, 3 + N:]), (name, M, "guard columns")


@pytest.mark.parametrize("N,K", STRIDE_SHAPES)
def test_gemv_row_same_bits_for_every_m_at_ragged_shapes(N, K):
    ops = _ops()
    g = torch.Generator().manual_seed(3 * N + K)
    x = torch.randn(32, K, generator=g).to(BF16).cuda()
    w = (torch.randn(N, K, generator=g) * 0.05).to(BF16).cuda()
    b = torch.randn(N, generator=g).to(BF16).cuda()
    wq = w.clone()
    pk = ops.quantize_rows_w8(wq)
    for dt in (BF16, torch.float32):
        y32, q32 = ops.gemv(x, w, bias=b, out_dtype=dt), _gemv_w8(ops, x, pk, K, bias=b, out_dtype=dt)
        for r in range(32):
            x1 = x[r:r + 1].contiguous()
            assert _same_bits(ops.gemv(x1, w, bias=b, out_dtype=dt)[0], y32[r]), (dt, r)
            assert _same_bits(_gemv_w8(ops, x1, pk, K, bias=b, out_dtype=dt)[0], q32[r]), (dt, r, "w8")


# ------------------------------------------------------------------------------------------------ decode attention
CHUNKS = {128: (16, 48, 128, 512), 64: (32, 96, 128, 512)}
# per sequence max|d| / max|ref|, the gate of test_attn_decode_matches_fp32_softmax.  The output is bf16: half an ulp is 2^-9 .. 2^-8 of an
# element (3.9e-3 just above a power of two), softmax and accumulation are fp32; measured 3.7e-3 at worst, flat and peaked rows alike
# (record_measurement "attn_decode_edges").
DECODE_TOL = 4e-3


def _attn_raw(q, ld_q, cache, ld_c, bs_c, v_off, kv_len, L_max, out, ld_o, B, H, Hkv, hd, chunk, scale=None, part_short=0):
    nch = (L_max + chunk - 1) // chunk if chunk > 0 else 1
    part = torch.empty(B * H * nch * (hd + 2) + 64, dtype=torch.float32, device="cuda")
    _call("rv_attn_decode_bf16", q, ld_q, cache, ld_c, bs_c, v_off, kv_len, L_max, out, ld_o, part,
          (B * H * nch * (hd + 2) - part_short) * 4, B, H, Hkv, hd, chunk, float(scale if scale is not None else 1.0 / math.sqrt(hd)))


def _packed(K, V):
    return torch.cat([K, V], dim=-1).contiguous()


class _Strided:
    """The same q / K / V values in the layout of the C contract's other corner: q as the first H*hd columns of a q|k|v row
    (ld_q = H*hd + 2 kvd), K at column 0 and V at v_off = kvd + 40 of rows of ld_c = 2 kvd + 72, sequences bs_c = L_max ld_c + 128 apart,
    out inside rows of ld_o = H*hd + 64.  Everything between is a NaN sentinel."""

    def __init__(self, q, K, V, rows_out=None):
        B, L, kvd = K.shape
        Hhd = q.shape[1]
        self.ld_q, self.ld_c, self.v_off, self.ld_o = Hhd + 2 * kvd, 2 * kvd + 72, kvd + 40, Hhd + 64
        self.bs_c = L * self.ld_c + 128
        self.qkv = _sentinel((q.shape[0], self.ld_q), BF16)
        self.qkv[:, :Hhd] = q
        self.flat = _sentinel((B * self.bs_c,), BF16)
        torch.as_strided(self.flat, (B, L, kvd), (self.bs_c, self.ld_c, 1), 0).copy_(K)
        torch.as_strided(self.flat, (B, L, kvd), (self.bs_c, self.ld_c, 1), self.v_off).copy_(V)
        self.obuf = _sentinel((rows_out if rows_out is not None else q.shape[0], self.ld_o), BF16)
        self.before = _bits(self.obuf)
        self.Hhd = Hhd

    def q(self):
        return self.qkv[:, :self.Hhd]

    def out(self):
        return self.obuf[:, 32:32 + self.Hhd]

    def guards_untouched(self):
        after = _bits(self.obuf)
        return torch.equal(after[:, :32], self.before[:, :32]) and torch.equal(after[:, 32 + self.Hhd:], self.before[:, 32 + self.Hhd:])


NEEDLE_L = 1100
NEEDLE_TARGETS = (0, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 1099)
NEEDLE_PAIRS = ((0, 1099), (15, 16), (16, 17), (31, 33), (127, 128), (129, 255), (255, 257), (511, 512), (128, 1099))


@functools.lru_cache(maxsize=None)
def _needles(hd):
    """One sequence per (target, kv_len in {target + 1, L_max}) and per pair of equal targets (kv_len = L_max, and second target + 1):
    q [B, H*hd], K and V [B, L_max, kvd] on the CPU, lens, and the expected output bits.  Built once per hd and never written to."""
    Hkv, G = 2, 2
    H = Hkv * G
    cases = [((t,), n) for t in NEEDLE_TARGETS for n in sorted({t + 1, NEEDLE_L})]
    cases += [(p, n) for p in NEEDLE_PAIRS for n in sorted({p[1] + 1, NEEDLE_L})]
    qs, Ks, Vs, want = [], [], [], []
    for i, (ts, n) in enumerate(cases):
        assert all(t < n for t in ts)
        q1, K, V = needle_cache(NEEDLE_L, hd, Hkv, list(ts), seed=hd * 1000 + i)
        qs.append(q1.repeat(H))
        Ks.append(K)
        Vs.append(V)
        v = V[ts[0]].float() if len(ts) == 1 else (V[ts[0]].float() + V[ts[1]].float()) / 2
        want.append(v.to(BF16).view(Hkv, hd).repeat_interleave(G, dim=0).reshape(H * hd))
    return dict(cases=cases, H=H, Hkv=Hkv, q=torch.stack(qs), K=torch.stack(Ks), V=torch.stack(Vs), lens=[n for _, n in cases],
                want=torch.stack(want))


def test_needle_pairs_cover_same_and_different_chunks():
    for hd, chunks in CHUNKS.items():
        for c in chunks:
            same = [p for p in NEEDLE_PAIRS if p[0] // c == p[1] // c]
            assert same and len(same) < len(NEEDLE_PAIRS), (hd, c)


@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_needles(hd):
    """Each sequence's softmax puts all its weight on one key (or equally on two): the output row must be that key's V row (their mean), to the
    bit.  A key dropped, read twice, or read from the neighbouring row or chunk gives another row."""
    ops = _ops()
    nd = _needles(hd)
    cache = _packed(nd["K"], nd["V"]).cuda()
    q = nd["q"].cuda()
    kv_len = torch.tensor(nd["lens"], dtype=torch.int32).cuda()
    for chunk in CHUNKS[hd]:
        got = ops.attn_decode(q, cache, kv_len, nd["H"], nd["Hkv"], hd, nd["Hkv"] * hd, chunk=chunk).cpu()
        for b, case in enumerate(nd["cases"]):
            assert torch.equal(got[b], nd["want"][b]), (hd, chunk, case)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("stale", ["decoy", "nan"])
def test_attn_decode_ignores_keys_at_and_past_kv_len(hd, stale):
    """kv_len = last target + 1; the rows from kv_len up hold what a reused slot may: a decoy with twice the target's score (K all 4) and V all
    1000, or NaN bit patterns.  Not a bit of the output changes."""
    ops = _ops()
    nd = _needles(hd)
    kvd = nd["Hkv"] * hd
    keep = [b for b, (ts, n) in enumerate(nd["cases"]) if n == ts[-1] + 1]
    assert len(keep) == len(NEEDLE_TARGETS) + len(NEEDLE_PAIRS)
    K, V = nd["K"][keep].clone(), nd["V"][keep].clone()
    for i, b in enumerate(keep):
        n = nd["lens"][b]
        if stale == "decoy":
            K[i, n:] = 4.0
            V[i, n:] = 1000.0
        else:
            K[i, n:] = float("nan")
            V[i, n:] = float("nan")
    q = nd["q"][keep].cuda()
    kv_len = torch.tensor([nd["lens"][b] for b in keep], dtype=torch.int32).cuda()
    clean, dirty = _packed(nd["K"][keep], nd["V"][keep]).cuda(), _packed(K, V).cuda()
    for chunk in CHUNKS[hd]:
        a = ops.attn_decode(q, clean, kv_len, nd["H"], nd["Hkv"], hd, kvd, chunk=chunk)
        b_ = ops.attn_decode(q, dirty, kv_len, nd["H"], nd["Hkv"], hd, kvd, chunk=chunk)
        assert _same_bits(a, b_), (hd, chunk, stale)
        assert torch.equal(b_.cpu(), nd["want"][keep]), (hd, chunk, stale)


@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_kv_len_zero(hd):
    """A free slot under continuous batching: its row is all zeros and its neighbours are what they are without it."""
    ops = _ops()
    Hkv, G, L_max = 2, 2, 300
    H, kvd = Hkv * G, Hkv * hd
    g = torch.Generator().manual_seed(hd)
    cache = torch.randn(3, L_max, 2 * kvd, generator=g).to(BF16).cuda()
    q = torch.randn(3, H * hd, generator=g).to(BF16).cuda()
    kv_len = torch.tensor([5, 0, 300], dtype=torch.int32).cuda()
    for chunk in CHUNKS[hd]:
        out = _sentinel((3, H * hd), BF16)
        ops.attn_decode(q, cache, kv_len, H, Hkv, hd, kvd, out=out, chunk=chunk)
        assert torch.equal(_bits(out[1]), torch.zeros(H * hd, dtype=torch.int16)), chunk
        for b in (0, 2):
            alone = ops.attn_decode(q[b:b + 1], cache[b:b + 1], kv_len[b:b + 1].contiguous(), H, Hkv, hd, kvd, chunk=chunk)
            assert _same_bits(alone[0], out[b]), (chunk, b)
            assert not torch.isnan(out[b]).any()
    out = ops.attn_decode(q, cache, torch.zeros(3, dtype=torch.int32).cuda(), H, Hkv, hd, kvd, out=_sentinel((3, H * hd), BF16))
    assert torch.equal(_bits(out), torch.zeros(3, H * hd, dtype=torch.int16))


EDGE_LENS = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 299, 300]


@pytest.mark.parametrize("Hkv", [1, 3])
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_lengths_groups_chunks_against_float64(hd, Hkv):
    """Random data, L_max = 300 (no multiple of any chunk), a length at every row step of the block and both sides of 128 and 256, every
    group size G = 1..8, four chunk sizes; and the same with q scaled by 8 (peaked rows).  Both under the gate of
    test_attn_decode_matches_fp32_softmax (DECODE_TOL above); the peaked rows need no wider one."""
    ops = _ops()
    L_max, B, kvd = 300, len(EDGE_LENS), Hkv * hd
    g = torch.Generator().manual_seed(hd + Hkv)
    K = torch.randn(B, L_max, kvd, generator=g).to(BF16)
    V = torch.randn(B, L_max, kvd, generator=g).to(BF16)
    cache = _packed(K, V).cuda()
    kv_len = torch.tensor(EDGE_LENS, dtype=torch.int32).cuda()
    worst = {"flat": 0.0, "peaked": 0.0}
    for G in range(1, 9):
        H = G * Hkv
        q0 = torch.randn(B, H * hd, generator=g)
        for variant, q in (("flat", q0.to(BF16)), ("peaked", (q0 * 8).to(BF16))):
            ref = attn_decode_ref(q, K, V, EDGE_LENS, H, Hkv, hd)
            qd = q.cuda()
            for chunk in CHUNKS[hd]:
                got = ops.attn_decode(qd, cache, kv_len, H, Hkv, hd, kvd, chunk=chunk).double().cpu()
                for b in range(B):
                    err = float((got[b] - ref[b]).abs().max() / ref[b].abs().max())
                    worst[variant] = max(worst[variant], err)
                    assert err <= DECODE_TOL, (hd, Hkv, G, variant, chunk, EDGE_LENS[b], err)
    from conftest import record_measurement
    record_measurement("attn_decode_edges", hd=hd, Hkv=Hkv, rel_inf_flat=worst["flat"], rel_inf_peaked=worst["peaked"])


@pytest.mark.parametrize("hd,H,Hkv", [(64, 4, 2), (128, 28, 4)])
def test_attn_decode_layout_strides_and_guards(hd, H, Hkv):
    """q as the engine passes it (a slice of the q|k|v row), a cache with ld_c > 2 kvd, v_off != kvd and slack between sequences, out inside
    wider rows: the same bits as the packed layout, nothing written outside out."""
    ops = _ops()
    L_max, lens, kvd = 300, [300, 1, 129, 17, 0], Hkv * hd
    B = len(lens)
    g = torch.Generator().manual_seed(hd * 3 + H)
    K = torch.randn(B, L_max, kvd, generator=g).to(BF16).cuda()
    V = torch.randn(B, L_max, kvd, generator=g).to(BF16).cuda()
    q = torch.randn(B, H * hd, generator=g).to(BF16).cuda()
    kv_len = torch.tensor(lens, dtype=torch.int32).cuda()
    for chunk in (CHUNKS[hd][1], 128):
        want = ops.attn_decode(q, _packed(K, V), kv_len, H, Hkv, hd, kvd, chunk=chunk)
        assert not torch.isnan(want).any()
        s = _Strided(q, K, V)
        _attn_raw(s.q(), s.ld_q, s.flat, s.ld_c, s.bs_c, s.v_off, kv_len, L_max, s.out(), s.ld_o, B, H, Hkv, hd, chunk)
        assert _same_bits(s.out(), want), (hd, chunk)
        assert s.guards_untouched(), (hd, chunk)


@pytest.mark.parametrize("hd,H,Hkv", [(64, 4, 2), (128, 28, 4)])
def test_attn_decode_row_same_bits_alone_and_in_batch(hd, H, Hkv):
    ops = _ops()
    lens, kvd = [300, 1, 129, 17], Hkv * hd
    g = torch.Generator().manual_seed(hd + H)
    cache = torch.randn(len(lens), 300, 2 * kvd, generator=g).to(BF16).cuda()
    q = torch.randn(len(lens), H * hd, generator=g).to(BF16).cuda()
    full = ops.attn_decode(q, cache, torch.tensor(lens, dtype=torch.int32).cuda(), H, Hkv, hd, kvd)
    for b, n in enumerate(lens):
        c1 = cache[b:b + 1, :n + 3].contiguous()                      # its own, smaller L_max
        one = ops.attn_decode(q[b:b + 1], c1, torch.tensor([n], dtype=torch.int32).cuda(), H, Hkv, hd, kvd)
        assert _same_bits(one[0], full[b]), (hd, n)


# ------------------------------------------------------------------------------------------------ extend attention, layout only
def test_attn_extend_layout_strides_and_guards():
    ops = _ops()
    hd, H, Hkv = 128, 28, 4
    rs, ns = [300, 0, 257], [17, 40, 1]
    kvd, B, M = Hkv * hd, len(rs), sum(ns)
    L_max = max(r + n for r, n in zip(rs, ns)) + 37
    g = torch.Generator().manual_seed(7)
    K = torch.randn(B, L_max, kvd, generator=g).to(BF16).cuda()
    V = torch.randn(B, L_max, kvd, generator=g).to(BF16).cuda()
    q = (torch.randn(M, H * hd, generator=g) * 1.3).to(BF16).cuda()
    cu = torch.tensor([0, 17, 57, 58], dtype=torch.int32).cuda()
    r = torch.tensor(rs, dtype=torch.int32).cuda()
    want = ops.attn_extend(q, _packed(K, V), cu, r, H, Hkv, hd, kvd, max(ns))
    assert not torch.isnan(want).any()
    s = _Strided(q, K, V)
    chunk = ops.EXTEND_CHUNK
    nch = (L_max + chunk - 1) // chunk
    part = torch.empty(M * H * nch * (hd + 2), dtype=torch.float32, device="cuda")
    _call("rv_attn_extend_bf16", s.q(), s.ld_q, s.flat, s.ld_c, s.bs_c, s.v_off, cu, r, L_max, s.out(), s.ld_o, part, part.numel() * 4,
          B, M, max(ns), H, Hkv, hd, chunk, 1.0 / math.sqrt(hd))
    assert _same_bits(s.out(), want)
    assert s.guards_untouched()


# ------------------------------------------------------------------------------------------------ cache append
@pytest.mark.parametrize("width", [8, 264, 2048, 2056, 8192])
def test_kv_append_skips_strides_and_touches_nothing_else(width):
    """Positions 0, L_max - 1 and 7 are written, -1 and L_max skipped; widths below, at and above one pass of the 256-thread block (2048);
    src a column slice; a cache with ld_c > width and slack between sequences.  The whole allocation is compared element by element."""
    _ops()
    B, L_max, pos = 5, 16, [0, 15, -1, 16, 7]
    ld_c = width + 24
    bs_c = L_max * ld_c + 8
    total = B * bs_c
    orig = ((torch.arange(total, dtype=torch.int64) * 7 + 13) % 30011 + 1).to(torch.int16)        # a sentinel per element
    flat = orig.cuda().view(BF16)
    g = torch.Generator().manual_seed(width)
    swide = torch.randn(B, width + 40, generator=g).to(BF16).cuda()
    src = swide[:, 16:16 + width]
    want = orig.clone()
    sb = _bits(src)
    for b, p in enumerate(pos):
        if 0 <= p < L_max:
            o = b * bs_c + p * ld_c
            want[o:o + width] = sb[b]
    _call("rv_kv_append_bf16", src, src.stride(0), flat, ld_c, bs_c, torch.tensor(pos, dtype=torch.int32).cuda(), L_max, B, width)
    got = _bits(flat)
    assert torch.equal(got, want), int((got != want).sum())
    assert int((got != orig).sum()) > 3 * width // 2                   # and the three rows were written


# ------------------------------------------------------------------------------------------------ argmax
def _argmax_rows(n):
    """(rows [r, n], expected index per row, written out by hand): NaN is the maximum, the lowest index wins, -0.0 == +0.0."""
    nan, inf = float("nan"), float("inf")
    if n == 1:
        return torch.tensor([[nan], [-inf], [5.0], [-0.0]]), [0, 0, 0, 0]
    if n == 7:
        x = torch.full((5, 7), -1.0)
        x[0, 5], x[0, 2] = nan, inf                  # NaN beats +inf
        x[1, 6] = x[1, 4] = nan                      # the lower NaN
        x[2, :] = -inf                               # all -inf: index 0
        x[3, 3], x[3, 5] = -0.0, 0.0                 # -0.0 == +0.0: the lower index
        x[4, 6] = 2.0                                # the last column
        return x, [5, 4, 0, 3, 6]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(6, n, generator=g)
    x[0, 50], x[0, 20] = nan, inf
    x[1, 200] = x[1, 100] = nan
    x[2, :] = -inf
    x[3, :] = -1.0
    x[3, 3], x[3, 210] = -0.0, 0.0
    x[4, n - 1] = 9.0                                # the last column (n = 257: the one element of the block's second pass)
    x[5, :] = -1.0
    x[5, n - 1] = nan
    return x, [50, 100, 0, 3, n - 1, n - 1]


@pytest.mark.parametrize("n", [1, 7, 256, 257])
def test_argmax_nan_inf_signed_zero_and_small_n(n):
    ops = _ops()
    x, want = _argmax_rows(n)
    assert torch.argmax(x, dim=1).tolist() == want
    wide = torch.empty(x.shape[0], n + 8)
    wide[:, :n] = x
    wide[:, n:] = torch.tensor([float("inf"), float("nan")] * 4)       # pad columns: never read
    for buf, nn in ((x.cuda(), n), (wide.cuda(), n)):
        assert ops.argmax_rows(buf, nn).cpu().tolist() == want, buf.shape
        for r in range(x.shape[0]):                                    # a single-row launch
            assert ops.argmax_rows(buf[r:r + 1], nn).cpu().tolist() == [want[r]], (buf.shape, r)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(name, *args):
    from radvlm_amd.lib import RadvlmHipError
    with pytest.raises(RadvlmHipError):
        _call(name, *args)


def test_attn_decode_refuses_bad_arguments():
    """Every one is an argument check that returns before any launch (the buffers are large enough for each call all the same)."""
    _ops()
    B, L_max = 2, 64
    buf = lambda n: torch.zeros(n, dtype=BF16, device="cuda")
    q, cache, out = buf(B * 2048), buf(B * L_max * 4096), buf(B * 2048)
    kv_len = torch.tensor([3, 64], dtype=torch.int32).cuda()

    def run(hd=64, H=4, Hkv=2, chunk=128, ld_q=None, ld_o=None, ld_c=None, v_off=None, part_short=0):
        kvd = Hkv * hd
        ld_c = 2 * kvd if ld_c is None else ld_c
        _attn_raw(q, H * hd if ld_q is None else ld_q, cache, ld_c, L_max * ld_c, kvd if v_off is None else v_off, kv_len, L_max, out,
                  H * hd if ld_o is None else ld_o, B, H, Hkv, hd, chunk, part_short=part_short)

    from radvlm_amd.lib import RadvlmHipError
    run()                                                              # the base call is accepted
    run(hd=128, chunk=16)
    bad = [dict(hd=64, chunk=16), dict(chunk=520), dict(chunk=0), dict(H=9, Hkv=1), dict(hd=96), dict(part_short=1),
           dict(ld_c=2 * 128 - 8), dict(ld_c=256, v_off=136), dict(ld_q=4 * 64 - 8), dict(ld_o=4 * 64 - 8)]
    for kw in bad:
        with pytest.raises(RadvlmHipError):
            run(**kw)
    torch.cuda.synchronize()


SPLIT_ATTN_ENTRIES = ("decode", "beam", "kv8", "verify", "shared", "extend", "extend_prefix")


@pytest.mark.parametrize("entry", SPLIT_ATTN_ENTRIES)
def test_split_attn_refuses_bad_arguments(entry):
    """The seven cache-attention entry points share one launcher (csrc/attn_split.h's attn_split_launch): each accepts the base call
    with `part` exactly large enough and refuses the same eight bad argument sets, every one before any launch (the buffers are large
    enough for each call all the same).  2 sequences, hd 64, H 4, Hkv 2, 128 key positions, chunk 64; verify: R = 2 rows per sequence;
    the extend pair: 2 new rows per sequence."""
    _ops()
    from radvlm_amd.lib import RadvlmHipError
    B, L_max, R = 2, 128, 2
    H_MAX, HD_MAX = 18, 128
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()
    rows = B if entry in ("decode", "beam", "kv8", "shared") else B * R
    q = torch.zeros(rows * (H_MAX * HD_MAX + 8), dtype=BF16, device="cuda")
    out = torch.zeros(rows * H_MAX * HD_MAX, dtype=BF16, device="cuda")
    cache = torch.zeros(B * L_max * 2 * 2 * HD_MAX, dtype=BF16, device="cuda")
    cache8 = torch.zeros(B * L_max * 2 * 2 * HD_MAX, dtype=torch.int8, device="cuda")
    cache_s = torch.ones(B * L_max * 2 * 2, dtype=torch.float32, device="cuda")
    part = torch.zeros(rows * H_MAX * 2 * (HD_MAX + 2), dtype=torch.float32, device="cuda")
    kv_len, own_row, cu_q = i32([3, L_max]), i32([0, 1]), i32([0, 2, 4])
    tile = i32([[0] + [-1] * 15, [1] + [-1] * 15])

    def run(q_null=False, H=4, Hkv=2, hd=64, chunk=64, ld_q=None, ld_o=None, part_short=0):
        qq = None if q_null else q
        ld_q = H * hd if ld_q is None else ld_q
        ld_o = H * hd if ld_o is None else ld_o
        kvd = Hkv * hd
        ld_c, bs_c = 2 * kvd, L_max * 2 * kvd
        nch = (L_max + chunk - 1) // chunk if chunk > 0 else 1
        pb = rows * H * nch * (hd + 2) * 4 - part_short
        tail = (out, ld_o, part, pb)
        dims = (H, Hkv, hd, chunk, 0.125)
        if entry == "decode":
            _call("rv_attn_decode_bf16", qq, ld_q, cache, ld_c, bs_c, kvd, kv_len, L_max, *tail, B, *dims)
        elif entry == "beam":
            _call("rv_attn_decode_beam_bf16", qq, ld_q, cache, ld_c, bs_c, kvd, kv_len, L_max, own_row, i32([L_max, L_max]), None, 0, 0, B, *tail, B,
                  *dims)
        elif entry == "kv8":
            _call("rv_attn_decode_kv8_bf16", qq, ld_q, cache8, ld_c, bs_c, kvd, cache_s, 2 * Hkv, L_max * 2 * Hkv, Hkv, kv_len, L_max, *tail, B, *dims)
        elif entry == "verify":
            _call("rv_attn_decode_verify_bf16", qq, ld_q, cache, ld_c, bs_c, kvd, i32([3, L_max - 1]), L_max, *tail, B, R, *dims)
        elif entry == "shared":
            _call("rv_attn_decode_shared_bf16", qq, ld_q, cache, ld_c, bs_c, kvd, kv_len, i32([0, 0]), tile, L_max, *tail, B, *dims)
        elif entry == "extend":
            _call("rv_attn_extend_bf16", qq, ld_q, cache, ld_c, bs_c, kvd, cu_q, i32([3, L_max - 2]), L_max, *tail, B, B * R, R, *dims)
        else:       # one prefix row of 64 positions and 64 tail positions per sequence: 128 key positions
            P = L_max // 2
            _call("rv_attn_extend_prefix_bf16", qq, ld_q, cache, ld_c, P * ld_c, 1, P, cache[P * ld_c:], ld_c, P * ld_c, P, kvd, cu_q, i32([0, 0]),
                  i32([3, P]), *tail, B, B * R, R, *dims)

    run()                                                              # accepted, the partial buffer exactly large enough
    bad = [dict(q_null=True), dict(H=5), dict(H=18), dict(hd=96), dict(chunk=0), dict(ld_q=4 * 64 + 4), dict(ld_o=4 * 64 - 8), dict(part_short=4)]
    for kw in bad:
        with pytest.raises(RadvlmHipError):
            run(**kw)
    torch.cuda.synchronize()


def test_kv_append_refuses_bad_arguments():
    _ops()
    B, L_max = 2, 4
    src = torch.zeros(B, 64, dtype=BF16, device="cuda")
    cache = torch.zeros(B * L_max * 64, dtype=BF16, device="cuda")
    pos = torch.tensor([0, 1], dtype=torch.int32).cuda()
    _call("rv_kv_append_bf16", src, 64, cache, 64, L_max * 64, pos, L_max, B, 16)        # accepted
    _refused("rv_kv_append_bf16", src, 64, cache, 64, L_max * 64, pos, L_max, B, 12)     # width % 8
    _refused("rv_kv_append_bf16", src, 64, cache, 8, L_max * 8, pos, L_max, B, 16)       # ld_c < width
    _refused("rv_kv_append_bf16", src, 8, cache, 64, L_max * 64, pos, L_max, B, 16)      # ld_src < width
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", ["bf16", "w8", "w4"])
def test_gemv_refuses_bad_arguments(kernel):
    """The three entry points share one argument check (gemv.hip's gemv_launch; rv_gemv_lora_bf16, the fourth behind it, is held to
    its refusals in test_lora_decode_kernels_gpu.py): each refuses the same six bad argument sets."""
    ops = _ops()
    N, K = 64, 2056
    split = ops.gemv_split(N, K)
    assert split > 1
    x = torch.zeros(40, K + 64, dtype=BF16, device="cuda")
    w = torch.ones(N, K, dtype=BF16, device="cuda")
    y = torch.zeros(40, N + 64, dtype=BF16, device="cuda")
    res = torch.zeros(40, N + 64, dtype=BF16, device="cuda")
    ws = torch.zeros(split * 40 * N, dtype=torch.float32, device="cuda")
    pk, sc = ops.quantize_rows_w8(w.clone())
    p4, s4 = ops.quantize_rows_mxfp4(w.clone())

    def run(M=32, K_=K, ldx=K, ldy=N, ws_bytes=None, ldr=None):
        ws_bytes = ops.gemv_split(N, K_) * M * N * 4 if ws_bytes is None else ws_bytes
        r, ldr = (None, 0) if ldr is None else (res, ldr)
        if kernel == "bf16":
            _call("rv_gemv_bf16", x, ldx, w, K, y, ldy, None, r, ldr, M, N, K_, 0, ws, ws_bytes)
        elif kernel == "w8":
            _call("rv_gemv_w8_bf16", x, ldx, pk, ops.w8_row_bytes(K_), sc, y, ldy, None, r, ldr, M, N, K_, 0, ws, ws_bytes)
        else:
            _call("rv_gemv_w4_bf16", x, ldx, p4, ops.w4_row_bytes(K_), s4, ops.w4_scale_row_bytes(K_), y, ldy, None, r, ldr, M, N, K_, 0, ws,
                  ws_bytes)

    from radvlm_amd.lib import RadvlmHipError
    run()                                                              # accepted, the workspace exactly large enough
    run(ldr=N)                                                         # accepted, a residual at the smallest row stride
    for kw in (dict(M=33), dict(K_=12), dict(ldx=K - 8), dict(ldy=N - 1), dict(ws_bytes=split * 32 * N * 4 - 4), dict(ldr=N - 1)):
        with pytest.raises(RadvlmHipError):
            run(**kw)
    torch.cuda.synchronize()

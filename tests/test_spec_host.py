"""CPU tests of speculative sampling's rule and streams (tests/spec_ref.py, the reference of rv_spec_accept_rows_f32): the rule is exact
(with Fractions: drafting from q, accepting with min(1, p / q) and resampling from the residual emits p), the three streams of a seed
are independent (a chi-square test that fails when they are forced equal), the inputs of the GPU kernel test stay clear of the band,
and the host's tagged uniform, the header and the binding agree."""
import itertools
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

import sample_ref
import spec_ref
from radvlm_amd import portable_rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rule_is_exact():
    """sum_x q(x) [a(x) 1{y = x} + (1 - a(x)) r(y)] == p(y) for every y, in exact arithmetic, zeros in p and in q included."""
    rng = np.random.default_rng(0)
    cases = 0
    for n in range(2, 7):
        for trial in range(60):
            def dist(zero_some):
                w = [int(v) for v in rng.integers(1, 12, n)]
                if zero_some:
                    for i in rng.choice(n, size=int(rng.integers(0, n)), replace=False):
                        w[int(i)] = 0
                if sum(w) == 0:
                    w[int(rng.integers(0, n))] = 1
                return [Fraction(v, sum(w)) for v in w]
            p, q = dist(trial % 2), dist(trial % 3 == 0)
            if trial == 0:
                q = list(p)                                               # equal distributions: everything accepted
            if trial == 1:
                p, q = [Fraction(1)] + [Fraction(0)] * (n - 1), [Fraction(0)] * (n - 1) + [Fraction(1)]      # disjoint supports
            a, r = spec_ref.rule_probs(p, q)
            assert sum(r) == 1 and all(0 <= v <= 1 for v in a)
            for y in range(n):
                out = sum(q[x] * (a[x] * (1 if x == y else 0) + (1 - a[x]) * r[y]) for x in range(n))
                assert out == p[y], (p, q, y)
            if trial == 0:
                assert all(a[x] == 1 for x in range(n) if q[x] > 0)
            cases += 1
    assert cases == 300


def test_rule_probs_residual_fallback():
    a, r = spec_ref.rule_probs([0.25, 0.75], [0.25, 0.75])
    assert a == [1.0, 1.0] and r == [0.25, 0.75]                         # r identically 0: the draw falls back to p
    a, r = spec_ref.rule_probs([0.5, 0.5, 0.0], [0.0, 0.5, 0.5])
    assert a == [1.0, 1.0, 0.0] and r == [1.0, 0.0, 0.0]


def _emit(p_row, q_row, seed, tags):
    """One assisted step end to end: the draft drawn from q, the accept test, the resample -- each with its stream."""
    Q = spec_ref.softmax(q_row)
    x = sample_ref.draw(Q, Q > 0, spec_ref.uniform(seed, tags[2], 0))
    res = spec_ref.accept_group(np.stack([p_row, p_row]), q_row[None], [x], seed, 0, tags=tags[:2])
    return x if res["n_accept"] == 1 else res["token"]


def test_streams_are_independent():
    """4096 fixed seeds on fixed p, q with n = 8: Pearson's statistic of the emitted token against p stays under the critical value of
    the chi-square distribution with 7 degrees of freedom at 1e-6, 40.52 (scipy.stats.chi2.isf(1e-6, 7) = 40.5218; Abramowitz & Stegun
    table 26.8 gives 24.32 at 1e-3 for comparison).  With the draft's draw and the accept test on ONE stream the same code is over it:
    a draft drawn with a small u is then also tested with a small u, which accepts too often."""
    p_row = np.log(np.array([0.30, 0.05, 0.20, 0.05, 0.10, 0.15, 0.05, 0.10])).astype(np.float32)
    q_row = np.log(np.array([0.05, 0.30, 0.05, 0.20, 0.15, 0.05, 0.10, 0.10])).astype(np.float32)
    P = spec_ref.softmax(p_row)
    N = 4096

    def pearson(tags):
        counts = np.zeros(8)
        for seed in range(N):
            counts[_emit(p_row, q_row, seed, tags)] += 1
        return float(((counts - N * P) ** 2 / (N * P)).sum())
    crit = 40.52
    good = pearson((spec_ref.TAG_DRAW, spec_ref.TAG_ACCEPT, spec_ref.TAG_DRAFT))
    assert good < crit, good
    assert len({spec_ref.TAG_DRAW, spec_ref.TAG_ACCEPT, spec_ref.TAG_DRAFT}) == 3
    for tags in ((0, 2, 2), (0, 0, 0)):                                   # the accept test shares the draft's stream
        bad = pearson(tags)
        assert bad > crit, (tags, bad)


def test_uniform_streams():
    for seed, tag, t in itertools.product((0, 1, 12345, (1 << 63) - 1), (0, 1, 2), (0, 1, 7, 4000)):
        want = (float(int(portable_rng._stream(seed, tag, t + 1)[t]) >> 40) + 0.5) * 2.0 ** -24 if seed < (1 << 40) else None
        got = spec_ref.uniform(seed, tag, t)
        assert want is None or got == want
        if tag == 0:
            assert got == sample_ref.uniform(seed, t) if seed < (1 << 40) else True
    from radvlm_amd.generation import sample_uniform
    assert all(sample_uniform(s, t) == spec_ref.uniform(s, 0, t) for s in (0, 5, (1 << 63) - 1) for t in (0, 3, 100))


KERNEL_N = (1, 2, 7, 64, 1000, 32003, 262144)
KERNEL_R = (1, 2, 5, 32)
KERNEL_GROUPS = (1, 3)


def kernel_cases():
    """(n, R, groups) of the GPU kernel test."""
    return [(n, R, g) for n in KERNEL_N for R in KERNEL_R for g in KERNEL_GROUPS]


def test_band_occupancy_of_the_kernel_tests_inputs():
    """On the exact inputs of the GPU kernel test the reference's accept tests and draws fall within DELTA of a boundary in at most 1 of
    1000 cases (here: none), so the kernel test's exemptions are not where its agreement comes from."""
    decisions = near = 0
    for n, R, groups in kernel_cases():
        p, q, draft, seeds, t0 = spec_ref.kernel_case(n, R, groups)
        for g in range(groups):
            res = spec_ref.accept_group(p[g * R:(g + 1) * R], q[g * (R - 1):(g + 1) * (R - 1)], draft[g], int(seeds[g]), int(t0[g]))
            decisions += len(res["margins"]) + 1
            near += spec_ref.near_boundary(res)
            assert res["token"] >= 0
    assert decisions > 300 and near * 1000 <= decisions, (near, decisions)


def test_kernel_cases_accept_and_reject():
    acc = rej = 0
    for n, R, groups in kernel_cases():
        if n > 1000 or R == 1:
            continue
        p, q, draft, seeds, t0 = spec_ref.kernel_case(n, R, groups)
        for g in range(groups):
            res = spec_ref.accept_group(p[g * R:(g + 1) * R], q[g * (R - 1):(g + 1) * (R - 1)], draft[g], int(seeds[g]), int(t0[g]))
            acc += res["n_accept"]
            rej += res["n_accept"] < R - 1
    assert acc > 20 and rej > 10, (acc, rej)


def test_header_band_and_binding():
    from radvlm_amd import lib
    hdr = open(os.path.join(ROOT, "include", "radvlm_hip.h")).read()
    m = re.search(r"band of delta = 2\^-(\d+)", hdr)
    assert m and 2.0 ** -int(m.group(1)) == spec_ref.DELTA <= sample_ref.DELTA
    assert {"rv_spec_accept_rows_f32", "rv_spec_ws_bytes", "rv_sample_rows_tagged_f32", "rv_sample_uniform24_tagged"} <= set(lib.SIGNATURES)
    so = os.path.join(ROOT, "radvlm_amd", "libradvlm_hip.so")
    if not os.path.exists(so):                                            # as tests/test_abi_and_ddp.py: the library is built, not skipped
        subprocess.check_call(["bash", os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")])
    L = lib.load()
    for seed, tag, t in itertools.product((0, 7, (1 << 63) - 1), (0, 1, 2), (0, 1, 999)):
        assert (L.rv_sample_uniform24_tagged(seed, tag, t) + 0.5) * 2.0 ** -24 == spec_ref.uniform(seed, tag, t)
        if tag == 0:
            assert L.rv_sample_uniform24_tagged(seed, 0, t) == L.rv_sample_uniform24(seed, t)
    assert L.rv_spec_ws_bytes(3, 5) == 3 * 9 * 16 and L.rv_spec_ws_bytes(1, 33) == 0 and L.rv_spec_ws_bytes(0, 2) == 0
    assert L.rv_spec_accept_rows_f32(None, 8, None, 8, None, None, None, 1, 2, 8, None, None, None, None, 0, None) == -1

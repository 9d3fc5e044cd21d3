"""CPU tests of score()'s host side (radvlm_amd/scoring.py): candidate validation, prefill groups with equal prompts prefilled once, packing
into launches under the row budget and the kernel's grid limit, the index arrays of a hand-written launch, the result's order, .best and
the fp64 sum; and the C-ABI declarations of the two scoring kernels."""
import os
import re

import numpy as np
import pytest
import torch

from radvlm_amd import scoring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_symbols_declared_and_bound():
    from radvlm_amd import lib
    assert {"rv_attn_extend_prefix_bf16", "rv_token_logprob_rows_f32"} <= set(lib.SIGNATURES)
    build = open(os.path.join(ROOT, "radvlm_amd", "csrc", "build.sh")).read()
    assert re.search(r'SRCS="[^"]*\bscore\b', build) and '$(printf "$OBJ/%s.res " $SRCS)' in build          # built, and under the scratch gate


def test_candidate_validation():
    ok = [[np.array([1, 2])], [torch.tensor([3]), [4, 5, 6]]]
    out = scoring.check_candidates(ok, 2, 10)
    assert [len(r) for r in out] == [1, 2] and out[1][1].dtype == np.int64 and out[1][1].tolist() == [4, 5, 6]
    bad = [
        (ok, 3),                                               # another length than the prompts
        ([[np.array([1])], []], 2),                            # an empty candidate list
        ([[np.array([1])], [np.array([], dtype=np.int64)]], 2),   # an empty candidate
        ([[np.array([1])], [np.array([10])]], 2),              # id == vocab
        ([[np.array([1])], [np.array([-200])]], 2),            # the image placeholder: candidates are text
        ([[np.array([1])], [np.array([[1, 2]])]], 2),          # not 1-D
        ([[np.array([1])], [np.array([1.5])]], 2),             # not integers
        ([[np.array([1])], np.array([1, 2])], 2),              # a bare sequence where a list of candidates belongs
        ("no", 2),
    ]
    for cands, n in bad:
        with pytest.raises(ValueError):
            scoring.check_candidates(cands, n, 10)


def test_duplicate_prompts_are_prefilled_once_per_group():
    a, b, c = np.array([1, 2, 3]), np.array([1, 2, 4]), np.array([1, 2])
    recs = [a, b, a.copy(), c, a.copy(), b.copy()]
    g = scoring.plan_groups(recs, 32)
    assert len(g) == 1 and g[0].requests == [0, 1, 2, 3, 4, 5]
    assert g[0].leaders == [0, 1, 3] and g[0].row == {0: 0, 1: 1, 2: 0, 3: 2, 4: 0, 5: 1}
    g = scoring.plan_groups(recs, 4)                          # groups of at most max_batch_size prompts; no sharing across groups
    assert [x.requests for x in g] == [[0, 1, 2, 3], [4, 5]]
    assert g[0].leaders == [0, 1, 3] and g[1].leaders == [4, 5] and g[1].row == {4: 0, 5: 1}
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            scoring.plan_groups(recs, bad)


def test_packing_under_the_row_budget_and_the_grid_limit():
    assert [scoring.query_tile(G) for G in (1, 2, 4, 7, 8)] == [64, 32, 16, 16, 16]
    lens = [4] * 10                                           # 3 rows each
    assert scoring.pack_launches(lens, 7, row_budget=9) == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9]]
    assert scoring.pack_launches(lens, 7, row_budget=8) == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    assert scoring.pack_launches([1, 1, 4, 1], 7, row_budget=3) == [[0, 1, 2, 3]]           # one-token candidates cost no row
    assert scoring.pack_launches([100, 2, 2], 7, row_budget=10) == [[0], [1, 2]]            # longer than the budget: a launch of its own
    # sequences * query tiles <= 65535: 40,000 two-token candidates fit one launch at one tile each ...
    many = [2] * 40000
    assert scoring.pack_launches(many, 7, row_budget=10 ** 9) == [list(range(40000))]
    # ... and stop fitting when one 34-token candidate (33 rows: 3 tiles of 16) joins them
    got = scoring.pack_launches(many + [34], 7, row_budget=10 ** 9)
    assert got == [list(range(40000)), [40000]]
    got = scoring.pack_launches([34] + many, 7, row_budget=10 ** 9)
    assert [len(x) for x in got] == [21845, 18156] and 21845 * 3 <= 65535 < 21846 * 3
    for launch in scoring.pack_launches([2] * 70000, 1, row_budget=10 ** 9):
        assert len(launch) <= 65535
    with pytest.raises(ValueError):
        scoring.pack_launches(lens, 7, row_budget=0)


def _hand_case():
    tails = [np.array([11]), np.array([21, 22]), np.array([31, 32, 33, 34]), np.array([41]), np.array([51, 52, 53])]
    return [5, 9], [0, 0, 0, 1, 1], tails


def test_launch_arrays_of_a_hand_written_case():
    plen, row, tails = _hand_case()
    a = scoring.launch_arrays(row, [plen[r] for r in row], tails)
    assert (a.C, a.M, a.T_max, a.max_q) == (5, 6, 3, 3)
    assert a.cu_q.dtype == np.int32 and a.cu_q.tolist() == [0, 0, 1, 4, 4, 6]              # the one-token candidates run no row
    assert a.tokens.tolist() == [21, 31, 32, 33, 51, 52]
    assert a.positions.tolist() == [5, 5, 6, 7, 9, 10]
    assert a.targets.tolist() == [22, 32, 33, 34, 52, 53]
    assert a.tail_rows.tolist() == [3, 6, 7, 8, 12, 13]
    assert a.first_targets.tolist() == [11, 21, 31, 41, 51]
    assert a.src_row.tolist() == [0, 0, 0, 1, 1] and a.prefix_row.tolist() == [0, 0, 0, 1, 1]
    assert a.prefix_len.tolist() == [5, 5, 5, 9, 9]
    assert a.offsets.tolist() == [0, 1, 3, 7, 8, 11]
    assert a.first_out.tolist() == [0, 1, 3, 7, 8] and a.row_out.tolist() == [2, 4, 5, 6, 9, 10]
    assert sorted(a.first_out.tolist() + a.row_out.tolist()) == list(range(11))            # every output slot exactly once
    for name in ("tokens", "positions", "targets", "first_targets", "src_row", "prefix_row", "prefix_len"):
        assert getattr(a, name).dtype == np.int32, name
    only_first = scoring.launch_arrays([0, 1], [5, 9], [np.array([1]), np.array([2])])
    assert only_first.M == 0 and only_first.T_max == 0 and only_first.cu_q.tolist() == [0, 0, 0] and only_first.tokens.size == 0
    with pytest.raises(ValueError):
        scoring.launch_arrays([0], [5], [np.array([], dtype=np.int64)])
    with pytest.raises(ValueError):
        scoring.launch_arrays([0, 1], [5], [np.array([1])])


def test_group_plan_rows_and_bytes():
    plen, row, tails = _hand_case()
    layers, kvd = 3, 256
    p = scoring.plan_group(plen, row, tails, 2, layers, kvd)
    assert len(p.launches) == 1 and p.launches[0][0] == [0, 1, 2, 3, 4]
    assert p.rows == 6 == sum(len(t) - 1 for t in tails)
    assert (p.prefix_rows, p.P_max, p.prefix_positions) == (2, 9, 18)                      # two prompt rows for five candidates
    assert p.tail_cache_bytes == layers * 5 * 3 * 2 * kvd * 2 == scoring.tail_cache_bytes(layers, kvd, 5, 3)
    p2 = scoring.plan_group(plen, row, tails, 2, layers, kvd, row_budget=3)
    assert [c for c, _ in p2.launches] == [[0, 1], [2, 3], [4]]
    assert [a.M for _, a in p2.launches] == [1, 3, 2] and p2.rows == 6
    assert p2.launches[1][1].prefix_row.tolist() == [0, 1] and p2.launches[1][1].prefix_len.tolist() == [5, 9]
    assert p2.tail_cache_bytes == layers * 2 * 3 * 2 * kvd * 2                             # the largest launch's
    with pytest.raises(ValueError):
        scoring.plan_group(plen, [0, 0, 0, 1, 2], tails, 2, layers, kvd)                   # no such prompt row


def test_memory_check_names_max_batch_size():
    scoring.check_memory(10, 10, 2, 9)
    scoring.check_memory(10, None, 2, 9)
    with pytest.raises(ValueError, match="max_batch_size"):
        scoring.check_memory(11, 10, 2, 9)


def _pieces():
    # (prompt, candidate, logprobs, argmax, tokens), out of order
    return [(1, 0, [-1.0, -2.0], [7, 9], [7, 8]),
            (0, 1, [-0.5], [3], [3]),
            (0, 0, [-0.25, -0.25], [1, 2], [1, 2]),
            (1, 1, [-3.0], [4], [4])]


def test_results_come_back_in_input_order():
    out = scoring.assemble([2, 2], _pieces())
    assert [[t.tolist() for t in row] for row in out.token_logprobs] == [[[-0.25, -0.25], [-0.5]], [[-1.0, -2.0], [-3.0]]]
    assert all(t.dtype == torch.float32 for row in out.token_logprobs for t in row)
    assert out.logprobs[0].dtype == torch.float64 and out.logprobs[0].tolist() == [-0.5, -0.5] and out.logprobs[1].tolist() == [-3.0, -3.0]
    assert out.is_greedy[0].tolist() == [True, True] and out.is_greedy[1].tolist() == [False, True]
    with pytest.raises(ValueError):
        scoring.assemble([2, 2], _pieces()[:3])               # a candidate is missing
    with pytest.raises(ValueError):
        scoring.assemble([2, 2], _pieces() + _pieces()[:1])   # one came twice


def test_best_ties_and_length_normalisation():
    out = scoring.assemble([2, 2], _pieces())
    assert out.best().tolist() == [0, 0]                      # equal sums: the lower index
    # per token: prompt 0 has -0.25 against -0.5, prompt 1 has -1.5 against -3.0
    assert out.best(length_normalized=True).tolist() == [0, 0]
    out = scoring.assemble([3], [(0, 0, [-1.0, -1.0, -1.0], [0] * 3, [0] * 3), (0, 1, [-2.0], [0], [0]), (0, 2, [-2.5], [0], [0])])
    assert out.best().tolist() == [1] and out.best(length_normalized=True).tolist() == [0]


def test_the_sum_runs_in_fp64_in_token_order():
    x = np.array([2.0 ** 60, 1.0, -(2.0 ** 60), 1.0], dtype=np.float32)
    assert scoring.sum_in_order(x) == 1.0                     # ((2^60 + 1) - 2^60) + 1 in fp64; pairwise or sorted sums give 2 or 0
    assert scoring.sum_in_order(x[::-1]) == 0.0
    y = np.array([0.1, 0.2, 0.3], dtype=np.float32)
    assert scoring.sum_in_order(y) == (np.float64(y[0]) + np.float64(y[1])) + np.float64(y[2])
    out = scoring.assemble([1], [(0, 0, x, [0] * 4, [0] * 4)])
    assert out.logprobs[0].tolist() == [1.0]

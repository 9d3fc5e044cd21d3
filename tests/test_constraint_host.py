"""Host tests of constrained decoding (radvlm_amd/constraints.py and the constraint keyword of the parsers): no GPU, no device code."""
import numpy as np
import pytest

import constraint_ref
from radvlm_amd import constraints as C
from radvlm_amd.constraints import DEAD, FREE, TokenConstraint, boxes_char_dfa, char_dfa_accepts
from radvlm_amd.data.create_instructions import format_boxes
from radvlm_amd.generation import ConstraintMirror, parse_batch_kwargs, parse_beam_kwargs, parse_generate_kwargs

i32 = lambda v: np.asarray(v, dtype=np.int32)


def _edges(c, s):
    return {int(t): int(n) for t, n in zip(c.allowed(s), c.edge_next[c.edge_off[s]:c.edge_off[s + 1]])}


def _language(c, limit=6):
    """Every token sequence the automaton accepts (ending in FREE), up to `limit` tokens."""
    out, front = set(), [((), c.start)]
    while front:
        seq, s = front.pop()
        if len(seq) == limit:
            continue
        for t, n in _edges(c, s).items():
            if n == FREE:
                out.add(seq + (t,))
            else:
                front.append((seq + (t,), n))
    return out


# ------------------------------------------------------------------------------------------------ from_choices
def test_from_choices_is_the_trie_with_eos_after_each_choice():
    c = TokenConstraint.from_choices([[5, 6, 7], [5, 6, 9], [5], [8, 2], [8, 2], [5, 6, 7]], eos=[1, 3])
    want = {(5, 6, 7), (5, 6, 9), (5,), (8, 2)}
    assert _language(c) == {s + (e,) for s in want for e in (1, 3)}
    assert c.n_states == 7                                       # root, 5, 5-6, 5-6-7, 5-6-9, 8, 8-2: shared prefixes and duplicates merged
    assert c.allowed(c.start).tolist() == [5, 8]
    after5 = _edges(c, c.start)[5]
    assert sorted(_edges(c, after5)) == [1, 3, 6]                # a choice that is a prefix of another: EOS and the continuation
    assert _edges(c, after5)[1] == FREE and _edges(c, after5)[3] == FREE
    assert c.max_token == 9 and c.edge_tok.dtype == np.int32 and c.edge_off.dtype == np.int32 and c.edge_next.dtype == np.int32
    one = TokenConstraint.from_choices([[4]], eos=2)             # a bare int
    assert _language(one) == {(4, 2)}
    assert c.accepts([5, 6, 9, 3]) and not c.accepts([5, 6, 9]) and not c.accepts([5, 7, 1]) and not c.accepts([5, 1, 1])


@pytest.mark.parametrize("seqs,eos", [([], [1]), ([[]], [1]), ([[3], []], [1]), ([[3]], []), ([[3, 1]], [1]), ([[-1]], [1]), ([[2.5]], [1]),
                                       (None, [1]), ([[3]], [True])])
def test_from_choices_refuses(seqs, eos):
    with pytest.raises(ValueError):
        TokenConstraint.from_choices(seqs, eos)


# ------------------------------------------------------------------------------------------------ the constructor
def test_constructor_refusals_name_the_state():
    off, tok, nxt = i32([0, 2, 3]), i32([4, 7, 1]), i32([1, -1, -1])
    TokenConstraint(off, tok, nxt, 0)
    with pytest.raises(ValueError, match="int32"):
        TokenConstraint(off.astype(np.int64), tok, nxt, 0)
    with pytest.raises(ValueError, match="int32"):
        TokenConstraint(off, tok.tolist(), nxt, 0)
    with pytest.raises(ValueError, match="1-D"):
        TokenConstraint(off, tok[None], nxt, 0)
    with pytest.raises(ValueError, match="edge_next"):
        TokenConstraint(off, tok, nxt[:2], 0)
    with pytest.raises(ValueError, match="start"):
        TokenConstraint(off, tok, nxt, 2)
    with pytest.raises(ValueError, match="start"):
        TokenConstraint(off, tok, nxt, True)
    with pytest.raises(ValueError, match="edge_off"):
        TokenConstraint(i32([0, 2, 4]), tok, nxt, 0)
    with pytest.raises(ValueError, match="edge_off"):
        TokenConstraint(i32([0]), tok[:0], nxt[:0], 0)
    with pytest.raises(ValueError, match="state 1.*decreases"):      # state 1's run would be [3, 2)
        TokenConstraint(i32([0, 3, 2, 3]), tok, nxt, 0)
    with pytest.raises(ValueError, match="state 0.*ascending"):
        TokenConstraint(off, i32([7, 4, 1]), nxt, 0)
    with pytest.raises(ValueError, match="state 0.*ascending"):
        TokenConstraint(off, i32([4, 4, 1]), nxt, 0)              # distinct
    with pytest.raises(ValueError, match="state 1.*negative"):
        TokenConstraint(off, i32([4, 7, -1]), nxt, 0)
    with pytest.raises(ValueError, match="state 0.*edge_next 2"):
        TokenConstraint(off, tok, i32([2, -1, -1]), 0)
    with pytest.raises(ValueError, match="state 1.*edge_next -2"):
        TokenConstraint(off, tok, i32([1, -1, -2]), 0)
    with pytest.raises(ValueError, match="state 1 is reachable.*no edge"):
        TokenConstraint(i32([0, 2, 2]), tok[:2], nxt[:2], 0)
    TokenConstraint(i32([0, 0, 1]), i32([3]), i32([-1]), 1)      # an edgeless state nothing reaches is no error
    assert C.MAX_EDGES == 1 << 24
    big = np.arange(C.MAX_EDGES + 1, dtype=np.int32)
    with pytest.raises(ValueError, match="at most"):
        TokenConstraint(i32([0, big.size]), big, np.full(big.size, -1, dtype=np.int32), 0)


# ------------------------------------------------------------------------------------------------ walk / advance / stack
def test_walk_and_advance_agree_with_the_restatement():
    c = TokenConstraint.from_choices([[5, 6, 7], [5, 9], [8]], eos=[2])
    states, allowed = c.walk([5, 6, 7, 2, 4, 4])
    assert states[0] == c.start and allowed[0].tolist() == [5, 8] and allowed[1].tolist() == [6, 9] and allowed[2].tolist() == [7]
    assert allowed[3].tolist() == [2] and states[4] == FREE and allowed[4] is None and states[5] == FREE
    states, allowed = c.walk([5, 7, 7])
    assert states.tolist()[2] == DEAD and allowed[2].size == 0    # 7 is no edge of the state after 5
    rng = np.random.default_rng(0)
    s = rng.integers(-2, c.n_states + 2, 400)
    t = rng.integers(-1, 11, 400)
    want = [constraint_ref.advance_ref(a, b, c.edge_off, c.edge_tok, c.edge_next) for a, b in zip(s, t)]
    assert c.advance(s, t).tolist() == want
    assert c.advance(np.array([0]), np.array([2 ** 40])).tolist() == [DEAD]


def test_stack_offsets_the_states_and_none_is_free():
    a = TokenConstraint.from_choices([[5, 6], [7]], eos=[2])
    b = TokenConstraint.from_choices([[9]], eos=[2, 3])
    table, starts = TokenConstraint.stack([a, None, b, a, None])
    assert starts.dtype == np.int32 and starts.tolist() == [0, FREE, a.n_states, 0, FREE]     # the same object is held once
    assert table.n_states == a.n_states + b.n_states and table.n_edges == a.n_edges + b.n_edges
    for c, s0 in ((a, starts[0]), (b, starts[2])):
        for seq in _language(c):
            st, al = table.walk(seq, start=s0)
            st2, al2 = c.walk(seq)
            assert (st - np.where(st >= 0, s0 - c.start, 0)).tolist() == st2.tolist()
            assert all((x is None and y is None) or x.tolist() == y.tolist() for x, y in zip(al, al2))
    table, starts = TokenConstraint.stack([None, None])
    assert table is None and starts.tolist() == [FREE, FREE]
    table, starts = TokenConstraint.stack([None, b])
    assert table is b and starts.tolist() == [FREE, b.start]
    with pytest.raises(ValueError):
        TokenConstraint.stack([a, "x"])


def test_resolve_constraints():
    a = TokenConstraint.from_choices([[5, 6], [7]], eos=[2])
    table, starts = C.resolve_constraints(a, 3, 10)
    assert table is a and starts.tolist() == [0, 0, 0]
    assert C.resolve_constraints(None, 2, 10)[0] is None
    assert C.resolve_constraints([None, None], 2, 10)[0] is None
    with pytest.raises(ValueError, match="2 entries for 3"):
        C.resolve_constraints([a, None], 3, 10)
    with pytest.raises(ValueError, match="vocabulary"):
        C.resolve_constraints([None, a], 2, 7)                    # the largest id, 7, is >= 7
    C.resolve_constraints([None, a], 2, 8)
    with pytest.raises(ValueError):
        C.resolve_constraints("yes", 1, 10)
    with pytest.raises(ValueError):
        C.resolve_constraints([a, 3], 2, 10)


# ------------------------------------------------------------------------------------------------ from_char_dfa
VOCAB = ["<s>", None, "", "a", "b", "ab", "ba", "abab", "c", "bc", "cc", "abc"]     # 0: special text that matches nothing; 1 = EOS


def _ab_dfa():
    """(ab)+ then an optional c: states 0 -a-> 1 -b-> 2 (accepting) -a-> 1, 2 -c-> 3 (accepting); 4 is a trap that accepts nothing."""
    return {(0, "a"): 1, (1, "b"): 2, (2, "a"): 1, (2, "c"): 3, (0, "c"): 4, (4, "c"): 4}, 0, {2, 3}


def test_from_char_dfa_lifts_multi_character_tokens_and_prunes():
    delta, start, acc = _ab_dfa()
    c = TokenConstraint.from_char_dfa(VOCAB, delta, start, acc, eos=[1])
    # state numbers follow discovery from the start; recover the DFA states by walking
    s0 = c.start
    e0 = _edges(c, s0)
    assert sorted(e0) == [3, 5, 7, 11]                            # a, ab, abab, abc; "c" / "cc" lead only to the trap: pruned
    s1, s2, s3 = e0[3], e0[5], e0[11]
    assert e0[7] == s2                                            # "abab" walks 0-1-2-1-2: a token that passes through several states
    assert sorted(_edges(c, s1)) == [4, 6, 9] and _edges(c, s1)[4] == s2 and _edges(c, s1)[6] == s1 and _edges(c, s1)[9] == s3
    assert sorted(_edges(c, s2)) == [1, 3, 5, 7, 8, 11] and _edges(c, s2)[1] == FREE and _edges(c, s2)[8] == s3
    assert _edges(c, s3) == {1: FREE}                             # accepting, no way on: EOS only
    assert c.n_states == 4                                        # the trap state is gone, and every state kept has an edge
    assert 0 not in c.edge_tok and 2 not in c.edge_tok            # special / empty / None strings are never allowed
    decode = lambda seq: "".join(VOCAB[t] for t in seq[:-1])
    lang = _language(c, limit=4)
    assert lang and all(char_dfa_accepts((delta, start, acc), decode(s)) and s[-1] == 1 for s in lang)
    assert (5, 8, 1) in lang and (3, 9, 1) in lang and (11, 1) in lang


def test_from_char_dfa_prunes_what_the_vocabulary_cannot_finish():
    delta, start, acc = {(0, "a"): 1, (1, "b"): 2, (0, "x"): 3, (3, "y"): 4}, 0, {2, 4}
    c = TokenConstraint.from_char_dfa(["a", "b", "x", None], delta, start, acc, eos=[3])      # no token spells "y": the x branch dies
    assert _language(c) == {(0, 1, 3)} and c.n_states == 3
    with pytest.raises(ValueError, match="accepting"):
        TokenConstraint.from_char_dfa(["a", "x", None], delta, start, acc, eos=[2])
    with pytest.raises(ValueError):
        TokenConstraint.from_char_dfa(["a", "b"], delta, start, acc, eos=[])
    with pytest.raises(ValueError):
        TokenConstraint.from_char_dfa(["a", "b"], {(0, "ab"): 1}, 0, {1}, eos=[1])
    # an EOS id is never text, whatever its string
    c = TokenConstraint.from_char_dfa(["a", "b"], {(0, "a"): 1, (1, "b"): 1}, 0, {1}, eos=[1])
    assert _language(c) == {(0, 1)}


# ------------------------------------------------------------------------------------------------ boxes
def _boxes(rng, k):
    b = rng.random((k, 4))
    b[rng.random((k, 4)) < 0.1] = 0.0
    b[rng.random((k, 4)) < 0.1] = 1.0
    b[rng.random((k, 4)) < 0.1] = 0.5
    b[rng.random((k, 4)) < 0.05] = 0.004                          # rounds to 0.0
    b[rng.random((k, 4)) < 0.05] = 0.996                          # rounds to 1.0
    return b.tolist()


@pytest.mark.parametrize("num_float", [2, 1, 3, 0])
def test_boxes_char_dfa_accepts_what_format_boxes_prints(num_float):
    dfa = boxes_char_dfa(num_float)
    rng = np.random.default_rng(7)
    seen = set()
    for i in range(300):
        s = format_boxes(_boxes(rng, 1 + i % 3), num_float)
        seen.add(s)
        assert char_dfa_accepts(dfa, s), s
    assert len(seen) > 200 or num_float < 2
    assert char_dfa_accepts(dfa, format_boxes([[0.0, 1.0, 0.0, 1.0]], num_float))
    assert char_dfa_accepts(dfa, format_boxes([[0.0, 0.0, 1.0, 1.0]] * 5, num_float))


def test_boxes_char_dfa_rejects_near_misses():
    dfa = boxes_char_dfa(2)
    good = "[0.1, 0.25, 0.5, 1.0], [0.0, 0.01, 0.3, 0.99] and [0.12, 0.2, 0.3, 0.4]"
    assert char_dfa_accepts(dfa, good)
    for bad in ["", "[0.1, 0.25, 0.5, 1.0", "0.1, 0.25, 0.5, 1.0]", "[0.1, 0.25, 0.5, 1.0, 0.3]", "[0.1, 0.25, 0.5]",
                "[0.1, 0.25, 0.5, 1.0], and [0.1, 0.2, 0.3, 0.4]", "[0.1, 0.25, 0.5, 1.5]", "[0.1, 0.25, 0.5, 1.0] ", good + " and",
                good + ".", "[0.1, 0.25, 0.5, 1.0], [0.1, 0.2, 0.3, 0.4]", "[0.1, 0.25, 0.5, 1.0] and [0.1, 0.2, 0.3, 0.4] and [0.1, 0.2, 0.3, 0.4]",
                "[0.1,0.25, 0.5, 1.0]", "[0.10, 0.25, 0.5, 1.0]", "[0.00, 0.25, 0.5, 1.0]", "[0.123, 0.25, 0.5, 1.0]", "[.1, 0.25, 0.5, 1.0]",
                "[1, 0.25, 0.5, 1.0]", "[0.1, 0.25, 0.5, 1.00]", "[1.1, 0.25, 0.5, 1.0]", "[0.1, 0.25, 0.5, 2.0]", "[-0.1, 0.25, 0.5, 1.0]",
                "[0.1, 0.25, 0.5, 1.0] and[0.1, 0.2, 0.3, 0.4]", "[[0.1, 0.25, 0.5, 1.0]]"]:
        assert not char_dfa_accepts(dfa, bad), bad
    for bad in (-1, 5, 2.0, True, None):
        with pytest.raises(ValueError):
            boxes_char_dfa(bad)


def test_boxes_constraint_over_a_vocabulary_generates_only_box_strings():
    pieces = ["<eos>", "[", "]", ", ", " and ", " and", " ", ",", "0", "1", "0.", "1.0", ".", "5", "25", "0.5", "], [", "]]", "a"] + list("2346789")
    c = TokenConstraint.from_char_dfa(pieces, *boxes_char_dfa(2), eos=[0])
    assert pieces.index("a") not in c.edge_tok and pieces.index("]]") not in c.edge_tok
    assert (np.diff(c.edge_off) > 0).all()
    dfa = boxes_char_dfa(2)
    rng = np.random.default_rng(3)
    for _ in range(200):                                          # random walks end in strings the character DFA accepts
        s, out = c.start, []
        while s != FREE and len(out) < 200:
            e = _edges(c, s)
            t = int(rng.choice(sorted(e)))
            if 0 in e and rng.random() < 0.3:
                t = 0
            out.append(t)
            s = e[t]
        if s == FREE:
            assert char_dfa_accepts(dfa, "".join(pieces[t] for t in out[:-1]))
    ids = [pieces.index(p) for p in ["[", "0.5", ", ", "0.", "25", ", ", "1.0", ", ", "0", ".", "5", "]"]] + [0]
    assert c.accepts(ids)


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_raises_at_the_dead_end_and_names_it():
    c = TokenConstraint.from_choices([[5, 6]], eos=[2])
    m = ConstraintMirror(c, 3)
    m.state[:] = [c.start, FREE, c.start]
    m.take(np.array([0, 1, 2]), np.array([5, 9, 5]), lambda k: False, lambda k: f"row {k}", 0)
    assert m.state[1] == FREE and m.state[0] == m.state[2] >= 0
    with pytest.raises(RuntimeError, match=r"row 2 reached a dead end at step 1.*\[6\]"):
        m.take(np.array([0, 2]), np.array([6, 0]), lambda k: False, lambda k: f"row {[0, 2][k]}", 1)
    z = TokenConstraint.from_choices([[0]], eos=[2])              # token 0 allowed, but its score was -inf: the argmax of an all -inf row
    m = ConstraintMirror(z, 1)
    m.state[:] = z.start
    with pytest.raises(RuntimeError, match="request 4 reached a dead end at step 7"):
        m.take(np.array([0]), np.array([0]), lambda k: True, lambda k: "request 4", np.array([7]))
    m.take(np.array([0]), np.array([0]), lambda k: False, lambda k: "request 4", np.array([7]))
    with pytest.raises(RuntimeError, match="dead end"):
        m.take(np.array([0]), np.array([-1]), None, lambda k: "row 0", 1)       # the sampler's mark for a row it cannot sample


# ------------------------------------------------------------------------------------------------ the parsers
def test_parsers_take_constraint_and_refuse_the_three_combinations():
    c = TokenConstraint.from_choices([[5, 6]], eos=[2])
    assert parse_generate_kwargs(dict(max_new_tokens=3)).constraint is None
    assert parse_generate_kwargs(dict(constraint=None)).constraint is None
    assert parse_generate_kwargs(dict(constraint=c)).constraint is c
    assert parse_generate_kwargs(dict(constraint=(c, None))).constraint == [c, None]
    assert parse_generate_kwargs(dict(constraint=c, do_sample=True, seed=3, repetition_penalty=1.2, kv_cache_dtype="int8")).constraint is c
    for bad in ("yes", 3, [c, "x"], {"a": c}, lambda b, ids: [1]):
        with pytest.raises(ValueError, match="constraint"):
            parse_generate_kwargs(dict(constraint=bad))
    with pytest.raises(NotImplementedError, match="constraint with prompt_lookup_num_tokens"):
        parse_generate_kwargs(dict(constraint=c, prompt_lookup_num_tokens=3), lookup=True)
    with pytest.raises(NotImplementedError, match="constraint with guidance_scale"):
        parse_generate_kwargs(dict(constraint=c, guidance_scale=1.5))
    with pytest.raises(NotImplementedError, match="constraint with dola_layers"):
        parse_generate_kwargs(dict(constraint=c, dola_layers="high"))
    cfg = parse_batch_kwargs(dict(constraint=[c, None, c], share_prefix=True, max_new_tokens=[1, 2, 3]), 3)
    assert cfg.constraint == [c, None, c] and cfg.share_prefix
    assert parse_batch_kwargs(dict(constraint=c), 3).constraint is c
    with pytest.raises(ValueError, match="2 entries for 3 requests"):
        parse_batch_kwargs(dict(constraint=[c, None]), 3)
    with pytest.raises(NotImplementedError, match="constraint with guidance_scale"):
        parse_batch_kwargs(dict(constraint=c, guidance_scale=2.0), 2)
    with pytest.raises(NotImplementedError, match="constraint with dola_layers"):
        parse_batch_kwargs(dict(constraint=c, dola_layers=[0]), 2)
    with pytest.raises(TypeError, match="constraint"):
        parse_beam_kwargs(dict(num_beams=2, constraint=c))
    with pytest.raises(TypeError):                                # HF's keyword stays unknown
        parse_generate_kwargs(dict(prefix_allowed_tokens_fn=lambda b, ids: [1]))


def test_the_module_imports_no_device_code():
    import subprocess
    import sys
    code = ("import sys; import radvlm_amd.constraints; "
            "assert not [m for m in sys.modules if m in ('radvlm_amd.ops', 'radvlm_amd.lib', 'radvlm_amd.engine', 'torch')], sorted(sys.modules)")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0

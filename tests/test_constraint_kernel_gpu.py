"""GPU tests of rv_constrain_rows_f32 (ops.constrain_rows) against the numpy restatement tests/constraint_ref.py: every comparison is
on bit patterns, over the whole buffer, guard columns and guard rows included."""
import numpy as np
import pytest
import torch

import constraint_ref
from radvlm_amd.constraints import TokenConstraint

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(12345.5)
KINDS = ["free", "dead", "beyond", "first", "last", "all", "past_n", "some"]      # one row of each in a launch


def _ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from radvlm_amd import ops
    return ops


_TABLES = {}


def _table(n):
    """Six states over the ids [0, n): 0 allows only column 0; 1 only column n - 1; 2 every id (a self loop); 3 two ids and one past
    n; 4 a random third of the ids, leading everywhere; 5 one id, to FREE."""
    if n not in _TABLES:
        rng = np.random.default_rng(n)
        some = np.sort(rng.choice(n, size=max(1, n // 3), replace=False))
        nxt = [-1, 0, 1, 2, 3, 4, 5]
        edges = [{0: 1}, {n - 1: 0}, {i: 2 for i in range(n)}, {n // 3: 3, n // 2: 4, n + 5: 0},
                 {int(t): nxt[k % 7] for k, t in enumerate(some)}, {n // 2: -1}]
        _TABLES[n] = TokenConstraint._from_edges(edges)
    return _TABLES[n]


STATE_OF = dict(free=-1, dead=-2, beyond=6, first=0, last=1, all=2, past_n=3, some=4)


def _rows(c, n, ld, states):
    """rows + 2 guard rows of ld floats: distinct finite values, the sentinel on guard rows and on columns >= n, one NaN and one -0.0
    on allowed columns of every live row, and a NaN on a column of every free row."""
    rows = len(states)
    x = (np.arange((rows + 2) * ld, dtype=np.float32).reshape(rows + 2, ld) * np.float32(0.25) - np.float32(1000.0)).astype(np.float32)
    assert np.unique(x).size == x.size
    x[0], x[-1], x[:, n:] = SENTINEL, SENTINEL, SENTINEL
    for r, s in enumerate(states):
        if s == -1:
            x[1 + r, n // 2] = np.nan
        al = c.allowed(s)
        if al is not None:
            al = al[al < n]
            if al.size:
                x[1 + r, al[0]] = np.nan
                x[1 + r, al[-1]] = -0.0 if al.size > 1 else np.nan
    return x


def _check(n, states, tok=None, slot=None, ld=None, state_rows=None):
    ops = _ops()
    c = _table(n)
    rows = len(states)
    ld = n + 3 if ld is None else ld
    if slot is None:
        st = np.asarray(states, dtype=np.int32)
    else:
        st = np.full(state_rows, 5, dtype=np.int32)               # slots no row names hold state 5 and must keep it
        st[np.asarray(slot)] = states
    live_in = st.copy()
    if tok is not None:
        # the NaN / -0.0 go on columns the state AFTER the advance allows
        after = [constraint_ref.advance_ref(s, t, c.edge_off, c.edge_tok, c.edge_next) for s, t in zip(states, tok)]
    else:
        after = list(states)
    x = _rows(c, n, ld, after)
    want_bits, want_state = constraint_ref.constrain_rows_ref(x[1:-1], n, live_in, c.edge_off, c.edge_tok, c.edge_next, tok=tok, slot=slot)
    dx = torch.from_numpy(x).cuda()
    dstate = torch.from_numpy(st).cuda()
    dtok = None if tok is None else torch.tensor(tok, dtype=torch.int64, device="cuda")
    dslot = None if slot is None else torch.tensor(slot, dtype=torch.int32, device="cuda")
    out = ops.constrain_rows(dx[1:-1], n, dstate, c.device_tables("cuda"), tok=dtok, slot=dslot)
    assert out.data_ptr() == dx[1:-1].data_ptr()
    got = dx.cpu().numpy().view(np.uint32)
    full = x.view(np.uint32).copy()
    full[1:-1] = want_bits
    assert np.array_equal(got, full)
    assert np.array_equal(got[0], x.view(np.uint32)[0]) and np.array_equal(got[:, n:], x.view(np.uint32)[:, n:])      # the guards, said once more
    assert np.array_equal(dstate.cpu().numpy(), want_state)
    return got[1:-1], want_state


def _tile():
    return _ops().CONSTRAIN_TILE


@pytest.mark.parametrize("n", [1, 33, "tile-1", "tile", "tile+1"])
def test_every_kind_of_state_in_one_launch(n):
    n = {"tile-1": _tile() - 1, "tile": _tile(), "tile+1": _tile() + 1}.get(n, n)
    states = [STATE_OF[k] for k in KINDS]
    got, state = _check(n, states)
    assert state.tolist() == states                               # tok=None: nothing is written back
    c = _table(n)
    x = _rows(c, n, n + 3, states).view(np.uint32)[1:-1]
    neg = constraint_ref.NEG_INF_BITS
    assert np.array_equal(got[0], x[0]) and np.isnan(got[0].view(np.float32)[n // 2])                 # free: bit-identical, its NaN included
    assert (got[1, :n] == neg).all() and (got[2, :n] == neg).all()                                     # dead, and a number >= n_states
    assert np.isnan(got[3].view(np.float32)[0]) and (got[3, 1:n] == neg).all()                         # only column 0
    assert np.isnan(got[4].view(np.float32)[n - 1]) and (got[4, :n - 1] == neg).all()                  # only column n - 1
    assert np.array_equal(got[5], x[5])                                                               # every id allowed: untouched
    keep = sorted({n // 3, n // 2})
    assert (np.flatnonzero(got[6, :n] != neg).tolist() == keep)                                        # the id past n is ignored
    al = c.allowed(4)
    assert np.array_equal(np.flatnonzero(got[7, :n] != neg), al)
    if al.size > 1:
        assert got[7, al[-1]] == np.uint32(0x80000000)                                                 # the allowed -0.0 keeps its sign


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [33, "tile+1"])
def test_row_counts_and_a_row_alone_gives_its_batch_bits(n, rows):
    n = _tile() + 1 if n == "tile+1" else n
    states = [STATE_OF[k] for k in ["some", "first", "all", "dead", "past_n"]][:rows]
    ops = _ops()
    got, _ = _check(n, states)
    c = _table(n)
    x = _rows(c, n, n + 3, states)
    for r, s in enumerate(states):                                # the same input row, launched alone
        one = torch.from_numpy(x[1 + r:2 + r].copy()).cuda()
        ops.constrain_rows(one, n, torch.tensor([s], dtype=torch.int32, device="cuda"), c.device_tables("cuda"))
        assert np.array_equal(one.cpu().numpy().view(np.uint32)[0], got[r])


def test_full_vocabulary_once():
    n = 152064
    got, _ = _check(n, [STATE_OF[k] for k in ["all", "some", "last", "free", "past_n"]], ld=n + 1)
    got, state = _check(n, [2, 4, 2], tok=[n - 1, int(_table(n).allowed(4)[-1]), 70000], ld=n)       # three rounds of the edge search
    assert state[0] == 2 and state[2] == 2


@pytest.mark.parametrize("n", [33, "tile+1"])
def test_advance(n):
    n = _tile() + 1 if n == "tile+1" else n
    c = _table(n)
    al = c.allowed(4)
    missing = next(t for t in range(n + 1) if t not in set(al.tolist()))      # n itself when the state allows every id
    states = [4, 4, 4, 4, -1, -2, 2, 0, 1, 6, 5]
    tok = [int(al[0]), int(al[-1]), int(al[al.size // 2]), missing, 0, int(al[0]), n - 1, 5, n - 1, 0, n // 2]
    got, state = _check(n, states, tok=tok)
    nxt = c.edge_next[c.edge_off[4]:c.edge_off[5]]
    assert state[:4].tolist() == [int(nxt[0]), int(nxt[-1]), int(nxt[al.size // 2]), -2]              # first, last and a middle edge; no edge
    assert state[4:].tolist() == [-1, -2, 2, -2, 0, -2, -1]                                            # negative states stay whatever tok holds
    assert c.advance(np.asarray(states), np.asarray(tok)).tolist() == state.tolist()                   # and the host's advance agrees
    big, state = _check(n, [4, 2], tok=[2 ** 40 + int(al[0]), -1])                                    # no int32: no edge
    assert state.tolist() == [-2, -2]


def test_slot_indirection_with_a_permuted_slot_list():
    n = _tile() + 1
    al = _table(n).allowed(4)
    slot = [6, 0, 3, 5]
    got, state = _check(n, [4, 0, 2, -1], tok=[int(al[1]), 0, 7, 3], slot=slot, state_rows=8)
    assert state[[1, 2, 4, 7]].tolist() == [5, 5, 5, 5]           # the slots no row names keep their state
    _check(n, [4, 0, 2, -1], slot=slot, state_rows=8)             # tok=None through slots
    plain, _ = _check(n, [4, 0, 2, -1], tok=[int(al[1]), 0, 7, 3])
    assert np.array_equal(got == constraint_ref.NEG_INF_BITS, plain == constraint_ref.NEG_INF_BITS)


def test_bad_arguments_are_refused():
    ops = _ops()
    from radvlm_amd import lib
    c = _table(33)
    off, tok, nxt = c.device_tables("cuda")
    x = torch.zeros(2, 40, device="cuda")
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    good = [x, 40, 2, 33, st, 2, None, None, off, tok, nxt, c.n_states, c.n_edges]
    lib.call("rv_constrain_rows_f32", *good)

    def bad(**kw):
        names = ["x", "ld", "rows", "n", "state", "state_rows", "slot", "tok", "off", "etok", "enext", "n_states", "n_edges"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        with pytest.raises(lib.RadvlmHipError):
            lib.call("rv_constrain_rows_f32", *args)

    bad(n=262145, ld=262145)
    bad(n=0)
    bad(rows=0)
    bad(rows=-1)
    bad(off=None)
    bad(etok=None)
    bad(enext=None)
    bad(x=None)
    bad(state=None)
    bad(ld=32)
    bad(rows=3)                                                   # no slot list: more rows than states
    bad(state_rows=0)
    bad(n_states=0)
    bad(n_edges=0)
    assert torch.equal(st.cpu(), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(AssertionError):
        ops.constrain_rows(x, 41, st, (off, tok, nxt))

"""numpy restatement of rv_constrain_rows_f32 (csrc/constrain.hip): advance, then mask.  Written from the contract in
include/radvlm_hip.h with plain loops, not from radvlm_amd/constraints.py, so the two check each other."""
import numpy as np

NEG_INF_BITS = np.uint32(0xFF800000)


def advance_ref(state, tok, edge_off, edge_tok, edge_next):
    """The state after taking token `tok`: a live state follows the token's edge or becomes -2; a negative one stays."""
    n_states = len(edge_off) - 1
    if state < 0:
        return int(state)
    if state >= n_states:
        return -2
    for e in range(int(edge_off[state]), int(edge_off[state + 1])):
        if int(edge_tok[e]) == int(tok):
            return int(edge_next[e])
    return -2


def constrain_rows_ref(x, n, state, edge_off, edge_tok, edge_next, tok=None, slot=None):
    """x: fp32 [rows, ld] (not modified); state: int32 [state_rows] (not modified).  Returns (the rows as uint32 bit patterns after
    the call, the state array after the call)."""
    bits = np.ascontiguousarray(x).view(np.uint32).copy()
    state = np.array(state, dtype=np.int32)
    n_states = len(edge_off) - 1
    for r in range(x.shape[0]):
        si = r if slot is None else int(slot[r])
        s = int(state[si])
        if tok is not None:
            s = advance_ref(s, int(tok[r]), edge_off, edge_tok, edge_next)
            state[si] = s
        if s == -1:
            continue
        keep = np.zeros(n, dtype=bool)
        if 0 <= s < n_states:
            for e in range(int(edge_off[s]), int(edge_off[s + 1])):
                if 0 <= int(edge_tok[e]) < n:
                    keep[int(edge_tok[e])] = True
        bits[r, :n][~keep] = NEG_INF_BITS
    return bits, state

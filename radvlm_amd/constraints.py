"""Constrained decoding: deterministic automata over token ids (generate(constraint=), generate_batch(constraint=)).

The host side, numpy only and checkable without a GPU: the automaton in the CSR form rv_constrain_rows_f32 reads
(csrc/constrain.hip), its validation, the builders (a trie of answer choices; a character DFA lifted to a tokenizer's vocabulary; the
character DFA of the box strings create_instructions.format_boxes prints), the replay of a token sequence and the stacking of several
automata into the one table a call uploads.

A row's state is a state number s >= 0 (live: the allowed ids are edge_tok[edge_off[s] : edge_off[s + 1]], and taking edge e leads to
edge_next[e]), FREE (-1: the row is not touched; where an EOS edge leads, so a finished row is free, and what an unconstrained row
carries) or DEAD (-2: a token was taken that the state does not allow; the row is all -inf)."""
import numpy as np

FREE, DEAD = -1, -2
MAX_EDGES = 1 << 24          # edges of one table (stacked tables included): three rounds of the kernel's 256-ary edge search


def _ids(name, v):
    try:
        out = [int(i) for i in v]
    except (TypeError, ValueError):
        raise ValueError(f"`{name}` has to be a sequence of token ids, but is {v!r}") from None
    if any(isinstance(i, (bool, np.bool_)) or not isinstance(i, (int, np.integer)) for i in v) or any(i < 0 or i >= 2 ** 31 for i in out):
        raise ValueError(f"`{name}` has to hold token ids in [0, 2^31), but is {v!r}")
    return out


class TokenConstraint:
    """A deterministic automaton over token ids in CSR form: edge_off int32 [n_states + 1], edge_tok int32 [n_edges] (strictly
    ascending within a state), edge_next int32 [n_edges] (a state number, or FREE), start.  The constructor validates and raises
    ValueError naming the state: dtypes and shapes; edge_off starting at 0, non-decreasing and ending at n_edges; ids >= 0, ascending
    and distinct per state; edge_next in [-1, n_states); start in [0, n_states); every state reachable from start with at least one
    edge (a live row could otherwise only die); at most MAX_EDGES edges."""

    def __init__(self, edge_off, edge_tok, edge_next, start):
        for name, a in (("edge_off", edge_off), ("edge_tok", edge_tok), ("edge_next", edge_next)):
            if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1:
                raise ValueError(f"`{name}` has to be a 1-D int32 numpy array, got {type(a).__name__}"
                                 f"{'' if not isinstance(a, np.ndarray) else f' {a.dtype} {a.shape}'}")
        if isinstance(start, (bool, np.bool_)) or not isinstance(start, (int, np.integer)):
            raise ValueError(f"`start` has to be a state number, but is {start!r}")
        n_states, n_edges = edge_off.shape[0] - 1, edge_tok.shape[0]
        if n_states < 1:
            raise ValueError("`edge_off` has to hold n_states + 1 >= 2 entries")
        if edge_next.shape[0] != n_edges:
            raise ValueError(f"`edge_tok` holds {n_edges} edges, `edge_next` {edge_next.shape[0]}")
        if n_edges > MAX_EDGES:
            raise ValueError(f"the automaton has {n_edges} edges; at most {MAX_EDGES} are taken")
        if not 0 <= start < n_states:
            raise ValueError(f"`start` is {start}, outside [0, {n_states})")
        off = edge_off.astype(np.int64)
        if off[0] != 0 or off[-1] != n_edges:
            raise ValueError(f"`edge_off` has to run from 0 to n_edges = {n_edges}, but runs from {off[0]} to {off[-1]}")
        bad = np.flatnonzero(np.diff(off) < 0)
        if bad.size:
            raise ValueError(f"state {int(bad[0])}: `edge_off` decreases")
        owner = np.repeat(np.arange(n_states, dtype=np.int64), np.diff(off))          # the state of every edge
        if n_edges:
            bad = np.flatnonzero(edge_tok < 0)
            if bad.size:
                raise ValueError(f"state {int(owner[bad[0]])}: a negative token id ({int(edge_tok[bad[0]])})")
            same = owner[1:] == owner[:-1]
            bad = np.flatnonzero(same & (np.diff(edge_tok.astype(np.int64)) <= 0))
            if bad.size:
                raise ValueError(f"state {int(owner[bad[0]])}: its token ids have to be strictly ascending (distinct), but "
                                 f"{int(edge_tok[bad[0]])} is followed by {int(edge_tok[bad[0] + 1])}")
            bad = np.flatnonzero((edge_next < FREE) | (edge_next >= n_states))
            if bad.size:
                raise ValueError(f"state {int(owner[bad[0]])}: edge_next {int(edge_next[bad[0]])} lies outside [-1, {n_states})")
        self.edge_off, self.edge_tok, self.edge_next = (np.ascontiguousarray(a) for a in (edge_off, edge_tok, edge_next))
        self.start = int(start)
        self.n_states, self.n_edges = n_states, n_edges
        self.max_token = int(edge_tok.max()) if n_edges else -1
        # one sorted key per edge: (state, token) in the order of the table, for the vectorised advance
        self._base = self.max_token + 2
        self._keys = owner * self._base + edge_tok.astype(np.int64)
        seen = np.zeros(n_states, dtype=bool)
        seen[self.start] = True
        front = [self.start]
        while front:
            s = front.pop()
            if off[s] == off[s + 1]:
                raise ValueError(f"state {s} is reachable from the start state {self.start} but has no edge: a row there could only die")
            for t in np.unique(edge_next[off[s]:off[s + 1]]):
                if t >= 0 and not seen[t]:
                    seen[t] = True
                    front.append(int(t))
        self._dev = {}

    # ------------------------------------------------------------------ replay
    def allowed(self, s):
        """The ids state s allows, ascending int32; None for FREE (everything); empty for DEAD or a number outside [0, n_states)."""
        if s == FREE:
            return None
        if not 0 <= s < self.n_states:
            return np.zeros(0, dtype=np.int32)
        return self.edge_tok[self.edge_off[s]:self.edge_off[s + 1]]

    def advance(self, states, tokens):
        """The states after taking tokens[i] in states[i] (int64 arrays, any shape): a live state follows the token's edge, or becomes
        DEAD without one; a negative state stays.  What rv_constrain_rows_f32 does with tok."""
        s = np.asarray(states, dtype=np.int64)
        t = np.broadcast_to(np.asarray(tokens, dtype=np.int64), s.shape)
        out = s.copy()
        live = (s >= 0) & (s < self.n_states)
        out[(s >= self.n_states)] = DEAD
        if live.any():
            ok = live & (t >= 0) & (t < self._base)
            key = np.where(ok, s * self._base + t, -1)
            pos = np.minimum(np.searchsorted(self._keys, key), max(self.n_edges - 1, 0))
            hit = ok & (self._keys[pos] == key) if self.n_edges else np.zeros_like(ok)
            out[live] = DEAD
            out[hit] = self.edge_next[pos[hit]]
        return out

    def walk(self, tokens, start=None):
        """Replay a token sequence from `start` (default: the start state).  Returns (states, allowed): states int64 [len(tokens)], the
        state BEFORE each token; allowed[i] = self.allowed(states[i])."""
        s = self.start if start is None else int(start)
        states, allowed = [], []
        for tk in np.asarray(tokens, dtype=np.int64).reshape(-1):
            states.append(s)
            allowed.append(self.allowed(s))
            s = int(self.advance(np.array([s]), np.array([tk]))[0])
        return np.asarray(states, dtype=np.int64), allowed

    def accepts(self, tokens):
        """True when the sequence is allowed token by token and ends in FREE (it took an EOS edge)."""
        s = self.start
        for tk in np.asarray(tokens, dtype=np.int64).reshape(-1):
            if s < 0:
                return False
            s = int(self.advance(np.array([s]), np.array([tk]))[0])
        return s == FREE

    # ------------------------------------------------------------------ tables
    @staticmethod
    def stack(constraints):
        """One table for a list of constraints (None entries: unconstrained): (table, starts).  table is a TokenConstraint holding
        every distinct object's states once, its state numbers offset (None when every entry is None); starts int32 [len] is each
        entry's start state in it, FREE for None.  A call uploads this one table whatever its rows or requests carry."""
        cs = list(constraints)
        for c in cs:
            if c is not None and not isinstance(c, TokenConstraint):
                raise ValueError(f"a constraint has to be a TokenConstraint or None, not {type(c).__name__}")
        parts, base, n = [], {}, 0
        for c in cs:
            if c is not None and id(c) not in base:
                base[id(c)] = n
                parts.append(c)
                n += c.n_states
        starts = np.array([FREE if c is None else base[id(c)] + c.start for c in cs], dtype=np.int32)
        if not parts:
            return None, starts
        if len(parts) == 1:
            return parts[0], starts
        if sum(c.n_edges for c in parts) > MAX_EDGES:
            raise ValueError(f"the constraints of this call hold {sum(c.n_edges for c in parts)} edges together; at most {MAX_EDGES}")
        off, e = [np.zeros(1, dtype=np.int64)], 0
        for c in parts:
            off.append(c.edge_off[1:].astype(np.int64) + e)
            e += c.n_edges
        nxt = [np.where(c.edge_next >= 0, c.edge_next + base[id(c)], c.edge_next) for c in parts]
        table = TokenConstraint(np.concatenate(off).astype(np.int32), np.concatenate([c.edge_tok for c in parts]),
                                np.concatenate(nxt).astype(np.int32), int(starts[starts >= 0][0]))
        return table, starts

    def device_tables(self, device):
        """(edge_off, edge_tok, edge_next) as int32 tensors on `device`, uploaded once per device."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.edge_off, self.edge_tok, self.edge_next))
        return self._dev[key]

    # ------------------------------------------------------------------ builders
    @classmethod
    def _from_edges(cls, edges, start=0):
        """edges: per state a dict {token id: next state}."""
        off = np.zeros(len(edges) + 1, dtype=np.int64)
        tok, nxt = [], []
        for s, d in enumerate(edges):
            ks = sorted(d)
            tok.extend(ks)
            nxt.extend(d[k] for k in ks)
            off[s + 1] = len(tok)
        if len(tok) > MAX_EDGES:
            raise ValueError(f"the automaton has {len(tok)} edges; at most {MAX_EDGES} are taken")
        return cls(off.astype(np.int32), np.asarray(tok, dtype=np.int32), np.asarray(nxt, dtype=np.int32), start)

    @classmethod
    def from_choices(cls, seqs, eos):
        """The trie of the token-id sequences `seqs` (closed answer sets): a row may generate exactly one of them and then an EOS id
        (`eos`: an id or a list of ids), which leads to FREE.  A choice that is a prefix of another allows both the EOS and the
        continuation; duplicates are merged.  ValueError for an empty list, an empty sequence or an empty `eos`."""
        eos = _ids("eos", [eos] if isinstance(eos, (int, np.integer)) and not isinstance(eos, bool) else eos)
        if not eos:
            raise ValueError("`eos` is empty: a choice could never end")
        try:
            seqs = [list(s) for s in seqs]
        except TypeError:
            raise ValueError(f"`seqs` has to be a list of token-id sequences, but is {seqs!r}") from None
        if not seqs:
            raise ValueError("`seqs` is empty: there is nothing to choose from")
        edges = [{}]
        for i, s in enumerate(seqs):
            s = _ids(f"seqs[{i}]", s)
            if not s:
                raise ValueError(f"`seqs[{i}]` is empty: a choice needs at least one token")
            at = 0
            for tk in s:
                if tk in eos:
                    raise ValueError(f"`seqs[{i}]` holds the EOS id {tk}")
                if tk not in edges[at]:
                    edges.append({})
                    edges[at][tk] = len(edges) - 1
                at = edges[at][tk]
            for e in eos:
                edges[at][e] = FREE
        return cls._from_edges(edges)

    @classmethod
    def from_char_dfa(cls, token_strings, delta, start, accepting, eos):
        """Lift a character DFA to a vocabulary.  delta: dict (state, char) -> state (states: any hashable); token_strings[i]: the
        decoded text of id i, None or "" for an id that is never allowed (special tokens; the EOS ids are taken as such whatever
        their text).  State s gets the edge (i -> s') when walking token_strings[i] from s stays inside delta and ends in s'; every
        accepting state also gets the EOS edges to FREE.  Only states the vocabulary can reach from `start` are built, and those
        from which no token path reaches an accepting state are pruned first, with the edges into them, so every state kept has an
        edge.  ValueError when `start` itself is pruned (the vocabulary cannot spell any accepted string), or for an empty `eos`."""
        eos = _ids("eos", [eos] if isinstance(eos, (int, np.integer)) and not isinstance(eos, bool) else eos)
        if not eos:
            raise ValueError("`eos` is empty: an accepted string could never end")
        accepting = set(accepting)
        by_state = {}
        for (s, ch), t in delta.items():
            if not isinstance(ch, str) or len(ch) != 1:
                raise ValueError(f"delta: the key ({s!r}, {ch!r}) has to pair a state with one character")
            by_state.setdefault(s, {})[ch] = t
        # the vocabulary as a trie: node = [children {char: node}, ids ending here]
        root = [{}, []]
        for i, text in enumerate(token_strings):
            if not text or i in eos:
                continue
            node = root
            for ch in text:
                node = node[0].setdefault(ch, [{}, []])
            node[1].append(i)
        # token edges of every state the vocabulary reaches from start: the trie and the DFA walked together
        number, order, edges = {start: 0}, [start], []
        k = 0
        while k < len(order):
            out = {}
            stack = [(root, order[k])]
            while stack:
                node, s = stack.pop()
                for i in node[1]:
                    out[i] = s
                row = by_state.get(s)
                if row:
                    for ch, child in node[0].items():
                        if ch in row:
                            stack.append((child, row[ch]))
            for i, t in out.items():
                if t not in number:
                    number[t] = len(order)
                    order.append(t)
            edges.append({i: number[t] for i, t in out.items()})
            k += 1
        # prune: keep the states with a token path to an accepting state
        n = len(order)
        rev = [[] for _ in range(n)]
        for s, d in enumerate(edges):
            for t in set(d.values()):
                rev[t].append(s)
        keep = np.zeros(n, dtype=bool)
        front = [s for s in range(n) if order[s] in accepting]
        keep[front] = True
        while front:
            for p in rev[front.pop()]:
                if not keep[p]:
                    keep[p] = True
                    front.append(p)
        if not keep[0]:
            raise ValueError("from_char_dfa: no sequence of this vocabulary's tokens leads from the start state to an accepting state")
        new = np.cumsum(keep) - 1
        final = []
        for s in range(n):
            if not keep[s]:
                continue
            d = {i: int(new[t]) for i, t in edges[s].items() if keep[t]}
            if order[s] in accepting:
                for e in eos:
                    d[e] = FREE
            final.append(d)
        return cls._from_edges(final)


BOXES_MAX_NUM_FLOAT = 4       # str(round(v, k)) switches to exponent notation below 1e-4


def boxes_char_dfa(num_float=2):
    """The character DFA of exactly the strings data.create_instructions.format_boxes(boxes, num_float) prints for float coordinates
    in [0, 1]: one or more "[a, b, c, d]", joined by ", " with " and " before the last.  A number is what str(round(v, num_float))
    prints for a float v in [0, 1]: "1.0", or "0." and 1 .. num_float digits of which the last is not 0 unless it is the only one
    ("0.0", "0.5", "0.05", never "0.50" or "0.00"; num_float 0: "0.0" and "1.0" alone).  Returns (delta, start, accepting) for TokenConstraint.from_char_dfa.
    num_float in 0 .. 4 (beyond that str() prints exponents)."""
    if isinstance(num_float, bool) or not isinstance(num_float, (int, np.integer)) or not 0 <= num_float <= BOXES_MAX_NUM_FLOAT:
        raise ValueError(f"`num_float` has to be an int in [0, {BOXES_MAX_NUM_FLOAT}], but is {num_float!r}")
    digits = max(int(num_float), 1)
    delta, count = {}, [0]

    def new():
        count[0] += 1
        return count[0] - 1

    def lit(s, text, to):
        """The chain of `text` from s; its last character leads to `to`."""
        for i, ch in enumerate(text):
            t = delta.get((s, ch))
            if t is None:
                t = to if i == len(text) - 1 else new()
                delta[(s, ch)] = t
            s = t

    def number(s, term, to):
        """A number from s, followed by the literal `term`, which ends in `to`."""
        one = new()
        lit(s, "1.0", one)
        lit(one, term, to)
        frac = new()                                           # after "0."
        lit(s, "0.", frac)
        prev = [frac]                                          # the states after j - 1 digits that may take a j-th
        if num_float == 0:                                     # round(v, 0) prints "0.0" or "1.0" only
            zero = new()
            delta[(frac, "0")] = zero
            lit(zero, term, to)
            return
        for j in range(1, digits + 1):
            nonzero = new()                                    # after j digits, the last one not 0
            zero = new() if j == 1 or j < digits else None     # the last one 0: "0.0" ends there, later zeros need a digit after them
            for p in prev:
                if zero is not None:
                    delta[(p, "0")] = zero
                for d in "123456789":
                    delta[(p, d)] = nonzero
            lit(nonzero, term, to)
            if j == 1:
                lit(zero, term, to)                            # "0.0"
            prev = [nonzero] if zero is None else [zero, nonzero]

    def box(s, end):
        a = new()
        lit(s, "[", a)
        for term in (", ", ", ", ", "):
            b = new()
            number(a, term, b)
            a = b
        number(a, "]", end)

    start, first_end, mid_end, last_end, mid, last = (new() for _ in range(6))
    box(start, first_end)
    box(mid, mid_end)
    box(last, last_end)
    for e in (first_end, mid_end):
        lit(e, ", ", mid)
        lit(e, " and ", last)
    return delta, start, {first_end, last_end}


def char_dfa_accepts(dfa, text):
    """True when the character DFA (delta, start, accepting) accepts `text`."""
    delta, s, accepting = dfa
    for ch in text:
        if (s, ch) not in delta:
            return False
        s = delta[(s, ch)]
    return s in accepting


def resolve_constraints(constraint, n, vocab, what="row"):
    """The constraint= argument of a call with n rows or requests on a vocabulary of `vocab` ids -> (table, starts) as
    TokenConstraint.stack gives them; table None when nothing is constrained.  One TokenConstraint serves every row; a list or tuple
    holds one entry (a TokenConstraint or None) per row.  ValueError for another type, another length, and an automaton whose largest
    token id is >= vocab (its edge could never be taken, and an EOS there would never end the answer)."""
    if constraint is None:
        return None, np.full(n, FREE, dtype=np.int32)
    if isinstance(constraint, TokenConstraint):
        cs = [constraint] * n
    elif isinstance(constraint, (list, tuple)):
        cs = list(constraint)
        if len(cs) != n:
            raise ValueError(f"`constraint` holds {len(cs)} entries for {n} {what}s")
    else:
        raise ValueError(f"`constraint` has to be a TokenConstraint or a list with one (or None) per {what}, not {type(constraint).__name__}")
    for i, c in enumerate(cs):
        if c is not None and not isinstance(c, TokenConstraint):
            raise ValueError(f"`constraint[{i}]` has to be a TokenConstraint or None, not {type(c).__name__}")
        if c is not None and c.max_token >= vocab:
            raise ValueError(f"{what} {i}: the constraint names token id {c.max_token}, but the model's vocabulary has {vocab} ids")
    return TokenConstraint.stack(cs)

"""numpy fp32 restatement of HF's greedy logits processors (transformers generation/logits_process.py), for the tests of
rv_logits_process_argmax_f32 and generate().  One row at a time; `hist` holds the tokens generated so far (inputs_embeds generation:
no prompt), pads of finished rows included.  Bad words set -inf, as the kernel does (HF adds -inf; the two differ only on a +inf / NaN
entry, which the tests leave out)."""
import numpy as np

NEG_INF = np.float32(-np.inf)


def process_row(x, hist, penalty=None, ngram=0, bad_words=None, eos=(), min_new=0, suppress=None, begin_suppress=None):
    """x: raw fp32 scores [V]; returns the processed copy, processors applied in HF's order.  bad_words: sequences with [eos] already
    dropped (generation.parse_generate_kwargs does that); min_new: the effective EOS minimum (generation.min_new_length)."""
    x = np.array(x, dtype=np.float32, copy=True)
    V = x.size
    h = [int(v) for v in hist]
    t = len(h)
    inv = lambda ids: [i for i in ids if 0 <= i < V]
    if penalty is not None and penalty != 1.0:                  # RepetitionPenaltyLogitsProcessor: once per distinct token
        p = np.float32(penalty)
        idx = np.array(sorted(set(inv(h))), dtype=np.int64)
        s = x[idx]
        x[idx] = np.where(s < 0, s * p, s / p)
    if ngram and t >= ngram:                                    # NoRepeatNGramLogitsProcessor
        pre = h[t - ngram + 1:]
        for i in range(t - ngram + 1):
            if h[i:i + ngram - 1] == pre and 0 <= h[i + ngram - 1] < V:
                x[h[i + ngram - 1]] = NEG_INF
    for w in bad_words or []:                                   # NoBadWordsLogitsProcessor
        w = list(w)
        if len(w) == 1 or (t >= len(w) and h[t - len(w) + 1:] == w[:-1]):
            x[w[-1]] = NEG_INF
    if t < min_new:                                             # MinLength / MinNewTokensLength
        x[inv(list(eos))] = NEG_INF
    x[inv(list(suppress or []))] = NEG_INF                      # SuppressTokensLogitsProcessor
    if t == 0:
        x[inv(list(begin_suppress or []))] = NEG_INF            # SuppressTokensAtBeginLogitsProcessor (begin_index 0)
    return x


def argmax(x):
    """torch.argmax: lowest index among equal maxima, NaN above everything, 0 for an all -inf row."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.flatnonzero(np.isnan(x))
    if nan.size:
        return int(nan[0])
    return int(np.argmax(x))


def same_values(a, b):
    """Equal by value, NaN equal to NaN (so -0.0 == +0.0)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def has_repeated_ngram(tokens, n):
    seen = set()
    for i in range(len(tokens) - n + 1):
        g = tuple(int(v) for v in tokens[i:i + n])
        if g in seen:
            return True
        seen.add(g)
    return False

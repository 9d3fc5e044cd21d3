"""Reward functions for GRPO training (host only).  A reward function is called as f(prompts=, completions=, completion_ids=,
**dataset columns) and returns one float per completion (TRL's convention)."""
import functools
import re

from .constraints import boxes_char_dfa, char_dfa_accepts

_NUMBER = re.compile(r"[01]\.[0-9]+")


@functools.lru_cache(maxsize=None)
def _dfa(num_float):
    return boxes_char_dfa(num_float)


def parse_boxes(text, num_float=2):
    """The inverse of data.create_instructions.format_boxes: "[a, b, c, d], [..] and [..]" -> [[a, b, c, d], ...] (floats), and None for
    any string that function cannot print for float coordinates in [0, 1] (constraints.boxes_char_dfa decides that: no extra space, no
    trailing zero, no missing " and ", no text around it)."""
    if not isinstance(text, str) or not char_dfa_accepts(_dfa(num_float), text):
        return None
    v = [float(t) for t in _NUMBER.findall(text)]
    return [v[i:i + 4] for i in range(0, len(v), 4)]


def box_iou(a, b):
    """Intersection over union of two [x1, y1, x2, y2] boxes; 0 for an empty or inverted box."""
    aw, ah, bw, bh = a[2] - a[0], a[3] - a[1], b[2] - b[0], b[3] - b[1]
    if aw <= 0 or ah <= 0 or bw <= 0 or bh <= 0:
        return 0.0
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / (aw * ah + bw * bh - inter)


def box_iou_reward(completions, boxes, num_float=2, **_):
    """The grounding reward: completions[i] (text) is parsed with parse_boxes and matched to the true boxes[i] greedily by descending
    IoU (each box used once; ties: the lower predicted, then the lower true index); the reward is the sum of the matched IoUs over
    max(n_pred, n_true), and 0 for a completion that does not parse or an empty truth."""
    out = []
    for text, truth in zip(completions, boxes):
        pred = parse_boxes(text, num_float)
        truth = [list(t[:4]) for t in (truth or [])]
        if not pred or not truth:
            out.append(0.0)
            continue
        pairs = sorted(((box_iou(p, t), i, j) for i, p in enumerate(pred) for j, t in enumerate(truth)), key=lambda x: (-x[0], x[1], x[2]))
        used_p, used_t, total = set(), set(), 0.0
        for iou, i, j in pairs:
            if iou <= 0:
                break
            if i in used_p or j in used_t:
                continue
            used_p.add(i)
            used_t.add(j)
            total += iou
        out.append(total / max(len(pred), len(truth)))
    return out

"""Host side of the 8-bit AdamW state (numpy only, importable without a GPU): which tensors take 8-bit moments, where their blocks
and the remaining fp32 moments live, the committed codebook and its hash, and the reading of --optim.

The format is defined in csrc/adam8_codebook.h (the tables) and tests/adam8_ref.py (the rule); DESIGN.md "8-bit optimizer state".

Layout of an 8-bit state over a FlatParams buffer:
  * an 8-bit tensor of n elements owns ceil(n / 256) consecutive blocks; block b's codes are bytes [256 b, 256 b + 256) of the code
    buffer (a short last block leaves its remaining bytes unused), its scale is absmax[b].  Blocks never straddle tensors;
  * consecutive 32-bit tensors form a segment whose fp32 moments sit in a compact buffer at the same offsets relative to the
    segment's (64-element aligned) start as in the flat buffer, so rv_adamw runs on a slice of it as it does on the full buffers.
"""
import hashlib
import os
import re

import numpy as np

BLOCK = 256
MIN_8BIT_SIZE = 4096
_ALIGN = 64
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "adam8_codebook.h")

OPTIM_8BIT = ("adamw_bnb_8bit", "adamw_8bit")
OPTIM_32BIT = ("adamw_torch", "adamw_hf", "adamw_torch_fused", "adamw_apex_fused", "adamw_anyprecision", "adamw_torch_xla",
               "adamw_torch_npu_fused")


def is_embedding(name):
    """nn.Embedding tables: the token table and the towers' position embeddings (they keep 32-bit state, as the reference's
    override for Adam8bit does)."""
    return name.endswith("embed_tokens.weight") or name.endswith("position_embedding.weight")


def takes_8bit(name, shape):
    return len(shape) >= 2 and int(np.prod(shape)) >= MIN_8BIT_SIZE and not is_embedding(name)


def optim_state_bits(optim, warn=None):
    """--optim -> 8 or 32.  A value that names neither an 8-bit nor an fp32 AdamW keeps fp32 AdamW; `warn` (a callable) is told once."""
    if optim in OPTIM_8BIT:
        return 8
    if optim not in OPTIM_32BIT and warn is not None:
        warn(f"--optim {optim}: not implemented here, training with fp32 AdamW (adamw_torch)")
    return 32


class StatePlan:
    """Per-tensor table of a flat parameter layout.  tensors: name -> dict(off, n, bits, and for 8 bits `block` (first block index),
    for 32 bits `pos` (offset of the tensor's moments in the compact fp32 buffer)).  nblocks / n32: sizes of absmax / compact buffers."""

    def __init__(self, offsets, shapes):
        self.tensors = {}
        nb, n32, seg = 0, 0, None                           # seg: (flat start rounded down to _ALIGN, compact start) of the open segment
        for name, (off, n) in offsets.items():
            if takes_8bit(name, shapes[name]):
                self.tensors[name] = dict(off=off, n=n, bits=8, block=nb)
                nb += (n + BLOCK - 1) // BLOCK
                seg = None
            else:
                if seg is None:
                    n32 = (n32 + _ALIGN - 1) // _ALIGN * _ALIGN
                    seg = (off // _ALIGN * _ALIGN, n32)
                pos = seg[1] + off - seg[0]
                self.tensors[name] = dict(off=off, n=n, bits=32, pos=pos)
                n32 = pos + n
        self.nblocks = nb
        self.n32 = (n32 + _ALIGN - 1) // _ALIGN * _ALIGN
        self.ncodes = nb * BLOCK

    def names(self, bits=None):
        return [k for k, t in self.tensors.items() if bits is None or t["bits"] == bits]

    def runs(self, start, end):
        """The tensors inside the flat slice [start, end), in order, as maximal runs of one width:
        (8, [names]) or (32, flat_start, flat_end, compact_start)."""
        out = []
        for name, t in self.tensors.items():
            if t["off"] < start or t["off"] + t["n"] > end:
                continue
            if t["bits"] == 8:
                if out and out[-1][0] == 8:
                    out[-1][1].append(name)
                else:
                    out.append((8, [name]))
            elif out and out[-1][0] == 32 and out[-1][3] + t["off"] - out[-1][1] == t["pos"]:
                out[-1] = (32, out[-1][1], t["off"] + t["n"], out[-1][3])
            else:
                out.append((32, t["off"], t["off"] + t["n"], t["pos"]))
        return out

    def block_table(self, names, origin=0):
        """int64 [3, T]: start (relative to `origin`), length and first block (relative to the first tensor's) of the 8-bit tensors
        `names`, which must own consecutive blocks."""
        ts = [self.tensors[k] for k in names]
        tab = np.array([[t["off"] - origin for t in ts], [t["n"] for t in ts], [t["block"] - ts[0]["block"] for t in ts]], np.int64)
        nb = (tab[1] + BLOCK - 1) // BLOCK
        assert all(t["bits"] == 8 for t in ts) and np.array_equal(tab[2], np.cumsum(nb) - nb), names
        return tab, int(nb.sum())


def read_codebook(path=_HEADER):
    """(signed, unsigned) fp32 [256] tables of the committed header."""
    text = open(path).read()
    out = []
    for name in ("rv_adam8_signed_bits", "rv_adam8_unsigned_bits"):
        m = re.search(name + r"\[256\]\s*=\s*\{([^}]*)\}", text)
        if not m:
            raise ValueError(f"{path}: table {name} not found")
        words = np.array([int(w, 16) for w in re.findall(r"0x[0-9a-fA-F]{8}", m.group(1))], np.uint32)
        if words.size != 256:
            raise ValueError(f"{path}: {name} has {words.size} entries")
        out.append(words.view(np.float32))
    return tuple(out)


def codebook_sha(path=_HEADER):
    """sha256 of the two tables' 2 x 256 little-endian fp32 words: what a checkpoint records and a resume compares."""
    s, u = read_codebook(path)
    return hashlib.sha256(s.astype("<f4").tobytes() + u.astype("<f4").tobytes()).hexdigest()

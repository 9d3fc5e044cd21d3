"""Host side of the NF4 frozen decoder base (QLoRA; numpy arithmetic only, usable without a GPU): the table and its midpoints, the fixed-order
mean of double quantisation, where every tensor's codes, absmax entries and second-level blocks live (BasePlan), the bytes of the store,
the committed tables' hash and the reading of --bits / --quant_type / --lora_enable.

The format is defined in csrc/nf4_codebook.h (the table), csrc/adam8_codebook.h (the second level's signed 8-bit table) and
tests/nf4_ref.py (the rule); DESIGN.md 5i.  bitsandbytes is not importable here and none of its files is read or written.

Layout of the store, all layers in one set of buffers:
  * codes: uint8; a tensor of n weights owns ceil(n / 2) bytes from a 16-byte aligned offset;
  * plain: absmax fp32, ceil(n / 64) entries per tensor from an entry that is a multiple of 4 (16 bytes);
  * double quantisation: absmax_codes uint8, ceil(n / 64) entries per tensor from a multiple of 16; scale2 fp32, one per 256 blocks of the
    tensor, from a multiple of 4; offset fp32, one per tensor (layer-major, seven per layer).
A second-level block never straddles two tensors, as a block never does.
"""
import hashlib
import os
import re

import numpy as np

from .params import ALIGN, LORA_TARGETS

BLOCK = 64
BLOCK2 = 256
CHUNK = 2048                      # weights one wave of rv_nf4_dequant_bf16 owns (csrc/nf4.hip NF4_CHUNK)
_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER = os.path.join(_HERE, "csrc", "nf4_codebook.h")
F32 = np.float32


def read_table(path=_HEADER):
    """The fp32 [16] table of the committed header."""
    m = re.search(r"rv_nf4_bits\[16\]\s*=\s*\{([^}]*)\}", open(path).read())
    if not m:
        raise ValueError(f"{path}: table rv_nf4_bits not found")
    words = np.array([int(w, 16) for w in re.findall(r"0x[0-9a-fA-F]{8}", m.group(1))], np.uint32)
    if words.size != 16:
        raise ValueError(f"{path}: rv_nf4_bits has {words.size} entries")
    return words.view(F32)


def midpoints(t):
    """mid[i] = fp32((float64(t[i]) + float64(t[i + 1])) / 2); the code of a is the number of midpoints strictly below it."""
    return ((t[:-1].astype(np.float64) + t[1:].astype(np.float64)) / 2.0).astype(F32)


def codebook_sha():
    """sha256 of the header tables a dequantised weight depends on: the sixteen NF4 levels, then the signed 8-bit table of the second
    level, as little-endian fp32 words.  trainer_state.json records it and a resume compares it."""
    from .optim8 import read_codebook
    return hashlib.sha256(read_table().astype("<f4").tobytes() + read_codebook()[0].astype("<f4").tobytes()).hexdigest()


def absmax_offset(absmax):
    """fp32(mean(absmax)) of ONE tensor, the float64 sum taken left to right from block 0 (np.add.accumulate adds in exactly that
    order; np.sum would add pairwise)."""
    a = np.asarray(absmax, F32).astype(np.float64)
    return F32(np.add.accumulate(a)[-1] / a.size)


def _ru(x, m):
    return (x + m - 1) // m * m


def matrix_shapes(geo):
    """(module, rows, cols) of the seven quantised matrices of a decoder layer, in storage order."""
    l = geo["lm"]
    kvd = l["d"] // l["heads"] * l.get("kv_heads", l["heads"])
    return [(t, kvd if t in ("self_attn.k_proj", "self_attn.v_proj") else l[o], l[k]) for t, o, k in LORA_TARGETS]


def matrix_names(geo):
    return [f"model.layers.{i}.{t}.weight" for i in range(geo["lm"]["layers"]) for t, _, _ in LORA_TARGETS]


class BasePlan:
    """Where the NF4 store of a geometry lives.  tensors: name -> dict(layer, n, shape, code (first code byte), block (first absmax
    entry), nblocks, scale2 / nscale2 (first second-level scale and their number; double quantisation only), slot (index into the
    per-tensor offsets), dst (first element in the one-layer scratch)).  The scratch holds q|k|v adjacent and gate|up adjacent, so the
    fused views of _layer_views are plain views of it; every group starts on 64 elements, as in FlatParams."""

    def __init__(self, geo, double_quant=False):
        self.geo, self.double_quant = geo, bool(double_quant)
        self.layers = geo["lm"]["layers"]
        mats = matrix_shapes(geo)
        dst, off = {}, 0
        for t, rows, cols in mats:
            if t not in ("self_attn.k_proj", "self_attn.v_proj", "mlp.up_proj"):
                off = _ru(off, ALIGN)
            dst[t] = off
            off += rows * cols
        self.scratch_numel = _ru(off, ALIGN)
        self.tensors = {}
        code, blk, s2 = 0, 0, 0
        for i in range(self.layers):
            for j, (t, rows, cols) in enumerate(mats):
                n = rows * cols
                nb = (n + BLOCK - 1) // BLOCK
                code, blk, s2 = _ru(code, 16), _ru(blk, 16 if self.double_quant else 4), _ru(s2, 4)
                ent = dict(layer=i, n=n, shape=(rows, cols), code=code, block=blk, nblocks=nb, slot=i * len(mats) + j, dst=dst[t])
                if self.double_quant:
                    ent.update(scale2=s2, nscale2=(nb + BLOCK2 - 1) // BLOCK2)
                    s2 += ent["nscale2"]
                self.tensors[f"model.layers.{i}.{t}.weight"] = ent
                code += (n + 1) // 2
                blk += nb
        self.code_bytes, self.nblocks, self.nscale2 = code, blk, s2
        self.per_layer = len(mats)

    def names(self, layer=None):
        return [k for k, t in self.tensors.items() if layer is None or t["layer"] == layer]

    @property
    def weights(self):
        return sum(t["n"] for t in self.tensors.values())

    def base_weight_bytes(self):
        """Bytes of the quantised store (alignment padding included; none at the built-in 7B and 13B geometries)."""
        if self.double_quant:
            return self.code_bytes + self.nblocks + 4 * self.nscale2 + 4 * len(self.tensors)
        return self.code_bytes + 4 * self.nblocks

    def scratch_bytes(self):
        return 2 * self.scratch_numel

    def table(self, names, dst=None):
        """int64 [6, T] of rv_nf4_dequant_bf16 for `names` and the number of chunks: first chunk, first code byte, first absmax entry,
        length, first destination element (dst: name -> element, default the scratch offsets), first second-level scale."""
        ts = [self.tensors[k] for k in names]
        nch = np.array([(t["n"] + CHUNK - 1) // CHUNK for t in ts], np.int64)
        tab = np.array([np.cumsum(nch) - nch, [t["code"] for t in ts], [t["block"] for t in ts], [t["n"] for t in ts],
                        [(t["dst"] if dst is None else dst[k]) for k, t in zip(names, ts)], [t.get("scale2", 0) for t in ts]], np.int64)
        return tab, int(nch.sum())


def bf16_matrix_bytes(geo):
    return 2 * geo["lm"]["layers"] * sum(r * c for _, r, c in matrix_shapes(geo))


def base_weight_bytes(geo, quant_type=None, double_quant=False):
    """Bytes the seven decoder matrices of every layer take: bf16 (quant_type None) or the NF4 store."""
    if quant_type is None:
        return bf16_matrix_bytes(geo)
    if quant_type != "nf4":
        raise ValueError(f"quant_type {quant_type!r}: only 'nf4' is built")
    return BasePlan(geo, double_quant).base_weight_bytes()


def base_quant_record(double_quant):
    """What trainer_state.json keeps under "base_quant" for an NF4 run."""
    return {"type": "nf4", "block": BLOCK, "double_quant": bool(double_quant), "codebook": codebook_sha()}


def base_quant_choice(bits, quant_type, lora_enable, say=None):
    """--bits / --quant_type / --lora_enable -> "nf4" (quantise the frozen base after the weights are loaded) or None (train as
    before).  Every combination but --bits 16 tells `say` (a callable) once what happens."""
    bits = int(bits)
    if bits == 4 and lora_enable and quant_type == "nf4":
        return "nf4"
    if say is not None and bits != 16:
        if bits == 4 and not lora_enable:
            why = "--bits 4 without --lora_enable: a 4-bit base cannot be trained itself"
        elif bits == 4:
            why = f"--bits 4 --quant_type {quant_type}: only nf4 is built"
        elif bits == 8:
            why = "--bits 8: LLM.int8 training is not built"
        else:
            why = f"--bits {bits}: not a width this build knows"
        say(f"[train] {why}; training on the bf16 base as with --bits 16")
    return None

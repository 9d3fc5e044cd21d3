"""Per-image attention maps from generate(output_attentions=True): where each projector row of an image sits on the key axis of the
returned attention rows, and the attention mass at every patch per generated token (the usual LLaVA reading: "which part of the
radiograph did the model look at when it wrote this word").  numpy only, importable without a GPU: this is post-processing of returned
data, not model arithmetic.

The key axis of .attentions is each sequence's CACHE positions 0 .. len_b - 1 -- the index among the valid positions of the spliced
row, whatever the padding side, as generation.position_records counts them -- so everything here works on those.
"""
import numpy as np


def image_token_positions(plan):
    """Where the splice put every image.  plan: LlavaEngine.plan()'s dict (idx, image_rows, attention_mask, lens are read).  Returns a
    list with one dict per image i: seq (the owning sequence b; -1: no row of the image was spliced, e.g. the dummy image of a
    text-only sample), pos (int64 [p1 - p0]: the cache position where projector row k of the image landed, -1 when the merge dropped
    it -- unpad crops, anyres_max resamples, maxpool pools) and extra_pos (int64 [e1 - e0]: the same for the rows the merge CREATED for
    the image, anyres_max's down-sampled grid in row-major order).  image_newline rows belong to no image and are left out."""
    am = np.asarray(plan["attention_mask"]).astype(bool)
    B, S = am.shape
    idx = np.asarray(plan["idx"]).reshape(B, S).astype(np.int64)
    lens = np.asarray(plan["lens"]).astype(np.int64)
    rank = np.cumsum(am, axis=1) - 1                               # cache position of every valid padded position
    assert (am.sum(1) == lens).all(), "the plan's attention_mask and lens disagree"
    n_feat = max([max(p1, e1) for _, p1, _, e1 in plan["image_rows"]], default=0)
    feat = np.where(am & (idx <= -2), -idx - 2, -1)                # feature-table row at every position; n_feat_rows = the newline
    where_b = np.full(n_feat, -1, dtype=np.int64)
    where_p = np.full(n_feat, -1, dtype=np.int64)
    bb, ss = np.nonzero((feat >= 0) & (feat < n_feat))
    where_b[feat[bb, ss]], where_p[feat[bb, ss]] = bb, rank[bb, ss]
    out = []
    for p0, p1, e0, e1 in plan["image_rows"]:
        owners = np.unique(np.concatenate([where_b[p0:p1], where_b[e0:e1]]))
        owners = owners[owners >= 0]
        assert owners.size <= 1, "an image's rows landed in more than one sequence"
        out.append(dict(seq=int(owners[0]) if owners.size else -1, pos=where_p[p0:p1].copy(), extra_pos=where_p[e0:e1].copy()))
    return out


def image_attention_map(attn_row, pos, n_tiles, side):
    """float32 [n_tiles, side, side]: attn_row[pos[k]] at patch k (tile-major, row-major inside a tile) and 0 where pos[k] is -1 or past
    the row's end.  attn_row: one attention row over the cache positions (1-D); pos: image_token_positions()[i]["pos"]."""
    attn_row, pos = np.asarray(attn_row).reshape(-1), np.asarray(pos, dtype=np.int64).reshape(-1)
    if pos.size != n_tiles * side * side:
        raise ValueError(f"pos holds {pos.size} rows, {n_tiles} tiles of {side} x {side} patches hold {n_tiles * side * side}")
    ok = (pos >= 0) & (pos < attn_row.size)
    out = np.zeros(pos.size, dtype=np.float32)
    out[ok] = attn_row[pos[ok]]
    return out.reshape(n_tiles, side, side)


def step_image_maps(out, plan, layer=-1, side=None, image=0):
    """One patch map per generated step from out.attentions (generate(output_attentions=True, return_dict_in_generate=True)) for image
    `image` of the call: float32 [steps, n_tiles, side, side].  layer indexes the asked layers (out.attention_layers; -1: the last
    asked one).  Both the per-head form [B, H, 1, L_t] and the "mean_heads" form [B, 1, 1, L_t] are taken; heads are averaged here on
    the host in float64.  side: patches per tile edge (engine.side); None: the image is one square tile."""
    im = image_token_positions(plan)[image]
    if im["seq"] < 0:
        raise ValueError(f"image {image} was not spliced into any sequence")
    n = im["pos"].size
    if side is None:
        side = int(round(n ** 0.5))
    if side <= 0 or n % (side * side):
        raise ValueError(f"image {image} has {n} projector rows, not a whole number of {side} x {side} tiles: pass side=")
    maps = []
    for step in out.attentions:
        a = step[layer]
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        row = a[im["seq"], :, 0, :].astype(np.float64).mean(0)
        maps.append(image_attention_map(row, im["pos"], n // (side * side), side))
    return np.stack(maps) if maps else np.zeros((0, n // (side * side), side, side), dtype=np.float32)

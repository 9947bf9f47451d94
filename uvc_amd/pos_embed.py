"""Position embeddings across image grids: a checkpoint trained at one img_size / patch_size loaded into a model with another grid
(DeiT's 384-px fine-tuning starts from its 224-px weights).  Host code, run once per load on the CPU."""
import math

import torch
import torch.nn.functional as F


def resize_pos_embed(state_dict, grid, num_tokens=None, key="pos_embed"):
    """Return a copy of ``state_dict`` whose ``key`` [1, ntok + g*g, D] is resampled to the ``grid`` = (gh, gw) patch grid.

    The class / distillation token rows (the first ``num_tokens``; by default 1 or 2, whichever leaves a square grid) are kept bit for bit; the g x g patch grid is
    resampled bicubically (``F.interpolate(mode="bicubic", align_corners=False)``), as DeiT's fine-tuning at another resolution does.
    The result has the input's dtype.  On an equal grid the state dict comes back unchanged."""
    gh, gw = (grid, grid) if isinstance(grid, int) else (int(grid[0]), int(grid[1]))
    pe = state_dict[key]
    n = pe.shape[1]
    ntok = num_tokens if num_tokens is not None else n - math.isqrt(n - 1) ** 2
    g0 = math.isqrt(n - ntok)
    if g0 * g0 != n - ntok:
        raise ValueError(f"{key}: {n} rows are not {ntok} token rows and a square patch grid")
    if (g0, g0) == (gh, gw):
        return state_dict
    tok, patches = pe[:, :ntok], pe[:, ntok:]
    d = pe.shape[-1]
    img = patches.reshape(1, g0, g0, d).permute(0, 3, 1, 2).to(torch.float32)
    img = F.interpolate(img, size=(gh, gw), mode="bicubic", align_corners=False)
    patches = img.permute(0, 2, 3, 1).reshape(1, gh * gw, d).to(pe.dtype)
    out = dict(state_dict)
    out[key] = torch.cat([tok, patches], dim=1)
    return out


def match_pos_embed(state_dict, model, key="pos_embed"):
    """``resize_pos_embed`` to ``model``'s grid where the checkpoint's ``key`` has another number of rows; prints one line when it does."""
    if state_dict is None or key not in state_dict or not hasattr(model, key):
        return state_dict
    want = getattr(model, key).shape
    have = state_dict[key].shape
    if tuple(have) == tuple(want):
        return state_dict
    ntok = getattr(model, "num_tokens", None)
    if ntok is None:
        ntok = want[1] - math.isqrt(want[1] - 1) ** 2
    g = math.isqrt(want[1] - ntok)
    out = resize_pos_embed(state_dict, (g, g), ntok, key)
    print(f"pos_embed: resized from {tuple(have)} to {tuple(out[key].shape)} (bicubic, {g} x {g} patch grid)")
    return out

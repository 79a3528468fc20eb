"""numpy restatements of the two functions the reference's picture logging rests on, written from their published rules:
torchvision.utils.make_grid(tensor, nrow=8, padding=2, normalize=False, pad_value=0) and utils/misc.py:82-98 colour_seg_masks.
torchvision is not installed where this project is tested, so the geometry is pinned by the hand-written arrays of
tests/test_visualise_cpu.py; tests/golden/make_golden_visualise.py runs the reference's own visualise_outputs on top of
`make_grid_torch`."""
import json
import os.path as osp

import numpy as np

PALETTE15 = osp.join(osp.dirname(osp.abspath(__file__)), 'golden', 'colour_palette15.json')


def make_grid(images, nrow=8, padding=2, pad_value=0.0):
    """[n, C, H, W] (C = 1 or 3) -> [3, ymaps (H + padding) + padding, xmaps (W + padding) + padding] of the same dtype; image i
    at row (i // xmaps)(H + padding) + padding, column (i % xmaps)(W + padding) + padding; the bare image for n = 1."""
    t = np.asarray(images)
    assert t.ndim == 4 and t.shape[1] in (1, 3)
    if t.shape[1] == 1:
        t = np.concatenate([t, t, t], 1)
    n, _, H, W = t.shape
    if n == 1:
        return t[0].copy()
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    grid = np.full((3, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding), pad_value, dtype=t.dtype)
    for i in range(n):
        r, c = (i // xmaps) * (H + padding) + padding, (i % xmaps) * (W + padding) + padding
        grid[:, r:r + H, c:c + W] = t[i]
    return grid


def make_grid_torch(tensor, nrow=8, padding=2, pad_value=0.0):
    """The same on a host torch tensor (or a list of [C, H, W] tensors), dtype kept: what stands in for torchvision's function."""
    import torch
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), 0)
    return torch.from_numpy(make_grid(tensor.detach().cpu().numpy(), nrow, padding, pad_value))


def load_palette(path=PALETTE15):
    with open(path) as f:
        return json.load(f)['palette']


def colour_seg_masks(masks, palette=None):
    """[B, H, W] or [B, 1, H, W] integer labels -> int64 [B, 3, H, W]: palette[label], black for negative labels, IndexError for a
    label outside the palette (what indexing the reference's list raises)."""
    palette = load_palette() if palette is None else palette
    m = np.asarray(masks)
    if m.ndim == 3:
        m = m[:, None]
    assert m.ndim == 4 and m.shape[1] == 1
    if m.max() >= len(palette):
        raise IndexError('list index out of range')
    out = np.zeros((m.shape[0], 3) + m.shape[2:], np.int64)
    for label, rgb in enumerate(palette):
        for c in range(3):
            out[:, c][m[:, 0] == label] = rgb[c]
    return out


def sheet_fp32(first_col, slot_rows, K, padding=2, pad_value=1.0):
    """The fp32 sheet of genesis_amd.visualise's reconstruction_sheet / generation_sheet for ONE image: first_col per row a
    [3, H, W] array or None, slot_rows per row K arrays [3 or 1, H, W]; empty cells hold pad_value.  -> [3, Hg, Wg]."""
    cells = []
    for first, slots in zip(first_col, slot_rows):
        shape = (3,) + np.asarray(slots[0]).shape[1:]
        cells.append(np.full(shape, pad_value, np.float32) if first is None else np.asarray(first, np.float32))
        cells += [np.broadcast_to(np.asarray(s, np.float32), shape) for s in slots]
    return make_grid(np.stack(cells), K + 1, padding, pad_value)


def to_u8_hwc(grid):
    """fp32 [3, H, W] -> uint8 [H, W, 3]: rint(clip(v, 0, 1) 255), half to even."""
    return np.rint(np.clip(grid, 0.0, 1.0).astype(np.float32) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0)

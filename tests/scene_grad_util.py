"""Shared by tests/test_scene_grad_host.py and tests/test_gpu_scene_grad.py: the scene shape, the table of overlapping windows, and the
sequential restatement of msst_scene_fold_at on the CPU."""
import torch

BS, HS, WS = 2, 19, 17   # Hs != Ws, neither a multiple of a window


def overlap_table(window, Bs=BS, Hs=HS, Ws=WS):
    """17 rows (scene, y0, x0) for window x window windows, built from the shapes alone: a window at each corner of scene 0 and of the
    last scene, an exact repeat in each, windows that overlap (0, 0, 0) by one row and by one column, windows one pixel apart (an almost
    full overlap) in x, in y and diagonally -- in a fixed shuffled order with the scenes interleaved.  At least one pixel of each
    scene is in no window (asserted)."""
    my, mx, last = Hs - window, Ws - window, Bs - 1
    assert my >= window - 1 and mx >= window - 1 and Bs >= 2
    rows = [(0, 0, 0), (0, 0, mx), (0, my, 0), (0, my, mx), (0, 0, 0),              # the corners of scene 0 and a repeat
            (0, window - 1, 0), (0, 0, window - 1), (0, min(1, my), min(1, mx)),     # one row, one column, almost all of (0, 0, 0)
            (last, my, mx), (last, my, mx), (last, max(my - 1, 0), mx), (last, my, max(mx - 1, 0)),
            (last, 0, 0), (last, 0, mx), (last, my, 0), (last, my // 2, mx // 2), (last, my // 2 + 1, mx // 2)]
    assert all(0 <= s < Bs and 0 <= y <= my and 0 <= x <= mx for s, y, x in rows)
    table = torch.tensor(rows, dtype=torch.int32)[torch.randperm(len(rows), generator=torch.Generator().manual_seed(window))]
    assert int(cover_of(table, Bs, Hs, Ws, window).flatten(1).min(dim=1).values.max()) == 0
    return table


def grid_table(window, stride, Bs=BS, Hs=HS, Ws=WS):
    """the regular grid in grid order: (scene, window row, window column)"""
    from maskedsst_amd.scene import scene_windows
    return torch.tensor([(b, y, x) for b in range(Bs) for y, x in scene_windows(Hs, Ws, window, stride)], dtype=torch.int32)


def cover_of(table, Bs, Hs, Ws, window):
    cover = torch.zeros(Bs, Hs, Ws, dtype=torch.int32)
    for s, y, x in table.tolist():
        cover[s, y:y + window, x:x + window] += 1
    return cover


def fold_restatement(dwin, table, Bs, Hs, Ws, window, dtype=torch.float32, start=None):
    """msst_scene_fold_at restated on the CPU: the windows sorted by (scene, y0, x0, number), then
    want[s, :, y0:y0 + w, x0:x0 + w] += dwin[i], one window at a time.  Every pixel thereby takes its addends in ascending (y0, x0, number)
    with one rounded addition each, from 0 (or from `start`): in float32 the kernel's order and so its bits; in float64 the reference of
    the error bound.  dwin [n, C, w w] -> (sum [Bs, C, Hs, Ws], sum of |addends|, both in dtype)."""
    rows = table.tolist()
    C = dwin.shape[1]
    d = dwin.detach().cpu().to(dtype).reshape(len(rows), C, window, window)
    want = torch.zeros(Bs, C, Hs, Ws, dtype=dtype) if start is None else start.detach().cpu().to(dtype).clone()
    mag = torch.zeros(Bs, C, Hs, Ws, dtype=dtype)
    for i in sorted(range(len(rows)), key=lambda i: (*rows[i], i)):
        s, y, x = rows[i]
        want[s, :, y:y + window, x:x + window] += d[i]
        mag[s, :, y:y + window, x:x + window] += d[i].abs()
    return want, mag


def stack_at(scene, table, window):
    return torch.stack([scene[s, :, y:y + window, x:x + window] for s, y, x in table.tolist()]).contiguous()

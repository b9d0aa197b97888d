"""The three scene folds are one fold (scene_fold_kernel, msst_fwd.hip): msst_scene_assemble, msst_scene_recon_assemble and
msst_scene_embed_assemble, fed the same per-window planes [nwin][C][win win], give the same bits on every covered pixel -- whole, one
window per call, or split so that a call straddles the boundary between two scenes -- and those are the bits of the host fold: an fp32
running sum over the covering windows in the order (window row, window column), then one fp32 division by their number.  Where no
window covers a pixel each keeps its own answer: logits 0 and class -1, a NaN cube, NaN features and cover 0.  No model, no
tolerance."""
import pytest
import torch

from util import host_fold

pytestmark = pytest.mark.gpu

# (Bs, Hs, Ws, win, stride): overlap with an uncovered last row ((11 - 4) % 3 = 1); no overlap with an uncovered last column; one window
GRIDS = [(2, 11, 13, 4, 3), (2, 16, 17, 8, 8), (1, 5, 5, 5, 1)]
# C -> (S, P) of the reconstruction: one channel, a full 16-register group, two groups (18 crosses the 16 of the logits and features)
RECON_SP = {1: (1, 1), 16: (1, 16), 18: (2, 9)}


def bits(t):
    return t.contiguous().view(torch.int32)


def fold_calls(name, win_d, splits, grid, C):
    """the entry point `name` over the windows in calls of the given sizes, finalizing on the last; every output prefilled (NaN,
    12345) to show that nothing needs initialising -> (planes [Bs, C, Hs, Ws], classes or cover [Bs, Hs, Ws])"""
    from maskedsst_amd import _lib
    from maskedsst_amd.engine import _p, _stream
    lib = _lib.load()
    Bs, Hs, Ws, w, stride = grid
    out = torch.full((Bs, C, Hs, Ws), float("nan"), device="cuda")
    side = torch.full((Bs, Hs, Ws), 12345, dtype=torch.int64 if name == "msst_scene_assemble" else torch.int32, device="cuda")
    S, P = RECON_SP[C]
    scene = torch.zeros(Bs, C, Hs, Ws, device="cuda")
    no_mask = torch.zeros(Bs, S, Hs, Ws, dtype=torch.uint8, device="cuda")
    total, win0 = win_d.shape[0], 0
    for n in splits:
        part, last = win_d[win0:win0 + n].contiguous(), int(win0 + n == total)
        if name == "msst_scene_assemble":
            rc = lib.msst_scene_assemble(_p(part), win0, n, _p(out), _p(side), Bs, C, Hs, Ws, w, stride, last, _stream())
        elif name == "msst_scene_recon_assemble":
            rc = lib.msst_scene_recon_assemble(_p(part), win0, n, _p(scene), _p(no_mask), _p(out), None, None, _p(side), Bs, S, P, Hs, Ws,
                                               w, stride, last, 0, _stream())
        else:
            rc = lib.msst_scene_embed_assemble(_p(part), win0, n, _p(out), _p(side), Bs, C, Hs, Ws, w, stride, last, 0, _stream())
        assert rc == 0, (name, rc, lib.msst_last_error())
        win0 += n
    assert win0 == total
    torch.cuda.synchronize()
    return out.cpu(), side.cpu()


@pytest.mark.parametrize("C", [1, 16, 18])
@pytest.mark.parametrize("grid", GRIDS)
def test_the_three_scene_folds_give_the_host_folds_bits(grid, C):
    Bs, Hs, Ws, w, stride = grid
    nr, nq = (Hs - w) // stride + 1, (Ws - w) // stride + 1
    wps, total = nr * nq, Bs * nr * nq
    g = torch.Generator().manual_seed(Hs * 1000 + Ws * 100 + stride * 10 + C)
    win = torch.randn(total, C, w * w, generator=g)
    acc, _, cover = host_fold(win, Bs, Hs, Ws, w, stride, dtype=torch.float32)
    covered = (cover > 0)[:, None].expand(Bs, C, Hs, Ws)
    want = acc / cover.float().clamp(min=1)[:, None]                  # one fp32 division
    assert want.dtype == torch.float32 and bool((~covered).any()) == (grid != GRIDS[2])
    splits = [[total], [1] * total]
    if Bs > 1:
        splits.append([wps - 1, 2, total - wps - 1])                  # the middle call holds the last window of scene 0 and the first of scene 1
    win_d = win.cuda()
    for sp in splits:
        tag = (grid, C, sp[:3], len(sp))
        logits, classes = fold_calls("msst_scene_assemble", win_d, sp, grid, C)
        cube, rcover = fold_calls("msst_scene_recon_assemble", win_d, sp, grid, C)
        feat, ecover = fold_calls("msst_scene_embed_assemble", win_d, sp, grid, C)
        for name, got in (("logits", logits), ("cube", cube), ("features", feat)):
            assert torch.equal(bits(got)[covered], bits(want)[covered]), (name, tag)
        # where no window covers a pixel
        assert (logits[~covered] == 0).all() and (classes[cover == 0] == -1).all() and (classes[cover > 0] >= 0).all(), tag
        assert torch.isnan(cube[~covered]).all() and torch.isnan(feat[~covered]).all(), tag
        assert torch.equal(rcover, cover) and torch.equal(ecover, cover), tag

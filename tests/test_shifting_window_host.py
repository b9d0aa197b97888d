"""shifting_window finetuning, host side (no GPU needed): ``stack_image_batch`` against the reference-made fixture
(tools/make_golden_shifting_window.py) and against the scene kernels' window numbering, the config flag, the C ABI of
msst_tokenize_scene_fwd_train / msst_tokenize_scene_bwd and their argument checks (they run before any HIP call, so null buffers and
no device are enough to see them), ``forward_windows``'s refusals, and the window branch of ``train_step`` on a stub model."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

BADARG, UNSUPPORTED = -3, -2   # include/msst.h: MSST_ERR_BADARG, MSST_ERR_UNSUPPORTED
CALLS = ("msst_tokenize_scene_fwd_train", "msst_tokenize_scene_bwd")


def _config(**kw):
    from maskedsst_amd.config import Dotdict
    return Dotdict(dict(dict(image_size=8, patch_sub=0, pixelwise=False, ignored_label=-1), **kw))


@pytest.mark.parametrize("case", ["s8", "s7"])
def test_stack_image_batch_equals_the_reference_fixture(case):
    from maskedsst_amd.utils import stack_image_batch
    g = load_golden("stack_image_batch.npz")
    image_size, patch_sub = (int(v) for v in g[case + "_cfg"])
    img, label = torch.from_numpy(g[case + "_img"]), torch.from_numpy(g[case + "_label"])
    simg, slabel = stack_image_batch(_config(image_size=image_size, patch_sub=patch_sub), img, label)
    s = image_size - patch_sub
    n = img.shape[0] * (img.shape[2] // s) * (img.shape[3] // s)
    assert simg.shape == (n, img.shape[1], s, s) and slabel.shape == (n, s, s)
    assert simg.dtype == img.dtype and slabel.dtype == label.dtype
    assert np.array_equal(simg.numpy(), g[case + "_stacked_img"]) and np.array_equal(slabel.numpy(), g[case + "_stacked_label"])


@pytest.mark.parametrize("H,W,s", [(16, 16, 8), (23, 23, 7), (64, 64, 8), (64, 64, 7), (15, 15, 7)])
def test_window_order_is_the_scene_kernels(H, W, s):
    """window i of tile b is scene_windows(H, W, s, s)[i]: the '(b h w)' order of the reference is the numbering of the scene kernels"""
    from maskedsst_amd.scene import scene_windows
    from maskedsst_amd.utils import stack_image_batch
    B, C = 2, 3
    img = torch.arange(B * C * H * W, dtype=torch.int32).reshape(B, C, H, W)
    label = torch.arange(B * H * W, dtype=torch.int32).reshape(B, H, W)
    simg, slabel = stack_image_batch(_config(image_size=s + 1, patch_sub=1), img, label)
    org = [(int(y), int(x)) for y, x in scene_windows(H, W, s, s)]
    assert simg.shape[0] == B * len(org) == B * (H // s) * (W // s)
    for b in range(B):
        for i, (y, x) in enumerate(org):
            assert torch.equal(simg[b * len(org) + i], img[b, :, y:y + s, x:x + s]), (b, i)
            assert torch.equal(slabel[b * len(org) + i], label[b, y:y + s, x:x + s]), (b, i)


def test_stack_image_batch_keeps_the_reference_assertion():
    from maskedsst_amd.utils import stack_image_batch
    with pytest.raises(AssertionError):   # 17 % 8 != 18 % 8
        stack_image_batch(_config(), torch.zeros(1, 2, 17, 18), torch.zeros(1, 17, 18))


def test_config_parses_shifting_window_as_the_reference():
    from maskedsst_amd.config import parse_flag
    assert [parse_flag(v) for v in (False, "false", "False")] == [False] * 3
    assert all(parse_flag(v) for v in (True, "true", "True", "yes", 1))
    spec = importlib.util.spec_from_file_location("finetune_script_sw", os.path.join(ROOT, "finetune.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    paths = (os.path.join(ROOT, "configs", "finetune_config_enmap.yaml"), os.path.join(ROOT, "configs", "config.yaml"))
    assert ft.get_finetune_config(*paths, 5, "cpu").shifting_window is False          # both shipped configs: False
    assert ft.get_finetune_config(*paths, 5, "cpu", shifting_window=True).shifting_window is True
    args = ft.build_parser().parse_args(["--shifting-window"])
    assert args.shifting_window is True and ft.build_parser().parse_args([]).shifting_window is None


def test_c_abi_declares_and_exports_the_tile_tokenizer_calls():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    lib = _lib.load()   # refuses a library of another revision or one that lacks a declared symbol
    # entry points only: the revision stays at 109, which the tests of the earlier additive calls pin (test_ce_host.py, test_linear_eval_host.py)
    assert lib.msst_version() == _lib.header_version() == 109
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in CALLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.declared_symbols() and re.search(r" T %s$" % name, out, re.M), name


def _fwd(lib, ptr=None, **k):
    a = {**dict(Bs=2, Hs=16, Ws=16, window=8, stride=8, win0=0, nwin=8, S=2, P=10, split=0), **k}
    return lib.msst_tokenize_scene_fwd_train(*([ptr] * 9), a["split"], ptr, a["Bs"], a["Hs"], a["Ws"], a["window"], a["stride"], a["win0"],
                                             a["nwin"], a["S"], a["P"], 0.1, 7, None)


def _bwd(lib, ptr=None, nchunk=2, **k):
    a = {**dict(Bs=2, Hs=16, Ws=16, window=8, stride=8, win0=0, nwin=8, S=2, P=10, split=0), **k}
    return lib.msst_tokenize_scene_bwd(*([ptr] * 9), nchunk, *([ptr] * 8), a["split"], a["Bs"], a["Hs"], a["Ws"], a["window"], a["stride"],
                                       a["win0"], a["nwin"], a["S"], a["P"], 0.1, 7, None)


def test_tile_tokenizer_calls_refuse_bad_arguments_before_launch():
    """null pointers throughout: no call can have reached a launch.  Geometry outside 1 <= stride <= window <= Hs, Ws, window^2 <= 64,
    P <= 16: UNSUPPORTED; sizes below 1, null required pointers, windows beyond the grids: BADARG"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    for call in (_fwd, _bwd):
        for bad in (dict(stride=9), dict(window=9, stride=9, Hs=32, Ws=32), dict(window=8, Hs=7), dict(window=8, Ws=7), dict(P=17),
                    dict(window=17, stride=4)):
            assert call(lib, **bad) == UNSUPPORTED, (call.__name__, bad)
        for bad in (dict(Bs=0), dict(Hs=0), dict(Ws=0), dict(window=0), dict(stride=0), dict(S=0), dict(P=0), dict(nwin=-1), dict(win0=-1),
                    dict()):   # last: good shapes, null pointers
            assert call(lib, **bad) == BADARG, (call.__name__, bad)
        assert b"msst_tokenize_scene" in lib.msst_last_error()
    # with (fake, never dereferenced) pointers the window range and the backward's own sizes are what is left to refuse
    fake = 4096
    assert _fwd(lib, fake, nwin=9) == BADARG and _fwd(lib, fake, win0=7, nwin=2) == BADARG
    assert _bwd(lib, fake, nwin=9) == BADARG and _bwd(lib, fake, nwin=0) == BADARG and _bwd(lib, fake, nchunk=0) == BADARG
    assert _fwd(lib, fake, split=96) == BADARG and _bwd(lib, fake, split=-1) == BADARG
    assert _fwd(lib, fake, nwin=0) == 0   # an empty forward call enqueues nothing


def _model(**kw):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        **{**dict(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=4, dim=96, depth=1, heads=2, mlp_dim=64, dropout=0.0,
                  emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2), blockwise_patch_embed=True), **kw})


def test_forward_windows_has_no_cpu_fallback():
    from maskedsst_amd._lib import MsstError
    with pytest.raises((MsstError, RuntimeError, NotImplementedError), match="(?i)cuda|cpu|fallback|device"):
        _model().forward_windows(torch.zeros(1, 20, 16, 16))


@pytest.mark.parametrize("shape", [(20, 16, 16), (1, 20, 16, 16, 1), (1, 30, 16, 16), (1, 20, 7, 16), (1, 20, 16, 7)])
def test_forward_windows_refuses_bad_shapes(shape):
    with pytest.raises(ValueError):
        _model().forward_windows(torch.zeros(*shape))


class _StubWindows:
    """a model that only records what train_step hands it"""

    def __init__(self, nc, pixelwise):
        self.nc, self.pixelwise, self.tiles, self.called = nc, pixelwise, None, []

    def _out(self, n, s):
        shape = (n, self.nc) if self.pixelwise else (n, self.nc, s, s)
        return torch.zeros(*shape, requires_grad=True) + torch.arange(self.nc, dtype=torch.float32).view(1, -1, *([1] * (len(shape) - 2)))

    def forward_windows(self, tiles):
        self.called.append("forward_windows")
        self.tiles = tiles
        s = 7 if self.pixelwise else 8
        return self._out(tiles.shape[0] * (tiles.shape[-1] // s) ** 2, s)

    def __call__(self, img):
        self.called.append("forward")
        self.tiles = img
        return self._out(img.shape[0], img.shape[-1])


class _StubOpt:
    def zero_grad(self):
        pass

    def step(self):
        pass


@pytest.mark.parametrize("pixelwise", [False, True])
def test_train_step_hands_whole_tiles_to_forward_windows(pixelwise):
    """shifting_window on 64 x 64 tiles: the tiles go to forward_windows unstacked and uncropped, the criterion sees the labels of all
    windows in stack_image_batch's order (pixelwise: each window's centre); flag off or absent: the crop path, draw for draw as before"""
    from maskedsst_amd.utils import stack_image_batch, train_step
    seen = []

    def criterion(out, label):
        seen.append(label.clone())
        return torch.nn.functional.cross_entropy(out, label, ignore_index=-1)

    cfg = _config(image_size=8, patch_sub=1 if pixelwise else 0, pixelwise=pixelwise, shifting_window=True)
    torch.manual_seed(0)
    img, label = torch.randn(2, 20, 64, 64), torch.randint(-1, 5, (2, 64, 64))
    m = _StubWindows(5, pixelwise)
    state = torch.get_rng_state()
    train_step(img, label, m, cfg, "cpu", criterion, _StubOpt())
    assert torch.equal(torch.get_rng_state(), state)   # no crop drawn
    assert m.called == ["forward_windows"] and m.tiles.shape == img.shape and torch.equal(m.tiles, img)
    _, want = stack_image_batch(cfg, img, label)
    if pixelwise:
        assert want.shape == (2 * 81, 7, 7)
        want = want[:, 3, 3]
    else:
        assert want.shape == (2 * 64, 8, 8)
    assert torch.equal(seen[-1], want)
    # flag off, and no such key: one random crop per tile through forward, the same draws
    outs = []
    for off in (dict(shifting_window=False), dict()):
        c = _config(image_size=8, patch_sub=1 if pixelwise else 0, pixelwise=pixelwise, **off)
        m = _StubWindows(5, pixelwise)
        torch.manual_seed(1)
        train_step(img, label, m, c, "cpu", criterion, _StubOpt())
        assert m.called == ["forward"] and m.tiles.shape[-1] == (7 if pixelwise else 8)
        outs.append((m.tiles.clone(), seen[-1].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # tiles that are not 64 wide, or a model of image_size 64: never the window path
    m = _StubWindows(5, pixelwise)
    s = 7 if pixelwise else 8
    train_step(torch.randn(2, 20, s, s), torch.randint(0, 5, (2, s, s)), m, cfg, "cpu", criterion, _StubOpt())
    assert m.called == ["forward"]

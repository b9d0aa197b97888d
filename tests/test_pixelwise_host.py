"""Pixelwise centre-pixel classifier (ViTSpatialSpectral(pixelwise=True)), host side: the module surface against the reference
captures of tools/make_golden_pixelwise.py (state_dict schema, parameter draw order, parameter count), the refused
configurations, the 8 x 8 -> 7 x 7 checkpoint hand-off of load_checkpoint, train_step's centre label and the C ABI's argument
checks (no GPU needed)."""
import numpy as np
import pytest
import torch

from conftest import load_golden, seed_all, fp_np

CASES = ["pixwise_200b_L4_B2.npz", "pixwise_50b_L2_B2_specpos.npz", "pixwise_30b_L1_B3_img5_h2.npz"]


def pixelwise_encoder(cfg, n_classes=None, pixelwise=True, image_size=None, pos_embed_len=None, precision=None):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=image_size or cfg.get("image_size", 7), spatial_patch_size=1, spectral_patch_size=10,
        num_classes=n_classes or cfg["n_classes"], dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64,
        dropout=0.0, emb_dropout=0.0, channels=cfg["bands"], spectral_pos_embed=cfg["spectral_pos_embed"],
        spectral_pos=torch.arange(cfg["bands"] // 10), blockwise_patch_embed=True, pixelwise=pixelwise,
        pos_embed_len=pos_embed_len, precision=precision)


@pytest.mark.parametrize("name", CASES)
def test_schema_and_draw_order_match_reference(name):
    g = load_golden(name)
    cfg = g["cfg"]
    seed_all(5)
    enc = pixelwise_encoder(cfg)
    w = cfg.get("image_size", 7)
    torch.randn(cfg["B"], cfg["bands"], w, w)
    label = torch.randint(0, cfg["n_classes"], (cfg["B"], w, w))
    np.testing.assert_array_equal(label.numpy().astype(np.int8), g["label"])   # the stream after construction is the reference's
    assert [k for k, _ in enc.named_parameters()] == g["names"]
    assert list(enc.state_dict().keys()) == g["names"]
    assert sum(p.numel() for p in enc.parameters()) == int(g["n_params"])
    for k, p in enc.named_parameters():
        np.testing.assert_array_equal(fp_np(p), g["p_fp/" + k], err_msg=k)
    assert enc.mlp_head[0].weight.shape == (96,) and enc.mlp_head[2].weight.shape == (cfg["n_classes"], 96 * w * w)
    assert g["logits"].shape == (cfg["B"], cfg["n_classes"])   # the reference's squeeze of [B, nc, 1, 1]


def test_parameter_count_enmap_finetune_shape():
    """EnMAP finetune encoder at the pixelwise size (200 bands, depth 4, 8 classes, image 7): the reference's counts"""
    cfg = dict(bands=200, depth=4, n_classes=8)
    assert sum(p.numel() for p in pixelwise_encoder(dict(cfg, spectral_pos_embed=True)).parameters()) == 1_739_228
    assert sum(p.numel() for p in pixelwise_encoder(dict(cfg, spectral_pos_embed=False)).parameters()) == 1_829_628


def test_head_modules_reproduce_the_reference_layout():
    """the head's parameter-free modules give the reference's shapes on a stand-in: flatten of [B, h, w, 96] in (h, w, d) order,
    then [B, nc, 1, 1] squeezed -- [nc] for a single sample"""
    enc = pixelwise_encoder(dict(bands=30, depth=1, n_classes=5, spectral_pos_embed=False), image_size=3)
    x = torch.arange(2 * 3 * 3 * 96, dtype=torch.float32).reshape(2, 3, 3, 96)
    flat = enc.mlp_head[1](x)
    assert flat.shape == (2, 864) and torch.equal(flat[1, 4 * 96 + 7], x[1, 1, 1, 7])
    z = torch.randn(2, 5)
    for B in (2, 1):
        y = enc.mlp_head[5](enc.mlp_head[4](enc.mlp_head[3](z[:B])))
        assert y.shape == ((2, 5) if B == 2 else (5,)) and torch.equal(y, z[:B].squeeze())


def test_refused_configurations():
    from maskedsst_amd import ViTSpatialSpectral
    base = dict(image_size=7, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=1, heads=8, mlp_dim=64,
                channels=50, spectral_pos_embed=False, spectral_pos=list(range(5)), pixelwise=True)
    for size in (8, 6, 4):
        with pytest.raises(NotImplementedError, match="no centre pixel"):
            ViTSpatialSpectral(**{**base, "image_size": size})
    with pytest.raises(NotImplementedError, match="pixelwise"):
        ViTSpatialSpectral(**base, spectral_mlp_head=True)
    with pytest.raises(NotImplementedError, match="num_classes=33"):
        ViTSpatialSpectral(**{**base, "num_classes": 33})
    with pytest.raises(NotImplementedError):
        ViTSpatialSpectral(**{**base, "image_size": 9})   # more than 64 spatial tokens
    assert ViTSpatialSpectral(**{**base, "num_classes": 32}).mlp_head[2].weight.shape == (32, 96 * 49)
    for size in (1, 3, 5):
        assert ViTSpatialSpectral(**{**base, "image_size": size}).mlp_head[2].in_features == 96 * size * size


def test_default_head_unchanged_by_the_option():
    """pixelwise=False draws exactly what it drew before at an odd size"""
    from maskedsst_amd import ViTSpatialSpectral
    cfg = dict(bands=50, depth=1, n_classes=8, spectral_pos_embed=False)
    seed_all(5)
    a = pixelwise_encoder(cfg, pixelwise=False)
    seed_all(5)
    b = ViTSpatialSpectral(image_size=7, spatial_patch_size=1, spectral_patch_size=10, num_classes=8, dim=96, depth=1, heads=8,
                           mlp_dim=64, channels=50, spectral_pos_embed=False, spectral_pos=torch.arange(5))
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert "mlp_head.1.weight" in sa and "mlp_head.2.weight" not in sa


class _Cfg:
    patch_sub = 1
    image_size = 8


def _simmim(cfg, n_classes):
    from maskedsst_amd import SimMIMSpatialSpectral
    return SimMIMSpatialSpectral(encoder=pixelwise_encoder(cfg, n_classes, pixelwise=False, image_size=8), intermediate_losses=False,
                                 masking_ratio=0.7, mask_patch_size=4, to_pixels_per_spectral_block=True, tube_masking=True)


@pytest.mark.parametrize("tag", ["specpos", "posemb"])
def test_load_checkpoint_8x8_to_pixelwise_7x7_matches_reference(tag):
    """an 8 x 8 SimMIM state_dict -> a 7 x 7 pixelwise classifier through load_checkpoint (tools/make_golden_pixelwise.py): the
    first 49 rows of pos_embed, or the checkpoint's pos_embedding when the model is built with its pos_embed_len; mlp_head.2 fresh"""
    from maskedsst_amd.utils import load_checkpoint
    g = load_golden("pixwise_load_checkpoint_50b_L2.npz")
    cfg = dict(g["cfg"], spectral_pos_embed=tag == "specpos")
    before = bytes(g[f"{tag}/before"]).decode().split("\n")
    after = bytes(g[f"{tag}/after"]).decode().split("\n")
    source = bytes(g[f"{tag}/after_source"]).decode().split("\n")
    seed_all(5)
    sd = _simmim(cfg, cfg["n_classes_pretrain"]).state_dict()
    assert list(sd.keys()) == before
    pel = None if tag == "specpos" else 5 * 64 + 1
    enc = pixelwise_encoder(cfg, cfg["n_classes_finetune"], pos_embed_len=pel)
    load_checkpoint(_Cfg(), enc, "mlp_head", "cpu", checkpoint={"model_state_dict": sd})
    got = enc.state_dict()
    assert list(got.keys()) == after
    assert source[after.index("mlp_head.2.weight")] == "fresh" and source[after.index("mlp_head.2.bias")] == "fresh"
    assert source[after.index("mlp_head.0.weight")] == "checkpoint"
    if tag == "specpos":
        assert bool(g["specpos/pos_embed_is_first_rows"])
        assert torch.equal(got["pos_embed"], sd["encoder.pos_embed"][:, :49])
    for k, src in zip(after, source):
        np.testing.assert_array_equal(fp_np(got[k]), g[f"{tag}/after_fp/" + k], err_msg=f"{k} ({src})")


def test_load_checkpoint_pos_embedding_without_length_fails_like_reference():
    from maskedsst_amd.utils import load_checkpoint
    g = load_golden("pixwise_load_checkpoint_50b_L2.npz")
    cfg = dict(g["cfg"], spectral_pos_embed=False)
    ref_err = bytes(g["posemb/error_without_pos_embed_len"]).decode()
    assert ref_err.startswith("RuntimeError: ") and "size mismatch for pos_embedding" in ref_err
    seed_all(5)
    sd = _simmim(cfg, cfg["n_classes_pretrain"]).state_dict()
    with pytest.raises(RuntimeError, match="size mismatch for pos_embedding") as e:
        load_checkpoint(_Cfg(), pixelwise_encoder(cfg, cfg["n_classes_finetune"]), "mlp_head", "cpu",
                        checkpoint={"model_state_dict": sd})
    mism = lambda s: sorted(l.strip() for l in s.splitlines() if l.strip().startswith("size mismatch"))   # noqa: E731
    assert mism(str(e.value)) == mism(ref_err)


class _StubModel:
    """records what train_step feeds the model and the criterion"""

    def __init__(self, nc):
        self.nc, self.seen = nc, None

    def __call__(self, img):
        self.seen = img
        return torch.zeros(img.shape[0], self.nc, requires_grad=True) + torch.arange(self.nc, dtype=torch.float32)


class _StubOpt:
    def zero_grad(self):
        pass

    def step(self):
        pass


def test_train_step_takes_the_centre_label():
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step
    labels = []

    def criterion(out, label):
        labels.append(label.clone())
        return torch.nn.functional.cross_entropy(out, label, ignore_index=-1)

    config = Dotdict(dict(image_size=8, patch_sub=1, pixelwise=True, ignored_label=-1))
    label = torch.arange(2 * 7 * 7).reshape(2, 7, 7) % 5
    m = _StubModel(5)
    train_step(torch.randn(2, 30, 7, 7), label, m, config, "cpu", criterion, _StubOpt())
    assert torch.equal(labels[-1], label[:, 3, 3])
    # a [B] label (the reference's Houston reader in pixelwise mode) passes through
    train_step(torch.randn(2, 30, 7, 7), torch.tensor([1, 4]), m, config, "cpu", criterion, _StubOpt())
    assert torch.equal(labels[-1], torch.tensor([1, 4]))
    # a 64 x 64 tile: cropped to 7 x 7, then the crop's centre
    torch.manual_seed(0)
    lab64 = torch.randint(0, 5, (2, 64, 64))
    img64 = torch.randn(2, 30, 64, 64)
    torch.manual_seed(1)
    train_step(img64, lab64, m, config, "cpu", criterion, _StubOpt())
    torch.manual_seed(1)
    x, y = torch.randint(0, 64 - 8 - 1, size=(2,))
    assert m.seen.shape == (2, 30, 7, 7) and torch.equal(m.seen, img64[:, :, x:x + 7, y:y + 7])
    assert torch.equal(labels[-1], lab64[:, x + 3, y + 3])
    # not pixelwise: the label map is untouched
    config.pixelwise = False
    train_step(torch.randn(2, 30, 7, 7), label, lambda img: torch.zeros(2, 5, 7, 7, requires_grad=True), config, "cpu", criterion,
               _StubOpt())
    assert torch.equal(labels[-1], label)


def test_finetune_config_pixelwise_override():
    import importlib
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("finetune_script", os.path.join(ROOT, "finetune.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    paths = (os.path.join(ROOT, "configs", "finetune_config_enmap.yaml"), os.path.join(ROOT, "configs", "config.yaml"))
    c = ft.get_finetune_config(*paths, 5, "cpu", pixelwise=True)
    assert c.pixelwise and c.patch_sub == 1 and c.image_size - c.patch_sub == 7
    c = ft.get_finetune_config(*paths, 5, "cpu")
    assert not c.pixelwise and c.patch_sub == 0


def test_pix_head_c_abi_symbols_and_argument_checks():
    """msst_pix_head_* and msst_scene_centre_assemble are exported (since MSST_VERSION 107: the loaded library is the revision of
    include/msst.h, and that is 107 or later) and refuse bad arguments before anything is enqueued"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    assert lib.msst_version() == _lib.header_version() >= 107
    unsupported, badarg = -2, -3   # include/msst.h: MSST_ERR_UNSUPPORTED, MSST_ERR_BADARG
    for B, S, N, nc in [(2, 20, 65, 8), (2, 65, 49, 8), (2, 20, 49, 33)]:
        assert lib.msst_pix_head_fwd(*([None] * 7), B, S, N, nc, None) == unsupported, (B, S, N, nc)
        assert lib.msst_pix_head_bwd(*([None] * 11), B, S, N, nc, None) == unsupported, (B, S, N, nc)
        assert lib.msst_pix_head_bwd_slab(B, S, N, nc) == 0
    for B, S, N, nc in [(0, 20, 49, 8), (2, 0, 49, 8), (2, 20, 0, 8), (2, 20, 49, 0), (2, 20, 49, 8)]:   # last: null pointers
        assert lib.msst_pix_head_fwd(*([None] * 7), B, S, N, nc, None) == badarg, (B, S, N, nc)
        assert lib.msst_pix_head_bwd(*([None] * 11), B, S, N, nc, None) == badarg, (B, S, N, nc)
    assert lib.msst_pix_head_fwd_ws(256, 49) == 256 * 49 * 96 and lib.msst_pix_head_fwd_ws(0, 49) == 0
    # G = ceil(B / 32) groups: dW partials [G][nc][96 N], db partials [G][32], dgamma / dbeta partials [G N][96] each
    G, K = 8, 96 * 49
    assert lib.msst_pix_head_bwd_slab(256, 20, 49, 8) == G * 8 * K + G * 32 + 2 * G * 49 * 96
    assert lib.msst_pix_head_bwd_slab(1, 3, 25, 20) == 20 * 96 * 25 + 32 + 2 * 25 * 96
    # the centre assembly: a window larger than the scene, a stride beyond the window, no output, windows out of range
    args = lambda **k: {**dict(win0=0, nwin=0, Bs=1, nc=8, Hs=20, Ws=22, window=7, stride=1), **k}   # noqa: E731
    for bad in (args(window=21), args(stride=8), args(stride=0), args(nc=0), args(win0=-1), args(nwin=14 * 16 + 1)):
        assert lib.msst_scene_centre_assemble(None, bad["win0"], bad["nwin"], None, None, bad["Bs"], bad["nc"], bad["Hs"],
                                              bad["Ws"], bad["window"], bad["stride"], 1, None) == badarg, bad

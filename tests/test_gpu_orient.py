"""GPU: D4 augmentation of listed windows -- the orientation applied where the kernels form a window's address (msst_tokenize_at_fwd_orient
/ _bwd_orient and their masked forms, msst_head_at_fwd_orient).  Every check is bit for bit (torch.equal) against the un-oriented path on
maskedsst_amd.orient_windows(gathered windows, orient): only addresses differ, so nothing may.  Scenes are not square (a Ws / Hs mix-up
shows), the data is randn (no orientation coincides with another), and every table holds all eight codes, windows in the four corners
of a scene (a wrong negative step leaves the scene exactly there) and one origin twice with two codes.  One check does not rest on this
project's kernels: the fp32 patch-head forward against the CPU oracle on the oriented windows, at the suite's fp32 bar (1e-4)."""
import pytest
import torch

from conftest import oracle_cfg_from, seed_all
from util import relerr

pytestmark = pytest.mark.gpu

HEADS = {"default": dict(), "spectral": dict(spectral_mlp_head=True), "pixelwise": dict(pixelwise=True)}
SCENE_HW = (13, 15)


def oriented_table(Bs, Hs, Ws, s, n):
    """(origins int32 [n, 3], orient uint8 [n]), from the shapes alone: rows 0 .. 15 walk the four corners of the first and the last
    scene, row i with code i % 8 -- every corner meets four codes, flipped and turned, transposing and not --, then positions inside
    the scenes with the codes going on in turn; the last row repeats the origin of the one before it with another code"""
    assert n >= 16 and Hs - s >= 2 and Ws - s >= 2
    my, mx = Hs - s, Ws - s
    corners = [(0, 0), (my, 0), (0, mx), (my, mx)]
    rows, codes = [], []
    for i in range(n - 1):
        if i < 16:
            y, x = corners[(i + i // 8) % 4]
            rows.append(((Bs - 1) * ((i // 4) % 2), y, x))
        else:
            rows.append((i % Bs, (3 * i) % (my + 1), (5 * i + 1) % (mx + 1)))
        codes.append(i % 8)
    rows.append(rows[-1])
    codes.append((codes[-1] + 3) % 8)
    assert sorted(set(codes)) == list(range(8))
    assert all(sum((r[1], r[2]) == c for r in rows[:16]) >= 3 for c in corners)
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(codes, dtype=torch.uint8)


def stack_at(scene, origins, s):
    return torch.stack([scene[b, :, y:y + s, x:x + s] for b, y, x in origins.tolist()]).contiguous()


def oriented_stack(scene, origins, orient, s):
    """the comparison leg's input: the gathered windows, each turned by the eager restatement"""
    from maskedsst_amd import orient_windows
    return orient_windows(stack_at(scene, origins, s), orient.to(scene.device)).contiguous()


def test_the_table_builder_and_orient_windows_agree_with_torch():
    """the test's own tools: the eager restatement is the normative torch expression (so the comparison leg is), on the device too"""
    from maskedsst_amd import orient_windows
    table, orient = oriented_table(2, 11, 13, 8, 24)
    assert table.shape == (24, 3) and torch.equal(table[-1], table[-2]) and orient[-1] != orient[-2]
    x = torch.randn(24, 3, 8, 8, device="cuda")
    got = orient_windows(x, orient)
    for i, o in enumerate(orient.tolist()):
        assert torch.equal(got[i], torch.rot90(torch.flip(x[i], (-1,)) if o >> 2 else x[i], o & 3, (-2, -1))), (i, o)
    assert len({got[i].cpu().numpy().tobytes() for i in (-1, -2)}) == 2


# ------------------------------------------------------------------------------------------ 1. the tokenizer alone
# (name, spectral patch P, window s, scene shape, windows): mfma: the fp32-MFMA kernels (P = 10, 8 x 8); generic: the run-time-P kernels
TOK_CASES = [("mfma", 10, 8, (2, 20, 11, 13), 24), ("generic", 5, 7, (2, 20, 9, 10), 16)]


def _tok_model(P, s):
    from maskedsst_amd import ViTSpatialSpectral
    seed_all(5)
    return ViTSpatialSpectral(image_size=s, spatial_patch_size=1, spectral_patch_size=P, num_classes=5, dim=96, depth=1, heads=2, mlp_dim=64,
                              dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(20 // P),
                              blockwise_patch_embed=True, precision="fp32").cuda()


@pytest.mark.parametrize("case", TOK_CASES, ids=[c[0] for c in TOK_CASES])
def test_oriented_tokenizer_is_the_tokenizer_on_the_oriented_copies(case):
    from maskedsst_amd.engine import Windows
    _, P, s, shape, n = case
    enc = _tok_model(P, s)
    eng = enc.engine()
    eng.ensure()
    assert (eng.S, eng.P, eng.N) == (20 // P, P, s * s)
    scene = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).cuda()
    table, orient = oriented_table(shape[0], shape[2], shape[3], s, n)
    table, orient = table.cuda(), orient.cuda()
    copies = oriented_stack(scene, table, orient, s)
    plain = stack_at(scene, table, s)
    dx0 = torch.randn(n, eng.S * eng.N, 96, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    for drop in ((0.0, 0),) + (((0.1, 12345),) if case[0] == "mfma" else ()):   # training: embedding dropout with a fixed seed
        got = eng.tokenize(Windows("listed", scene, table, orient=orient), None, emb_drop=drop)
        want = eng.tokenize(copies, None, emb_drop=drop)
        torch.cuda.synchronize()
        assert got.shape == (n, eng.S * eng.N, 96) and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), (case[0], drop)
        assert not torch.equal(got, eng.tokenize(plain, None, emb_drop=drop))   # the orientations did something
        if drop[0]:
            assert 0.05 < float((got == 0).float().mean()) < 0.15   # the dropout is on
        # the parameter backward into the flat gradient buffer, over the same two sources
        grads = []
        for src in (Windows("listed", scene, table, orient=orient), copies):
            eng.fp.grad.fill_(float("nan"))
            eng.tokenize_bwd(src, None, dx0, emb_drop=drop)
            torch.cuda.synchronize()
            g = {k: eng.fp.view(k, eng.fp.grad).clone() for k in ("pre_g", "pre_b", "embed.w.0", "embed.b.0", "post_g", "post_b")}
            g["pos_embedding"] = eng.fp.view("pos_embedding", eng.fp.grad).reshape(-1, 96)[:eng.S * eng.N].clone()   # the rows the tokens use
            grads.append(g)
        bad = [k for k in grads[0] if not (torch.equal(grads[0][k], grads[1][k]) and bool(torch.isfinite(grads[0][k]).all()))]
        assert not bad, (case[0], drop, bad)
    # code 0 throughout: the un-oriented entry point's bits
    zero = torch.zeros_like(orient)
    assert torch.equal(eng.tokenize(Windows("listed", scene, table, orient=zero), None), eng.tokenize(Windows("listed", scene, table), None))


# ------------------------------------------------------------------------------------------ 2. forward_at(..., orient=), the three heads
def _encoder(head, precision="fp32"):
    from maskedsst_amd import ViTSpatialSpectral
    return ViTSpatialSpectral(
        image_size=7 if head == "pixelwise" else 8, spatial_patch_size=1, spectral_patch_size=10, num_classes=5, dim=96, depth=1, heads=2,
        mlp_dim=64, dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2),
        blockwise_patch_embed=True, precision=precision, **HEADS[head])


def _scene_and_table(head, n=19):
    s = 7 if head == "pixelwise" else 8
    scene = torch.randn(2, 20, *SCENE_HW, generator=torch.Generator().manual_seed(8))
    return (s, scene) + oriented_table(2, *SCENE_HW, s, n)


def _run(enc, fwd):
    enc.zero_grad(set_to_none=True)
    out = fwd()
    out.square().mean().backward()
    torch.cuda.synchronize()
    return out.detach().clone(), {k: q.grad.clone() for k, q in enc.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("head", list(HEADS))
def test_forward_at_orient_is_forward_of_the_oriented_windows(head, precision):
    seed_all(5)
    enc = _encoder(head, precision).cuda().train()
    s, scene, table, orient = _scene_and_table(head)
    scene = scene.cuda()
    copies = oriented_stack(scene, table, orient, s)
    out_o, g_o = _run(enc, lambda: enc.forward_at(scene, table, orient=orient))
    out_c, g_c = _run(enc, lambda: enc(copies))
    out_d, g_d = _run(enc, lambda: enc.forward_at(scene, table.cuda(), check=False, orient=orient.cuda().long()))   # other device, dtype
    assert out_o.shape == ((19, 5) if head == "pixelwise" else (19, 5, s, s)) and bool(torch.isfinite(out_o).all())
    assert torch.equal(out_o, out_c) and torch.equal(out_d, out_c)
    want = sorted(k for k, q in enc.named_parameters() if q.requires_grad)
    assert sorted(g_o) == sorted(g_c) == sorted(g_d) == want
    bad = [k for k in want if not (torch.equal(g_o[k], g_c[k]) and torch.equal(g_d[k], g_c[k]) and bool(torch.isfinite(g_o[k]).all()))]
    assert not bad, bad
    assert sum(float(g_o[k].abs().max()) > 0 for k in want) > len(want) // 2
    # all-zero codes: the bits of the call without the keyword; and the orientations did something
    out_n, g_n = _run(enc, lambda: enc.forward_at(scene, table))
    out_z, g_z = _run(enc, lambda: enc.forward_at(scene, table, orient=torch.zeros(19, dtype=torch.uint8)))
    assert torch.equal(out_z, out_n) and not [k for k in want if not torch.equal(g_z[k], g_n[k])]
    assert not torch.equal(out_o, out_n)
    # the repeated origin with two codes: two different samples
    assert not torch.equal(out_o[-1], out_o[-2])


def test_forward_at_orient_refusals_on_the_device():
    seed_all(5)
    enc = _encoder("default").cuda()
    s, scene, table, orient = _scene_and_table("default")
    scene = scene.cuda()
    bad = orient.clone().long()
    bad[7] = 8
    with pytest.raises(ValueError, match=r"orient\[7\] = 8"):
        enc.forward_at(scene, table.cuda(), orient=bad.cuda())
    with pytest.raises(NotImplementedError, match="orient"):
        enc.forward_at(scene.clone().requires_grad_(True), table, scene_grad=True, orient=orient)
    with pytest.raises(NotImplementedError, match="orient"):
        enc.forward_at(scene.clone().requires_grad_(True), table, orient=orient)


# ------------------------------------------------------------------------------------------ 3. SimMIM forward_at(..., orient=)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_simmim_forward_at_orient_is_forward_of_the_oriented_windows(precision):
    """mask_patch_size = 1: random masks, symmetric under no orientation -- a mask read in the wrong frame moves the loss"""
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=5, dim=96, depth=1, heads=2, mlp_dim=64,
                             dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=True, spectral_pos=torch.arange(2),
                             blockwise_patch_embed=True, precision=precision)
    mim = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=1, tube_masking=False, to_pixels_per_spectral_block=True).cuda()
    tiles = torch.randn(2, 20, 11, 14, generator=torch.Generator().manual_seed(21)).cuda()
    table, orient = oriented_table(2, 11, 14, 8, 19)
    copies = oriented_stack(tiles, table, orient, 8)
    masks = mim.draw_masks(19)
    runs = []
    for fwd in (lambda: mim.forward_at(tiles, table, masks, orient=orient), lambda: mim(copies, masks),
                lambda: mim.forward_at(tiles, table, masks), lambda: mim.forward_at(tiles, table, masks, orient=torch.zeros_like(orient))):
        mim.zero_grad(set_to_none=True)
        loss = fwd()
        (loss * 3.0).backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {k: q.grad.clone() for k, q in mim.named_parameters() if q.grad is not None}))
    (l_o, g_o), (l_c, g_c), (l_n, g_n), (l_z, g_z) = runs
    assert l_o.shape == () and bool(torch.isfinite(l_o)) and torch.equal(l_o, l_c) and not torch.equal(l_o, l_n)
    want = sorted(g_c)
    assert sorted(g_o) == want and "mask_token" in want and any(k.startswith("to_pixels") for k in want)
    bad = [k for k in want if not (torch.equal(g_o[k], g_c[k]) and bool(torch.isfinite(g_o[k]).all()))]
    assert not bad, bad
    assert float(g_o["mask_token"].abs().max()) > 0
    assert torch.equal(l_z, l_n) and not [k for k in want if not torch.equal(g_z[k], g_n[k])]
    with torch.no_grad():   # the graphless path (eval): the same entry points
        assert torch.equal(mim.eval().forward_at(tiles, table, masks, orient=orient), mim(copies, masks))


# ------------------------------------------------------------------------------------------ 4. against the CPU oracle
def test_forward_at_orient_vs_oracle():
    """independent of this project's kernels: the fp32 patch-head logits against the oracle on the oriented windows, at the bar the other
    GPU-against-oracle forwards of the classification path use (1e-4 of the largest logit)"""
    from oracle import classify_forward
    seed_all(5)
    enc = _encoder("default", "fp32")
    s, scene, table, orient = _scene_and_table("default")
    params = {"encoder." + k: v.detach().clone() for k, v in enc.state_dict().items()}
    cfg = oracle_cfg_from(dict(bands=20, depth=1, heads=2, n_classes=5, image_size=8))
    with torch.no_grad():
        ref = classify_forward(params, oriented_stack(scene, table, orient, s), cfg)
        logits = enc.cuda().eval().forward_at(scene.cuda(), table, orient=orient)
    assert logits.shape == ref.shape
    err = relerr(logits, ref)
    print("forward_at(orient) vs oracle, max error relative to the largest logit:", err)
    assert err < 1e-4, err


# ------------------------------------------------------------------------------------------ 5. predict_at(tta="d4")
@pytest.mark.parametrize("head", ["pixelwise", "default"])
def test_predict_at_d4_is_the_mean_over_the_eight_orientations(head):
    from maskedsst_amd import orient_windows
    seed_all(5)
    enc = _encoder(head).cuda().train()   # predict_at runs the eval forward whatever the mode
    s, scene, table, orient = _scene_and_table(head)
    scene = scene.cuda()
    n = table.shape[0]
    total = None
    for code in range(8):
        codes = torch.full((n,), code, dtype=torch.uint8)
        _, lg = enc.predict_at(scene, table, return_logits=True, orient=codes)
        if head != "pixelwise":
            lg = orient_windows(lg, codes, inverse=True)
        total = lg if total is None else total + lg
    want = total / 8
    cls, got = enc.predict_at(scene, table, return_logits=True, tta="d4")
    assert enc.training and got.shape == ((n, 5) if head == "pixelwise" else (n, 5, s, s))
    assert torch.equal(got, want) and torch.equal(cls, want.argmax(dim=1)) and bool(torch.isfinite(got).all())
    assert torch.equal(enc.predict_at(scene, table, return_logits=True, tta="d4", max_windows=3)[1], want)
    assert torch.equal(enc.predict_at(scene, table.cuda(), tta="d4"), cls)
    _, plain = enc.predict_at(scene, table, return_logits=True)
    assert not torch.equal(plain, got)
    # orient alone is passed through per chunk
    _, one = enc.predict_at(scene, table, return_logits=True, orient=orient)
    assert torch.equal(enc.predict_at(scene, table, return_logits=True, orient=orient, max_windows=3)[1], one)
    with torch.no_grad():
        assert torch.equal(one, enc.eval()(oriented_stack(scene, table, orient, s)).reshape(one.shape))


# ------------------------------------------------------------------------------------------ 6. the scripts' steps, in process
def _finetune_script():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("finetune_script_orient", os.path.join(ROOT, "finetune.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    return ft


# (head, --train-at mode, loss): torch's CrossEntropyLoss over [n, nc, s, s] logits sums with atomics, so the patch head steps with the HIP loss
SCRIPT_CASES = [("pixelwise", "labelled", "torch"), ("default", "random", "fused")]


@pytest.mark.parametrize("head,mode,loss", SCRIPT_CASES, ids=[f"{h}-{m}" for h, m, _ in SCRIPT_CASES])
def test_finetune_augment_d4_step_is_the_step_on_the_oriented_copies(head, mode, loss, capsys):
    """finetune.py --train-at ... --augment d4: its step (train_step_at_listed) against train_step on the oriented stacked copy of the
    windows and codes it draws -- the table first, then the codes, from the one generator --, loss and every updated parameter bit for
    bit; then --val-at --val-tta prints its line"""
    from maskedsst_amd import centre_origins, random_orients, random_origins, window_labels
    from maskedsst_amd.config import Dotdict
    from maskedsst_amd.utils import train_step
    ft = _finetune_script()
    pix = head == "pixelwise"
    s, n = (7 if pix else 8), 16
    cfg = Dotdict(dict(image_size=8, patch_sub=1 if pix else 0, pixelwise=pix, ignored_label=-1, lr=1e-3, mlp_head_lr=3e-3,
                       weight_decay=1e-4, linear_eval=False))
    seed_all(5)
    scene = torch.randn(2, 20, *SCENE_HW)
    label_map = torch.randint(-1, 5, (2, *SCENE_HW))
    results = []
    for at in (True, False):
        seed_all(7)
        enc = _encoder(head).cuda().train()
        opt = ft.make_optimizer(enc, cfg, "torch")
        criterion = ft.make_criterion(loss, -1)
        gen = torch.Generator().manual_seed(9)
        if at:
            out = ft.train_step_at_listed(scene.cuda(), label_map, enc, cfg, criterion, opt, mode, n, gen, augment="d4")
        else:
            if pix:
                origins, labels = centre_origins(label_map, s, -1)
                pick = torch.randperm(origins.shape[0], generator=gen)[:n]
                origins, labels = origins[pick], labels[pick]
                orient = random_orients(n, generator=gen)
            else:
                origins = random_origins(2, *SCENE_HW, s, n, generator=gen, labels=label_map, ignore_index=-1)
                orient = random_orients(n, generator=gen)
                labels = window_labels(label_map, origins, s, orient)
            assert len(set(orient.tolist())) > 3
            out = train_step(oriented_stack(scene.cuda(), origins, orient, s), labels, enc, cfg, "cuda", criterion, opt)
        torch.cuda.synchronize()
        results.append((out[0].detach().clone(), float(out[1]), {k: q.detach().clone() for k, q in enc.named_parameters()}))
    (loss_at, acc_at, p_at), (loss_st, acc_st, p_st) = results
    bad = [k for k in p_at if not (torch.equal(p_at[k], p_st[k]) and bool(torch.isfinite(p_at[k]).all()))]
    assert not bad, bad
    assert bool(torch.isfinite(loss_at)) and torch.equal(loss_at, loss_st) and acc_at == acc_st
    capsys.readouterr()
    val = (torch.randn(2, 20, *SCENE_HW).cuda(), torch.randint(-1, 5, (2, *SCENE_HW)).cuda())
    lines = []
    for tta in (True, False):
        ft.validate_at(enc, val, 1, -1, tta=tta)
        lines.append(capsys.readouterr().out.strip())
    assert all(line.startswith("val step 1 loss ") and "nan" not in line for line in lines) and lines[0] != lines[1], lines


def test_resident_tile_loader_d4_feeds_simmim_forward_at():
    """pretrain.py --resident-tiles --augment d4: the loader's (tiles, origins, orient) through SimMIMSpatialSpectral.forward_at, against
    the loss of the oriented stacked windows with the masks it drew"""
    from maskedsst_amd import ViTSpatialSpectral, SimMIMSpatialSpectral
    from maskedsst_amd.data import ResidentTileLoader
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=5, dim=96, depth=1, heads=2, mlp_dim=64,
                             dropout=0.0, emb_dropout=0.0, channels=20, spectral_pos_embed=False, spectral_pos=torch.arange(2),
                             blockwise_patch_embed=True, precision="fp32")
    mim = SimMIMSpatialSpectral(encoder=enc, masking_ratio=0.7, mask_patch_size=4, tube_masking=True).cuda().eval()
    loader = ResidentTileLoader(6, 20, image_size=8, tile_size=16, pool_tiles=3, steps=2, seed=11, device="cuda", crop="sample", augment="d4")
    steps = 0
    with torch.no_grad():
        for tiles, origins, orient in loader:
            loss = mim.forward_at(tiles, origins, check=False, orient=orient)
            want = mim(oriented_stack(tiles, origins, orient, 8), mim.last_masks)
            assert tiles.is_cuda and torch.equal(loss, want) and bool(torch.isfinite(loss))
            steps += 1
    assert steps == 2

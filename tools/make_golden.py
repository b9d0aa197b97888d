#!/usr/bin/env python3
"""Generate golden vectors by importing the reference (HSG-AIML/MaskedSST) in THIS container.

The reference Python cannot travel to the GPU box, so its outputs are captured here as small
``.npz`` fixtures under ``tests/golden/`` and committed together with this script.

Protocol: ``random.seed(5); np.random.seed(5); torch.manual_seed(5)``; build the
reference encoder, wrap it in the reference SimMIM module, ``x = torch.randn(B, C, 8, 8)``,
``eval()`` (dropout off), forward -> loss, backward -> grads.  For every case we store

* the config, the bool mask (bit-packed) and the masked indices (bit-exact parity targets),
* per-tensor fingerprints of every parameter and every gradient
  (float64 sum, float64 abs-sum, first 8 elements) -- the oracle re-draws the parameters from the
  same seed in the same order, so a fingerprint is enough to pin it,
* fingerprints of the intermediates (tokens after embed / after mask scatter / after the spatial
  stack / after the spectral stack / predicted pixels) and the loss,
* for the ``tiny`` case the FULL state_dict, input and gradients (element-wise checks).

Also captured: an AdamW loss trajectory on the BASELINE config-1 shape (5 steps, clamp hook,
dropout 0) and a finetune (classification) step.

Run:  PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/make_golden.py
"""
import os
import sys
import random
import json

import numpy as np

np.float = float  # reference src/pos_embed.py:52 uses the alias removed in numpy>=1.24

import torch
import torch.nn.functional as F

REF = os.environ.get("MSST_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

from src.vit_spatial_spectral import ViTSpatialSpectral  # noqa: E402
from src.vit_simmim_original import SimMIMSpatialSpectral  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
SEED = 5


def seed_all():
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)


def fp(t):
    """fingerprint: [sum, abs-sum] in float64 + first 8 elements + shape."""
    t = t.detach().to(torch.float64).reshape(-1)
    head = np.zeros(8, dtype=np.float64)
    n = min(8, t.numel())
    head[:n] = t[:n].numpy()
    return np.concatenate([[t.sum().item(), t.abs().sum().item(), float(t.numel())], head])


def build(cfg):
    P = cfg.get("spectral_patch", 10)
    enc = ViTSpatialSpectral(
        image_size=cfg.get("image_size", 8),
        spatial_patch_size=1,
        spectral_patch_size=P,
        num_classes=cfg.get("n_classes", 8),
        dim=96,
        depth=cfg["depth"],
        heads=cfg.get("heads", 8),
        mlp_dim=64,
        dropout=cfg.get("dropout", 0.0),
        emb_dropout=cfg.get("dropout", 0.0),
        channels=cfg["bands"],
        spectral_pos_embed=cfg.get("spectral_pos_embed", False),
        spectral_pos=torch.arange(cfg["bands"] // P),
        blockwise_patch_embed=True,
        spectral_only=False,
    )
    model = SimMIMSpatialSpectral(
        encoder=enc,
        intermediate_losses=False,
        masking_ratio=cfg.get("masking_ratio", 0.7),
        mask_patch_size=cfg.get("mask_patch_size", 4),
        to_pixels_per_spectral_block=cfg.get("to_pixels_per_spectral_block", True),
        tube_masking=cfg.get("tube_masking", True),
    )
    if cfg.get("qkv_scale"):
        # "peaky attention" cases: a randomly initialised model has logits O(0.3) and near-uniform attention
        # rows, where a softmax error is invisible.  Every to_qkv.weight (vit_spatial_spectral.py:58) is scaled after construction:
        # q and k both grow, so the logits of :67-71 go with the SQUARE of the factor.
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n.endswith("to_qkv.weight"):
                    p.mul_(float(cfg["qkv_scale"]))
    return model


def attention_stats(model, x):
    """logit spread and mean row maximum of the softmax (vit_spatial_spectral.py:67-76) of the first / last block of both stacks,
    measured by hooks on the reference's own modules: says how peaky a fixture's attention is."""
    from src.vit_spatial_spectral import Attention
    from einops import rearrange
    rows = []

    def hook(mod, inp):
        with torch.no_grad():
            q, k, _ = mod.to_qkv(inp[0]).chunk(3, dim=-1)
            q, k = (rearrange(t, "b n (h d) -> b h n d", h=mod.heads) for t in (q, k))
            dots = torch.matmul(q, k.transpose(-1, -2)) * mod.scale
            rows.append([dots.std().item(), dots.abs().max().item(), dots.softmax(-1).max(-1).values.mean().item()])

    hs = [m.register_forward_pre_hook(hook) for m in model.modules() if isinstance(m, Attention)]
    state = (np.random.get_state(), torch.get_rng_state())
    with torch.no_grad():
        model(x)
    np.random.set_state(state[0])
    torch.set_rng_state(state[1])
    for h in hs:
        h.remove()
    L = len(rows) // 2
    return np.array([rows[0], rows[L - 1], rows[L], rows[-1]], dtype=np.float64)


def staged_forward(model, x):
    """Re-run the reference forward stage by stage using the reference's own sub-modules
    (same RNG draws as SimMIMSpatialSpectral.forward) to expose intermediates."""
    enc = model.encoder
    patches = model.to_patch(x)
    B = patches.shape[0]
    tokens = model.patch_to_emb(patches)
    patches = patches.reshape(B, -1, patches.shape[-1])
    T = tokens.shape[1]
    if enc.spectral_pos_embed:
        pos = enc.get_pos_embeddings()
    else:
        pos = enc.pos_embedding[:, :T]
    tok_embed = tokens
    tokens = tokens + pos
    mask_tokens = model.mask_token[None, None, :] + pos
    num_masked = int(model.masking_ratio * T)
    if model.mask_patch_size == 1:
        idx = torch.rand(B, T).topk(k=num_masked, dim=-1).indices
        bm = torch.zeros((B, T)).scatter_(-1, idx, 1).bool()
    elif model.tube_masking:
        bm, idx = model.mask_generator.get_batch_tube_masked(
            batch_size=B, channel_tokens=enc.num_spectral_patches, num_masked=num_masked, device=x.device
        )
    else:
        bm, idx = model.mask_generator.get_batch(
            batch_size=B, channel_tokens=enc.num_spectral_patches, num_masked=num_masked, device=x.device
        )
    tok_masked = torch.where(bm[..., None], mask_tokens, tokens)
    seq = enc.spatial_spectral_transformer
    t0 = seq[0](tok_masked)
    t1 = seq[1](t0)  # spatial stack
    t2 = seq[2](t1)
    t3 = seq[3](t2)  # spectral stack
    enc_out = seq[4](t3)
    after_spatial = t1.reshape(B, enc.num_spectral_patches, enc.num_spatial_patches, -1).reshape(B, T, -1)
    br = torch.arange(B)[:, None]
    enc_m = enc_out[br, idx]
    if model.to_pixels_per_spectral_block:
        blk = torch.arange(enc.num_spectral_patches).repeat_interleave(enc.num_spatial_patches)
        blk = blk.unsqueeze(0).repeat(B, 1)[br, idx]
        pred = model.to_pixels(enc_m, blk)
    else:
        pred = model.to_pixels(enc_m)
    target = patches[br, idx]
    loss = F.l1_loss(pred, target) / num_masked
    return dict(
        tok_embed=tok_embed, tok_masked=tok_masked, after_spatial=after_spatial, enc_out=enc_out,
        pred=pred, target=target, loss=loss, bool_mask=bm, masked_indices=idx,
    )


def run_case(name, cfg, full=False, save=True):
    """save=False: return the capture instead of writing simmim_<name>.npz"""
    seed_all()
    model = build(cfg)
    B, C = cfg["B"], cfg["bands"]
    x = torch.randn(B, C, cfg.get("image_size", 8), cfg.get("image_size", 8))
    if cfg.get("zero_pad_bands"):
        x[:, C - cfg["zero_pad_bands"]:] = 0.0
    model.eval()
    attn = attention_stats(model, x) if cfg.get("qkv_scale") else None

    np_state = np.random.get_state()
    t_state = torch.get_rng_state()
    loss = model(x)
    model.zero_grad()
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}

    # staged re-run with the same RNG state
    np.random.set_state(np_state)
    torch.set_rng_state(t_state)
    with torch.no_grad():
        st = staged_forward(model, x)
    assert torch.equal(st["loss"], loss.detach()), (st["loss"].item(), loss.item())

    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "loss": np.array(loss.item(), dtype=np.float64),
        "loss_f32": loss.detach().numpy(),
        "x_fp": fp(x),
        "bool_mask_bits": np.packbits(st["bool_mask"].numpy().astype(np.uint8), axis=-1),
        "masked_indices": st["masked_indices"].numpy().astype(np.int16),
        "n_params": np.array(sum(p.numel() for p in model.parameters()), dtype=np.int64),
    }
    if attn is not None:
        out["attn_stats"] = attn    # rows: spatial block 0 / L-1, spectral block 0 / L-1; columns: logit std, max |logit|, mean row max of p
    gsq = 0.0
    names = []
    for k, p in model.named_parameters():
        names.append(k)
        out["p_fp/" + k] = fp(p)
        g = grads[k]
        if g is None:
            out["g_none/" + k] = np.array(1)
        else:
            out["g_fp/" + k] = fp(g)
            gsq += float((g.double() ** 2).sum())
    out["names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)
    out["grad_l2"] = np.array(gsq ** 0.5, dtype=np.float64)
    for k in ["tok_embed", "tok_masked", "after_spatial", "enc_out", "pred", "target"]:
        out["i_fp/" + k] = fp(st[k])
        # a deterministic 64-element strided slice for element-wise checks
        flat = st[k].reshape(-1)
        stride = max(1, flat.numel() // 64)
        out["i_slice/" + k] = flat[::stride][:64].numpy().astype(np.float32)
    if full:
        out["x"] = x.numpy()
        for k, v in model.state_dict().items():
            out["sd/" + k] = v.numpy()
        for k, g in grads.items():
            if g is not None:
                out["grad/" + k] = g.numpy()
        for k in ["tok_embed", "tok_masked", "after_spatial", "enc_out", "pred", "target"]:
            out["full/" + k] = st[k].numpy()
    if not save:
        return out
    np.savez_compressed(os.path.join(OUT, f"simmim_{name}.npz"), **out)
    print(f"{name}: loss={loss.item():.9e} grad_l2={gsq ** 0.5:.6e} n_params={int(out['n_params'])} "
          f"idx[1,:4]={st['masked_indices'][min(1, B - 1), :4].tolist()}")


PEAKY = [("50b_L12_B8", dict(bands=50, depth=12, B=8)), ("200b_L12_B4", dict(bands=200, depth=12, B=4))]


def run_peaky():
    """Both BASELINE depth-12 shapes with every to_qkv.weight scaled x4 / x8 after construction.  Logits grow with the square:
    x4 -> logit std ~5, mean row maximum 0.5-0.8 (the regime a trained model lives in); x8 -> std ~22, row maximum 0.9 (`attn_stats`
    in each fixture holds the measured numbers).  x16 (std ~86, rows one-hot to 0.98, gradient norm 1e8) was generated once and is
    NOT kept: the oracle -- a second fp32 CPU evaluation of the same formulas -- already differs from the reference by 4e-3 / 8e-3 in
    the loss there (x8: 2e-5 / 1.2e-4 in the loss, 8e-2 of max in enc_out; x4: 1e-5 everywhere), so it pins nothing."""
    for tag, cfg in PEAKY:
        for s in (4, 8):
            run_case(f"{tag}_qkv{s}", dict(cfg, qkv_scale=s))


def run_f64_anchor(name, cfg):
    """`loss_f64`, added to an existing fixture: the reference's loss in float64 on the same parameters, input and masks.  The x8
    fixtures amplify fp32 round-off to ~1e-3 of the loss, and which round-off depends on the CPU (MKL picks its kernels by
    processor), so their fp32 loss pins the oracle only on a CPU like the one that wrote it; in float64 two evaluations of the
    same formulas agree to ~1e-12 on any CPU."""
    path = os.path.join(OUT, f"simmim_{name}.npz")
    z = np.load(path)
    out = {k: z[k] for k in z.files}
    seed_all()
    model = build(cfg)
    B, C = cfg["B"], cfg["bands"]
    x = torch.randn(B, C, cfg.get("image_size", 8), cfg.get("image_size", 8))
    model.eval()
    attention_stats(model, x)   # run_case's draws, in run_case's order
    model.double()
    if hasattr(model.to_pixels, "dtype"):
        model.to_pixels.dtype = torch.float64   # the per-block decoder allocates its output in this dtype (vit_simmim_original.py:25-31)
    dtype = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            loss = model(x.double())
    finally:
        torch.set_default_dtype(dtype)
    assert loss.dtype == torch.float64
    out["loss_f64"] = np.array(loss.item(), dtype=np.float64)
    np.savez_compressed(path, **out)
    print(f"{name}: loss_f64={loss.item():.15e} (fp32 capture {float(out['loss']):.9e})")


def run_f64_anchors():
    for tag, cfg in PEAKY:
        run_f64_anchor(f"{tag}_qkv8", dict(cfg, qkv_scale=8))


def run_adamw_traj():
    """BASELINE config 1 plumbing case: depth 2, 32 cubes 8x8x200, AdamW lr 0.008 wd 0.05,
    clamp hook (pretrain.py:71-73), dropout 0 (deterministic), 5 steps."""
    cfg = dict(bands=200, depth=2, B=32, dropout=0.0)
    seed_all()
    model = build(cfg)
    x = torch.randn(32, 200, 8, 8)
    opt = torch.optim.AdamW(model.parameters(), lr=0.008, weight_decay=0.05)
    for p in model.parameters():
        p.register_hook(lambda grad: torch.clamp(grad, -1, 1))
    model.train()
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model(x)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "losses": np.array(losses, dtype=np.float64),
        "lr": np.array(0.008), "weight_decay": np.array(0.05),
    }
    for k, p in model.named_parameters():
        out["p_fp_after/" + k] = fp(p)
    np.savez_compressed(os.path.join(OUT, "adamw_traj_200b_L2_B32.npz"), **out)
    print("adamw traj:", losses)


def run_finetune_case(name, cfg, save=True):
    """Classification step (finetune.py / src/utils.py:608-663): logits [B,ncls,8,8], CE(ignore -1).
    save=False: return the capture instead of writing finetune_<name>.npz"""
    seed_all()
    P, w = cfg.get("spectral_patch", 10), cfg.get("image_size", 8)
    enc = ViTSpatialSpectral(
        image_size=w, spatial_patch_size=1, spectral_patch_size=P, num_classes=cfg["n_classes"],
        dim=96, depth=cfg["depth"], heads=cfg.get("heads", 8), mlp_dim=64, dropout=0.0, emb_dropout=0.0,
        channels=cfg["bands"], spectral_pos_embed=cfg["spectral_pos_embed"],
        spectral_pos=torch.arange(cfg["bands"] // P), blockwise_patch_embed=True,
    )
    B = cfg["B"]
    x = torch.randn(B, cfg["bands"], w, w)
    label = torch.randint(-1, cfg["n_classes"], (B, w, w))
    enc.eval()
    logits = enc(x)
    loss = F.cross_entropy(logits, label, ignore_index=-1)
    loss.backward()
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "loss": np.array(loss.item(), dtype=np.float64),
        "label": label.numpy().astype(np.int8),
        "logits_fp": fp(logits),
        "logits": logits.detach().numpy() if logits.numel() <= 8192 else logits.detach().numpy()[:4],
        "n_params": np.array(sum(p.numel() for p in enc.parameters()), dtype=np.int64),
    }
    gsq = 0.0
    names = []
    for k, p in enc.named_parameters():
        names.append(k)
        out["p_fp/" + k] = fp(p)
        out["g_fp/" + k] = fp(p.grad)
        gsq += float((p.grad.double() ** 2).sum())
    out["names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)
    out["grad_l2"] = np.array(gsq ** 0.5, dtype=np.float64)
    if not save:
        return out
    np.savez_compressed(os.path.join(OUT, f"finetune_{name}.npz"), **out)
    print(f"finetune {name}: loss={loss.item():.9e} grad_l2={gsq ** 0.5:.6e} n_params={int(out['n_params'])}")


def _stub_reference_script_imports():
    """src/utils.py imports wandb, torchvision, torchmetrics, rasterio and spectral at module level (absent here; none
    of them is touched by load_checkpoint): satisfy those imports with inert placeholder modules."""
    import importlib.abc
    import importlib.machinery
    import types

    class _Any:
        def __init__(self, *a, **k):
            pass

        def __call__(self, *a, **k):
            return _Any()

        def __getattr__(self, k):
            return _Any()

        def __mro_entries__(self, bases):
            return (object,)

    class _Stub(types.ModuleType):
        __path__ = []

        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return _Any()

    class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
        ROOTS = ("wandb", "torchvision", "torchmetrics", "rasterio", "spectral")

        def find_spec(self, name, path, target=None):
            if name.split(".")[0] in self.ROOTS:
                return importlib.machinery.ModuleSpec(name, self, is_package=True)

        def create_module(self, spec):
            return _Stub(spec.name)

        def exec_module(self, m):
            pass

    sys.meta_path.insert(0, Finder())


def run_load_checkpoint():
    """Checkpoint hand-off pretrain -> finetune (reference src/utils.py:276-313): a SimMIM state_dict in the
    reference's checkpoint dictionary (pretrain.py:135-148) is loaded into a fresh encoder with a different class count by
    the REFERENCE's load_checkpoint.  Stored: the key list before (checkpoint) and after (encoder.state_dict()), which
    tensors carry checkpoint values / fresh values (fingerprints), so that the product's load_checkpoint can be held to
    the same renames, drops and strictness without the reference."""
    import tempfile
    _stub_reference_script_imports()
    from src.utils import load_checkpoint

    class Cfg:
        pass

    cfg = dict(bands=50, depth=2, B=2, n_classes_pretrain=8, n_classes_finetune=20)
    seed_all()
    mim = build(dict(bands=50, depth=2, B=2, n_classes=cfg["n_classes_pretrain"]))
    sd = mim.state_dict()
    before = list(sd.keys())
    before_fp = {k: fp(v) for k, v in sd.items()}
    enc = ViTSpatialSpectral(
        image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=cfg["n_classes_finetune"],
        dim=96, depth=2, heads=8, mlp_dim=64, dropout=0.0, emb_dropout=0.0, channels=50,
        spectral_pos_embed=False, spectral_pos=torch.arange(5), blockwise_patch_embed=True)
    fresh_fp = {k: fp(v) for k, v in enc.state_dict().items()}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ck.pth")
        torch.save({"model_state_dict": sd, "losses": torch.zeros(1)}, path)
        c = Cfg()
        c.checkpoint_path, c.patch_sub, c.image_size = path, 0, 8
        enc = load_checkpoint(c, enc, "mlp_head", "cpu")
    after = list(enc.state_dict().keys())
    out = {
        "cfg": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8),
        "before": np.frombuffer("\n".join(before).encode(), dtype=np.uint8),
        "after": np.frombuffer("\n".join(after).encode(), dtype=np.uint8),
    }
    src = []
    for k, v in enc.state_dict().items():
        got = fp(v)
        if np.array_equal(got, before_fp.get("encoder." + k, None)):
            src.append("checkpoint")
        elif np.array_equal(got, fresh_fp[k]):
            src.append("fresh")
        else:
            src.append("other")
        out["after_fp/" + k] = got
    out["after_source"] = np.frombuffer("\n".join(src).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "load_checkpoint_50b_L2.npz"), **out)
    print("load_checkpoint:", len(before), "keys before,", len(after), "after;",
          {s_: src.count(s_) for s_ in set(src)},
          "dropped:", [k for k in before if not k.startswith("encoder.")][:3], "...")


def run_config_kat():
    """Merged hyper-parameter bags of the reference's own config loaders on the reference's own YAML files
    (src/utils.py:316-364): every key and every value that is not a filesystem path."""
    _stub_reference_script_imports()
    from src.utils import get_pretrain_config, get_finetune_config
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        pre = get_pretrain_config("configs/pretrain_config.yaml", "configs/config.yaml", SEED, "cpu").__dict__
        fin = get_finetune_config("configs/finetune_config_enmap.yaml", "configs/config.yaml", SEED, "cpu").__dict__
    finally:
        os.chdir(cwd)

    def clean(d):
        out = {}
        for k, v in d.items():
            if torch.is_tensor(v):
                v = v.tolist()
            if isinstance(v, str) and ("/" in v):
                v = "<path>"
            out[k] = v
        return out
    blob = json.dumps({"pretrain": clean(pre), "finetune_enmap": clean(fin)}, sort_keys=True)
    np.savez_compressed(os.path.join(OUT, "config_kat.npz"), json=np.frombuffer(blob.encode(), dtype=np.uint8))
    print("config KAT:", len(pre), "pretrain keys,", len(fin), "finetune keys")


# spectral patch depths other than the shipped 10 (configs' band_patch_size): the generic tokenizer and to-pixels head paths.
# Not named simmim_*: tests/test_oracle_golden.py globs that prefix with a config that has no spectral patch depth.
PATCH_CASES = [("P5_50b_L1_B2", dict(bands=50, depth=1, B=2, spectral_patch=5), dict(n_classes=8)),
               ("P16_64b_L1_B3_img6_mps2_h2", dict(bands=64, depth=1, B=3, image_size=6, mask_patch_size=2, heads=2, spectral_patch=16),
                dict(n_classes=5))]


def run_patch_cases():
    """For each PATCH_CASES shape, one fixture patch_<name>.npz: the SimMIM capture of run_case (same keys) and, under "ft/", the
    default-head classifier step of run_finetune_case at the same spectral patch depth and image size"""
    for name, cfg, ft in PATCH_CASES:
        out = run_case(name, cfg, save=False)
        ft_cfg = dict(bands=cfg["bands"], depth=cfg["depth"], B=cfg["B"], heads=cfg.get("heads", 8), image_size=cfg.get("image_size", 8),
                      spectral_patch=cfg["spectral_patch"], spectral_pos_embed=False, **ft)
        for k, v in run_finetune_case(name, ft_cfg, save=False).items():
            out["ft/" + k] = v
        np.savez_compressed(os.path.join(OUT, f"patch_{name}.npz"), **out)
        print(f"patch {name}: loss={float(out['loss']):.9e} ft loss={float(out['ft/loss']):.9e}")


def run_spectral_pos_kat():
    """Houston2018 -> EnMAP spectral-position lookup (reference src/utils.py:415-429 -> vit_spatial_spectral.py:767-800):
    the sensors' band-centre tables (data), the reference's answer for the shipped spectral patch depth (the SURVEY 8c KAT
    [0, 3, 5, 7, 9]) and for two other depths (ragged last block)."""
    _stub_reference_script_imports()
    from src.data_enmap import wavelengths as enmap_waves, invalid_l2_bands
    from src.data_houston2018 import wavelengths as houston_waves
    from src.vit_spatial_spectral import get_pos_for_spectral_embedding
    ref = np.array(enmap_waves)[~np.array(invalid_l2_bands)]
    out = {"houston_waves": np.array(houston_waves, dtype=np.float64), "enmap_waves_valid": ref.astype(np.float64)}
    for depth in (10, 7, 16):
        out[f"pos_depth{depth}"] = np.array(get_pos_for_spectral_embedding(depth, houston_waves, ref), dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "spectral_pos_houston.npz"), **out)
    print("spectral pos KAT:", out["pos_depth10"].tolist(), len(houston_waves), len(ref))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    if len(sys.argv) > 1 and sys.argv[1] == "spectral_pos":
        run_spectral_pos_kat()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "config":
        run_config_kat()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "load_checkpoint":
        run_load_checkpoint()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "peaky":   # depth-12 cases with peaky attention rows (to_qkv.weight x4 / x8)
        run_peaky()
        run_f64_anchors()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "f64":   # float64 loss anchors of the x8 fixtures, added to the files run_peaky wrote
        run_f64_anchors()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "shapes":   # other image sizes / sequence packings (padding rows in the 64-row tiles)
        run_case("70b_L1_B3_img4_mps2", dict(bands=70, depth=1, B=3, image_size=4, mask_patch_size=2))
        run_case("30b_L1_B2_img6_mps2_h2", dict(bands=30, depth=1, B=2, image_size=6, mask_patch_size=2, heads=2))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "patch":   # spectral patch depths 5 and 16 (SimMIM + default-head classifier)
        run_patch_cases()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "tiny":  # regenerate only the element-wise cases
        run_case("tiny_20b_L1_B2_h2", dict(bands=20, depth=1, B=2, heads=2), full=True)
        run_case("tiny_30b_L1_B3_h2_nontube", dict(bands=30, depth=1, B=3, heads=2, tube_masking=False), full=True)
        sys.exit(0)
    # element-wise case: everything stored in full
    run_case("tiny_20b_L1_B2_h2", dict(bands=20, depth=1, B=2, heads=2), full=True)
    run_case("tiny_30b_L1_B3_h2_nontube", dict(bands=30, depth=1, B=3, heads=2, tube_masking=False), full=True)
    # BASELINE shapes (fingerprints only)
    run_case("200b_L2_B32", dict(bands=200, depth=2, B=32))
    run_case("50b_L12_B8", dict(bands=50, depth=12, B=8))
    run_case("50b_L12_B8_zeropad", dict(bands=50, depth=12, B=8, zero_pad_bands=2))
    run_case("200b_L12_B4", dict(bands=200, depth=12, B=4))
    # option coverage
    run_case("50b_L2_B4_mps1", dict(bands=50, depth=2, B=4, mask_patch_size=1))
    run_case("50b_L2_B4_nontube", dict(bands=50, depth=2, B=4, tube_masking=False))
    run_case("50b_L2_B4_specpos", dict(bands=50, depth=2, B=4, spectral_pos_embed=True))
    run_case("50b_L2_B4_sharedpix", dict(bands=50, depth=2, B=4, to_pixels_per_spectral_block=False))
    run_case("50b_L2_B4_mps2_r50", dict(bands=50, depth=2, B=4, mask_patch_size=2, masking_ratio=0.5))
    run_case("70b_L1_B3_img4_mps2", dict(bands=70, depth=1, B=3, image_size=4, mask_patch_size=2))
    run_case("30b_L1_B2_img6_mps2_h2", dict(bands=30, depth=1, B=2, image_size=6, mask_patch_size=2, heads=2))
    run_peaky()
    run_f64_anchors()
    run_adamw_traj()
    run_finetune_case("200b_L4_B2", dict(bands=200, depth=4, B=2, n_classes=8, spectral_pos_embed=False))
    run_finetune_case("50b_L2_B2_specpos", dict(bands=50, depth=2, B=2, n_classes=20, spectral_pos_embed=True))
    run_patch_cases()
    run_load_checkpoint()
    run_spectral_pos_kat()
    run_config_kat()

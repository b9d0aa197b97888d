"""Parameters and inputs like those of a trained model, for the parity tests of the block kernels (tests/test_gpu_trained_state.py,
tests/test_trained_state_host.py).  At random initialisation every LayerNorm has gamma = 1 and beta = 0 and the residual stream has
|x| ~ std: a kernel that forgets gamma or beta somewhere, or loses small channels beside large ones, computes the same bits as a right
one.  Three states, each drawn from a seeded torch.Generator on the CPU:

  affine   every block: both LayerNorms gamma = sign x magnitude, magnitude ~ U[0.5, 1.5], sign = -1 on a random quarter of the
           channels (a structural gamma slip is then an O(1) error, not a 30 % one), beta ~ U[-0.3, 0.3]; to_out.0.bias, net.0.bias,
           net.3.bias ~ N(0, 0.3^2).  max |beta / gamma| <= 0.6.
  stream   the block input: one scale per channel, exp(U[-ln 4, ln 4]), two random channels at 30 ("massive" channels), then +30 or
           -30 per sample.  The scale is the same for every token, so the per-sequence offsets of tokens_with_offsets survive.
  both     the two together.
"""
import math

import torch

STATES = ("affine", "stream", "both")
# (block mode, L): spectral 20 -- three sequences per tile, plain rows; spectral 22 -- two per tile, peaky rows (qkv_scale 4);
# spatial 25 -- two per tile, peaky; spatial 64 -- a full tile, plain.  Built by test_gpu_seq_lengths.case_cfg: two attention tiles,
# the last one partly filled where a tile packs several sequences
SHAPES = [(1, 20), (1, 22), (0, 25), (0, 64)]
SNAME = {0: "spatial", 1: "spectral"}
SHAPE_IDS = [f"{SNAME[m]}-{L}" for m, L in SHAPES]
BLOCKS = "spatial_spectral_transformer"
GAMMA_LO, GAMMA_HI, BETA_MAX, BIAS_STD = 0.5, 1.5, 0.3, 0.3
MAX_RATIO = BETA_MAX / GAMMA_LO            # 0.6
MASSIVE, SAMPLE_OFFSET = 30.0, 30.0


def signed_gamma(n, g):
    """magnitude ~ U[0.5, 1.5], negative on a random quarter of the n channels"""
    w = GAMMA_LO + (GAMMA_HI - GAMMA_LO) * torch.rand(n, generator=g)
    w[torch.randperm(n, generator=g)[:n // 4]] *= -1.0
    return w


def new_value(name, p, g, everything):
    """the trained-state value of parameter `name` (shape and dtype of p), or None where it keeps its initial value.  Block
    parameters: LayerNorm weights and biases and the three bias vectors.  everything=True: the same recipe for every other LayerNorm
    and bias (tokenizer norms, embedding and to_pixels biases), and N(0, 0.3^2) added to the position table and the mask token."""
    if not everything and BLOCKS not in name:
        return None
    leaf = name.rsplit(".", 1)[-1]
    if "norm" in name and leaf == "weight":
        return signed_gamma(p.numel(), g).reshape(p.shape)
    if "norm" in name and leaf == "bias":
        return (BETA_MAX * (2.0 * torch.rand(p.numel(), generator=g) - 1.0)).reshape(p.shape)
    if leaf == "bias":
        return BIAS_STD * torch.randn(p.shape, generator=g)
    if everything and (name.endswith("pos_embedding") or name == "mask_token"):
        return p.detach().cpu().float() + BIAS_STD * torch.randn(p.shape, generator=g)
    return None


def make_affine(model, params, seed=77, everything=False):
    """writes the `affine` state into the model's parameters and, bit for bit the same, into `params` (the dict the float64 reference
    reads).  Run it before model.engine() is first called.  -> the names it wrote"""
    g = torch.Generator().manual_seed(seed)
    wrote = []
    with torch.no_grad():
        for name, p in model.named_parameters():
            v = new_value(name, p, g, everything)
            if v is None:
                continue
            v = v.to(torch.float32)
            p.copy_(v)
            params[name].copy_(v)
            wrote.append(name)
    return wrote


def affine_edit(state, seed=77, everything=False):
    """the `edit` hook of test_gpu_seq_lengths.make_model for a state (None where the state leaves the parameters alone)"""
    if state not in ("affine", "both"):
        return None
    return lambda model, params: make_affine(model, params, seed, everything)


def max_beta_over_gamma(params):
    """max |beta / gamma| over the LayerNorms of every block in params"""
    worst = 0.0
    for k, v in params.items():
        if BLOCKS in k and k.endswith("norm.weight"):
            worst = max(worst, float((params[k[:-len("weight")] + "bias"].abs() / v.abs()).max()))
    return worst


def make_stream(x, seed=88):
    """the `stream` state of a block input x [B, tokens, 96] -> a new tensor"""
    g = torch.Generator().manual_seed(seed)
    D = x.shape[-1]
    scale = torch.exp((2.0 * torch.rand(D, generator=g) - 1.0) * math.log(4.0))
    scale[torch.randperm(D, generator=g)[:2]] = MASSIVE
    off = SAMPLE_OFFSET * (2.0 * torch.randint(0, 2, (x.shape[0],), generator=g).float() - 1.0)
    return (x * scale + off[:, None, None]).contiguous()


def state_inputs(state, x):
    return make_stream(x) if state in ("stream", "both") else x

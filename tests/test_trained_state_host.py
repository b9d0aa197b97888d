"""The trained states of tests/trained_util.py on the host: they are well conditioned, and the fp32 bars of the device tests
(tests/test_gpu_trained_state.py) are reachable by correct arithmetic.

For every state x shape: oracle.model.block in float32 against the same in float64 stays below a quarter of FP32_BARS on the
increment y - x, dx - dy and the worst parameter gradient (max-norm relative, as the fp32 families are measured); the state helper
leaves bit-identical values in the model and in the `params` dict the reference reads; max |beta / gamma| <= 0.6.
Measured (float32 against float64, worst over the twelve cases): increment 8.9e-6 (stream, spatial 64: y is stored at magnitude ~100
and the increment is ~1), dx - dy 5.0e-6 (stream, spectral 22), worst gradient 2.8e-6 (both, spatial 25) -- 2.8x, 10x and 18x inside
the quarter bars.  The whole file runs in 4 s.
"""
import pytest
import torch

from util import build_product, relerr
from test_gpu_seq_lengths import FP32_BARS, Q, case_cfg, block_prefix, block_inputs, block_reference
from trained_util import STATES, SHAPES, SHAPE_IDS, MAX_RATIO, affine_edit, state_inputs, max_beta_over_gamma


@pytest.mark.parametrize("mode,L", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("state", STATES)
def test_states_are_well_conditioned(state, mode, L):
    cfg = case_cfg(mode, L, 8)
    model, params, _ = build_product(cfg, precision="fp32", device="cpu")
    init = {k: v.clone() for k, v in params.items()}
    edit = affine_edit(state)
    wrote = edit(model, params) if edit else []
    named = dict(model.named_parameters())
    assert all(torch.equal(p.detach(), params[n]) for n, p in named.items())            # the same bits on both sides
    changed = sorted(n for n in named if not torch.equal(params[n], init[n]))
    assert changed == sorted(wrote)
    if edit:
        # both LayerNorms and the three bias vectors of both blocks, nothing else
        assert len(wrote) == 2 * 7 and all("spatial_spectral_transformer" in n for n in wrote)
        for n in wrote:
            if n.endswith("norm.weight"):
                assert int((params[n] < 0).sum()) == 24 and 0.5 <= float(params[n].abs().min()) and float(params[n].abs().max()) <= 1.5
        assert 0.3 < max_beta_over_gamma(params) <= MAX_RATIO
    i = 0 if mode == 0 else 1
    S, N = cfg["bands"] // cfg["spectral_patch"], cfg["image_size"] ** 2
    x, dy = block_inputs(cfg, S, N, i)
    x = state_inputs(state, x)
    if state != "affine":
        # |row mean| >> the token noise, and two channels far above the rest
        assert float(x.mean(dim=(1, 2)).abs().min()) > 20.0 and float(x.abs().max()) > 60.0
    r64 = block_reference(params, cfg, S, N, i, x, dy)
    r32 = block_reference(params, cfg, S, N, i, x, dy, dtype=torch.float32)
    pre = block_prefix(i)
    errs = dict(inc_err=relerr(r32["inc"], r64["inc"]), dx=relerr(r32["dxi"], r64["dxi"]),
                worst_grad=max(relerr(r32["grads"][k], r64["grads"][k]) for k in r64["grads"] if k.startswith(pre)))
    print(state, mode, L, errs)
    bad = [(q, errs[q], FP32_BARS[q] / 4) for q in Q if not errs[q] < FP32_BARS[q] / 4]
    assert not bad, bad

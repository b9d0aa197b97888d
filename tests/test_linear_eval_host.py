"""Linear evaluation, host side (no GPU needed): the C ABI of the grouped Adam launch (MSST_VERSION 109), the range table
``FusedAdam`` builds from the parameter groups (``maskedsst_amd.optim.adam_ranges``, on a CPU-flattened bare encoder) and the
two new flags of finetune.py."""
import ctypes
import re
import subprocess

import pytest
import torch

from conftest import seed_all

BADARG = -3   # include/msst.h: MSST_ERR_BADARG


def test_c_abi_declares_and_exports_grouped_adam():
    from maskedsst_amd import _lib
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"^int msst_adam_groups\(", header, re.M) and re.search(r"\}\s*MsstAdamGroup;", header)
    assert _lib.header_version() == 109
    lib = _lib.load()   # refuses a library of another revision or one that lacks a declared symbol
    assert lib.msst_version() == 109 and "msst_adam_groups" in _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T msst_adam_groups$", out, re.M)
    # the struct the binding hands over is the header's: two longs, two floats, two ints
    assert ctypes.sizeof(_lib.MsstAdamGroup) == 32
    m = re.search(r"#define\s+MSST_ADAM_MAX_GROUPS\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.ADAM_MAX_GROUPS


def test_grouped_adam_refuses_bad_tables_on_the_host():
    """every check runs before anything is enqueued, so null buffers and no device are enough to see it"""
    from maskedsst_amd import _lib
    lib = _lib.load()
    G = _lib.MsstAdamGroup
    nbytes = ctypes.sizeof(G)

    def call(rows, n=None, group_bytes=nbytes):
        t = (G * max(1, len(rows)))(*[G(*r) for r in rows])
        return lib.msst_adam_groups(None, None, None, None, t, len(rows) if n is None else n, group_bytes, 0.9, 0.999, 1e-8, 1.0, None)

    ok = (0, 8, 1e-3, 0.0, 1, 0)
    assert call([ok, (4, 12, 1e-3, 0.0, 1, 0)]) == BADARG                      # overlap
    assert b"overlap" in lib.msst_last_error()
    assert call([(8, 16, 1e-3, 0.0, 1, 0), ok]) == BADARG                      # not sorted
    assert call([(8, 4, 1e-3, 0.0, 1, 0)]) == BADARG                           # end < start
    assert call([(0, 8, 1e-3, 0.0, 0, 0)]) == BADARG                           # step 0
    assert call([ok], group_bytes=nbytes - 4) == BADARG                        # another revision's struct
    assert call([(i, i + 1, 1e-3, 0.0, 1, 0) for i in range(_lib.ADAM_MAX_GROUPS + 1)]) == BADARG   # over the cap
    assert call([ok]) == BADARG                                                # a real range over null buffers
    assert call([]) == 0                                                       # empty table: nothing to do
    assert call([(5, 5, 1e-3, 0.0, 1, 0), (9, 9, 1e-3, 0.0, 3, 1)]) == 0       # only empty ranges: nothing launched


def encoder(num_classes=8, depth=2, **kw):
    from maskedsst_amd import ViTSpatialSpectral
    from maskedsst_amd.flat import FlatParams
    seed_all(5)
    enc = ViTSpatialSpectral(image_size=8, spatial_patch_size=1, spectral_patch_size=10, num_classes=num_classes, dim=96, depth=depth,
                             heads=8, mlp_dim=64, channels=50, spectral_pos_embed=False, spectral_pos=torch.arange(5), **kw)
    fp = FlatParams(enc, None).flatten()
    return enc, fp


def give_grads(enc, fp, skip=()):
    """what the HIP backward leaves: every .grad the parameter's own view of the flat gradient buffer"""
    base = fp.flat.data_ptr()
    for n, p in enc.named_parameters():
        if p.requires_grad and n not in skip:
            off = (p.data_ptr() - base) // 4
            p.grad = fp.grad[off:off + p.numel()].view(p.shape)


def two_groups(enc, lr=5e-4, head_lr=5e-3):
    head = [p for n, p in enc.named_parameters() if "mlp_head" in n]
    body = [p for n, p in enc.named_parameters() if "mlp_head" not in n]
    return [dict(params=body, lr=lr, weight_decay=5e-3), dict(params=head, lr=head_lr, weight_decay=5e-3)]


def head_span(fp):
    segs = [v for k, v in fp.segments.items() if k.startswith("mlp_head.")]
    return min(o for o, _, _ in segs), max(o + n for o, n, _ in segs)


def test_ranges_full_finetune_two_learning_rates():
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder()
    give_grads(enc, fp)
    groups = two_groups(enc)
    r = adam_ranges(fp, groups)
    lo, hi = head_span(fp)
    assert lo == 0   # bare encoder: mlp_head | body
    assert [(x.start, x.end) for x in r] == [(0, hi), (hi, fp.total)]
    assert [groups[x.group]["lr"] for x in r] == [5e-3, 5e-4] and [x.step for x in r] == [1, 1]
    assert sum(len(x.params) for x in r) == len(list(enc.parameters()))


def test_ranges_linear_eval_is_the_head_alone():
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder()
    for n, p in enc.named_parameters():
        p.requires_grad_("mlp_head" in n)
    give_grads(enc, fp)
    for groups in (two_groups(enc), [dict(params=[p for n, p in enc.named_parameters() if "mlp_head" in n], lr=5e-4, weight_decay=0.0)]):
        r = adam_ranges(fp, groups)
        assert [(x.start, x.end) for x in r] == [head_span(fp)] and len(r[0].params) == 4


def test_ranges_frozen_tensor_leaves_a_hole_of_itself_and_missing_grad_is_skipped():
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder()
    frozen = "spatial_spectral_transformer.1.layers.0.1.fn.net.0.weight"   # w1 of spatial block 0: in the middle of the body
    nograd = "to_patch_embedding.pre_norm.weight"
    dict(enc.named_parameters())[frozen].requires_grad_(False)
    give_grads(enc, fp, skip=(nograd,))
    r = adam_ranges(fp, two_groups(enc))
    hi = head_span(fp)[1]
    assert len(r) == 4 and (r[0].start, r[0].end) == (0, hi) and r[1].start == hi and r[-1].end == fp.total
    holes = [(a.end, b.start) for a, b in zip(r, r[1:]) if a.end != b.start]
    want = []
    for name in (frozen, nograd):
        p = dict(enc.named_parameters())[name]
        off = (p.data_ptr() - fp.flat.data_ptr()) // 4
        want.append((off, off + p.numel()))
    assert sorted(holes) == sorted(want)


def test_ranges_step_counters_split_and_merge():
    """segments merge only while their step counters are equal (a tensor that got its first gradient late runs at its own step)"""
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder()
    give_grads(enc, fp)
    head = {id(p) for n, p in enc.named_parameters() if "mlp_head" in n}
    r = adam_ranges(fp, [dict(params=list(enc.parameters()), lr=1e-3, weight_decay=0.0)], step_of=lambda p: 7 if id(p) in head else 0)
    assert [(x.start, x.end, x.step) for x in r] == [(0, head_span(fp)[1], 8), (head_span(fp)[1], fp.total, 1)]
    r = adam_ranges(fp, [dict(params=list(enc.parameters()), lr=1e-3, weight_decay=0.0)])
    assert [(x.start, x.end, x.step) for x in r] == [(0, fp.total, 1)]   # one group, equal counters: one range


def test_ranges_report_an_unaligned_boundary():
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder(num_classes=7)
    give_grads(enc, fp)
    r = adam_ranges(fp, two_groups(enc))
    hi = head_span(fp)[1]
    assert hi == 96 * 2 + 7 * 96 + 7 and hi % 4 == 3
    assert [x.aligned for x in r] == [False, False] and r[0].end == r[1].start == hi
    enc8, fp8 = encoder(num_classes=8)
    give_grads(enc8, fp8)
    assert all(x.aligned for x in adam_ranges(fp8, two_groups(enc8))[:1])


def test_ranges_over_the_cap_and_foreign_gradients_raise():
    from maskedsst_amd import _lib
    from maskedsst_amd.optim import adam_ranges
    enc, fp = encoder(depth=6)
    for i, p in enumerate(enc.parameters()):   # every other tensor frozen: one range per surviving tensor
        p.requires_grad_(i % 2 == 0)
    give_grads(enc, fp)
    with pytest.raises(ValueError, match="ranges"):
        adam_ranges(fp, two_groups(enc), max_ranges=_lib.ADAM_MAX_GROUPS)
    enc, fp = encoder()
    give_grads(enc, fp)
    p = next(enc.parameters())
    p.grad = p.grad.clone()   # e.g. a hook that replaced the gradient: the flat buffer no longer holds it
    with pytest.raises(RuntimeError, match="no view of the flat gradient buffer"):
        adam_ranges(fp, two_groups(enc))


def test_finetune_parser_flags_and_defaults():
    import finetune
    ap = finetune.build_parser()
    d = ap.parse_args([])
    assert d.optimizer == "torch" and d.linear_eval is None   # None: the config's linear_eval key decides, as before
    a = ap.parse_args(["enmap", "--linear-eval", "--optimizer", "fused"])
    assert a.linear_eval is True and a.optimizer == "fused"
    with pytest.raises(SystemExit):
        ap.parse_args(["--optimizer", "sgd"])
    # the optimizer the flags select: torch.optim.Adam over body + head by default, the head alone under linear evaluation
    enc, _ = encoder()
    cfg = finetune.Dotdict(dict(linear_eval=False, lr=5e-4, mlp_head_lr=5e-3, weight_decay=5e-3))
    opt = finetune.make_optimizer(enc, cfg, "torch")
    assert type(opt) is torch.optim.Adam and [g["lr"] for g in opt.param_groups] == [5e-4, 5e-3]
    assert all(g["weight_decay"] == 5e-3 for g in opt.param_groups)
    cfg.linear_eval = True
    opt = finetune.make_optimizer(enc, cfg, "torch")
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 4
    from maskedsst_amd.optim import FusedAdam
    opt = finetune.make_optimizer(enc, cfg, "fused")
    assert isinstance(opt, FusedAdam) and len(opt.param_groups[0]["params"]) == 4 and not opt.decoupled

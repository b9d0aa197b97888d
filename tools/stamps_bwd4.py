"""kernel study: cycle stamps of all eight waves of one workgroup of block_bwd_attn_r4 (msst_bwd4.hip), one mid-walk tile,
spatial and spectral block.  needs a stamps build first:  python -m maskedsst_amd.build --stamps"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from util import build_product

cfg = dict(bands=200, depth=1, B=256)
model, params, x = build_product(cfg, precision="bf16", device="cuda")
eng = model.engine()
masks = model.draw_masks(cfg["B"])
drop = (0.1, 5)
out = eng.simmim_forward_stages(x.cuda(), masks[0], masks[1], drop=drop)
torch.cuda.synchronize(); print("forward done", flush=True)
dy = torch.randn_like(out["enc_out"]) * 1e-3
buf = torch.zeros(512, dtype=torch.int64, device="cuda")
assert eng.lib.msst_debug_stamps(ctypes.c_void_p(buf.data_ptr())) == 0, "build with --stamps"
names = ["P1", "B1", "P2", "B2", "P3", "B3", "P4", "B4", "out"]
acts, x1s = out["acts"], out["x1s"]
other = torch.empty_like(dy)
for i in (0, 1):
    sname, l = eng._layers()[i]
    os.environ["MSST_DBG"] = "8"
    for rep in range(2):
        buf.zero_()
        eng.block_bwd_single(i, acts[i], x1s[i], dy, other, drop=drop)
        torch.cuda.synchronize(); print("bwd call done", i, rep, flush=True)
    s = buf.cpu().numpy()
    t0 = min(int(s[16 * w]) for w in range(8))
    for w in range(8):
        st = [int(s[16 * w + k]) for k in range(13)]
        d = [st[k + 1] - st[k] for k in range(8)]
        # sub-phase stamps: 12 = phase 1's MFMAs done, 11 = phase 3's contraction done, 9 = weight-gradient GEMM done, 10 = phase 4's MFMAs done
        sub = f"p1 mfma {st[12] - st[0]} | p3 mfma {st[11] - st[4]} | wgrad {st[9] - st[6]} p4 mfma {(st[10] - st[9]) if st[10] else 0} p4 epi {(st[7] - st[10]) if st[10] else st[7] - st[9]}"
        print(f"{sname} head {'AB'[w >> 2]} wave {'QKVO'[w & 3]}: start {st[0] - t0:6d} total {st[8] - st[0]:6d} | " + " ".join(f"{n}:{v}" for n, v in zip(names, d)) + " || " + sub)
os.environ["MSST_DBG"] = "0"

#!/usr/bin/env python3
"""Gaussian mixture (EM) iteration time (GPU box): the three launches of one iteration of maskedsst_amd.fit_mixture -- msst_gauss_score
(the scores), msst_gmm_moments (the responsibility-weighted moments) and msst_gmm_update (the per-component M-step with its Cholesky
factorisation) -- apart and together, against an eager restatement on the same bank.

Per shape -- M rows [M, 96] of a planted mixture around 50, K components, full or diag:
  hip     score_us, moments_us, update_us: each launch alone; iter_us: the three queued back to back (one EM iteration).
  eager   one iteration in torch: per component z = (x - mu_c) @ A_c.T and its squared norm, torch.logsumexp, the responsibilities,
          N, the means, the weighted covariance as a batched einsum over row chunks (every [K, chunk, 96] intermediate under 1 GiB),
          torch.linalg.cholesky and torch.linalg.solve_triangular for A = L^-1.  diag: the same with the off-diagonal entries zeroed.
  naive   moments_over_feat: moments_us over K launches of msst_feat_moments on the same rows (feat_moments_us, measured here) --
          the cost of K unweighted passes, the yardstick of the moments launch.
Both sides are warmed up, then timed alternately in one process between device events (the device time of the queued launches, as
in tools/gauss_time.py); the medians of --runs runs are reported.  No speed bar hangs on this tool; every shape is reported, the ones
eager wins included.  Prints ONE JSON line per shape and appends it to --append (default profiles/gmm_measured.jsonl; '' to skip).
--smoke: the smallest shape alone, two runs, nothing appended.

Run:  python tools/gmm_time.py [--rows 8192,262144] [--components 4,16] [--runs 20]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from maskedsst_amd import fit_mixture  # noqa: E402
from maskedsst_amd.gaussian import gauss_score  # noqa: E402
from maskedsst_amd.mixture import gmm_moments, gmm_scratch_floats, gmm_update  # noqa: E402
from maskedsst_amd.pca import feature_moments  # noqa: E402

SEED = 5
REPEAT = 4      # calls queued between two events
LOG_2PI_HALF_DIM = 48.0 * math.log(2.0 * math.pi)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEAT):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPEAT


def alternate(fns, runs, warmup):
    """the medians, in microseconds, of the given calls timed in turn"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    t = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            t[i].append(event_ms(fn))
    return [1e3 * statistics.median(v) for v in t]


def planted(M, K, gen):
    """M rows of K Gaussians around 50: one random rotation per component, a spectrum exp(-j / 24)"""
    lam = torch.exp(-torch.arange(96) / 24.0)
    means = 50.0 + 0.3 * torch.randn(K, 96, generator=gen)
    which = torch.randint(0, K, (M,), generator=gen)
    x = torch.empty(M, 96)
    for c in range(K):
        q = torch.linalg.qr(torch.randn(96, 96, generator=gen))[0]
        sel = which == c
        x[sel] = means[c] + (torch.randn(int(sel.sum()), 96, generator=gen) * lam) @ q.t()
    return x.contiguous()


def eager_iteration(x, state, diag, reg_covar, chunk):
    """one EM iteration in torch from state (weights, means, tables, logdet): the new (weights, means, covariances, tables, logdet)"""
    K = state["means"].shape[0]
    M = x.shape[0]
    N = torch.zeros(K, device=x.device)
    s1 = torch.zeros(K, 96, device=x.device)
    s2 = torch.zeros(K, 96, 96, device=x.device)
    const = state["weights"].log() - 0.5 * state["logdet"] - LOG_2PI_HALF_DIM
    for r0 in range(0, M, chunk):
        d = x[r0:r0 + chunk][None] - state["means"][:, None]                  # [K, chunk, 96]
        z = torch.bmm(d, state["tables"].transpose(1, 2))
        s = const[:, None] - 0.5 * z.square().sum(2)                          # [K, chunk]
        r = (s - torch.logsumexp(s, dim=0, keepdim=True)).exp()
        N += r.sum(1)
        rd = r[:, :, None] * d
        s1 += rd.sum(1)
        s2 = torch.baddbmm(s2, rd.transpose(1, 2), d)
    delta = s1 / N[:, None]
    cov = s2 / N[:, None, None] - torch.einsum("ki,kj->kij", delta, delta) + reg_covar * torch.eye(96, device=x.device)
    if diag:
        cov = torch.diag_embed(torch.diagonal(cov, dim1=1, dim2=2))
    L = torch.linalg.cholesky(cov)
    A = torch.linalg.solve_triangular(L, torch.eye(96, device=x.device).expand(K, 96, 96), upper=False)
    logdet = 2.0 * torch.diagonal(L, dim1=1, dim2=2).log().sum(1)
    return N / N.sum(), state["means"] + delta, cov, A, logdet


def shape_row(M, K, covariance, args, gen, device):
    x = planted(M, K, gen).to(device)
    gm = fit_mixture(x, K, covariance=covariance, iters=2, reg_covar=args.reg_covar, seed=0)
    state = {n: getattr(gm, n).clone() for n in ("weights", "means", "covariances", "tables", "logdet", "consts")}
    offsets = torch.zeros(K, 96, device=device)
    slab = torch.empty(gmm_scratch_floats(M, K), device=device)
    rec = torch.zeros(4, device=device)

    def score():
        return gauss_score(x, state["means"], state["tables"], range(K), offsets, state["consts"], scores=True)[2]

    scores = score()
    scratch = {n: v.clone() for n, v in state.items()}                          # the update alone writes here, so the inputs stay put

    def update():
        gmm_update(slab, M, scratch, covariance, args.reg_covar, 1.0, rec)

    def iteration():
        gmm_moments(x, score(), state["means"], slab)
        update()

    # (the moments of a slab of a finished iteration: every launch below reads the same inputs in every run)
    chunk = max(1024, min(M, (1 << 27) // (K * 96)))                            # [K, chunk, 96] floats: half a GiB
    names = ("score_us", "moments_us", "update_us", "iter_us", "eager_us", "feat_moments_us")
    fns = (score, lambda: gmm_moments(x, scores, state["means"], slab), update, iteration,
           lambda: eager_iteration(x, state, covariance == "diag", args.reg_covar, chunk), lambda: feature_moments(x, state["means"][0]))
    t = dict(zip(names, (round(v, 2) for v in alternate(fns, args.runs, args.warmup))))
    w, mu, cov, A, logdet = eager_iteration(x, state, covariance == "diag", args.reg_covar, chunk)
    scratch["means"].copy_(state["means"])
    iteration()
    agree = float((scratch["covariances"] - cov).abs().max() / cov.abs().max())
    return dict(tool="gmm_time", M=M, K=K, covariance=covariance, runs=args.runs, **t,
                moments_over_feat=round(t["moments_us"] / (K * t["feat_moments_us"]), 2), slab_mib=round(slab.numel() * 4 / 2 ** 20, 1),
                covariances_agree=agree, eager_faster=bool(t["eager_us"] < t["iter_us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,262144", help="comma separated row counts M")
    ap.add_argument("--components", default="4,16", help="comma separated component counts K")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reg-covar", type=float, default=1e-6)
    ap.add_argument("--append", default=os.path.join(ROOT, "profiles", "gmm_measured.jsonl"))
    ap.add_argument("--smoke", action="store_true", help="the smallest shape alone (full covariances), two runs, nothing appended")
    args = ap.parse_args()
    kinds = ("full", "diag")
    if args.smoke:
        args.rows, args.components, args.runs, args.warmup, args.append, kinds = "8192", "4", 2, 1, "", ("full",)
    device = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    for M in (int(v) for v in args.rows.split(",")):
        for K in (int(v) for v in args.components.split(",")):
            for covariance in kinds:
                line = json.dumps(shape_row(M, K, covariance, args, gen, device))
                print(line, flush=True)
                if args.append:
                    os.makedirs(os.path.dirname(os.path.abspath(args.append)), exist_ok=True)
                    with open(args.append, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()

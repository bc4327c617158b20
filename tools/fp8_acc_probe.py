#!/usr/bin/env python3
"""Accumulation error of the e4m3 GEMM (x2i_gemm_fp8 with unit scales, no bias, bf16 output) against the exact float64 sum, over kernel forms,
shapes and operand variants: worst (|err| - 1/2 ulp_bf16)+ / sum_k |a w| per launch and per 256^2 tile, and relative to max |a| max |w| of
the element's row and column.  The numbers next to tests/fp8_ref.py: U_ACC8 come from here (profiles/fp8_acc_probe.log); run on the GPU box."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fp8_ref as R, gemm_ref as G  # noqa: E402
from x2i_amd import ops, _lib  # noqa: E402

DEV = "cuda"
FP8 = torch.float8_e4m3fn
def gen(s): return torch.Generator(device=DEV).manual_seed(s)
def variant(M, N, K, v, g):
    if v in R.KINDS:
        return [t for t in R.operands(M, N, K, v, g, DEV)]
    A = R.random_codes((1, M, K), g, DEV, sprinkle=False); W = R.random_codes((N, K), g, DEV, sprinkle=False)
    if v == "plain": return A, W
    r = torch.rand((1, M, K), generator=g, device=DEV)
    sign = (torch.rand((1, M, K), generator=g, device=DEV) < 0.5).to(torch.uint8) << 7
    if v == "sub": A = torch.where(r < 1 / 64, sign | 3, A)
    if v == "zero": A = torch.where(r < 1 / 64, sign, A)
    if v == "max": A = torch.where(r < 1 / 512, sign | 0x7E, A)
    if v == "small": A = R.random_codes((1, M, K), g, DEV, std=0.25, sprinkle=False)
    if v == "one_big":   # one 448 x 448 product per row, the rest small: error relative to the largest product
        A = R.random_codes((1, M, K), g, DEV, std=1.0, sprinkle=False); W = R.random_codes((N, K), g, DEV, std=1.0, sprinkle=False)
        A[:, :, 5] = 0x7E; W[:, 5] = 0x7E
    return A, W
rows = [("7256 k128", 300, 520, 128, {}), ("7256 k256", 300, 520, 256, {}), ("8256 k384", 300, 520, 384, {}), ("7256 k384", 300, 520, 384, {"gemm_fp8_persist": 0}),
        ("8256 k512", 4136, 3856, 512, {}), ("9256 k2048", 5928, 3856, 2048, {}), ("8256 k2048", 5928, 3856, 2048, {"gemm_streamk": 0})]
for name, M, N, K, o in rows:
    old = {k: _lib.set_option(k, v) for k, v in o.items()}
    for v in ("plain", "sub", "zero", "max", "small", "one_big", "random", "cancel", "tagged"):
        A, W = variant(M, N, K, v, gen(3))
        C = ops.gemm_fp8(A[0].contiguous().view(FP8), W.view(FP8), None)
        form = _lib.get_option("last_gemm_tile")
        torch.cuda.synchronize()
        worst, wmax, per_tile, nbig = 0.0, 0.0, {}, 0
        for r0 in range(0, M, 2048):
            a, w = R.decode(A[0, r0:r0 + 2048]), R.decode(W)
            acc = a @ w.T
            mag = a.abs() @ w.abs().T
            pmax = (a.abs().amax(1)[:, None] * w.abs().amax(1)[None, :])   # >= the largest product of the element
            c = C[r0:r0 + 2048].double()
            over = ((c - acc).abs() - 0.5 * G.ulp_bf16(c)).clamp_min(0)
            ratio = over / mag.clamp_min(2.0 ** -18)
            worst = max(worst, float(ratio.max()))
            wmax = max(wmax, float((over / pmax.clamp_min(2.0 ** -18)).max()))
            nbig += int((ratio > 2.0 ** -20).sum())
            for t0 in range(0, ratio.shape[0], 256):
                for c0 in range(0, N, 256):
                    per_tile[((r0 + t0) // 256, c0 // 256)] = float(ratio[t0:t0 + 256, c0:c0 + 256].max())
        tv = sorted(per_tile.values())
        print(f"{name} form {form} {v:8s}: worst/mag {worst:.3e} (2^{torch.log2(torch.tensor(max(worst, 1e-30))).item():.1f}) worst/(amax_a amax_w) {wmax:.3e} "
              f"elements over 2^-20: {nbig}/{M * N}; per tile min {tv[0]:.2e} median {tv[len(tv) // 2]:.2e} max {tv[-1]:.2e}", flush=True)
    for k, v_ in old.items(): _lib.set_option(k, v_)
ops.streamk_check(sync=True)

"""Same launches from two builds of the library: the A/B of a change to csrc/gemm.hip that must not change what is launched.

    X2I_LIB_VARIANT=<name> python tools/gemm_launcher_ab.py --replay OUT.json     # libx2i_hip_<name>.so; without the variable: libx2i_hip.so
    python tools/gemm_launcher_ab.py --compare A.json B.json                      # every launch: same form (last_gemm_tile), same output hashes
    python tools/gemm_launcher_ab.py --compare-traces A_kernel_trace.csv B_kernel_trace.csv
    X2I_LIB_VARIANT=<name> python tools/gemm_launcher_ab.py --eager 2000          # host time per launch of a launch-bound eager loop

--replay runs one fixed, seeded launch list in this process and records, per launch, last_gemm_tile and a hash of every output: the forty GEMM
launches of the model (one double + one single block at full width, prepare_conditioning + denoise, in the four configurations of
tests/test_gemm_fp64_gpu.py), the convolutions of tests/test_conv_w4_gpu.py (plain, ReLU + per-batch bias, residual, moments; gemm_min256 = 1
as there) and the e4m3 shapes and epilogues of tests/test_fp8_gpu.py.  Under `rocprofv3 --kernel-trace ... -- python tools/gemm_launcher_ab.py
--replay ...` the same run gives the kernel trace that --compare-traces reads: kernel name, grid, workgroup and LDS bytes, launch by launch.
One build per process: start a fresh process for the other one."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"b1_512": (1, 512), "b1_1024": (1, 1024), "b4_1024": (4, 1024), "b2_1008": (2, 1008)}
CONVS = [(256, 256, 3, 3, 1, 1, 64, 64, 2), (128, 256, 3, 3, 1, 1, 48, 80, 3), (512, 512, 3, 3, 1, 1, 32, 40, 2), (256, 320, 3, 3, 1, 1, 40, 40, 2),
         (128, 256, 3, 3, 2, 1, 96, 96, 2), (128, 256, 5, 5, 2, 2, 96, 64, 2), (256, 3072, 2, 2, 2, 0, 64, 64, 1), (64, 256, 3, 3, 1, 1, 40, 56, 2),
         (128, 128, 3, 3, 1, 1, 64, 64, 2), (256, 128, 3, 3, 1, 1, 48, 80, 2), (128, 128, 5, 5, 2, 2, 128, 96, 2), (128, 128, 3, 3, 2, 1, 128, 128, 1),
         (256, 128, 1, 1, 1, 0, 64, 64, 2), (64, 128, 3, 3, 1, 1, 72, 64, 2), (128, 96, 3, 3, 1, 1, 64, 48, 2)]
FP8_SHAPES = [(4 * 4608, 3072, 3072), (2 * 4608 + 40, 2048, 1536), (4608, 12288, 3072)]


def tensor_hash(t):
    """position-sensitive 64-bit hash of a tensor's bytes, computed on the device"""
    import torch
    b = t.contiguous().view(torch.uint8).reshape(-1)
    pad = (-b.numel()) % 4
    if pad:
        b = torch.cat((b, b.new_zeros(pad)))
    v = b.view(torch.int32).to(torch.int64)
    w = torch.arange(v.numel(), device=v.device, dtype=torch.int64) % 1000003 + 1
    return [int(v.sum()), int((v * w).sum())]


def replay(path):
    import torch

    from x2i_amd import _lib, ops
    from x2i_amd.flux import FluxTransformer2DModel
    dev = "cuda"
    rows = []

    def row(name, outs):
        rows.append(dict(name=name, tile=int(_lib.get_option("last_gemm_tile")), hashes=[tensor_hash(t) for t in outs]))

    # ---- the model's GEMM launches, each hashed as it returns
    outputs = {"gemm": lambda a, k: [k["out"]] if k.get("out") is not None else [],
               "gemm_pair": lambda a, k: [a[0]["out"], a[1]["out"]],
               "gemm_qkv": lambda a, k: list(a[3:6]),
               "gemm_qkv_pair": lambda a, k: [a[0][n] for n in ("Q", "K", "VT")]}
    orig = {n: getattr(ops, n) for n in outputs}
    label = [""]

    def wrap(n):
        def f(*a, **k):
            r = orig[n](*a, **k)
            row(f"{label[0]} {n}", outputs[n](a, k) or [r])
            return r
        return f
    ST = 512
    model = FluxTransformer2DModel(num_layers=1, num_single_layers=1, device=dev).init_random_(seed=3)
    try:
        for n in outputs:
            setattr(ops, n, wrap(n))
        for cfg, (B, side) in CONFIGS.items():
            label[0] = cfg
            hw = side // 16
            g = torch.Generator().manual_seed(5)
            enc = torch.randn((B, ST, 4096), generator=g).to(dev, torch.bfloat16)
            pooled = torch.randn((B, 768), generator=g).to(dev, torch.bfloat16)
            img_ids = torch.zeros((hw, hw, 3))
            img_ids[..., 1] += torch.arange(hw)[:, None]
            img_ids[..., 2] += torch.arange(hw)[None, :]
            hs = torch.randn((B, hw * hw, 64), generator=g).to(dev, torch.bfloat16)
            state = model.prepare_conditioning(enc, pooled, torch.zeros((ST, 3)).to(dev), img_ids.reshape(-1, 3).to(dev))
            model.denoise(state, hs, torch.full((B,), 0.75, device=dev))
            torch.cuda.synchronize()
    finally:
        for n, f in orig.items():
            setattr(ops, n, f)
    ops.streamk_check(sync=True)
    assert len(rows) == 40, len(rows)
    del model, state

    # ---- convolutions
    def seeded(shape, seed, scale=1.0):
        return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))).to(torch.bfloat16).to(dev)
    _lib.set_option("gemm_min256", 1)
    try:
        for i, (Cin, Cout, KH, KW, s, p, H, W, B) in enumerate(CONVS):
            x, w, b = seeded((B, H, W, Cin), 100 + i), seeded((Cout, KH * KW * Cin), 200 + i, (KH * KW * Cin) ** -0.5), seeded((Cout,), 300 + i)
            OH, OW = (H + 2 * p - KH) // s + 1, (W + 2 * p - KW) // s + 1
            res = seeded((B, OH, OW, Cout), 400 + i)
            b2 = torch.randn((B, Cout), generator=torch.Generator().manual_seed(500 + i)).to(dev)
            for kind, kw in (("plain", {}), ("relu_bias2", dict(act=ops.ACT_RELU, bias2=b2)), ("res", dict(res=res)), ("moments", {}), ("res_moments", dict(res=res))):
                if "moments" in kind and Cout > 2048:      # (the moments serve N <= 2048)
                    continue
                mom = torch.zeros((B, Cout, 2), device=dev) if "moments" in kind else None
                y = ops.conv2d_nhwc(x, w, b, H, W, Cin, Cout, KH, KW, s, p, moments=mom, **kw)
                row(f"conv{i} {kind}", [y] + ([mom] if mom is not None else []))
    finally:
        _lib.set_option("gemm_min256", 128)

    # ---- e4m3 operands
    for M, N, K in FP8_SHAPES:
        g = torch.Generator(device=dev).manual_seed(7)
        A8, sa = ops.quantize_rows_fp8((torch.randn((M, K), device=dev, generator=g) * 1.5).bfloat16())
        W8, sw = ops.quantize_rows_fp8((torch.randn((N, K), device=dev, generator=g) * 0.03).bfloat16())
        b = torch.randn((N,), device=dev, generator=g).bfloat16()
        res = torch.randn((M, N), device=dev, generator=g).bfloat16()
        gate = torch.randn((1, N), device=dev, generator=g)
        row(f"fp8 {M}x{N}x{K} plain", [ops.gemm_fp8(A8, W8, b, a_scale=sa, w_scale=sw)])
        row(f"fp8 {M}x{N}x{K} gelu_bf16", [ops.gemm_fp8(A8, W8, b, a_scale=sa, w_scale=sw, act=ops.ACT_GELU_TANH)])
        row(f"fp8 {M}x{N}x{K} gelu_e4m3", [ops.gemm_fp8(A8, W8, b, a_scale=sa, w_scale=sw, act=ops.ACT_GELU_TANH, out_fp8=True, out_inv_scale=0.75)])
        out = res.clone()
        ops.gemm_fp8(A8, W8, b, out=out, a_scale=sa, w_scale=sw, alpha=1.25, res=out, gate=gate)
        row(f"fp8 {M}x{N}x{K} gated_residual", [out])
    ops.streamk_check(sync=True)
    with open(path, "w") as f:
        json.dump(dict(library=os.path.basename(_lib.LIB_PATH), rows=rows), f, indent=0)
    print(f"{os.path.basename(_lib.LIB_PATH)}: {len(rows)} launches recorded -> {path}")


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = [(x["name"], x["tile"], y["tile"]) for x, y in zip(a["rows"], b["rows"]) if x != y]
    forms = {}
    for x in a["rows"]:
        forms[x["tile"]] = forms.get(x["tile"], 0) + 1
    print(f"{a['library']} vs {b['library']}: {len(a['rows'])} / {len(b['rows'])} launches, {len(bad)} differ (form or output hash); forms {dict(sorted(forms.items()))}")
    for x in bad[:20]:
        print("  DIFFERS:", x)
    return 1 if bad or len(a["rows"]) != len(b["rows"]) else 0


def trace_rows(path):
    with open(path) as f:
        rd = list(csv.DictReader(f))
    rd.sort(key=lambda r: int(r["Dispatch_Id"]))
    keys = ["Kernel_Name"] + sorted(k for k in rd[0] if k.startswith(("Grid_Size", "Workgroup_Size"))) + ["LDS_Block_Size"]
    assert len(keys) >= 4, list(rd[0])
    return [tuple(r[k] for k in keys) for r in rd]


def compare_traces(pa, pb):
    a, b = trace_rows(pa), trace_rows(pb)
    ours = lambda rows: [r for r in rows if "gemm" in r[0] or "conv_moments" in r[0]]
    oa, ob = ours(a), ours(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(oa, ob)) if x != y]
    print(f"kernel traces: {len(a)} / {len(b)} dispatches, {sum(x != y for x, y in zip(a, b))} differ; of the GEMM launcher's kernels {len(oa)} / {len(ob)}, "
          f"{len(bad)} differ in (kernel name, grid, workgroup, LDS bytes)")
    for x in bad[:20]:
        print("  DIFFERS:", x)
    return 1 if bad or len(oa) != len(ob) else 0


def eager(n, reps=7):
    """n back-to-back ops.gemm calls at M = N = 256, K = 192 (four 128^2 tiles: launch-bound), host clock around a final synchronise"""
    import torch

    from x2i_amd import _lib, ops
    A = torch.randn((256, 192), device="cuda").bfloat16()
    W = torch.randn((256, 192), device="cuda").bfloat16()
    out = torch.empty((256, 256), device="cuda", dtype=torch.bfloat16)
    for _ in range(500):
        ops.gemm(A, W, None, out=out)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(n):
            ops.gemm(A, W, None, out=out)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / n * 1e6)
    print(f"{os.path.basename(_lib.LIB_PATH)}: eager loop of {n} gemm launches (form {_lib.get_option('last_gemm_tile')}), us per launch over {reps} repetitions: "
          f"median {statistics.median(us):.3f} min {min(us):.3f} max {max(us):.3f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--replay", metavar="OUT.json")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    ap.add_argument("--compare-traces", nargs=2, metavar="CSV")
    ap.add_argument("--eager", type=int, metavar="N")
    args = ap.parse_args()
    if args.replay:
        replay(args.replay)
    if args.eager:
        eager(args.eager)
    if args.compare:
        sys.exit(compare(*args.compare))
    if args.compare_traces:
        sys.exit(compare_traces(*args.compare_traces))

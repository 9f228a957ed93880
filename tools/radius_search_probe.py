#!/usr/bin/env python3
"""What the search over the alphabet scalar costs on one GPU, timed with HIP events around each call on the
current stream (median / min of --reps calls after a warm-up of every shape):

  * the search (layer.quantize_dense_search / quantize_conv2d_search, per="channel") with K = 4 and K = 8 candidates on
      Dense(4096 -> 512), 1024 samples, ternary;  Dense(4096 -> 4096), 1024 samples, ternary;
      cfg4's first 3 x 3 conv layer (3 -> 32 @ 32 x 32, 5008 images, 3-bit);
  * against K sequential calls of layer.quantize_dense_channels / quantize_conv2d_channels -- one per candidate scalar, what a
    sweep costs without the search -- in the same process, alternating with the search; the conv layer both with the residual
    norms (the drivers' default, and what the search needs) and without them (how the class surface calls it);
  * the two new kernels alone (hip.candidate_kernels, hip.select_candidates); the candidate kernel against (1 + K) * R * C * 4
    bytes at the HBM rate of a float4 copy (6.29 TB/s measured, 8.0 TB/s spec).

The one requirement: the search is not slower than the K sequential calls on any of the three shapes.

    python tools/radius_search_probe.py [--reps 10] [--out profiles/radius_search.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_COPY_TBS = 6.29


def _data(N, m, C, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((N, C)) / np.sqrt(N)).astype(np.float32)
    G = rng.standard_normal((N, m))
    X = np.maximum(G, 0).astype(np.float32)
    Xq = np.maximum(G + 0.1 * rng.standard_normal((N, m)), 0).astype(np.float32)
    return W, X, Xq


def _time_pair(fns, reps):
    """Median / min per function, the functions alternating inside every repetition (other work shares the host)."""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t))) for t in ts]


def _scalars(K):
    return [1.0 + 0.75 * k for k in range(K)]


def gpu(reps):
    import torch
    from quantized_neural_networks_amd import hip, layer
    dev = torch.device("cuda", 0)
    lines = [f"# {torch.cuda.get_device_name(0)}; median (min) of {reps} timed calls after a warm-up, search and sweep alternating; ms"]
    worst = 0.0
    unit = np.linspace(-1, 1, 3)
    for N, m, C in ((4096, 1024, 512), (4096, 1024, 4096)):
        W, X, Xq = (torch.from_numpy(a).to(dev) for a in _data(N, m, C, seed=4))
        for K in (4, 8):
            s = _scalars(K)

            def search():
                layer.quantize_dense_search(W, X, Xq, unit, s, per="channel", overlap=True, kernel_ready=True)

            def sweep():
                for v in s:
                    layer.quantize_dense_channels(W, X, Xq, unit, v, overlap=True, kernel_ready=True)

            (a, amin), (b, bmin) = _time_pair((search, sweep), reps)
            worst = max(worst, a / b)
            lines.append(f"Dense({N}->{C}) m={m} ternary K={K}: search {a:8.3f} ({amin:.3f})   {K} x quantize_dense_channels {b:8.3f} ({bmin:.3f})   "
                         f"search / sweep {a / b:.3f}   search / one call {a / (b / K):.2f}")
            Wk = W
            med = hip.median_abs(Wk.reshape(-1), on_device=True)
            base = hip.column_radii(Wk, 1.0, layer_median=med)[0]
            r, _ = hip.candidate_kernels(Wk, base, s, scale=(0, K * C))
            idx = torch.randint(-1, 3, (N, K * C), device=dev, dtype=torch.int8)
            rho = torch.rand((1, K * C), device=dev, dtype=torch.float64)
            (c, cmin), (d, dmin) = _time_pair((lambda: hip.candidate_kernels(Wk, base, s, scale=(0, K * C)),
                                               lambda: hip.select_candidates(idx, rho, r, unit, K)), reps)
            nbytes = (1 + K) * N * C * 4
            lines.append(f"    candidate_kernels [{N}][{C}] K={K}: {c:8.3f} ({cmin:.3f})  {nbytes / (c / 1e3) / 1e12:.2f} TB/s of (1 + K) R C 4 bytes = "
                         f"{100 * nbytes / (c / 1e3) / 1e12 / HBM_COPY_TBS:.0f} % of a float4 copy's {HBM_COPY_TBS} TB/s;   "
                         f"select_candidates (two launches): {d:8.3f} ({dmin:.3f})")
        del W, X, Xq
        torch.cuda.empty_cache()
    # cfg4's first 3 x 3 conv layer (tools/bench_configs.py: 3 -> 32 @ 32 x 32, 5008 images, 3-bit)
    g = torch.Generator(device=dev).manual_seed(2)
    act_w = torch.rand((5008, 32, 32, 3), device=dev, generator=g)
    act_q = torch.relu(act_w + 0.05 * torch.randn((5008, 32, 32, 3), device=dev, generator=g))
    Wc = torch.randn((3, 3, 3, 32), device=dev, generator=g) / 3
    unit8 = np.linspace(-1, 1, 8)
    conv = ((1, 1), "SAME", (1, 1))
    for K in (4, 8):
        s = _scalars(K)

        def search():
            layer.quantize_conv2d_search(Wc, act_w, act_q, unit8, s, *conv, per="channel")

        def sweep(want_resid):
            for v in s:
                layer.quantize_conv2d_channels(Wc, act_w, act_q, unit8, v, *conv, want_resid=want_resid)

        (a, amin), (b, bmin), (c, cmin) = _time_pair((search, lambda: sweep(True), lambda: sweep(False)), max(3, reps // 2))
        worst = max(worst, a / b)
        lines.append(f"cfg4 conv 3->32 @32x32, 5008 images, 3-bit K={K}: search {a:8.3f} ({amin:.3f})   {K} x quantize_conv2d_channels {b:8.3f} "
                     f"({bmin:.3f})   search / sweep {a / b:.3f}   [{K} x the same without residual norms, as the class surface calls it: "
                     f"{c:8.3f} ({cmin:.3f}); search / that {a / c:.2f}]")
    lines.append(f"# requirement (search not slower than the K sequential calls on any shape): worst search / sweep = {worst:.3f} -> "
                 f"{'met' if worst <= 1.0 else 'NOT met'}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    text = "\n".join(gpu(args.reps)) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

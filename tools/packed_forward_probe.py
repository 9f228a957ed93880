"""Measures a Dense layer run four ways at small batches -> profiles/packed_forward_tiled.txt
(profiles/packed_forward.txt is the record of the first three, taken before the fourth existed):

    packed    gpfq_packed_dense_forward on the packed rows
    float     x @ Q on the float32 kernel (torch.matmul)
    decode    gpfq_unpack_kernel + torch.matmul
    tiled     gpfq_packed_dense_forward_tiled on the packed rows
    i8        (--i8 only) gpfq_quantize_rows_i8 + gpfq_packed_dense_forward_i8 on the packed rows, timed together
              -> profiles/packed_forward_i8.txt, batches up to 1024; no routing constant follows from it

Shapes 4096 x 4096 (ternary, 16 levels) and 25088 x 4096 (ternary), and 4096 x 1000 (ternary) for what a layer of few column tiles
costs the tiled kernel (63 workgroups on 256 compute units); batches 1 .. 256.  Every figure is device time per call: the call is
captured `--chain` times into a graph (a launch from Python costs more host time than these kernels run), the graph is replayed, the
replays are timed with device events and the four ways alternate; median (min) over the replays.  Two cache states: "same" -- every
call reads the same weights (what a repeated loop sees: a 64 MB float kernel stays in the 256 MiB last-level cache) -- and "rotated"
-- the calls of a chain walk over copies of the layer that together exceed that cache in float32 (what a network of many layers
sees).

The switch-over constant keras_shim.PACKED_FORWARD_MAX_BATCH follows from the "same" table, the state that favours the float kernel:
the largest measured batch at which the packed kernel beat both other ways on both 4096 x 4096 shapes (1 if there is none).
keras_shim.PACKED_TILED_MAX_BATCH follows from the same table: the largest probed batch such that at it, and at every smaller probed
batch above 4, the tiled kernel's median is at most 0.95 of decode + matmul's -- the only other way a layer that holds no float kernel
has -- on both 4096 x 4096 shapes (4 if there is none: nothing is routed).

Also the file sizes of a VGG16-shaped Dense stack written by save_model and by export_packed.

    python tools/packed_forward_probe.py [--out profiles/packed_forward_tiled.txt] [--quick]
    python tools/packed_forward_probe.py --i8 --out profiles/packed_forward_i8.txt

--pairs: the chain mode of DESIGN.md section 11c (tools/packed_chain_pairs.py; `--chain` is taken: it counts the calls captured into
one graph) -> the Dense part of profiles/packed_chain.txt.  VGG16's fc1 -> fc2 -> predictions as one network, loaded with fuse=False
and fuse=True and timed in alternation at 1, 8, 32 and 256 rows; the unfused network, captured twice, is the yardstick.

    python tools/packed_forward_probe.py --pairs --out chain_dense.txt

--i8-only: the fifth way alone, with hip.quantize_rows_i8 choosing its form (the row kernel, or from hip.QUANTIZE_SPLIT_MIN_N columns on
the split form), the same shapes, batches and cache states.  --tree PATH: take the package (and its built library) from another
checkout of this repository, e.g. the parent commit built in a scratch worktree; the two together, alternating between two trees, are
the Dense table of profiles/packed_conv_i8_split.txt.

    python tools/packed_forward_probe.py --i8-only [--tree ../parent] --out dense.txt
"""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch


def _tree():
    """--tree PATH, read before the package is imported."""
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if a.startswith("--tree="):
            return os.path.abspath(a[len("--tree="):])
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


sys.path.insert(0, _tree())
from quantized_neural_networks_amd import deploy, hip, keras_shim as ks  # noqa: E402

BATCHES = (1, 2, 4, 5, 8, 16, 32, 64, 128, 256)
I8_BATCHES = BATCHES + (512, 1024)                  # --i8: the batch sizes a network is evaluated at
TILED_MARGIN = 0.95                                 # tiled / (decode + matmul) at or below this: the tiled kernel is routed


def on_alphabet(rng, N, C, M, dev):
    """A random kernel on the alphabet radius * linspace(-1, 1, M), one radius per channel, built on the device."""
    unit = np.linspace(-1, 1, M)
    radii = torch.from_numpy(rng.uniform(0.5, 1.5, C)).to(dev)
    idx = torch.randint(0, M, (N, C), device=dev, dtype=torch.int8)
    Q, _ = hip.assemble_kernel_colrad(idx, unit, radii, layout=hip.GPFQ_LAYOUT_KERAS)
    return unit, radii, Q


def timed(graphs, replays):
    """Median and minimum device time (ms) of one replay of each graph, the graphs alternating."""
    times = [[] for _ in graphs]
    for _ in range(replays):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def capture(fn, chain):
    for i in range(3):
        fn(i)                                           # warm up outside the capture (code objects, LDS limits, library heuristics)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(chain):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    return g


def measure_i8_only(label, N, C, M, args, dev, out):
    """quantize + i8 alone: median (min .. max) per batch and cache state."""
    rng = np.random.default_rng(N + M)
    copies_rot = max(2, -(-(512 << 20) // (N * C * 4)))
    layers = []
    for _ in range(copies_rot):
        unit, radii, Q = on_alphabet(rng, N, C, M, dev)
        layers.append(deploy.pack_kernel(Q, radii, unit))
        del Q
    out(f"{label}: N={N} C={C} M={M}; rotated = {copies_rot} copies; quantize+i8 us per call, median (min .. max)")
    for B in I8_BATCHES:
        x = torch.randn((B, N), device=dev)
        y = torch.empty((B, C), device=dev)
        xq = (torch.empty((B, (N + 15) // 16 * 16), dtype=torch.int8, device=dev), torch.empty(B, device=dev))
        cells = []
        for ncopies in (1, copies_rot):
            def f_i8(i):
                p = layers[i % ncopies]
                hip.quantize_rows_i8(x, out=xq)
                hip.packed_dense_forward_i8(xq[0], p["codes"], p["bits"], p["zero_code"], p["radii"], M, N, out=y, scales=xq[1])

            g = capture(f_i8, args.chain)
            t = []
            for _ in range(args.replays):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                g.replay()
                b.record()
                b.synchronize()
                t.append(1e3 * a.elapsed_time(b) / args.chain)
            cells.append(f"{np.median(t):8.2f} ({np.min(t):7.2f} ..{np.max(t):8.2f})")
            del g
        out(f"    B {B:5d}   same {cells[0]}   rotated {cells[1]}")


def measure(label, N, C, M, args, dev, out):
    rng = np.random.default_rng(N + M)
    copies_rot = max(2, -(-(512 << 20) // (N * C * 4)))
    layers = []
    for _ in range(copies_rot):
        unit, radii, Q = on_alphabet(rng, N, C, M, dev)
        layers.append((deploy.pack_kernel(Q, radii, unit), Q))
    p0 = layers[0][0]
    out(f"{label}: N={N} C={C} M={M}: {p0['bits']}-bit codes, {p0['codes'].numel() / 1e6:.1f} MB packed against "
        f"{N * C * 4 / 1e6:.1f} MB float32; rotated = {copies_rot} copies")
    wins, tiled = {}, {}
    for state, ncopies in (("same", 1), ("rotated", copies_rot)):
        out(f"  weights {state}; us per call, median (min):   B    packed          float           decode+matmul   tiled           "
            f"packed/float  packed/decode  tiled/decode  tiled/packed" + ("   quantize+i8     i8/decode  i8/tiled" if args.i8 else ""))
        for B in (I8_BATCHES if args.i8 else BATCHES):
            x = torch.randn((B, N), device=dev)
            y = [torch.empty((B, C), device=dev) for _ in range(5 if args.i8 else 4)]
            xq = (torch.empty((B, (N + 15) // 16 * 16), dtype=torch.int8, device=dev), torch.empty(B, device=dev))

            def f_packed(i):
                p = layers[i % ncopies][0]
                hip.packed_dense_forward(x, p["codes"], p["bits"], p["zero_code"], p["radii"], p["alphabet"], N, out=y[0])

            def f_float(i):
                torch.matmul(x, layers[i % ncopies][1], out=y[1])

            def f_decode(i):
                p = layers[i % ncopies][0]
                Qd, _ = hip.unpack_kernel(p["codes"], p["bits"], p["zero_code"], p["radii"], p["alphabet"], N)
                torch.matmul(x, Qd, out=y[2])

            def f_tiled(i):
                p = layers[i % ncopies][0]
                hip.packed_dense_forward_tiled(x, p["codes"], p["bits"], p["zero_code"], p["radii"], p["alphabet"], N, out=y[3])

            def f_i8(i):
                p = layers[i % ncopies][0]
                hip.quantize_rows_i8(x, out=xq)
                hip.packed_dense_forward_i8(xq[0], p["codes"], p["bits"], p["zero_code"], p["radii"], M, N, out=y[4], scales=xq[1])

            graphs = [capture(f, args.chain) for f in (f_packed, f_float, f_decode, f_tiled) + ((f_i8,) if args.i8 else ())]
            res = timed(graphs, args.replays)
            us = [(1e3 * m / args.chain, 1e3 * lo / args.chain) for m, lo in res]
            ref64 = x.double() @ layers[(args.chain - 1) % ncopies][1].double()
            err = [float((t.double() - ref64).abs().max() / ref64.abs().max()) for t in y]
            assert max(err[:4]) < 1e-4, err
            assert not args.i8 or err[4] < 0.05, err            # (int8 activations: the rounding of x, half a step of 1/127 of a row's amax)
            out(f"                                              {B:4d}  {us[0][0]:7.2f} ({us[0][1]:6.2f})  {us[1][0]:7.2f} ({us[1][1]:6.2f})  "
                f"{us[2][0]:7.2f} ({us[2][1]:6.2f})  {us[3][0]:7.2f} ({us[3][1]:6.2f})     {us[0][0] / us[1][0]:5.2f}        "
                f"{us[0][0] / us[2][0]:5.2f}         {us[3][0] / us[2][0]:5.2f}         {us[3][0] / us[0][0]:5.2f}"
                + (f"      {us[4][0]:7.2f} ({us[4][1]:6.2f})    {us[4][0] / us[2][0]:5.2f}     {us[4][0] / us[3][0]:5.2f}" if args.i8 else ""))
            wins[(state, B)] = us[0][0] < us[1][0] and us[0][0] < us[2][0]
            tiled[(state, B)] = us[3][0] <= TILED_MARGIN * us[2][0]
            del graphs
    return wins, tiled


def file_sizes(dev, out):
    """save_model against export_packed for the Dense stack of VGG16 (25088 -> 4096 -> 4096 -> 1000), ternary, put on the alphabet by hand."""
    net = ks.Sequential([ks.Dense(4096, activation="relu", input_shape=(25088,)), ks.Dense(4096, activation="relu"),
                         ks.Dense(1000, activation="softmax")], device=dev)
    rng = np.random.default_rng(0)
    stats = {}
    for k, layer in enumerate(net.layers):
        N, C = layer._weights[0].shape
        unit, radii, Q = on_alphabet(rng, N, C, 3, dev)
        layer.set_weights([Q, layer._weights[1]])
        stats[k] = dict(rad=radii.cpu().numpy())
    quantizer = types.SimpleNamespace(quantized_net=net, alphabet=np.linspace(-1, 1, 3), last_layer_stats=stats,
                                      _will_quantize=lambda k: True)
    with tempfile.TemporaryDirectory() as d:
        ks.save_model(net, os.path.join(d, "float"))
        path = deploy.export_packed(quantizer, os.path.join(d, "packed"))
        a, b = os.path.getsize(os.path.join(d, "float.npz")), os.path.getsize(path)
        back = deploy.load_packed(path, device=dev)
        same = all(torch.equal(l._kernel(), m._weights[0]) for l, m in zip(back.layers, net.layers))
    out(f"VGG16-shaped Dense stack 25088 -> 4096 -> 4096 -> 1000, ternary, one radius per output channel: save_model {a / 1e6:.1f} MB, "
        f"export_packed {b / 1e6:.1f} MB ({a / b:.1f}x smaller); loaded kernels equal: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chain", type=int, default=32, help="calls captured into one graph")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="4096 x 4096 ternary only, no file sizes")
    ap.add_argument("--i8", action="store_true", help="a fifth way: row quantization + the int8 kernel, timed together; batches up to 1024")
    ap.add_argument("--i8-only", action="store_true", help="row quantization + the int8 kernel alone (see the module's text)")
    ap.add_argument("--pairs", action="store_true", help="producer -> consumer links, fuse=False against fuse=True (see the module's text)")
    ap.add_argument("--tree", default=None, help="another checkout of this repository to take the package and its library from")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if (args.i8_only or args.pairs) and args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    if args.pairs:
        import packed_chain_pairs as pairs
        out(f"# {torch.cuda.get_device_name(dev)}; Dense links, device time per predict_on_batch: {args.chain} calls captured into one graph, "
            f"{args.replays} timed replays per graph, three graphs alternating (unfused, fused, unfused again); median (min .. max); us")
        with torch.no_grad():
            pairs.run(pairs.dense_links(), (1, 8, 32, 256), args, dev, out, deploy, hip, ks,
                      members=(3,) if args.quick else (3, 16))
        return
    if args.i8_only:
        out(f"# {torch.cuda.get_device_name(dev)}; device time per call: {args.chain} calls captured into one graph, {args.replays} timed "
            f"replays; package from {'--tree' if args.tree else 'this tree'}")
    else:
        out(f"# {torch.cuda.get_device_name(dev)}; device time per call: {args.chain} calls captured into one graph, {args.replays} timed "
            f"replays per form, the {'five' if args.i8 else 'four'} forms alternating; median (min); us")
    shapes = [("fc 4096 x 4096 ternary", 4096, 4096, 3)]
    if not args.quick:
        shapes += [("fc 4096 x 4096 16 levels", 4096, 4096, 16), ("VGG16 fc1 25088 x 4096 ternary", 25088, 4096, 3),
                   ("fc 4096 x 1000 ternary (63 column tiles)", 4096, 1000, 3)]
    if args.i8_only:
        for s in shapes:
            measure_i8_only(*s, args, dev, out)
        return
    results = [measure(*s, args, dev, out) for s in shapes]
    square, square_tiled = [w for w, _ in results[:2]], [t for _, t in results[:2]]
    both = [B for B in BATCHES if all(w[("same", B)] for w in square)]
    out(f"# switch-over: batches at which the packed kernel beat both other ways on {'both' if len(square) == 2 else 'the'} 4096 x 4096 "
        f"shape{'s' if len(square) == 2 else ''}, weights same: {both or 'none'} -> PACKED_FORWARD_MAX_BATCH = {max(both) if both else 1}")
    routed = 4
    for B in (b for b in BATCHES if b > 4):
        if not all(t[("same", B)] for t in square_tiled):
            break
        routed = B
    out(f"# tiled kernel: the largest probed batch with tiled <= {TILED_MARGIN} x (decode + matmul) at it and at every smaller probed batch "
        f"above 4, on {'both' if len(square) == 2 else 'the'} 4096 x 4096 shape{'s' if len(square) == 2 else ''}, weights same "
        f"-> PACKED_TILED_MAX_BATCH = {routed}")
    if not args.quick:
        file_sizes(dev, out)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""tests/golden/conv_trace.json: what the Conv2D per-channel driver (layer.quantize_conv2d) puts on the GPU queue, which collectives it
enters and what it returns -- per cell of a grid of kernel size x kernel family x flagged pairs x sharding, in one process and over two
and eight gloo ranks -- RECORDED FROM COMMIT d1af445 ("Refinement sweeps on Gram matrices: any row length"), the last one before the
driver was split into a plan, a source of patch matrices and one gather.  tests/test_conv_driver_trace.py recomputes the grid with this
module's functions and compares cell by cell; the golden is never regenerated from the code under test (a deliberate change of the
driver's behaviour records it anew from the commit that makes it, and says so here).

    python tools/gen_conv_trace_golden.py            # writes tests/golden/conv_trace.json

No GPU and no library: public names of the binding and the two collectives of torch.distributed are replaced by a scripted stand-in on
CPU tensors (hip.load itself raises while it is installed); no private helper of layer.py is touched.  The stand-in's model of the
library: the three geometry queries answer what the cell scripts (conv_records_supported per rank, and conv_channel_records can raise on
rank 1), patch_out_dim is restated here (or reports LONG_DIM, the cell whose patch matrices are "long"), and a list of (channel, filter)
pairs comes back flagged from every whole-shard call.

Values are stamps: W[ky][kx][c][f] holds ((ky * kw + kx) * Cin + c) * F + f, every stand-in quantizer answers idx = stamp % M,
Q = alphabet[idx] and resid = the stamp of the row's first weight for the rows it is given (a whole-shard call answers the WRONG member
and residual for the pairs it flags: only their rerun puts them right), pack_indices really packs to 2 / 4 bits and assemble_kernel
unpacks.  run_cell checks the returned kernel against the stamps of W in the Keras layout ("layout" of a trace): that check does not
depend on the recorded file.

Events (in order): channel_planes, extract_patches, the five whole-shard entry points, quantize_conv1x1, quantize_neurons, pack_indices,
assemble_kernel, all_gather_into_tensor and all_reduce, each with the arguments that tell the driver's paths apart.  The queries are not
events."""
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_trace.json")

F = 5
LONG_DIM = 64                                     # what patch_out_dim reports in a "long" cell: 8 images x 64 x 64 columns > GPFQ_GRAM_MIN_M (and > GPFQ_ONCHIP_MAX_M)
SUPPORT = {"planes": (False, False), "nhwc3x3": (True, False), "nhwc": (False, True)}      # (conv3x3_nhwc_supported, conv_channels_nhwc_supported)
FLAGS = {"none": (), "one": ((1, 3),), "three": ((0, 1), (0, 4), (2, 2)), "one_c0": ((0, 3),)}
WHOLE_SHARD = ("quantize_conv_channels", "quantize_conv_channels_nhwc", "quantize_conv3x3_nhwc", "conv_channels_from_records")
EVENTS = ("channel_planes", "extract_patches") + WHOLE_SHARD + ("conv_channel_records", "quantize_conv1x1", "quantize_neurons", "pack_indices",
                                                                "assemble_kernel", "all_gather", "all_reduce")


def cell(k=3, Cin=3, n=4, hw=6, M=4, want_resid=False, support="planes", flags="none", same=False, strides=(1, 1), padding="SAME",
         rate=(1, 1), long=False, records=None):
    """records: None (not supported) / "both" / "rank0" (supported on rank 0 only) / "raise1" (supported; conv_channel_records raises on rank 1)."""
    return dict(k=k, Cin=Cin, n=n, hw=hw, M=M, want_resid=want_resid, support=support, flags=flags, same=same, strides=strides,
                padding=padding, rate=rate, long=long, records=records)


def one_process_cells():
    yield "k1/noresid", cell(k=1)
    yield "k1/resid", cell(k=1, want_resid=True)
    for support in SUPPORT:
        for flags in ("none", "one", "three"):
            yield f"k3/{support}/{flags}", cell(support=support, flags=flags)
    yield "k3/resid/loop", cell(want_resid=True)
    yield "k3/resid/long", cell(want_resid=True, n=8, long=True, flags="one")
    yield "k9/loop", cell(k=9, n=1, hw=12, padding="valid")
    yield "k3/same_act", cell(same=True, flags="one")
    yield "k3/int16", cell(M=200, flags="one")
    yield "k3/rate_none", cell(rate=None, strides=(2, 2), padding="VALID")


def sharded_cells():
    """The cells of the two- and the eight-rank grid: 8 images, so that the record cells have an image for every rank."""
    for support in ("planes", "nhwc3x3"):
        yield f"cin3/{support}/noresid", cell(n=8, support=support, flags="one")
        yield f"cin3/{support}/resid", cell(n=8, support=support, want_resid=True)
    yield "cin3/int16", cell(n=8, M=200, flags="one")
    yield "cin1/records", cell(n=8, Cin=1, records="both", flags="one_c0")
    yield "cin1/records_one_rank", cell(n=8, Cin=1, records="rank0", flags="one_c0")
    yield "cin1/records_raise", cell(n=8, Cin=1, records="raise1", flags="one_c0")
    yield "cin1/resid", cell(n=8, Cin=1, records="both", want_resid=True)


def stamps(k, Cin):
    """W f32 [k][k][Cin][F] whose every weight holds its own coordinates."""
    return torch.arange(k * k * Cin * F, dtype=torch.float32).reshape(k, k, Cin, F)


def alphabet_of(M):
    return 0.25 * np.linspace(-1, 1, M)


def _bits(M):
    return 2 if M <= 4 else 4 if M <= 16 else 8 if M <= 64 else 16


class StandIn:
    """The scripted binding.  install() swaps it in, restore() puts the originals back."""

    def __init__(self, spec, rank=0):
        from quantized_neural_networks_amd import hip
        self.hip = hip
        self.spec, self.rank = spec, rank
        self.Cin, self.M = spec["Cin"], spec["M"]
        self.flags = FLAGS[spec["flags"]]
        self.events = []
        self.planes = []                          # what channel_planes returned (kept: extract_patches tells a plane by its storage)
        self.kept = None

    # ---- the model ----
    def _members(self, alphabet):
        assert len(alphabet) == self.M
        return torch.tensor(np.asarray(alphabet, dtype=np.float64))

    def _walk(self, Wt, alphabet, wrong=None):
        """(idx, Q, resid) of rows Wt [..., K] of stamps; `wrong` (bool [...]) marks the rows that take the next member instead."""
        s = Wt.long()
        if wrong is not None:
            s = s + wrong.long().unsqueeze(-1)
        idx = (s % self.M).to(self.hip.index_dtype(self.M))
        resid = Wt[..., 0].double()
        if wrong is not None:
            resid = torch.where(wrong, torch.full_like(resid, -1.0), resid)
        return idx, self._members(alphabet)[idx.long()].float(), resid

    def _flagged(self, Wt):
        """bool [nch][F']: the scripted pairs among the rows of Wt [nch][F'][K], told by their stamps."""
        s0 = Wt[..., 0].long()
        c, f = (s0 // F) % self.Cin, s0 % F
        unc = torch.zeros(s0.shape, dtype=torch.bool)
        for fc, ff in self.flags:
            unc |= (c == fc) & (f == ff)
        return unc

    def _whole_shard(self, name, act_w, act_q, Wt, alphabet, idx, Q, resid, unc, c=None):
        for t in (act_w, act_q, Wt, idx, Q, unc) + (() if resid is None else (resid,)):
            assert t.is_contiguous(), f"{name} needs contiguous tensors"
        assert idx.dtype == self.hip.index_dtype(self.M) and Q.dtype == torch.float32 and unc.dtype == torch.int32
        assert tuple(idx.shape) == tuple(Q.shape) == tuple(Wt.shape) and tuple(unc.shape) == tuple(Wt.shape[:2])
        self.events.append(dict(ev=name, Wt=list(Wt.shape), idx=list(idx.shape), unc=list(unc.shape), c=None if c is None else list(c),
                                resid=resid is not None, same=act_q is act_w, nimg=act_w.shape[1 if c is None else 0]))
        flagged = self._flagged(Wt)
        i, q, r = self._walk(Wt, alphabet, wrong=flagged)
        idx.copy_(i)
        Q.copy_(q)
        unc.copy_(flagged.int())
        if resid is not None:
            assert resid.dtype == torch.float64 and tuple(resid.shape) == tuple(unc.shape)
            resid.copy_(r)

    # ---- queries: not events ----
    def load(self):
        raise AssertionError("the conv driver's trace runs without the library: a call reached hip.load()")

    def conv3x3_nhwc_supported(self, n, H, W, nch):
        return SUPPORT[self.spec["support"]][0]

    def conv_channels_nhwc_supported(self, n, H, W, nch, kernel_size, strides, rate, padding):
        return SUPPORT[self.spec["support"]][1]

    def conv_records_supported(self, n, H, W, nch, kernel_size, strides, rate, padding):
        return self.spec["records"] in ("both", "raise1") or (self.spec["records"] == "rank0" and self.rank == 0)

    def patch_out_dim(self, size, k, stride, rate, same):
        if self.spec["long"]:
            return LONG_DIM
        return -(-size // stride) if same else max((size - (k - 1) * rate - 1) // stride + 1, 0)

    # ---- what reaches the queue ----
    def channel_planes(self, act, c_lo, c_hi):
        assert act.is_contiguous()
        self.events.append(dict(ev="channel_planes", c=[c_lo, c_hi], nimg=act.shape[0]))
        self.planes.append(act[..., c_lo:c_hi].permute(3, 0, 1, 2).clone(memory_format=torch.contiguous_format))     # (always a storage of its own)
        return self.planes[-1]

    def extract_patches(self, act, channel, kernel_size, strides, rate, padding, out=None):
        assert act.dim() == 4 and act.is_contiguous()
        store = act.untyped_storage().data_ptr()
        plane = any(p.numel() and p.untyped_storage().data_ptr() == store for p in self.planes)
        self.events.append(dict(ev="extract_patches", channel=channel, channels=act.shape[3], src="plane" if plane else "nhwc",
                                reuses_out=out is not None))
        if out is not None:
            return out
        rh, rw = rate if rate else (1, 1)
        same = str(padding).upper() == "SAME"
        cols = (act.shape[0] * self.patch_out_dim(act.shape[1], kernel_size[0], strides[0], rh, same)
                * self.patch_out_dim(act.shape[2], kernel_size[1], strides[1], rw, same))
        return torch.zeros((kernel_size[0] * kernel_size[1], cols), dtype=torch.float32)

    def quantize_conv_channels(self, act_w_cm, act_q_cm, Wt_all, alphabet, kernel_size, strides, rate, padding, idx, Q, resid, unc):
        self._whole_shard("quantize_conv_channels", act_w_cm, act_q_cm, Wt_all, alphabet, idx, Q, resid, unc)

    def quantize_conv_channels_nhwc(self, act_w, act_q, c_lo, c_hi, Wt_all, alphabet, kernel_size, strides, rate, padding, idx, Q, unc):
        self._whole_shard("quantize_conv_channels_nhwc", act_w, act_q, Wt_all, alphabet, idx, Q, None, unc, c=(c_lo, c_hi))

    def quantize_conv3x3_nhwc(self, act_w, act_q, c_lo, c_hi, Wt_all, alphabet, idx, Q, unc):
        self._whole_shard("quantize_conv3x3_nhwc", act_w, act_q, Wt_all, alphabet, idx, Q, None, unc, c=(c_lo, c_hi))

    def conv_channel_records(self, act_w_cm, act_q_cm, kernel_size, strides, rate, padding):
        assert act_w_cm.is_contiguous() and act_q_cm.is_contiguous()
        raises = self.spec["records"] == "raise1" and self.rank == 1
        self.events.append(dict(ev="conv_channel_records", planes=list(act_w_cm.shape), same=act_q_cm is act_w_cm, raises=raises))
        if raises:
            raise self.hip.GpfqError("conv_channel_records: scripted failure")
        nch, K = act_w_cm.shape[0], kernel_size[0] * kernel_size[1]
        return torch.zeros((nch, K * K * 2 + K), dtype=torch.float64), torch.zeros((nch,), dtype=torch.int32)

    def conv_channels_from_records(self, records, negflags, act_w_cm, act_q_cm, Wt_all, alphabet, kernel_size, strides, rate, padding,
                                   idx, Q, unc):
        K = kernel_size[0] * kernel_size[1]
        assert tuple(records.shape) == (act_w_cm.shape[0], K * K * 2 + K) and tuple(negflags.shape) == (act_w_cm.shape[0],)
        self._whole_shard("conv_channels_from_records", act_w_cm, act_q_cm, Wt_all, alphabet, idx, Q, None, unc)

    def quantize_conv1x1(self, act_q, W2, alphabet, strides=(1, 1)):
        assert act_q.is_contiguous() and W2.is_contiguous()
        self.events.append(dict(ev="quantize_conv1x1", W2=list(W2.shape), strides=list(strides)))
        idx, Q, _ = self._walk(W2.unsqueeze(-1), alphabet)
        return Q.squeeze(-1), idx.squeeze(-1)

    def quantize_neurons(self, X, Xq, Wt, alphabet, nrm32=None, want_u=False, path=0, want_values=True, want_resid=True):
        assert Wt.is_contiguous() and X.shape == Xq.shape and X.shape[0] == Wt.shape[1]
        s0 = Wt[:, 0].long()
        self.events.append(dict(ev="quantize_neurons", rows=Wt.shape[0], path=path, same=Xq is X, channels=sorted(set(((s0 // F) % self.Cin).tolist())),
                                filters=(s0 % F).tolist()))
        idx, Q, resid = self._walk(Wt, alphabet)
        return dict(idx=idx, Q=Q, resid=resid, u=None, workspace=None)

    def pack_indices(self, qidx, M):
        assert qidx.dim() == 2 and qidx.is_contiguous() and qidx.dtype == self.hip.index_dtype(M)
        self.events.append(dict(ev="pack_indices", shape=list(qidx.shape)))
        bits = _bits(M)
        if bits >= 8:
            return qidx, bits
        per = 8 // bits
        C, N = qidx.shape
        v = torch.zeros((C, -(-N // per) * per), dtype=torch.int64)
        v[:, :N] = qidx.long()
        shifts = bits * torch.arange(per)
        return (v.reshape(C, v.shape[1] // per, per) << shifts).sum(-1).to(torch.uint8), bits

    def assemble_kernel(self, qidx, alphabet, want_idx=True, bits=None, N=None):
        assert qidx.dim() == 2 and qidx.is_contiguous()
        self.events.append(dict(ev="assemble_kernel", bits=bits, N=N, shape=list(qidx.shape)))
        if bits is None:
            bits = 8 if len(alphabet) <= 64 else 16
        assert qidx.dtype == (torch.int16 if bits == 16 else torch.int8 if bits == 8 else torch.uint8)
        if bits < 8:
            per = 8 // bits
            assert qidx.shape[1] == (N * bits + 7) // 8
            shifts = bits * torch.arange(per)
            qidx = ((qidx.long().unsqueeze(-1) >> shifts) & ((1 << bits) - 1)).reshape(qidx.shape[0], qidx.shape[1] * per)[:, :N]
        idx = qidx.to(self.hip.index_dtype(len(alphabet))).t().contiguous()
        return self._members(alphabet)[idx.long()].float(), idx

    def _all_gather(self, out, inp, group=None):
        self.events.append(dict(ev="all_gather", count=inp.numel(), dtype=str(inp.dtype)))
        return self.kept["all_gather_into_tensor"](out, inp, group=group)

    def _all_reduce(self, t, op=None, group=None):
        self.events.append(dict(ev="all_reduce", op=str(op).split(".")[-1], count=t.numel()))
        return self.kept["all_reduce"](t, op=op, group=group)

    NAMES = ("load", "conv3x3_nhwc_supported", "conv_channels_nhwc_supported", "conv_records_supported", "patch_out_dim", "channel_planes",
             "extract_patches", "quantize_conv_channels", "quantize_conv_channels_nhwc", "quantize_conv3x3_nhwc", "conv_channel_records",
             "conv_channels_from_records", "quantize_conv1x1", "quantize_neurons", "pack_indices", "assemble_kernel")

    def install(self):
        import torch.distributed as dist
        self.kept = {k: getattr(self.hip, k) for k in self.NAMES}
        self.kept["all_gather_into_tensor"], self.kept["all_reduce"] = dist.all_gather_into_tensor, dist.all_reduce
        for k in self.NAMES:
            setattr(self.hip, k, getattr(self, k))
        dist.all_gather_into_tensor, dist.all_reduce = self._all_gather, self._all_reduce
        return self

    def restore(self):
        import torch.distributed as dist
        for k in self.NAMES:
            setattr(self.hip, k, self.kept[k])
        dist.all_gather_into_tensor, dist.all_reduce = self.kept["all_gather_into_tensor"], self.kept["all_reduce"]


def entry_points():
    """(object, attribute) of everything install() replaces: the test checks that each is put back."""
    import torch.distributed as dist
    from quantized_neural_networks_amd import hip
    return [(hip, k) for k in StandIn.NAMES] + [(dist, "all_gather_into_tensor"), (dist, "all_reduce")]


def run_cell(spec, group=None, rank=0):
    """One cell: the trace of one driver call under the stand-in (which is removed again, however the call ends), what it returned,
    and "layout": the returned kernel checked against the stamps of W."""
    from quantized_neural_networks_amd import layer
    s = StandIn(spec, rank).install()
    try:
        k, Cin, M = spec["k"], spec["Cin"], spec["M"]
        W = stamps(k, Cin)
        act_w = torch.rand((spec["n"], spec["hw"], spec["hw"], Cin), generator=torch.Generator().manual_seed(1))
        act_q = act_w if spec["same"] else act_w + 0.5
        alphabet = alphabet_of(M)
        out = layer.quantize_conv2d(W, act_w, act_q, alphabet, spec["strides"], spec["padding"], spec["rate"], group=group,
                                    want_resid=spec["want_resid"])
        want_idx = W.long() % M
        resid, first = out["resid"], W[0, 0].double()
        layout = dict(idx=tuple(out["idx"].shape) == tuple(W.shape) and bool((out["idx"].long() == want_idx).all()),
                      Q=tuple(out["Q"].shape) == tuple(W.shape)
                      and torch.equal(out["Q"], torch.tensor(alphabet, dtype=torch.float64)[out["idx"].long()].float()),
                      resid=tuple(resid.shape) == (Cin, F) and bool((torch.isnan(resid) | (resid == first)).all()),
                      contiguous=all(out[key].is_contiguous() for key in ("Q", "idx", "resid")))
        return dict(events=s.events, keys=sorted(out), dtypes={key: str(out[key].dtype) for key in ("Q", "idx", "resid")},
                    reruns=int(out["reruns"]) if "reruns" in out else None, resid_nan=int(torch.isnan(resid).sum()), layout=layout)
    finally:
        s.restore()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, world, port, result_dir):
    """A rank that left a collective out would leave the others waiting: the group's timeout then fails the run instead of hanging it."""
    import datetime
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    cells = {name: run_cell(spec, group=dist.group.WORLD, rank=rank) for name, spec in sharded_cells()}
    with open(os.path.join(result_dir, f"world{world}_rank{rank}.json"), "w") as f:
        json.dump(cells, f)
    dist.barrier()
    dist.destroy_process_group()


GRIDS = {"two_ranks": 2, "eight_ranks": 8}


def compute(tmp_dir):
    """{"one_process": {cell: trace}, "two_ranks": {cell: {"rank0": trace, "rank1": trace}}, "eight_ranks": {cell: {"rank0": ..}}}"""
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    grid = dict(one_process={name: run_cell(spec) for name, spec in one_process_cells()})
    for gname, world in GRIDS.items():
        mp.spawn(_rank_worker, args=(world, _free_port(), str(tmp_dir)), nprocs=world, join=True)
        ranks = [json.load(open(os.path.join(tmp_dir, f"world{world}_rank{r}.json"))) for r in range(world)]
        grid[gname] = {k: {f"rank{r}": ranks[r][k] for r in range(world)} for k in ranks[0]}
    return json.loads(json.dumps(grid))            # (as the golden file holds it: lists, not tuples)


def main():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        grid = compute(tmp)
    with open(GOLDEN, "w") as f:
        f.write("{\n")
        for gi, (gname, cells) in enumerate(grid.items()):
            f.write(f' "{gname}": {{\n')
            f.write(",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in cells.items()))
            f.write("\n }" + ("," if gi + 1 < len(grid) else "") + "\n")
        f.write("}\n")
    print(f"{GOLDEN}: " + ", ".join(f"{len(cells)} {gname} cells" for gname, cells in grid.items()) + f", {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()

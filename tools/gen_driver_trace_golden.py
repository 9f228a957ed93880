"""tests/golden/driver_trace.json: what the Dense layer drivers of layer.py put on the GPU queue, wait for, log and return -- per cell of
a grid of entry point x kernel family x scripted deferred statuses -- RECORDED FROM COMMIT 96efaf2 ("One options table, one snapshot per
C-ABI call, gpfq_get_option"), the last one before the drivers' repair ladder became one helper.  tests/test_dense_driver_trace.py
recomputes the grid with this module's functions and compares cell by cell; the golden is never regenerated from the code under test
(a deliberate change of the drivers' behaviour records it anew from the commit that makes it, and says so here).

    python tools/gen_driver_trace_golden.py            # writes tests/golden/driver_trace.json

No GPU and no library: the binding's entry points are replaced by a scripted stand-in on CPU tensors (as tests/test_sharding_gloo.py
does).  The stand-in's whole model of the library is three booleans per family -- the block kernel takes the shape with the cluster form
on / it takes it with blk_cluster = 0 / a launch with the cluster form on IS the cluster form -- a dict of options and a list of statuses
that call_status pops (0 when it is empty).  Outputs are zero tensors of the right shapes and dtypes: the trace is compared, not values.

Events (in order): every launch (quantize_dense_layer / quantize_neurons with the family it takes under the blk_cluster in force, and
keras_out / want_values / want_resid / prepared), every call_status (a host wait) with the status it returned, every
DeviceAlphabet.values() read-back (a host wait), neuron_major, pack_indices, both assembly calls, and -- under a process group -- every
all-gather.  Queries (dense_layer_supported, last_dense_kernel, get_option) and set_option calls are not events."""
import json
import os
import socket
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_trace.json")

# family -> (block kernel with the cluster form on, block kernel with blk_cluster = 0, the launch with it on is the cluster form)
FAMILIES = {"classic": (True, True, False), "twin": (True, True, True), "cluster_only": (True, False, True), "no_block": (False, False, False)}
TIMEOUT, ALPHABET = "timeout", "alphabet"
SCRIPTS = {"none": (), "timeout": (TIMEOUT,), "alphabet": (ALPHABET,), "timeout+timeout": (TIMEOUT, TIMEOUT),
           "timeout+alphabet": (TIMEOUT, ALPHABET), "alphabet+timeout": (ALPHABET, TIMEOUT)}
ENTRIES = ("device", "device_radius_ok", "host", "checked")
N, C, M_SAMPLES = 6, 5, 8                         # 5 neurons over 2 ranks: uneven shards
UNIT = np.linspace(-1, 1, 4)


class StandIn:
    """The scripted binding.  install() swaps it in, restore() puts the originals back."""

    def __init__(self, family, statuses=()):
        from quantized_neural_networks_amd import hip
        self.hip = hip
        self.blk_on, self.blk_off, self.cluster = FAMILIES[family]
        self.statuses = [dict(timeout=hip.GPFQ_ERR_CLUSTER_TIMEOUT, alphabet=hip.GPFQ_ERR_ALPHABET)[s] for s in statuses]
        self.options = {"blk_cluster": 1}
        self.events = []
        self.last = "none"
        self.kept = None

    # ---- the model ----
    def _block(self):
        return self.blk_on if self.options["blk_cluster"] else self.blk_off

    def _family(self):
        if not self._block():
            return "other"
        return "cluster" if self.options["blk_cluster"] and self.cluster else "classic"

    def _launch(self, fn, **kw):
        self.last = self._family()
        self.events.append(dict(ev="launch", fn=fn, family=self.last, **kw))

    # ---- queries and options: not events ----
    def dense_layer_supported(self, N, m, C, unit_alphabet):
        return self._block()

    def last_dense_kernel(self):
        return {"cluster": "gpfq_blk_kernel (cluster form)", "classic": "gpfq_blk_kernel", "other": "another family", "none": ""}[self.last]

    def get_option(self, key):
        return self.options[key]

    def set_option(self, key, value):
        self.options[key] = int(value)

    # ---- what reaches the queue or waits for it ----
    def quantize_neurons(self, X, Xq, Wt, alphabet, nrm32=None, want_u=False, path=0, want_values=True, want_resid=True):
        self._launch("quantize_neurons", keras_out=None, want_values=bool(want_values), want_resid=want_resid, prepared=False)
        Cl, Nl = Wt.shape
        return dict(idx=torch.zeros((Cl, Nl), dtype=self.hip.index_dtype(len(alphabet))), Q=torch.zeros((Cl, Nl)) if want_values else None,
                    resid=torch.zeros(Cl, dtype=torch.float64), u=None, workspace=torch.zeros(16, dtype=torch.uint8))

    def quantize_dense_layer(self, X, Xq, W, dalpha, lo=0, hi=None, nrm32=None, keras_out=True, want_values=True, want_idx=True,
                             want_resid=True, prepared=None):
        Nl, Ctot = W.shape
        hi = Ctot if hi is None else hi
        self._launch("quantize_dense_layer", keras_out=bool(keras_out), want_values=bool(want_values), want_resid=want_resid,
                     prepared=prepared is not None)
        shape = (Nl, Ctot) if keras_out else (hi - lo, Nl)
        return dict(idx=torch.zeros(shape, dtype=torch.int8), Q=torch.zeros(shape) if want_values else None,
                    resid=torch.zeros(hi - lo, dtype=torch.float64) if want_resid is not False else None, u=None,
                    workspace=torch.zeros(16, dtype=torch.uint8))

    def call_status(self, result):
        st = self.statuses.pop(0) if self.statuses else 0
        self.events.append(dict(ev="call_status", status=st))
        return st

    def neuron_major(self, W, lo=0, hi=None):
        self.events.append(dict(ev="neuron_major"))
        return W[:, lo:hi].t().contiguous()

    def pack_indices(self, qidx, M):
        self.events.append(dict(ev="pack_indices"))
        return qidx, 8

    def assemble_kernel(self, qidx, alphabet, want_idx=True, bits=None, N=None):
        self.events.append(dict(ev="assemble_kernel"))
        return torch.zeros(qidx.shape[::-1]), qidx.t().contiguous()

    def assemble_kernel_device(self, qidx, dalpha, want_idx=True, bits=8, N=None):
        self.events.append(dict(ev="assemble_kernel_device"))
        return torch.zeros(qidx.shape[::-1]), qidx.t().contiguous()

    def _values(self, dalpha):
        self.events.append(dict(ev="values"))
        return dalpha.rad() * dalpha.unit

    def _all_gather(self, out, inp, group=None):
        self.events.append(dict(ev="all_gather"))
        return self.kept["all_gather_into_tensor"](out, inp, group=group)

    NAMES = ("dense_layer_supported", "last_dense_kernel", "get_option", "set_option", "quantize_neurons", "quantize_dense_layer",
             "call_status", "neuron_major", "pack_indices", "assemble_kernel", "assemble_kernel_device")

    def install(self):
        import torch.distributed as dist
        hip = self.hip
        self.kept = {k: getattr(hip, k) for k in self.NAMES}
        self.kept["values"] = hip.DeviceAlphabet.values
        self.kept["all_gather_into_tensor"] = dist.all_gather_into_tensor
        for k in self.NAMES:
            setattr(hip, k, getattr(self, k))
        standin = self
        hip.DeviceAlphabet.values = lambda dalpha: standin._values(dalpha)
        dist.all_gather_into_tensor = self._all_gather
        return self

    def restore(self):
        import torch.distributed as dist
        for k in self.NAMES:
            setattr(self.hip, k, self.kept[k])
        self.hip.DeviceAlphabet.values = self.kept["values"]
        dist.all_gather_into_tensor = self.kept["all_gather_into_tensor"]


def entry_points():
    """(object, attribute) of everything install() replaces: the test checks that each is put back."""
    import torch.distributed as dist
    from quantized_neural_networks_amd import hip
    return [(hip, k) for k in StandIn.NAMES] + [(hip.DeviceAlphabet, "values"), (dist, "all_gather_into_tensor")]


def _device_alphabet(hip, radius_ok):
    buf = torch.zeros(hip.GPFQ_DEVICE_ALPHABET_BYTES, dtype=torch.uint8)
    buf[:8] = torch.from_numpy(np.array([0.75]).view(np.uint8))
    d = hip.DeviceAlphabet(buf, UNIT, 3.0)
    d.radius_ok = radius_ok
    return d


def run_cell(entry, family, script, check=True, group=None):
    """One cell: the trace of one driver call under the stand-in (which is removed again, however the call ends)."""
    from quantized_neural_networks_amd import hip, layer
    s = StandIn(family, SCRIPTS[script]).install()
    logged, raised, keys = [], False, None
    try:
        W, X, Xq = torch.ones((N, C)), torch.ones((N, M_SAMPLES)), torch.ones((N, M_SAMPLES))
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                if entry == "checked":
                    out = layer.quantize_neurons_checked(X, Xq, W.t().contiguous(), 0.75 * UNIT, log=logged.append, want_values=False)
                elif entry == "host":
                    out = layer.quantize_dense(W, X, Xq, 0.75 * UNIT, group=group, log=logged.append, check=check)
                else:
                    out = layer.quantize_dense(W, X, Xq, _device_alphabet(hip, entry == "device_radius_ok"), group=group, log=logged.append,
                                               check=check)
                keys = sorted(k for k in out if not k.startswith("cluster_"))     # (96efaf2 also returned two cluster_* keys that nothing read)
            except hip.GpfqError:
                raised = True
        return dict(events=s.events, log=logged, warnings=[str(w.message) for w in caught], raised=raised, keys=keys, options=dict(s.options),
                    statuses_left=len(s.statuses))
    finally:
        s.restore()


def one_process_cells():
    for entry in ENTRIES:
        for family in FAMILIES:
            for script in SCRIPTS:
                if ALPHABET in SCRIPTS[script] and not entry.startswith("device"):
                    continue                                       # (no device alphabet in the call: no alphabet status)
                for check in ((True,) if entry == "checked" else (True, False)):     # (quantize_neurons_checked has no `check`)
                    yield entry, family, script, check


def two_rank_cells():
    for entry in ("device", "host"):
        for family in ("classic", "twin", "cluster_only"):
            for script in ("none", "timeout", "alphabet", "timeout+alphabet"):
                if ALPHABET in SCRIPTS[script] and entry != "device":
                    continue
                yield entry, family, script


def _name(*parts):
    return "/".join(str(p) for p in parts)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_worker(rank, port, result_dir):
    """Rank 1 carries each cell's script, rank 0 is healthy.  A GpfqError ahead of the all-gather would leave the other rank waiting: the
    group's timeout then fails the run instead of hanging it."""
    import datetime
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=120))
    cells = {}
    for entry, family, script in two_rank_cells():
        cells[_name(entry, family, script)] = run_cell(entry, family, script if rank == 1 else "none", group=dist.group.WORLD)
    with open(os.path.join(result_dir, f"rank{rank}.json"), "w") as f:
        json.dump(cells, f)
    dist.barrier()
    dist.destroy_process_group()


def compute(tmp_dir):
    """{"one_process": {cell: trace}, "two_ranks": {cell: {"rank0": trace, "rank1": trace}}}"""
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    one = {_name(e, f, s, "check" if c else "nocheck"): run_cell(e, f, s, check=c) for e, f, s, c in one_process_cells()}
    mp.spawn(_rank_worker, args=(_free_port(), str(tmp_dir)), nprocs=2, join=True)
    ranks = [json.load(open(os.path.join(tmp_dir, f"rank{r}.json"))) for r in (0, 1)]
    two = {k: dict(rank0=ranks[0][k], rank1=ranks[1][k]) for k in ranks[0]}
    return json.loads(json.dumps(dict(one_process=one, two_ranks=two)))      # (as the golden file holds it: lists, not tuples)


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
    one = grid["one_process"].values()
    print(f"{GOLDEN}: {len(grid['one_process'])} one-process cells ({sum(c['raised'] for c in one)} raise, {sum(bool(c['log']) for c in one)} log a "
          f"failure, {sum(any(e['ev'] == 'call_status' for e in c['events']) for c in one)} read a status), {len(grid['two_ranks'])} two-rank cells, "
          f"{os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()

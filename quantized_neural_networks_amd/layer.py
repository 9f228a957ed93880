"""Device-side layer drivers: what the reference's ``_quantize_layer_parallel``
(scripts/quantized_network.py:523-574) and ``_quantize_conv2D_layer_parallel_jit`` (:815-867) do
between "activations and weights are available" and "Q is handed to set_weights", on GPU tensors.

Multi-GPU: the independent units -- neurons of a Dense layer, (input-channel, filter)
pairs of a conv layer -- are partitioned contiguously over the ranks of a ``torch.distributed``
process group (one process per GPU, backend "nccl" = RCCL over xGMI).  Every rank holds the full
activation matrices and the full analog kernel, quantizes its shard, and ONE all-gather per layer
reassembles the quantized kernel; there is no other communication.
"""
from collections import namedtuple

import numpy as np
import torch

from . import hip


# ------------------------------------------------------------------------------------------
# alphabet radius
# ------------------------------------------------------------------------------------------
# Below this many weights one GPU selects the median faster than three dependent all-reduces take.  Round 6: the one-GPU select is two reads
# of the data in two launches (70 us at 16.8 M weights), the sharded protocol three reads of a 1 / world share + three all-reduces of 16 KiB
# (tens of microseconds EACH over RCCL, and every one waits for the slowest rank): the break-even moved from 4 M to about 32 M weights --
# the north-star layer (16.8 M) selects locally on every rank, VGG16's fc1 (102.8 M) shards its counting.
_SHARDED_MEDIAN_MIN = 1 << 25


def _median_slice(flat, world, rank):
    """The slice of the flattened kernel that `rank` counts for the sharded median: slices start on multiples of 4 elements."""
    n = flat.numel()
    per = -(-n // (4 * world)) * 4
    return flat[min(rank * per, n):min((rank + 1) * per, n)]


def median_abs(W, group=None, meanwhile=None):
    """np.median(np.abs(W.flatten())) for float32 W (:544, :831) as a float32 value: the middle
    element, or for an even count the float32 mean of the two middle elements (NumPy semantics;
    torch.median would return the lower one).  With a process group (every rank holds W) each rank counts
    one slice of the flattened kernel and the histograms are summed over the ranks -- the same value.
    `meanwhile`: see hip.median_abs (called exactly once, also for an empty kernel)."""
    if W.numel() == 0:
        if meanwhile is not None:
            meanwhile()
        return np.float32(np.nan)
    flat = W.detach().reshape(-1)
    n = flat.numel()
    world, rank = _group_info(group)
    if world == 1 or n < _SHARDED_MEDIAN_MIN or not flat.is_cuda:
        return hip.median_abs(flat, meanwhile)
    import torch.distributed as dist
    return hip.median_abs_sharded(_median_slice(flat, world, rank), n, lambda t: dist.all_reduce(t, group=group), meanwhile)


def layer_alphabet_device(W, alphabet, alphabet_scalar, group=None):
    """The layer alphabet of :544-545 formed and kept ON THE DEVICE (hip.DeviceAlphabet): the median of |W| stays a device scalar and one
    single-thread kernel forms rad = float64(alphabet_scalar) * float64(median) and rad * alphabet -- nothing waits for the host.
    quantize_dense() takes it in place of the host alphabet wherever the block-pipelined kernel runs (hip.dense_layer_supported)."""
    flat = W.detach().reshape(-1)
    n = flat.numel()
    if n == 0:
        raise hip.GpfqError("layer_alphabet_device: empty kernel")
    world, rank = _group_info(group)
    if world == 1 or n < _SHARDED_MEDIAN_MIN:
        return hip.layer_alphabet_from_kernel(flat, alphabet, alphabet_scalar)      # median + alphabet: one call, two launches
    import torch.distributed as dist
    med = hip.median_abs_sharded(_median_slice(flat, world, rank), n, lambda t: dist.all_reduce(t, group=group), on_device=True)
    return hip.layer_alphabet_device(med, alphabet, alphabet_scalar)


def layer_alphabet(W, alphabet, alphabet_scalar, group=None, meanwhile=None):
    """(rad * alphabet, rad) with the reference's legacy-NumPy typing (:544-545): the python
    scalar times the float32 median is a float64 product.  `meanwhile()` may queue GPU work that does not need the
    alphabet; it runs while the host waits for the median."""
    rad = np.float64(alphabet_scalar) * np.float64(median_abs(W, group, meanwhile))
    return rad * np.asarray(alphabet, dtype=np.float64), rad


# ------------------------------------------------------------------------------------------
# sharding helpers
# ------------------------------------------------------------------------------------------
def shard_bounds(n_units, world_size, rank):
    """Contiguous partition of n_units over world_size ranks: [lo, hi) of `rank`."""
    per = -(-n_units // world_size)
    lo = min(rank * per, n_units)
    return lo, min(lo + per, n_units)


_warned_unsharded = False


def _warn_unsharded_once():
    """group=None inside an initialised multi-rank job: every rank quantizes the whole layer on its own.  That is the
    documented meaning, but a caller who expected the default group gets N redundant copies of the
    work and no error -- say so once."""
    global _warned_unsharded
    if _warned_unsharded:
        return
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        _warned_unsharded = True
        import warnings
        warnings.warn("quantized_neural_networks_amd.layer: torch.distributed is initialised with "
                      f"{dist.get_world_size()} ranks but no process group was passed: this rank quantizes the whole layer "
                      "alone (pass group=dist.group.WORLD / process_group=... to shard the neurons over the ranks)",
                      RuntimeWarning, stacklevel=3)


def _group_info(group):
    """(world, rank) of an EXPLICIT process group; ``None`` means "this process alone" even inside an initialised
    torch.distributed job (a rank-0-only quantization under torchrun must not wait for collectives the other ranks
    never enter).  Pass ``dist.group.WORLD`` to shard over all ranks."""
    if group is None:
        _warn_unsharded_once()
        return 1, 0
    import torch.distributed as dist
    return dist.get_world_size(group), dist.get_rank(group)


def all_gather_units(local, n_units, group=None):
    """Reassemble a [units_local, ...] shard into [n_units, ...] on every rank with one all-gather.
    Shards are padded to the common size ceil(n_units / world) so a single
    all_gather_into_tensor (ncclAllGather on RCCL) moves them."""
    import torch.distributed as dist
    world, rank = _group_info(group)
    if world == 1:
        return local
    if local.dtype == torch.int16 and local.dim() >= 2:
        # RCCL (like NCCL and gloo) has no 16-bit integer type: the indices of 65..256-member alphabets travel as bytes
        return all_gather_units(local.contiguous().view(torch.uint8), n_units, group).view(torch.int16)
    per = -(-n_units // world)
    pad = torch.zeros((per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    pad[:local.shape[0]] = local
    out = torch.empty((world * per,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    return out[:n_units]


# ------------------------------------------------------------------------------------------
# Dense layer
# ------------------------------------------------------------------------------------------
def _log_failure(log, msg):
    import warnings
    warnings.warn(msg, RuntimeWarning, stacklevel=4)             # (the caller of the driver that ran the ladder)
    if log is not None:
        log(msg)


def _can_defer(r, alphabet):
    """Whether the launch that has just returned `r` can still fail late -- asked once, right after it (hip.last_dense_kernel names the
    process's last launch): an exchange of the block kernel's CLUSTER FORM (several workgroups per group of neurons, which rests on their
    being co-resident) can time out, and a device alphabet nobody vouched for (DeviceAlphabet.radius_ok) can be one the block kernel does
    not run.  Every other launch has no status word and costs no host wait."""
    if r.get("workspace") is None:                               # (nothing launched -- an empty shard -- or a kernel without status words)
        return False
    return (isinstance(alphabet, hip.DeviceAlphabet) and not alphabet.radius_ok) or "cluster form" in hip.last_dense_kernel()


def _neurons_timed_out(rows, m, st):
    return (f"quantize_neurons: the cluster form's exchange timed out on {rows} neurons x {m} samples (status {st}); rerunning them "
            f"through the classic kernels")


def _launch_repaired(launch, finish, alphabet, log, line, block_kernel=None, check=True, status_first=False):
    """The repair ladder of every dense launch, at the reference's granularity (it logs the failing unit and re-raises at once,
    scripts/quantized_network.py:563-565): launch(alphabet) -> the status word where the launch can have one (_can_defer; one host wait)
    -> GPFQ_ERR_CLUSTER_TIMEOUT: logged once, rerun with the cluster form off -- on the device alphabet while block_kernel(dalpha) holds,
    else (rows of more than 5120 samples: only the cluster form reads a device alphabet there) on the host alphabet's kernels
    -> GPFQ_ERR_ALPHABET (radius 0 / infinite / NaN, or members the kernel cannot index): logged once, rerun on the host alphabet, the
    cluster form allowed again -> any other status, or a second timeout, raises.  A device alphabet whose shape block_kernel() never took
    goes to the host alphabet unlogged (one read-back).  line(what, alphabet, status): the caller's wording of "timeout" / "no classic" /
    "alphabet".  finish(r, alphabet) queues what follows the kernel and returns the driver's result.  status_first=False (one GPU): it
    is queued BEHIND the kernel before the status is read -- the host's wait then costs no bubble between the two (cfg4's
    Dense(128 -> 10): 0.06 ms of a 0.15 ms layer); nothing is RETURNED unchecked.  status_first=True (a process group): the status is read
    and the shard repaired BEFORE finish() packs and gathers it -- the other ranks never see garbage and nobody has to agree on anything.
    A rerun's status is always read, and ahead of finish().  check=False (device alphabets): no status is read; the caller owes it."""
    cluster, timed_out = True, 0
    while True:
        with (hip.options() if cluster else hip.option("blk_cluster", 0)):
            if isinstance(alphabet, hip.DeviceAlphabet) and not block_kernel(alphabet):
                if timed_out:
                    _log_failure(log, line("no classic", alphabet, timed_out))
                alphabet, timed_out = alphabet.values(), 0
            elif timed_out:
                _log_failure(log, line("timeout", alphabet, timed_out))
            on_device = isinstance(alphabet, hip.DeviceAlphabet)
            r = launch(alphabet)
            wait = bool(timed_out) or ((check or not on_device) and _can_defer(r, alphabet))
            out = None if (status_first or timed_out) else finish(r, alphabet)
            st = hip.call_status(r) if wait else 0
        if st == 0:
            return finish(r, alphabet) if out is None else out
        if st == hip.GPFQ_ERR_CLUSTER_TIMEOUT and cluster:
            cluster, timed_out = False, st
        elif st == hip.GPFQ_ERR_ALPHABET and on_device:
            _log_failure(log, line("alphabet", alphabet, st))
            alphabet, cluster, timed_out = alphabet.values(), True, 0
        else:
            raise hip.GpfqError(f"dense launch failed with status {st}" + ("" if cluster else " again without the cluster form"))


def quantize_neurons_checked(X, Xq, Wt, alphabet, log=None, **kw):
    """hip.quantize_neurons through the repair ladder (_launch_repaired): where the call went through the cluster form its status word
    is read (one host wait) BEFORE the result is used; a timed-out exchange is logged and the same neurons are rerun at once through the
    classic kernels, and only a failure of that run raises.  Every other kernel family has no deferred failure and no wait."""
    return _launch_repaired(lambda a: hip.quantize_neurons(X, Xq, Wt, a, **kw), lambda r, a: r, alphabet, log,
                            lambda what, a, st: _neurons_timed_out(Wt.shape[0], X.shape[1], st))


_side_streams = {}


def _side_stream(device):
    st = _side_streams.get(device.index)
    if st is None:
        st = _side_streams[device.index] = torch.cuda.Stream(device=device)
    return st


def _beside_prepare(W, from_kernel, kernel_ready, X, Xq, unit_alphabet, rows):
    """The two independent halves of a Dense layer on two HIP streams: from_kernel() -- what depends on the kernel W alone (the median,
    the alphabet, the radii) -- on the side stream; the row norms and the record pre-pass, which depend on the activations alone, on the
    caller's (gpfq_dense_layer_prepare for `rows` neurons); ONE join.  kernel_ready says when W was complete: None -- unknown, the side
    stream first waits for everything outstanding on the caller's (always safe; the wait then sits on the longer of the two chains and the
    overlap buys little); a torch.cuda.Event -- the side stream waits for that; True -- W was complete before anything now outstanding
    here was queued (a trained network's analog kernel: the reference never writes it), no wait at all.
    Returns (from_kernel()'s tuple of tensors / DeviceAlphabets, the prepared workspace)."""
    main = torch.cuda.current_stream(W.device)
    side = _side_stream(W.device)
    if kernel_ready is None:
        side.wait_stream(main)
    elif kernel_ready is not True:
        side.wait_event(kernel_ready)
    with torch.cuda.stream(side):
        made = from_kernel()
    W.record_stream(side)                                         # (the allocator's bookkeeping: both streams use W and what was made of it)
    for t in made:
        getattr(t, "buf", t).record_stream(main)
    ws = hip.dense_layer_workspace(X.shape[0], X.shape[1], rows, W.device)
    hip.dense_layer_prepare(X, Xq, unit_alphabet, rows, ws)
    main.wait_stream(side)
    return made, ws


def check_refine(refine, name="refine"):
    """The number of refinement sweeps as an int >= 0 (ValueError otherwise; a bool is not a count)."""
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {refine!r}")
    return int(refine)


REFINE_FORMS = ("residual", "gram")
_GRAM_CHUNK_ELEMS = 1 << 24        # float64 elements of one operand chunk of the Gram form's products (128 MiB)


def check_refine_form(form, name="refine_form"):
    """The form of the refinement sweeps: "residual" (gpfq_refine_neurons) or "gram" (gpfq_refine_gram_neurons); ValueError otherwise."""
    if form not in REFINE_FORMS:
        raise ValueError(f"{name} must be one of {REFINE_FORMS}, got {form!r}")
    return form


def refine_dense(W, X, Xq, idx, radii, unit_alphabet, sweeps, form="residual"):
    """Refinement sweeps after the walk: coordinate descent on the walk's own objective ||X w - Xq q|| over
    the members a_k = radii[j] * unit_alphabet[k] of every neuron's alphabet, started from the walk's indices.

    W        f32 [N][C]  the ORIGINAL Keras kernel (not a rescaled W')
    X, Xq    f32 [N][m]  the rows the walk ran on; form="residual": m <= hip.GPFQ_REFINE_MAX_M
    idx      [N][C]      the walk's Keras-layout indices (int8; int16 beyond 64 members); left as it is
    radii    f64 [C]     on the device; a layer radius: the same number C times
    sweeps   >= 1        at most this many sweeps; a neuron whose sweep changed nothing stops
    form     "residual": the sweeps on the residual held on chip (two launches, no sync).  "gram": the sweeps on h = Xq u and the Gram
             matrix Xq Xq^T (_refine_dense_gram): rows of any length, N <= hip.GPFQ_REFINE_GRAM_MAX_N

    Returns dict(Q f32 [N][C], idx, resid_before f64 [C], resid_after f64 [C], changed i32 [C], sweeps i32 [C]) -- "gram": + gain f64
    [C]: the norms are those of the true float64 residual of the installed kernel before / after."""
    if check_refine_form(form, "form") == "gram":
        return _refine_dense_gram(W.detach(), X, Xq, idx, radii, unit_alphabet, sweeps)
    r = hip.refine_neurons(X, Xq, W.detach(), idx, radii, unit_alphabet, sweeps)
    return dict(Q=r["Q"], idx=r["idx"], resid_before=r["resid_before"], resid_after=r["resid_after"], changed=r["changed"],
                sweeps=r["sweeps"])


def _index_values(idx, radii, unit):
    """f64 [N][C]: a_{k_t} = radii[j] * unit[k] of every index (a float64 product, as the kernels form it); 0 outside the alphabet."""
    M = unit.numel()
    k = idx.long()
    on = (k >= 0) & (k < M)
    return torch.where(on, radii[None, :] * unit[k.clamp(0, M - 1)], torch.zeros((), dtype=torch.float64, device=idx.device))


def _gram_chunks(N, m):
    """Column ranges of the Gram form's chunked products: at most _GRAM_CHUNK_ELEMS float64 elements per [N][chunk] operand (at
    least 256 columns)."""
    step = max(256, _GRAM_CHUNK_ELEMS // max(N, 1))
    return [(c, min(c + step, m)) for c in range(0, m, step)]


def _residual_sumsq(W64, A, X, Xq, G=None, H=None):
    """Column sums of squares (f64 [C]) of the true residual U = X^T W - Xq^T A, by chunks of columns; on the way, where given,
    G += Xq Xq^T and H += (Xq U)^T."""
    N, m = X.shape
    same = X is Xq
    D = W64 - A if same else None
    ss = torch.zeros(W64.shape[1], dtype=torch.float64, device=W64.device)
    for c0, c1 in _gram_chunks(N, m):
        q = Xq[:, c0:c1].double()
        U = q.T @ D if same else X[:, c0:c1].double().T @ W64 - q.T @ A
        ss += (U * U).sum(0)
        if G is not None:
            G.addmm_(q, q.T)
        if H is not None:
            H.addmm_(U.T, q.T)
    return ss


def _mirror_upper(G, rows=1024):
    """G made symmetric bit for bit, in place: the upper triangle copied onto the lower one, `rows` rows at a time."""
    N = G.shape[0]
    for r0 in range(0, N, rows):
        r1 = min(r0 + rows, N)
        if r0:
            G[r0:r1, :r0] = G[:r0, r0:r1].T
        blk = G[r0:r1, r0:r1]
        blk.copy_(torch.triu(blk) + torch.triu(blk, 1).T)
    return G


def _refine_dense_gram(W, X, Xq, idx, radii, unit_alphabet, sweeps):
    """refine_dense's form="gram".  The m-long work is float64 matrix products shared by the C neurons: G = Xq Xq^T [N][N], the start
    vectors H = (Xq (X^T W - Xq^T A))^T [C][N] (A = the values of the walk's indices) and the residual norms before / after, all by
    chunks of columns (_gram_chunks); X is Xq (the same tensor: a first layer): one product per chunk less.  Memory: G (N^2 f64), H
    and three more [N][C] f64 matrices (W, A and the products' results), and per chunk two [N][chunk] and one [chunk][C] f64
    operands, chunk * N <= 2^24 elements (128 MiB each; chunk >= 256).  The norms come from the data, not from the kernel's gain."""
    N, C = W.shape
    if N > hip.GPFQ_REFINE_GRAM_MAX_N:
        raise NotImplementedError(f"refinement sweeps on the Gram matrix take walks of at most GPFQ_REFINE_GRAM_MAX_N = "
                                  f"{hip.GPFQ_REFINE_GRAM_MAX_N} steps, got {N}")
    dev = W.device
    unit = torch.as_tensor(np.asarray(unit_alphabet, dtype=np.float64), device=dev)
    W64 = W.double()
    G = torch.zeros((N, N), dtype=torch.float64, device=dev)
    H = torch.zeros((C, N), dtype=torch.float64, device=dev)
    before = _residual_sumsq(W64, _index_values(idx, radii, unit), X, Xq, G, H).sqrt_()
    r = hip.refine_gram_neurons(_mirror_upper(G), H, hip.row_norms(Xq), idx, radii, unit_alphabet, sweeps)
    del G, H
    after = _residual_sumsq(W64, _index_values(r["idx"], radii, unit), X, Xq).sqrt_()
    return dict(Q=r["Q"], idx=r["idx"], resid_before=before, resid_after=after, changed=r["changed"], sweeps=r["sweeps"], gain=r["gain"])


def _refined(out, W, X, Xq, radii, unit, refine, group, refine_form="residual"):
    """A dense driver's result with `refine` sweeps applied against the original kernel W: Q and idx replaced, + "refine" =
    dict(resid_before, resid_after, changed, sweeps) (refine_form="gram": + gain).  "resid" stays the walk's."""
    check_refine_form(refine_form)
    if not refine:
        return out
    if _group_info(group)[0] > 1:
        raise NotImplementedError("refinement sweeps are not sharded over a process group yet")
    if W.numel() == 0:
        return out
    if refine_form == "residual" and X.shape[1] > hip.GPFQ_REFINE_MAX_M:
        raise NotImplementedError(f"refinement sweeps take rows of at most GPFQ_REFINE_MAX_M = {hip.GPFQ_REFINE_MAX_M} samples, got "
                                  f"{X.shape[1]} (refine_form=\"gram\" takes longer rows)")
    r = refine_dense(W, X, Xq, out["idx"], radii, unit, refine, form=refine_form)
    out["Q"], out["idx"] = r.pop("Q"), r.pop("idx")
    out["refine"] = r
    return out


def _alphabet_radii(alphabet, C, device):
    """(radii f64 [C] on the device, unit alphabet) with radii[j] * unit[k] = member k of a layer alphabet: a DeviceAlphabet's radius is
    broadcast on the device (no read-back); a host alphabet is its own unit alphabet under the radius 1."""
    if isinstance(alphabet, hip.DeviceAlphabet):
        return alphabet.buf[:8].view(torch.float64).expand(C).contiguous(), alphabet.unit
    return torch.ones(C, dtype=torch.float64, device=device), np.asarray(alphabet, dtype=np.float64)


def quantize_dense_layer(W, X, Xq, unit_alphabet, alphabet_scalar, group=None, want_resid=True, log=None, check=True, overlap=False,
                         kernel_ready=None, refine=0, refine_form="residual"):
    """The body of _quantize_layer_parallel (scripts/quantized_network.py:523-574) from "the activations are there" to the tensors
    set_weights takes, with nothing crossing to the host: median of |W| -> rad * alphabet on the device (:544-545), row norms, record
    pre-pass, the recurrence reading the Keras kernel in place.

    overlap=True runs the median and the alphabet on a side stream beside the row norms and the record pre-pass (_beside_prepare, which
    also explains kernel_ready), then the alphabet-dependent rest (gpfq_dense_layer_run); with kernel_ready=True the median of layer
    k + 1 also fills the tail of layer k.  Measured at the north-star layer: 3.05 -> 3.00 ms per layer (profiles/r06/overlap_ab.txt).
    (Round 6's first scheme -- the pre-pass on the side stream behind a fork wait -- measured a wash and is gone.)

    Same tensors as quantize_dense(W, X, Xq, rad * unit_alphabet), bit for bit.  Returns its dict + "alphabet" (the hip.DeviceAlphabet).
    refine, refine_form: as quantize_dense."""
    refine = check_refine(refine)
    check_refine_form(refine_form)
    N, C = W.shape
    world, rank = _group_info(group)
    lo, hi = shard_bounds(C, world, rank)
    m = X.shape[1]
    side_ok = world == 1 or W.numel() < _SHARDED_MEDIAN_MIN      # (the sharded median's collectives stay on the caller's stream)
    if overlap and side_ok and W.numel() and m > 0 and hi > lo and hip.dense_layer_supported(N, m, hi - lo, unit_alphabet):
        (dalpha,), ws = _beside_prepare(W, lambda: (layer_alphabet_device(W, unit_alphabet, alphabet_scalar, None),), kernel_ready,
                                        X, Xq, unit_alphabet, hi - lo)
    else:
        dalpha, ws = layer_alphabet_device(W, unit_alphabet, alphabet_scalar, group), None
    out = quantize_dense(W, X, Xq, dalpha, group=group, want_resid=want_resid, log=log, check=check, prepared=ws, refine=refine,
                         refine_form=refine_form)
    out["alphabet"] = dalpha
    return out


def quantize_dense(W, X, Xq, alphabet, group=None, want_resid=True, log=None, check=True, prepared=None, refine=0,
                   refine_form="residual"):
    """Quantize every neuron (column) of a Dense kernel.

    W        f32 [N][C]  Keras kernel layout (row = input feature), on the GPU
    X, Xq    f32 [N][m]  feature-major analog / quantized activations (the transposed wX, qX)
    alphabet f64 [M]     the layer alphabet rad * linspace(-1, 1, M) -- or a hip.DeviceAlphabet (layer_alphabet_device): the radius then
                         never crosses to the host, the kernel reads W in its Keras layout and, on one GPU, writes Q and the indices
                         in it (no neuron-major copy, no assembly pass); shapes the block-pipelined kernel does not take fall back
                         to the host alphabet (one read-back)

    Returns dict(Q f32 [N][C], idx i8 [N][C], resid f64 [C]) on every rank.  want_resid=None: residual norms only
    where the kernel holds the residual anyway (NaN from the Gram path, which would replay it in an extra pass).
    Deferred failures are logged and repaired before anything is returned or sent to another rank (_launch_repaired).
    check=False (device alphabets; benchmarks): the deferred status of the launch is NOT read here -- no host wait at all; the result
    carries "workspace" and the caller owes hip.call_status(result) before it trusts Q.
    refine > 0: that many refinement sweeps (refine_dense) follow the walk, against W on the members of `alphabet`; Q and idx are the
    refined ones, "refine" holds dict(resid_before, resid_after, changed, sweeps), "resid" stays the walk's.  0: today's path, untouched.
    refine_form: refine_dense's form, "residual" or "gram" (the latter: rows of any length, + "gain" in "refine").
    """
    refine = check_refine(refine)
    check_refine_form(refine_form)
    N, C = W.shape
    m = X.shape[1]
    world, rank = _group_info(group)
    lo, hi = shard_bounds(C, world, rank)
    Wc = W.contiguous()
    shard = []                                                    # neuron-major shard [C_local][N], laid out when a host alphabet first needs it

    def launch(a):
        nonlocal prepared
        if isinstance(a, hip.DeviceAlphabet):
            ws, prepared = prepared, None                         # (quantize_dense_layer's side stream has run the pre-pass into it: the first launch's only)
            return hip.quantize_dense_layer(X, Xq, Wc, a, lo, hi, keras_out=(world == 1), want_values=(world == 1), want_resid=want_resid,
                                            prepared=ws)
        if not shard:
            shard.append(hip.neuron_major(Wc, lo, hi))
        if hi == lo:
            return dict(idx=torch.empty((0, N), dtype=hip.index_dtype(len(a)), device=W.device),
                        resid=torch.empty((0,), dtype=torch.float64, device=W.device), workspace=None)
        return hip.quantize_neurons(X, Xq, shard[0], a, want_values=False, want_resid=want_resid)

    def finish(r, a):
        on_device = isinstance(a, hip.DeviceAlphabet)
        if world > 1:
            # only the indices travel over xGMI -- packed to 2 or 4 bits per weight when the alphabet allows; values are looked up while
            # transposing to the Keras layout
            packed, bits = hip.pack_indices(r["idx"], len(a))
            assemble = hip.assemble_kernel_device if on_device else hip.assemble_kernel
            Q, idx = assemble(all_gather_units(packed, C, group).contiguous(), a, bits=bits, N=N)
        else:
            Q, idx = (r["Q"], r["idx"]) if on_device else hip.assemble_kernel(r["idx"], a)
        out = dict(Q=Q, idx=idx)
        if on_device:
            out["workspace"] = r["workspace"]
        if want_resid is not False:
            out["resid"] = all_gather_units(r["resid"], C, group)
        return out

    def line(what, a, st):
        if world > 1 and not isinstance(a, hip.DeviceAlphabet):
            return _neurons_timed_out(hi - lo, m, st)
        if what == "alphabet":
            return (f"Dense layer {N} x {C}: the device alphabet (radius {float(a.rad())!r}) is not one the block kernel runs; rerunning "
                    f"the layer with the host alphabet")
        if what == "no classic":
            return (f"Dense layer {N} x {C}: the cluster form's exchange timed out and no classic block kernel takes rows of {m} samples; "
                    f"rerunning the layer with the host alphabet without the cluster form")
        return f"Dense layer {N} x {C}: the cluster form's exchange timed out; rerunning the layer through the classic kernels"

    out = _launch_repaired(launch, finish, alphabet, log, line, check=check, status_first=world > 1,
                           block_kernel=lambda a: m > 0 and hip.dense_layer_supported(N, m, max(hi - lo, 1), a.unit))
    if refine:
        radii, unit = _alphabet_radii(alphabet, C, W.device)
        out = _refined(out, Wc, X, Xq, radii, unit, refine, group, refine_form)
    return out


# ------------------------------------------------------------------------------------------
# Conv2D layer
# ------------------------------------------------------------------------------------------
def _quantize_conv1x1(W, act_q, alphabet, strides):
    """1x1 kernels: every (channel, filter) pair is a ONE-step walk.  u = 0, hence <Xq_0, u> = 0 and rule
    (ii) (:86-87) returns nearest(alphabet, w) -- plain MSQ -- unless the channel's (sub-sampled) quantized
    activations are identically zero, where rule (i) (:83-84) returns the literal 0.  So the layer needs the
    per-channel norms and one MSQ pass instead of Cin patch matrices; cheaper than any all-gather, so it is
    not sharded.  (The reference reaches the same values through its general path: its (1,1) shortcut is
    dead code, :835-842.)  The residual norms are not formed (NaN)."""
    _, _, Cin, F = W.shape
    sh, sw = strides
    # all the layer needs of its activations is whether each channel's float32-rounded row norm is below 1e-16: partial sums
    # of squares only grow, so a prefix of the positions settles every live channel and only what is left undecided is
    # summed in full (hip.channel_dead; SAME == VALID for k = 1) -- no pass over the whole NHWC tensor
    Q, idx = hip.quantize_conv1x1(act_q.contiguous(), W.reshape(Cin, F), alphabet, (sh, sw))     # one library call, no host round trip
    resid = torch.full((Cin, F), float("nan"), dtype=torch.float64, device=W.device)
    return dict(Q=Q.reshape(1, 1, Cin, F), idx=idx.reshape(1, 1, Cin, F), resid=resid)


# What quantize_conv2d decides before it queues anything.  Geometry: kh, kw, K = kh * kw (the length of a pair's walk), sh, sw, rh, rw,
# same_pad, cols (n * oh * ow, the columns of a channel's patch matrix), conv = (kernel_size, strides, rate, padding) as the binding takes
# them.  Shard: world, rank, by_channel (the ranks split the channels; else every rank walks all channels for its filters), [c_lo, c_hi),
# [f_lo, f_hi).  same: act_q is act_w.  form: see _conv_plan; second: what "records" falls to where a rank lacks its kernels.
_ConvPlan = namedtuple("_ConvPlan", "kh kw K sh sw rh rw same_pad cols conv world rank by_channel c_lo c_hi f_lo f_hi same form second")


def _conv_plan(W, act_w, same, alphabet, strides, padding, rate, group, want_resid):
    """The forms in the order they are tried.  "conv1x1": one MSQ call, not sharded.  "empty": no filter is this rank's.  "loop":
    patch matrices and one quantize_neurons_checked per channel -- walks beyond GPFQ_GRAM_AUTO_MAX_N steps, and residual norms on patch
    matrices too short for the whole-shard call's replay to pay.  Everything else is ONE whole-shard Gram call: "planes_filters" (fewer
    channels than ranks) or, by channel, "nhwc3x3" (3 x 3 / stride 1 / SAME shards of 32+ channels, narrower ones where image groups
    fill the lanes) and "nhwc" (7 x 7 / stride 2 / VALID, the shift-sum form: ResNet50's conv1), which read the NHWC tensors directly
    and form no residual norms, else "planes".  (No layer the two NHWC queries take is a "loop" layer.)  Ahead of them all, with fewer
    channels than ranks, short walks and an image for every rank: "records" -- it needs the ranks' agreement at run time (_agreed_form)."""
    kh, kw, Cin, F = W.shape
    conv = ((kh, kw), strides, rate, padding)
    _, _, sh, sw, rh, rw, same_pad = hip.conv_geometry(*conv)
    K, (n, H, Wd) = kh * kw, act_w.shape[:3]
    cols = n * hip.patch_out_dim(H, kh, sh, rh, same_pad) * hip.patch_out_dim(Wd, kw, sw, rw, same_pad)
    one_by_one = K == 1 and not want_resid
    world, rank = (1, 0) if one_by_one else _group_info(group)
    by_channel = Cin >= world
    (c_lo, c_hi), (f_lo, f_hi) = (shard_bounds(Cin, world, rank), (0, F)) if by_channel else ((0, Cin), shard_bounds(F, world, rank))
    gram = K <= hip.GPFQ_GRAM_AUTO_MAX_N
    if one_by_one:
        form = "conv1x1"
    elif f_hi <= f_lo:
        form = "empty"
    elif not gram or cols <= (hip.GPFQ_GRAM_MIN_M if want_resid else 0):
        form = "loop"
    elif not by_channel:
        form = "planes_filters"
    elif want_resid or len(alphabet) > hip.GPFQ_MAX_ALPHABET:
        form = "planes"
    elif (kh, kw, sh, sw, rh, rw, same_pad) == (3, 3, 1, 1, 1, 1, True) and hip.conv3x3_nhwc_supported(n, H, Wd, c_hi - c_lo):
        form = "nhwc3x3"
    elif hip.conv_channels_nhwc_supported(n, H, Wd, c_hi - c_lo, *conv):
        form = "nhwc"
    else:
        form = "planes"
    records = not by_channel and not want_resid and gram and n >= world
    return _ConvPlan(kh, kw, K, sh, sw, rh, rw, same_pad, cols, conv, world, rank, by_channel, c_lo, c_hi, f_lo, f_hi, same,
                     "records" if records else form, form)


class _ConvPatches:
    """The one source of a quantize_conv2d call's channel planes and patch matrices.  The channel-major copies [nch][n][H][W] of this
    rank's channels are formed lazily and at most once (one transposing pass per activation tensor: a channel's gather then reads
    contiguous planes instead of one float out of every Cin); the NHWC forms have none: their (rare) reruns slice that channel alone
    out of the NHWC tensors.  The patch matrices [K][cols] are allocated for the first channel asked for and reused for the others."""

    def __init__(self, plan, act_w, act_q):
        self.plan, self.act = plan, (act_w, act_q)
        self.cm = self.Pw = self.Pq = None

    def planes(self):
        if self.cm is None:
            w = hip.channel_planes(self.act[0], self.plan.c_lo, self.plan.c_hi)
            self.cm = (w, w if self.plan.same else hip.channel_planes(self.act[1], self.plan.c_lo, self.plan.c_hi))
        return self.cm

    def _channel(self, which, c):
        if self.plan.form in ("nhwc3x3", "nhwc"):
            return self.act[which][..., c:c + 1].contiguous()
        return self.planes()[which][c - self.plan.c_lo].unsqueeze(-1)

    def of(self, c):
        """(Pw, Pq) of channel c, valid until the next call."""
        self.Pw = hip.extract_patches(self._channel(0, c), 0, *self.plan.conv, out=self.Pw)
        self.Pq = self.Pw if self.plan.same else hip.extract_patches(self._channel(1, c), 0, *self.plan.conv, out=self.Pq)
        return self.Pw, self.Pq


def _agreed_form(plan, patches, group):
    """(the form the layer takes, the summed records or None).  Only "records" is open at run time.  Fewer input channels than ranks
    (an image input has 3): the Gram records are sums over the patch columns, so every rank forms them over its share of the IMAGES,
    one all-reduce of Cin * (2 K^2 + K) doubles sums them, and every rank finishes (decide + repair, milliseconds) from the same
    records -- no gather afterwards; certified decisions do not depend on the summation order.  Both phases must have a kernel for
    their shape (the first sees this rank's images, the second all of them): all ranks agree on that first, and take plan.second if not."""
    if plan.form != "records":
        return plan.form, None
    import torch.distributed as dist
    act_w, act_q = patches.act
    n, H, Wd, Cin = act_w.shape
    n_lo, n_hi = shard_bounds(n, plan.world, plan.rank)
    try:
        pw = hip.channel_planes(act_w[n_lo:n_hi].contiguous(), 0, Cin)
        pq = pw if plan.same else hip.channel_planes(act_q[n_lo:n_hi].contiguous(), 0, Cin)
        rec, neg = hip.conv_channel_records(pw, pq, *plan.conv)
        supported = 1 if hip.conv_records_supported(n, H, Wd, Cin, *plan.conv) else 0
    except hip.GpfqError:                                           # (a rank that failed here still enters the all-reduce, and loses)
        supported = 0
    ok = torch.tensor([supported], dtype=torch.int32, device=act_w.device)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)          # all ranks take the same branch
    if not int(ok.item()):
        return plan.second, None
    dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(neg, op=dist.ReduceOp.MAX, group=group)
    return "records", (rec, neg)


def _walk_conv_shard(form, records, plan, patches, Wt_all, alphabet, want_resid, Qc, Ic, Rc):
    """This rank's (channel, filter) pairs through `form`, written into Qc / Ic [Cin][F][K] and Rc [Cin][F].  Returns the flags
    int32 [Cin][F] of the pairs a whole-shard call could not certify (_rerun_flagged), None from the forms that have none.  A
    whole-shard call is the channel loop (:844-860) in one library call: no per-channel allocation, Python or sync."""
    p, f = plan, slice(plan.f_lo, plan.f_hi)
    if form == "empty":
        return None
    if form == "loop":
        for c in range(p.c_lo, p.c_hi):
            r = quantize_neurons_checked(*patches.of(c), Wt_all[c, f], alphabet)
            Qc[c, f], Ic[c, f], Rc[c, f] = r["Q"], r["idx"], r["resid"]
        return None
    (Cin, F), dev, c = Wt_all.shape[:2], Wt_all.device, slice(p.c_lo, p.c_hi)
    Unc = torch.zeros((Cin, F), dtype=torch.int32, device=dev)
    if form == "records":
        hip.conv_channels_from_records(*records, *patches.planes(), Wt_all, alphabet, *p.conv, Ic, Qc, Unc)
    elif form == "nhwc3x3":
        hip.quantize_conv3x3_nhwc(*patches.act, p.c_lo, p.c_hi, Wt_all[c], alphabet, Ic[c], Qc[c], Unc[c])
    elif form == "nhwc":
        hip.quantize_conv_channels_nhwc(*patches.act, p.c_lo, p.c_hi, Wt_all[c], alphabet, *p.conv, Ic[c], Qc[c], Unc[c])
    elif form == "planes":
        hip.quantize_conv_channels(*patches.planes(), Wt_all[c], alphabet, *p.conv, Ic[c], Qc[c], Rc[c] if want_resid else None, Unc[c])
    else:                                      # "planes_filters": every rank walks all channels for its filters
        Wt_f = Wt_all[:, f].contiguous()
        i_f = torch.empty((Cin, p.f_hi - p.f_lo, p.K), dtype=Ic.dtype, device=dev)
        q_f = torch.empty((Cin, p.f_hi - p.f_lo, p.K), dtype=torch.float32, device=dev)
        r_f = torch.full((Cin, p.f_hi - p.f_lo), float("nan"), dtype=torch.float64, device=dev)
        u_f = torch.empty((Cin, p.f_hi - p.f_lo), dtype=torch.int32, device=dev)
        hip.quantize_conv_channels(*patches.planes(), Wt_f, alphabet, *p.conv, i_f, q_f, r_f if want_resid else None, u_f)
        Ic[:, f], Qc[:, f], Rc[:, f], Unc[:, f] = i_f, q_f, r_f, u_f
    return Unc


def _rerun_flagged(Unc, patches, Wt_all, alphabet, Qc, Ic, Rc):
    """The (channel, filter) pairs the Gram path left flagged, through the verbatim flow on the channel's patch matrices: ONE
    exact call per CHANNEL for all its flagged filters (round 5).  Normally about one pair in 10^4; but where the quantized
    network's activations have drifted orders of magnitude away from the analog ones (the last blocks of a 50-layer network
    whose 1 x 1 layers are plain MSQ: ResNet50's conv5_block3_2_conv flagged 179 000 of its 262 144 pairs) the prediction's
    bound is wider than the alphabet's spacing for most walks -- one call per PAIR was 33 s of launches for that layer.  Returns
    the number of pairs; Rc None: their residual norms are not kept."""
    flagged = torch.nonzero(Unc)                                   # one sync per layer
    if flagged.numel() == 0:
        return 0
    by_c = {}
    for c, f in flagged.tolist():
        by_c.setdefault(c, []).append(f)
    for c, fs in by_c.items():
        Pw, Pq = patches.of(c)
        fsel = torch.tensor(fs, dtype=torch.long, device=Unc.device)
        path = hip.GPFQ_PATH_ONCHIP if Pw.shape[1] <= hip.GPFQ_ONCHIP_MAX_M else hip.GPFQ_PATH_STREAM
        r = quantize_neurons_checked(Pw, Pq, Wt_all[c].index_select(0, fsel).contiguous(), alphabet, path=path)     # (rows of up to 28672 samples: possibly the cluster form)
        Qc[c, fsel], Ic[c, fsel] = r["Q"], r["idx"]
        if Rc is not None:
            Rc[c, fsel] = r["resid"]
    return int(flagged.shape[0])


def _gather_conv_kernel(Ic, Rc, want_resid, plan, alphabet, group):
    """(Q, idx [kh][kw][Cin][F], resid [Cin][F]) on every rank from the ranks' shards of Ic [Cin][F][K] and Rc [Cin][F]; a shard's unit
    is the channel, or the filter where the filters are split.  ONE all-gather of the packed alphabet indices ((unit, other) pairs are
    rows of K weights; a shard may be empty); the float32 values never travel: every rank looks them up while laying the kernel out
    ([K][pairs] is [kh][kw][unit][other]).  Residual norms: a second all-gather where they are wanted, this rank's own where not."""
    p, (Cin, F, K) = plan, Ic.shape
    if p.by_channel:                           # shard(t): this rank's units of t in front; back(t): [..][unit][other] as [..][Cin][F]
        units, other, shard, back = Cin, F, (lambda t: t[p.c_lo:p.c_hi]), (lambda t: t)
    else:
        units, other, shard, back = F, Cin, (lambda t: t[:, p.f_lo:p.f_hi].transpose(0, 1)), (lambda t: t.transpose(-2, -1))
    local = shard(Ic)
    packed, bits = hip.pack_indices(local.reshape(-1, K).contiguous(), len(alphabet))
    g = all_gather_units(packed.reshape(local.shape[0], other * packed.shape[1]), units, group)
    Qk, Ik = hip.assemble_kernel(g.reshape(units * other, packed.shape[1]).contiguous(), alphabet, bits=bits, N=K)
    Q, idx = (back(t.reshape(p.kh, p.kw, units, other)).contiguous() for t in (Qk, Ik))
    if not want_resid:
        return Q, idx, Rc
    return Q, idx, back(all_gather_units(shard(Rc).contiguous(), units, group))


def quantize_conv2d(W, act_w, act_q, alphabet, strides, padding, rate, group=None, want_resid=True):
    """Quantize a Conv2D / DepthwiseConv2D kernel channel by channel.

    W          f32 [kh][kw][Cin][F]   Keras kernel layout
    act_w/q    f32 NHWC [n][H][W][Cin] analog / quantized layer inputs
    Each (input channel c, filter f) pair is an independent neuron of kh*kw weights whose data are
    the rows of channel c's patch matrix (:652-727); channels are partitioned over the ranks.  When Cin < world the
    Gram records are formed over image shards and all-reduced (or, where that does not apply, the filters of each
    channel are partitioned instead).  Sharded runs exchange ONE all-gather per layer: the alphabet indices of the
    rank's (channel, filter) pairs, packed to 2 / 4 bits per weight as the dense path's are; values are looked up
    locally (+ one all-gather of the residual norms when they are requested).  _conv_plan names the forms a layer can take.

    Returns dict(Q f32 [kh][kw][Cin][F], idx i8 same shape, resid f64 [Cin][F], reruns: this rank's pairs rerun through the exact path).
    """
    (kh, kw, Cin, F), dev = W.shape, W.device
    plan = _conv_plan(W, act_w, act_q is act_w, alphabet, strides, padding, rate, group, want_resid)
    if plan.form == "conv1x1":
        return _quantize_conv1x1(W, act_q, alphabet, strides)
    Qc = torch.zeros((Cin, F, plan.K), dtype=torch.float32, device=dev)
    Ic = torch.zeros((Cin, F, plan.K), dtype=hip.index_dtype(len(alphabet)), device=dev)
    Rc = torch.full((Cin, F), 0.0 if want_resid else float("nan"), dtype=torch.float64, device=dev)
    act_w = act_w.contiguous()
    patches = _ConvPatches(plan, act_w, act_w if plan.same else act_q.contiguous())
    # neuron-major filters [Cin][F][K]: row-major flattening of each kh x kw filter (:215), t = ky*kw + kx
    Wt_all = W.permute(2, 3, 0, 1).reshape(Cin, F, plan.K).contiguous()
    form, records = _agreed_form(plan, patches, group)
    Unc = _walk_conv_shard(form, records, plan, patches, Wt_all, alphabet, want_resid, Qc, Ic, Rc)
    replicated = form == "records"             # every rank already holds the whole result; its residual norms are left unformed
    reruns = 0 if Unc is None else _rerun_flagged(Unc, patches, Wt_all, alphabet, Qc, Ic, None if replicated else Rc)
    if plan.world > 1 and not replicated:
        Q, idx, Rc = _gather_conv_kernel(Ic, Rc, want_resid, plan, alphabet, group)
    else:
        Q, idx = (t.reshape(Cin, F, kh, kw).permute(2, 3, 0, 1).contiguous() for t in (Qc, Ic))
    return dict(Q=Q, idx=idx, resid=Rc.contiguous(), reruns=torch.tensor(reruns))


def _pair_radii(radii, Cin, F, depthwise, device):
    """f64 [Cin][F] on the device, one radius per (input channel, filter) pair, with no read-back: a DeviceAlphabet's radius or a host
    number broadcast; f64 [F] (one per Conv2D filter) repeated over the channels; f64 [Cin * F] of a depthwise kernel (output channel
    c * mult + d) viewed as it is."""
    if isinstance(radii, hip.DeviceAlphabet):
        return radii.buf[:8].view(torch.float64).expand(Cin, F).contiguous()
    if not isinstance(radii, torch.Tensor):
        return torch.full((Cin, F), float(radii), dtype=torch.float64, device=device)
    if radii.dtype != torch.float64 or radii.numel() != (Cin * F if depthwise else F):
        raise ValueError(f"radii must be f64 [{Cin * F if depthwise else F}], got {radii.dtype} {tuple(radii.shape)}")
    return radii.reshape(Cin, F).contiguous() if depthwise else radii.reshape(1, F).expand(Cin, F).contiguous()


def refine_conv2d(W, act_w, act_q, idx, radii, unit_alphabet, sweeps, strides, padding, rate, depthwise=False, group=None):
    """Refinement sweeps for the walks per (input channel, filter) pair of a Conv2D / DepthwiseConv2D kernel: the
    coordinate descent of refine_dense's Gram form for every pair -- a neuron of kh*kw weights over the rows of its channel's patch
    matrices -- on the pair's own objective ||X_c^T w - Xq_c^T q||, started from the walk's indices.  It runs after quantize_conv2d (or
    its radius="channel" / search forms), on their result.  No patch matrix is formed: the channels' Gram matrices come from
    hip.conv_channel_records, called once, or twice with swapped arguments when act_q is not act_w (the second call's lower triangle is
    the upper one of Xq_c X_c^T); one kernel call walks all pairs (hip.refine_conv_pairs).

    W        f32 [kh][kw][Cin][F]  the ORIGINAL Keras kernel (not a rescaled W'); a depthwise kernel: F = the depth multiplier
    act_w/q  f32 NHWC              the layer inputs the walk ran on
    idx      [kh][kw][Cin][F]      the walk's indices (int8; int16 beyond 64 members); left as it is
    radii    a hip.DeviceAlphabet or a host number (the layer radius), f64 [F] on the device (one per filter: radius="channel" and the
             search on Conv2D), or -- depthwise=True -- f64 [Cin * F] (radius="channel" on a depthwise kernel)
    sweeps   >= 1

    NotImplementedError: kh * kw beyond hip.GPFQ_REFINE_PAIRS_MAX_K, a shape the record kernels do not take, a group of several ranks.
    Returns dict(Q f32 [kh][kw][Cin][F], idx, changed i32 [Cin][F], sweeps i32 [Cin][F], gain f64 [Cin][F])."""
    sweeps = check_refine(sweeps, "sweeps")
    if sweeps < 1:
        raise ValueError("sweeps must be >= 1")
    kh, kw, Cin, F = W.shape
    K, dev = kh * kw, W.device
    if _group_info(group)[0] > 1:
        raise NotImplementedError("refinement sweeps are not sharded over a process group yet")
    if K > hip.GPFQ_REFINE_PAIRS_MAX_K:
        raise NotImplementedError(f"refinement sweeps per (input channel, filter) pair take kernels of at most GPFQ_REFINE_PAIRS_MAX_K = "
                                  f"{hip.GPFQ_REFINE_PAIRS_MAX_K} weights, got {kh} x {kw} = {K}")
    conv = ((kh, kw), strides, rate, padding)
    n, H, Wd = act_w.shape[:3]
    if not hip.conv_records_supported(n, H, Wd, Cin, *conv):
        raise NotImplementedError(f"refinement sweeps per (input channel, filter) pair need the Gram records of the layer's channels, and "
                                  f"no record kernel takes {n} images of {H} x {Wd} under a {kh} x {kw} kernel, strides {tuple(strides)}, "
                                  f"rate {tuple(rate) if rate else (1, 1)}, padding {padding}")
    R = _pair_radii(radii, Cin, F, depthwise, dev)
    same = act_q is act_w
    pw = hip.channel_planes(act_w.contiguous(), 0, Cin)
    pq = pw if same else hip.channel_planes(act_q.contiguous(), 0, Cin)
    rec, _ = hip.conv_channel_records(pw, pq, *conv)
    swapped = None if same else hip.conv_channel_records(pq, pw, *conv)[0]
    Wt = W.detach().permute(2, 3, 0, 1).reshape(Cin, F, K).contiguous()
    It = idx.permute(2, 3, 0, 1).reshape(Cin, F, K).contiguous()
    if It.data_ptr() == idx.data_ptr():             # (a 1 x 1 kernel of one channel: the permutation is the tensor itself)
        It = It.clone()
    r = hip.refine_conv_pairs(rec, swapped, K, Wt, R, unit_alphabet, sweeps, It)
    Q, out_idx = (t.reshape(Cin, F, kh, kw).permute(2, 3, 0, 1).contiguous() for t in (r["Q"], It))
    return dict(Q=Q, idx=out_idx, changed=r["changed"], sweeps=r["sweeps"], gain=r["gain"])


# ------------------------------------------------------------------------------------------
# radius = "channel": one alphabet radius per output channel
# ------------------------------------------------------------------------------------------
_unit_alphabets = {}


def _unit_alphabet_device(unit, device):
    """DeviceAlphabet of radius exactly 1 (1.0 * float64(1.0f)) over the unit alphabet, one per device and alphabet: what the
    block-pipelined kernel reads when it walks a scaled kernel W'.  Known good on the host, so no deferred alphabet status is waited for."""
    key = (device.index, tuple(float(v) for v in unit))
    d = _unit_alphabets.get(key)
    if d is None:
        one = torch.ones(1, dtype=torch.float32, device=device)
        d = hip.layer_alphabet_device(one, unit, 1.0)
        d._rad = np.float64(1.0)
        d.radius_ok = hip.device_alphabet_ok(np.float32(1.0), unit, 1.0)
        _unit_alphabets[key] = d
    return d


def _channel_radii(W2d, alphabet_scalar, scale):
    """(layer median f32 device scalar or None, radii f64 [C'], W') of a row-major [R][C'] view of a kernel: two launches, no sync."""
    med = hip.median_abs(W2d.reshape(-1), on_device=True) if W2d.numel() else None
    r, Wp = hip.column_radii(W2d, alphabet_scalar, layer_median=med, scale=scale)
    return med, r, Wp


def quantize_dense_channels(W, X, Xq, unit_alphabet, alphabet_scalar, group=None, overlap=False, kernel_ready=None, want_resid=True,
                            log=None, check=True, refine=0, refine_form="residual"):
    """quantize_dense with one radius per neuron (radius="channel"): r_j = alphabet_scalar * median(|W[:, j]|) (the layer radius
    where that is not a finite positive number, then 0), the walk run by quantize_dense -- every kernel, fallback and repair as there --
    on W' = float32(W / r_j) with the unit alphabet (a device alphabet of radius 1 up to 64 members), and
    Q = float32(r_j * unit[idx]), resid_j = r_j * the walk's residual norm.

    Sharded (group): every rank computes all radii itself (deterministic, no collective) and scales only its own neurons; the one
    all-gather still carries packed indices only.  overlap=True: the median and the radii / W' launch go to a side stream beside the row
    norms and the record pre-pass (_beside_prepare, which explains kernel_ready).

    Returns quantize_dense's dict with Q, resid as above + "radii" (f64 [C]) and "layer_median" (f32 device scalar).
    refine > 0: refinement sweeps (refine_dense) against the original W -- not W' -- on the members r_j * unit[k]; as quantize_dense."""
    refine = check_refine(refine)
    check_refine_form(refine_form)
    N, C = W.shape
    world, rank = _group_info(group)
    lo, hi = shard_bounds(C, world, rank)
    m = X.shape[1]
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    Wc = W.detach().contiguous()
    dalpha = _unit_alphabet_device(unit, W.device) if len(unit) <= 64 else None
    alphabet = dalpha if dalpha is not None else unit
    if overlap and dalpha is not None and Wc.numel() and m > 0 and hi > lo and hip.dense_layer_supported(N, m, hi - lo, unit):
        (med, r, Wp), ws = _beside_prepare(Wc, lambda: _channel_radii(Wc, alphabet_scalar, (lo, hi)), kernel_ready, X, Xq, unit, hi - lo)
    else:
        (med, r, Wp), ws = _channel_radii(Wc, alphabet_scalar, (lo, hi)), None
    out = quantize_dense(Wp, X, Xq, alphabet, group=group, want_resid=want_resid, log=log, check=check, prepared=ws)
    out["Q"], _ = hip.assemble_kernel_colrad(out["idx"], unit, r, layout=hip.GPFQ_LAYOUT_KERAS)
    if "resid" in out:
        out["resid"] = out["resid"] * r
    out["radii"], out["layer_median"] = r, med
    return _refined(out, Wc, X, Xq, r, unit, refine, group, refine_form)


def quantize_conv2d_channels(W, act_w, act_q, unit_alphabet, alphabet_scalar, strides, padding, rate, group=None, want_resid=True,
                             depthwise=False):
    """quantize_conv2d with one radius per output channel (radius="channel"): filter f of a Conv2D kernel -- column f of the view
    [kh*kw*Cin][F] -- or output channel (c, d) of a DepthwiseConv2D kernel -- column c*mult + d of [kh*kw][Cin*mult].  The
    (channel, filter) pairs walk on W' = float32(W / r) with the unit alphabet through quantize_conv2d (its reruns and sharding
    included); Q = float32(r * unit[idx]), resid scaled by the pair's radius.  Every rank computes all radii itself.
    Returns quantize_conv2d's dict + "radii" (f64 [F] or [Cin*mult]) and "layer_median"."""
    kh, kw, Cin, F = W.shape
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    Wc = W.detach().contiguous()
    W2 = Wc.reshape(kh * kw, Cin * F) if depthwise else Wc.reshape(kh * kw * Cin, F)
    med, r, Wp = _channel_radii(W2, alphabet_scalar, (0, W2.shape[1]))
    out = quantize_conv2d(Wp.reshape(kh, kw, Cin, F), act_w, act_q, unit, strides, padding, rate, group=group, want_resid=want_resid)
    Q, _ = hip.assemble_kernel_colrad(out["idx"].reshape(W2.shape), unit, r, layout=hip.GPFQ_LAYOUT_KERAS)
    out["Q"] = Q.reshape(kh, kw, Cin, F)
    out["resid"] = out["resid"] * (r.reshape(Cin, F) if depthwise else r.reshape(1, F))
    out["radii"], out["layer_median"] = r, med
    return out


# ------------------------------------------------------------------------------------------
# a sequence as alphabet_scalar: search the scalar on the device
# ------------------------------------------------------------------------------------------
# One walk call takes whole candidates while its kernel W'' [rows][g * C] stays below this many elements (8 GiB of float32, and every
# element offset of the passes around the walk within 32 bits); beyond it the candidates are split into groups of g.
_SEARCH_MAX_ELEMS = (1 << 31) - 1


def check_scalars(alphabet_scalar):
    """The candidates of a search as a list of floats: 1..16 finite positive numbers (ValueError names the offender otherwise)."""
    if isinstance(alphabet_scalar, (str, bytes)):
        raise ValueError(f"alphabet_scalar must be a number or a sequence of 1..{hip.GPFQ_SEARCH_MAX_CANDIDATES} numbers, got "
                         f"{alphabet_scalar!r}")
    try:
        raw = list(alphabet_scalar)
    except TypeError:
        raise ValueError(f"alphabet_scalar candidates must be a sequence of numbers, got {alphabet_scalar!r}")
    if not 1 <= len(raw) <= hip.GPFQ_SEARCH_MAX_CANDIDATES:
        raise ValueError(f"alphabet_scalar holds {len(raw)} candidates: a search takes 1..{hip.GPFQ_SEARCH_MAX_CANDIDATES}")
    out = []
    for v in raw:
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"alphabet_scalar candidate {v!r} is not a number")
        if not (np.isfinite(f) and f > 0):
            raise ValueError(f"alphabet_scalar candidate {v!r} is not a finite positive number")
        out.append(f)
    return out


def _check_per(per):
    if per not in ("channel", "layer"):
        raise ValueError(f"per must be 'channel' or 'layer', got {per!r}")
    return per == "layer"


def _candidate_groups(K, rows, C):
    """[k_lo, k_hi) of the groups of whole candidates one walk call takes: the fewest equal-sized groups whose kernel
    [rows][g * C] stays within _SEARCH_MAX_ELEMS elements (one candidate per group at the least)."""
    g = max(1, min(K, _SEARCH_MAX_ELEMS // max(rows * C, 1)))
    n = -(-K // g)
    g = -(-K // n)
    return [(k, min(k + g, K)) for k in range(0, K, g)]


def _search_base(W2d, per_layer):
    """(layer median f32 device scalar, the base radii of a search): per="channel" the radii of scalar 1 (f64 [C'], two launches), per="layer" the
    median itself (the candidate kernel broadcasts it).  No sync."""
    if W2d.numel() == 0:
        return None, torch.zeros(W2d.shape[1], dtype=torch.float64, device=W2d.device)
    med = hip.median_abs(W2d.reshape(-1), on_device=True)
    return med, (med if per_layer else hip.column_radii(W2d, 1.0, layer_median=med)[0])


def quantize_dense_search(W, X, Xq, unit_alphabet, alphabet_scalars, per="channel", group=None, overlap=False, kernel_ready=None,
                          log=None, check=True, refine=0, refine_form="residual"):
    """quantize_dense with the alphabet scalar SEARCHED over the candidates alphabet_scalars = (s_0 .. s_{K-1}), 1 <= K <= 16: base
    radius b_j = median(|W[:, j]|) (per="channel"; the layer median where that is not finite and positive, then 0) or median(|W|) for
    every j (per="layer"), r_{k,j} = s_k * b_j, and ONE quantize_dense call -- every kernel, fallback and repair as there -- walks the
    K * C columns W''[:, k * C + j] = float32(W[:, j] / r_{k,j}) with the unit alphabet (a device alphabet of radius 1 up to 64 members).
    Candidate k of neuron j scores (r_{k,j} * its residual norm)^2; per="channel" keeps, for every neuron, the first candidate with
    the smallest score, per="layer" the first candidate with the smallest sum over the neurons (hip.select_candidates: on the device,
    in a fixed order).  The search ALWAYS walks the rescaled kernel, also for per="layer" and for K = 1: [s] with per="channel" is
    quantize_dense_channels(.., s) bit for bit, [s] with per="layer" is the reference's un-rescaled walk only up to the rounding of W''
    (DESIGN.md section 8 measured 0.006-0.04 % of the indices).

    Candidates are split into groups of whole candidates where one call cannot take all K * C columns (_candidate_groups); the columns
    are independent, the result is the same.  Sharded (group): every rank forms all radii, quantize_dense shards the K * C columns and
    its one all-gather brings every candidate's indices and norms to every rank (K times the traffic of one candidate); every rank
    selects for itself.  overlap=True: the median, the radii and the candidate launch go to a side stream beside the row norms and the
    record pre-pass for the K * C columns (_beside_prepare, which explains kernel_ready).  check=False holds for a single group only.

    Returns dict(Q f32 [N][C], idx [N][C], resid f64 [C] = r * norm, radii f64 [C] -- all of the selected candidates --, best i32 [C],
    scores f64 [K][C], layer_median f32 device scalar).  refine > 0: refinement sweeps (refine_dense) run ONCE, after the selection,
    against the original W on the selected radii; "resid" and "scores" stay the walk's."""
    scalars = check_scalars(alphabet_scalars)
    per_layer = _check_per(per)
    refine = check_refine(refine)
    check_refine_form(refine_form)
    K = len(scalars)
    N, C = W.shape
    world, rank = _group_info(group)
    m = X.shape[1]
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    Wc = W.detach().contiguous()
    dalpha = _unit_alphabet_device(unit, W.device) if len(unit) <= 64 else None
    alphabet = dalpha if dalpha is not None else unit
    groups = _candidate_groups(K, N, C)
    base = {}
    parts = []
    for k_lo, k_hi in groups:
        gC = (k_hi - k_lo) * C
        lo, hi = shard_bounds(gC, world, rank)

        def from_kernel():
            if not base:
                base["med"], base["b"] = _search_base(Wc, per_layer)
            return (base["med"], base["b"]) + hip.candidate_kernels(Wc, base["b"], scalars[k_lo:k_hi], scale=(lo, hi))

        if overlap and dalpha is not None and Wc.numel() and m > 0 and hi > lo and hip.dense_layer_supported(N, m, hi - lo, unit):
            made, ws = _beside_prepare(Wc, from_kernel, kernel_ready, X, Xq, unit, hi - lo)
        else:
            made, ws = from_kernel(), None
        r, Wpp = made[2], made[3]
        out = quantize_dense(Wpp, X, Xq, alphabet, group=group, want_resid=True, log=log, check=check or len(groups) > 1, prepared=ws)
        parts.append((out, r))
    if len(parts) == 1:
        idx, resid, r = parts[0][0]["idx"], parts[0][0]["resid"], parts[0][1]
    else:                                                         # (k-major blocks: the groups' columns back to back)
        idx = torch.cat([p[0]["idx"] for p in parts], dim=1)
        resid = torch.cat([p[0]["resid"] for p in parts])
        r = torch.cat([p[1] for p in parts])
    sel = hip.select_candidates(idx.contiguous(), resid.reshape(1, K * C).contiguous(), r, unit, K, per_layer)
    res = dict(Q=sel["Q"], idx=sel["idx"], resid=sel["resid"].reshape(C), radii=sel["radii"], best=sel["best"], scores=sel["scores"],
               layer_median=base["med"])
    if len(parts) == 1 and "workspace" in parts[0][0]:
        res["workspace"] = parts[0][0]["workspace"]
    return _refined(res, Wc, X, Xq, res["radii"], unit, refine, group, refine_form)


def quantize_conv2d_search(W, act_w, act_q, unit_alphabet, alphabet_scalars, strides, padding, rate, per="channel", group=None):
    """quantize_conv2d with the alphabet scalar searched per filter (per="channel") or for the layer (per="layer"), as
    quantize_dense_search: the output channels are the columns f of the view [kh*kw*Cin][F], the candidates the K * F columns of
    W'' viewed as (kh, kw, Cin, K * F), walked by ONE quantize_conv2d(.., want_resid=True) call per group of candidates (its reruns and
    sharding included).  Candidate k of filter f scores sum_c (r_{k,f} * norm[c][k * F + f])^2 over the input channels c, ascending.
    1 x 1 kernels go through the same call and the same formula.  DepthwiseConv2D kernels are not searched (their output channels
    are (c, d) pairs, which the k-major blocks of (kh, kw, Cin, K * mult) do not hold).

    Returns dict(Q f32 [kh][kw][Cin][F], idx same shape, resid f64 [Cin][F] = r * norm, radii f64 [F], best i32 [F],
    scores f64 [K][F], layer_median, reruns)."""
    scalars = check_scalars(alphabet_scalars)
    per_layer = _check_per(per)
    K = len(scalars)
    kh, kw, Cin, F = W.shape
    R = kh * kw * Cin
    unit = np.asarray(unit_alphabet, dtype=np.float64)
    W2 = W.detach().contiguous().reshape(R, F)
    med, b = _search_base(W2, per_layer)
    idx, resid, radii, reruns = [], [], [], 0
    for k_lo, k_hi in _candidate_groups(K, R, F):
        g = k_hi - k_lo
        r, Wpp = hip.candidate_kernels(W2, b, scalars[k_lo:k_hi], scale=(0, g * F))
        out = quantize_conv2d(Wpp.reshape(kh, kw, Cin, g * F), act_w, act_q, unit, strides, padding, rate, group=group, want_resid=True)
        idx.append(out["idx"].reshape(R, g * F))
        resid.append(out["resid"])
        radii.append(r)
        reruns = out["reruns"] + reruns
    one = len(idx) == 1
    sel = hip.select_candidates((idx[0] if one else torch.cat(idx, dim=1)).contiguous(),
                                (resid[0] if one else torch.cat(resid, dim=1)).contiguous(), radii[0] if one else torch.cat(radii),
                                unit, K, per_layer)
    return dict(Q=sel["Q"].reshape(kh, kw, Cin, F), idx=sel["idx"].reshape(kh, kw, Cin, F), resid=sel["resid"], radii=sel["radii"],
                best=sel["best"], scores=sel["scores"], layer_median=med, reruns=reruns)


# ------------------------------------------------------------------------------------------
# conv_walk = "filter": a Conv2D filter walked as ONE neuron of kh*kw*Cin weights
# ------------------------------------------------------------------------------------------
def _filter_rows(W, act_w, act_q, strides, padding, rate, columns, seed):
    """(W2 [N][F] -- the Keras kernel viewed with row (ky*kw + kx)*Cin + c --, X, Xq [N][m], m, total): the Dense problem whose neurons
    are the layer's filters, on a sample of the patch columns (hip.gather_patch_columns: one launch; every rank of a group forms the
    same rows itself, no collective)."""
    kh, kw, Cin, F = W.shape
    act_w = act_w.contiguous()
    act_q = act_w if (act_q is None or act_q is act_w) else act_q.contiguous()
    X, Xq, m, total = hip.gather_patch_columns(act_w, act_q, (kh, kw), tuple(strides), tuple(rate) if rate else None, padding,
                                               columns=columns, seed=seed)
    return W.detach().contiguous().reshape(kh * kw * Cin, F), X, Xq, m, total


def _as_filters(out, W, m, total):
    """A dense driver's [N][F] results in the Keras kernel's shape (views), + the sample's size."""
    for key in ("Q", "idx"):
        if out.get(key) is not None:
            out[key] = out[key].reshape(W.shape)
    out["columns"], out["total"] = m, total
    return out


def quantize_conv2d_filters(W, act_w, act_q, alphabet, strides, padding, rate, columns=8192, seed=0, group=None, want_resid=True, log=None,
                            refine=0, refine_form="residual"):
    """Quantize a Conv2D kernel filter by filter: filter f is neuron f of the Dense problem (W2, X, Xq) of _filter_rows -- a walk of
    kh*kw*Cin steps over the im2col rows of ALL input channels, where quantize_conv2d walks every (channel, filter) pair on its own.

    W          f32 [kh][kw][Cin][F]   Keras kernel layout
    act_w/q    f32 NHWC [n][H][W][Cin] analog / quantized layer inputs (act_q is act_w: one matrix)
    alphabet   f64 [M] or a hip.DeviceAlphabet, as quantize_dense takes
    columns    the patch columns sampled out of total = n*oh*ow (hip.patch_column with `seed`); None or >= total: all of them

    The walk is quantize_dense's: its kernels, repairs and fallbacks, its sharding (filters over the ranks, one all-gather of packed
    indices).  Returns dict(Q f32 [kh][kw][Cin][F], idx same shape, resid f64 [F], columns=m, total=total) (+ quantize_dense's
    "workspace" for a device alphabet).  refine > 0: quantize_dense's refinement sweeps on the gathered columns the walk used
    (columns <= hip.GPFQ_REFINE_MAX_M)."""
    W2, X, Xq, m, total = _filter_rows(W, act_w, act_q, strides, padding, rate, columns, seed)
    return _as_filters(quantize_dense(W2, X, Xq, alphabet, group=group, want_resid=want_resid, log=log, refine=refine,
                                      refine_form=refine_form), W, m, total)


def quantize_conv2d_filters_channels(W, act_w, act_q, unit_alphabet, alphabet_scalar, strides, padding, rate, columns=8192, seed=0,
                                     group=None, want_resid=True, log=None, refine=0, refine_form="residual"):
    """quantize_conv2d_filters with one radius per filter (radius="channel"): quantize_dense_channels on the rows of _filter_rows (the
    columns of W2 are the filters).  Returns its dict with Q, idx in the kernel's shape + columns, total."""
    W2, X, Xq, m, total = _filter_rows(W, act_w, act_q, strides, padding, rate, columns, seed)
    return _as_filters(quantize_dense_channels(W2, X, Xq, unit_alphabet, alphabet_scalar, group=group, want_resid=want_resid, log=log,
                                               refine=refine, refine_form=refine_form), W, m, total)


def quantize_conv2d_filters_search(W, act_w, act_q, unit_alphabet, alphabet_scalars, strides, padding, rate, per="channel", columns=8192,
                                   seed=0, group=None, log=None, refine=0, refine_form="residual"):
    """quantize_conv2d_filters with the alphabet scalar searched per filter (per="channel") or for the layer (per="layer"):
    quantize_dense_search on the rows of _filter_rows.  Returns its dict with Q, idx in the kernel's shape + columns, total."""
    W2, X, Xq, m, total = _filter_rows(W, act_w, act_q, strides, padding, rate, columns, seed)
    return _as_filters(quantize_dense_search(W2, X, Xq, unit_alphabet, alphabet_scalars, per=per, group=group, log=log, refine=refine,
                                             refine_form=refine_form),
                       W, m, total)

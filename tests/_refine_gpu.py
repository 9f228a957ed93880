"""What the GPU tests of the refinement sweeps share (tests/test_refine_gpu.py, test_refine_gram_gpu.py, test_refine_pairs_gpu.py):
the device and host conversions, the unit alphabets of the exact cases, the exact-data MLP and the small CNN the classes are run on,
the packed round trip, and the table-driven check of an entry's status codes."""
import numpy as np
import torch

DEV = torch.device("cuda", 0)
EPS = 2.0 ** -53


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(out):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def index_type(unit):
    return np.int16 if len(unit) > 64 else np.int8


def ulp_equal(a, b, ulps=1):
    return bool((np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def unit(kind):
    """Unit alphabets: 1 member, linspace(-1, 1, M), and the dyadic "d4" (4 members, not uniform) and "d16" (16, not ascending).
    linspace(-1, 1, M) has dyadic members for M = 2, 3 and 65 (step 1 / 32); the 4- and 16-level linspace members (thirds, fifteenths)
    are not dyadic, so with them the sums over a_k * Xq are NOT exact (dyadic(kind)): d4 and d16 carry the exact check at those sizes."""
    if kind == "d4":
        return np.array([-1.0, -0.25, 0.25, 1.0])
    if kind == "d16":
        return np.random.default_rng(16).permutation(np.arange(-15, 16, 2) / 16.0)
    M = int(kind)
    return np.linspace(-1, 1, M) if M > 1 else np.array([1.0])


def dyadic(kind):
    return kind in ("d4", "d16", "1", "2", "3", "65")


class Quiet:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def exact_mlp():
    """Two Dense layers whose kernels are multiples of 1/8 (the bias of 1/4): on integer inputs every activation of the analog and of
    the quantized network, every radius (scalar 2 times a dyadic median) and every sum of the refinement is exact."""
    from quantized_neural_networks_amd import keras_shim as ks
    net = ks.Sequential([ks.Dense(11, activation="relu", input_shape=(24,)), ks.Dense(5)], seed=1)
    r = np.random.default_rng(8)
    for layer, shape in zip(net.layers, ((24, 11), (11, 5))):
        layer.set_weights([(r.integers(-8, 9, shape) / 8.0).astype(np.float32), (r.integers(-2, 3, shape[1]) / 4.0).astype(np.float32)])
    return net


def capture_layer_data(q, capture, clone=False):
    """capture: a dict that takes the (wX, qX) every layer of the quantizer q is given (clone: copies of them)."""
    orig = q._get_layer_data_generator

    def wrapped(layer_idx, transpose=False):
        wX, qX = orig(layer_idx, transpose)
        capture[layer_idx] = (wX.clone(), qX.clone()) if clone else (wX, qX)
        return wX, qX

    q._get_layer_data_generator = wrapped


def cnn(refine_passes, input_shape=(8, 8, 3), images=32, batch=16, signed=False, layers=None, capture=None, **kw):
    """A small CNN, quantized: Conv2D(6, 3x3, same, relu) - DepthwiseConv2D(3x3, valid, 2 per channel) - Flatten - Dense(3) (layers:
    other layers in front of Flatten) on `images` random images (uniform in [0, 1); signed: standard normal), 2 bits, scalar 3.
    Returns (the quantizer, its logger)."""
    from quantized_neural_networks_amd import keras_shim as ks, quantized_network as qn
    if layers is None:
        layers = [ks.Conv2D(6, 3, padding="same", activation="relu", input_shape=input_shape),
                  ks.DepthwiseConv2D(3, padding="valid", depth_multiplier=2, use_bias=False)]
    net = ks.Sequential(layers + [ks.Flatten(), ks.Dense(3)], seed=3)
    r = np.random.default_rng(5)
    x = (r.standard_normal((images,) + input_shape) if signed else r.random((images,) + input_shape)).astype(np.float32)
    log = Quiet()
    q = qn.QuantizedCNN(network=net, batch_size=batch, get_data=qn.CIFAR10Sequence(x, np.zeros((images, 3), np.float32), batch), logger=log,
                        bits=2, alphabet_scalar=3, refine_passes=refine_passes, **kw)
    if capture is not None:
        capture_layer_data(q, capture)
    q.quantize_network()
    return q, log


def packed_round_trip(q, tmp_path):
    """The packed export accepts the quantized kernels (a kernel off its alphabet does not encode) and returns them."""
    from quantized_neural_networks_amd import deploy
    back = deploy.load_packed(deploy.export_packed(q, tmp_path / "net"))
    for k, layer in enumerate(q.quantized_net.layers):
        if q._will_quantize(k):
            assert np.array_equal(np.asarray(back.layers[k].get_weights()[0]), np.asarray(layer.get_weights()[0])), k


def entry_call(fn, defaults):
    """call(**changes) of a C entry: defaults holds every argument in the order of the C parameters."""
    def call(**kw):
        assert set(kw) <= set(defaults), kw
        return fn(*{**defaults, **kw}.values())
    return call


def assert_status(lib, call, code, cases, text=None):
    """Every case (a dict of changed arguments) returns `code`; text: bytes gpfq_last_error() holds after each of them."""
    for kw in cases:
        assert call(**kw) == code, (kw, code)
        assert text is None or text in lib.gpfq_last_error(), (kw, lib.gpfq_last_error())

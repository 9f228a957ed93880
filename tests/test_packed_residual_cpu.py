"""No GPU: the host side of the residual join in the int8 Conv2D epilogue -- rule RES of deploy.plan_fusion
on keras_shim.ResNet50, and the new argument checks of gpfq_packed_conv2d_forward_i8_residual (before any launch: safe without a
device)."""
import ctypes

import pytest

FAKE = ctypes.c_void_p(256)          # a non-NULL, 16-byte aligned pointer that validation must never dereference


def test_plan_lists_sixteen_hosts_and_nothing_else_moves():
    from quantized_neural_networks_amd import deploy, keras_shim as ks
    net = ks.ResNet50(input_shape=(32, 32, 3), classes=10, device="cpu")
    at = [k for k, l in enumerate(net.layers) if isinstance(l, (ks.Conv2D, ks.Dense))]
    today = deploy.plan_fusion(net, at, adds=True)
    plan = deploy.plan_fusion(net, at, adds=True, residuals=True)
    hosts = {e["layer"]: e["residual"] for e in plan if e["residual"] is not None}
    assert len(hosts) == 16 and all(name.endswith("_3_conv") for name in hosts)
    assert all(add == name[:-len("3_conv")] + "add" and which == 0 for name, (add, which) in hosts.items())
    assert "conv5_block3_3_conv" in hosts and not any(e["add"] == "conv5_block3_add" for e in plan)     # (a join JOIN does not list)
    assert [{k: v for k, v in e.items() if k != "residual"} for e in plan] == today
    assert deploy.plan_fusion(net, at, adds=True, residuals=False) == today and "residual" not in today[0]
    assert list(plan[0])[-2:] == ["residual", "hands_to"]
    with pytest.raises(ValueError, match="adds=True"):
        deploy.plan_fusion(net, at, residuals=True)


def test_entry_checks_res_before_launch():
    from quantized_neural_networks_amd import build, hip
    build.build()
    lib = hip.load()
    fwd, err = lib.gpfq_packed_conv2d_forward_i8_residual, lib.gpfq_last_error
    assert len(hip.SYMBOLS["gpfq_packed_conv2d_forward_i8_residual"][1]) == 26
    # xq n ldq scales | H W Cin kh kw sh sw rh rw same | packed bits zero_code radii M bias F | y res relu amax stream: y is 2*5*5*7 floats
    call = lambda y, res, n=2: fwd(FAKE, n, 80, FAKE, 5, 5, 3, 3, 3, 1, 1, 1, 1, 1, FAKE, 2, 0, FAKE, 3, None, 7, y, res, 0, None, None)
    y = 4096
    assert call(ctypes.c_void_p(y), None) == -1 and b"NULL" in err()
    for res in (y, y + 4 * 349, y - 4 * 349):
        assert call(ctypes.c_void_p(y), ctypes.c_void_p(res)) == -1 and b"overlaps" in err(), res
    assert call(None, None, n=0) == 0                                   # nothing to do: success whatever the pointers
    assert fwd(FAKE, 2, 80, FAKE, 5, 5, 3, 3, 3, 1, 1, 1, 1, 1, FAKE, 2, 0, FAKE, 3, None, 7, FAKE, FAKE, 2, None, None) == -1 and b"relu" in err()

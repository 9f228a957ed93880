"""Self-test of tests/_layouts.py on CPU tensors: the view's values and pitch, its offset from the 16-byte grid, what bands() returns
and how much guard band there is -- the GPU layout tests (tests/test_operand_layouts_gpu.py) rest on these."""
import numpy as np
import pytest
import torch

from _layouts import bands, intact, place, slack_of

FILLS = {np.float32: float("nan"), np.float64: -7.0, np.int8: 77, np.int16: -12345}


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int8, np.int16])
@pytest.mark.parametrize("shape,ld,offset", [((5, 9), 12, 0), ((5, 9), None, 1), ((3, 8), 11, 3), ((1, 7), 7, 2), ((6, 1), 5, 1), ((4, 16), 20, 0)])
def test_place_values_pitch_offset_and_bands(dtype, shape, ld, offset):
    a = (np.arange(shape[0] * shape[1]).reshape(shape) % 100 - 50).astype(dtype)
    fill = FILLS[dtype]
    v = place(a, ld=ld, offset=offset, fill=fill, slack=64, device="cpu")
    pitch = shape[1] if ld is None else ld
    es = a.dtype.itemsize
    assert v.dtype == torch.from_numpy(a).dtype and tuple(v.shape) == shape
    assert np.array_equal(v.numpy(), a)
    assert v.stride(1) == 1 and (shape[0] == 1 or v.stride(0) == pitch)
    assert v.data_ptr() % 16 == (es * offset) % 16
    before, after = slack_of(v)
    assert before >= 64 and after >= 64
    buf = v._placed[0]
    assert buf.dim() == 1 and buf.numel() == before + shape[0] * pitch + after
    b = bands(v)
    assert b.numel() == buf.numel() - a.size                      # the pads between the rows and both guard bands, nothing of the view
    assert intact(v)
    if fill != fill:
        assert torch.isnan(b).all()
    else:
        assert (b == fill).all()
    # ... and exactly the complement of the view's elements, in order
    inside = {before + r * pitch + c for r in range(shape[0]) for c in range(shape[1])}
    outside = [i for i in range(buf.numel()) if i not in inside]
    stamped = torch.arange(buf.numel()).to(buf.dtype)              # (a copy of the allocation with every element its own position)
    v2 = torch.as_strided(stamped, v.shape, v.stride(), before)
    v2._placed = (stamped,) + v._placed[1:]
    assert torch.equal(bands(v2), stamped[outside])


def test_bands_see_a_stray_write_and_ignore_the_view():
    a = np.ones((4, 6), dtype=np.float32)
    v = place(a, ld=8, offset=1, fill=-7.0, device="cpu")
    buf, start = v._placed[0], v._placed[1]
    v[2, 3] = 5.0                                                  # inside the view: not a band
    assert intact(v)
    for at in (start - 1, start + 6, start + 7, start + 3 * 8 + 6, start + 4 * 8, 0, buf.numel() - 1):
        old = buf[at].item()
        assert old == -7.0
        buf[at] = 1.0
        assert not intact(v), at
        buf[at] = old
    assert intact(v)


def test_nan_fill_reaches_whatever_reads_a_pad():
    a = np.ones((3, 5), dtype=np.float32)
    v = place(a, ld=8, device="cpu")
    buf, start = v._placed[0], v._placed[1]
    assert torch.isnan(buf[start + 5]) and torch.isnan(buf[start - 1]) and torch.isnan(buf[start + 3 * 8])
    assert float(v.sum()) == 15.0


def test_one_dimensional_and_empty():
    r = place(np.arange(10, dtype=np.float64), offset=1, fill=-7.0, device="cpu")
    assert r.dim() == 1 and r.data_ptr() % 16 == 8 and np.array_equal(r.numpy(), np.arange(10.0))
    assert bands(r).numel() == r._placed[0].numel() - 10 and intact(r)
    q = place(np.zeros((3, 7), dtype=np.int8), offset=1, fill=77, device="cpu")
    assert q.data_ptr() % 16 == 1 and q.data_ptr() % 2 == 1
    h = place(np.zeros((3, 7), dtype=np.int16), offset=1, fill=77, device="cpu")
    assert h.data_ptr() % 16 == 2 and h.data_ptr() % 4 == 2
    e = place(np.zeros((0, 4), dtype=np.float32), device="cpu")
    assert e.numel() == 0 and intact(e)

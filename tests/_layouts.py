"""Operand layouts for the GPU tests: a matrix as a strided view inside a larger, poisoned allocation.

place() lays a 2-D (or 1-D) array out with a chosen row pitch and a chosen offset from a 16-byte boundary, inside a 1-D tensor filled
with `fill`; bands() returns everything of that tensor that is not an element of the view -- the pads between the rows and a guard band
of at least `slack` elements on either side.  A kernel that reads a pad shows it by value (NaN poison reaching a result), one that
writes outside its output by a changed sentinel -- and because the bands are live memory of the test's own, neither can fault."""
import numpy as np
import torch

_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int8: np.int8, torch.int16: np.int16}


def place(a, ld=None, offset=0, fill=float("nan"), slack=64, device="cuda"):
    """A view equal to `a` (float32 / float64 / int8 / int16, 2-D, or 1-D = one row) with row pitch `ld` elements (default: the row
    length) whose first element lies `offset` elements behind a 16-byte boundary, inside an allocation filled with `fill`; at least
    `slack` elements of `fill` in front of the first row and behind the last FULL-PITCH row."""
    a = np.asarray(a)
    one_d = a.ndim == 1
    a2 = a.reshape(1, -1) if one_d else a
    assert a2.ndim == 2
    t = torch.from_numpy(np.array(a2, order="C"))               # (a copy: read-only inputs stay as they are)
    assert t.dtype in _NP, t.dtype
    rows, cols = a2.shape
    ld = cols if ld is None else int(ld)
    assert ld >= cols and slack >= 0 and offset >= 0
    es = t.element_size()
    total = slack + 16 + rows * ld + slack
    buf = torch.empty(total, dtype=t.dtype, device=device)
    buf.fill_(fill)
    start = slack
    while (buf.data_ptr() + start * es) % 16 != (offset * es) % 16:      # (the allocation is aligned to its element at least)
        start += 1
    assert start < slack + 16
    view = torch.as_strided(buf, (rows, cols), (ld, 1), start)
    view.copy_(t)
    if one_d:
        view = view[0]
    view._placed = (buf, start, rows, cols, ld, fill)
    return view


def bands(view):
    """Every element of the allocation behind a place()d view that is not an element of the view, front to back."""
    buf, start, rows, cols, ld, _ = view._placed
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    if rows and cols:
        at = start + torch.arange(rows, device=buf.device)[:, None] * ld + torch.arange(cols, device=buf.device)[None, :]
        keep[at.reshape(-1)] = False
    return buf[keep]


def intact(view):
    """Whether bands(view) still holds the fill value everywhere (bit patterns apart, NaN counts as NaN)."""
    fill = view._placed[5]
    b = bands(view)
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(b).all())
    return bool((b == fill).all())


def slack_of(view):
    """(elements in front of the first row, elements behind the last full-pitch row)."""
    buf, start, rows, cols, ld, _ = view._placed
    return start, buf.numel() - (start + rows * ld)

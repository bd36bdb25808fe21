"""Device-side placement shared by the exact operator tests (tests/test_gpu_gemm_exact.py, tests/test_gpu_spmm_exact.py): operands
inside NaN-filled buffers, outputs inside a sentinel, and the report of the first differing elements."""
import torch

NAN = float("nan")
SLACK = 64          # elements around every operand (a multiple of 8: the alignment of the buffer carries over)
_KEEP = []          # what the running case placed on the device (the test modules release it when the case ends)


def place(t, ld, off, dtype, fill=NAN):
    """The (rows, cols) CPU matrix (or vector) inside a device buffer of `fill`: SLACK + off elements ahead of it, row pitch ld, two more
    rows and SLACK behind.  Returns (buffer, matrix view, address of the first element)."""
    t2 = t if t.dim() == 2 else t[None, :]
    rows, cols = t2.shape
    ld = cols if ld is None else ld
    buf = torch.full((SLACK + off + (rows + 2) * ld + SLACK,), fill, dtype=dtype, device="cuda")
    view = buf[SLACK + off: SLACK + off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t2.to(dtype).cuda())
    _KEEP.append(buf)
    return buf, view, buf.data_ptr() + (SLACK + off) * buf.element_size()


def mismatch(got, want, what):
    bad = (got != want).nonzero()
    rows = ["%s: %d of %d elements differ" % (what, bad.shape[0], want.numel())]
    for ix in bad[:8].tolist():
        rows.append("  %s: got %r, want %r" % (tuple(ix), got[tuple(ix)].item(), want[tuple(ix)].item()))
    return "\n".join(rows)

"""Sentinel-filled buffers for tests that hand raw pointers and strides to a kernel: every operand and result is a strided view inside
a flat allocation filled with NaN (0xA5 for bytes), and reading it back asserts that nothing outside the view was written.  Unlike
`gapped` / `check_operand` of tests/test_backward_kernels_gpu.py (2-D views, 16-byte rows) this form states base pointers that are off by
one element, row strides that are no multiple of 8, batch strides, piece planes and uint8 payloads, which the forward GEMM descriptors need.
All views are in bounds."""
import torch

NAN = float("nan")


class Buf:
    """A matrix [batch][rows][cols] (of `planes` pieces) as a strided view inside a flat sentinel-filled buffer: element (z, r, c) of piece
    p at front + off + z sb + r ld + p (ld / planes) + c.  `front` is a multiple of 128 elements, so `off` alone decides the alignment
    of the base pointer.  read() returns the pieces and asserts that everything else still holds the sentinel."""
    FRONT = 256

    def __init__(self, batch, rows, cols, ld, dtype, *, off=0, planes=1, sb=0, tail_rows=2):
        self.shape, self.ld, self.off, self.planes, self.sb, self.dtype = (batch, rows, cols), ld, off, planes, sb, dtype
        self.ps = ld // planes
        extent = off + (batch - 1) * sb + (rows - 1) * ld + (planes - 1) * self.ps + cols
        self.fill = 0xA5 if dtype == torch.uint8 else NAN
        self.cpu = torch.full((self.FRONT + extent + tail_rows * ld + 8,), self.fill, dtype=dtype)
        self.dev = None

    def view(self, flat, p=0):
        b, r, c = self.shape
        return torch.as_strided(flat, (b, r, c), (self.sb, self.ld, 1), self.FRONT + self.off + p * self.ps)

    def put(self, pieces, dev):
        for p, piece in enumerate(pieces):
            self.view(self.cpu, p).copy_(piece.to(self.dtype))
        self.dev = self.cpu.to(dev)
        return self

    def blank(self, dev):
        self.dev = self.cpu.to(dev)
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + (self.FRONT + self.off) * self.dev.element_size()

    def read(self, name):
        flat = self.dev.cpu()
        pieces = [self.view(flat, p).clone() for p in range(self.planes)]
        for p in range(self.planes):
            self.view(flat, p).fill_(self.fill)
        clean = bool((flat == 0xA5).all()) if self.dtype == torch.uint8 else bool(torch.isnan(flat.float()).all())
        assert clean, f"{name}: elements outside the view (gap columns / guard rows) were written"
        return pieces

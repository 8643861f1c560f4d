"""Sentinel-filled buffers for tests that hand raw pointers and strides to a kernel: every operand and result is a strided view inside
a flat allocation filled with NaN (0xA5 for bytes), and reading it back asserts that nothing outside the view was written.  Unlike
`gapped` / `check_operand` of tests/test_backward_kernels_gpu.py (2-D views, 16-byte rows) this form states base pointers that are off by
one element, row strides that are no multiple of 8, batch strides, piece planes and uint8 payloads, which the forward GEMM descriptors need.
All views are in bounds.  `Flat` is the one-dimensional sibling for the scene kernels: int64, int32, float32 and uint8 payloads inside
an integer sentinel, compared byte for byte."""
import torch

NAN = float("nan")
BYTE = 0xA5                                            # the sentinel byte: as a word neither 0, -1, a key of a small cloud nor a 24-bit colour


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


class Flat:
    """`n` contiguous elements of int64, int32, float32 or uint8 inside a flat sentinel-filled allocation, `off` elements past a front of
    FRONT elements (so `off` alone decides the alignment of the base pointer).  The sentinel is the byte 0xA5 repeated (BYTE), an integer
    pattern that is neither an empty splat key (-1), a key of a small cloud nor a 24-bit colour; nan=True (float32 operands that a kernel
    only reads) fills with NaN instead, so that a read of the padding shows in the result.  Everything is compared as bytes: read()
    returns the view and asserts that every byte outside it still holds the sentinel, unchanged() that nothing at all was written.
    fill=value (an element of `dtype`) is for an operand whose rule would ignore both sentinels (a label that is negative, a depth that
    is not a number): the padding holds a value the rule counts, so that a read of it changes the result; it is compared like the others."""
    FRONT, TAIL = 256, 264

    def __init__(self, n, dtype, *, off=0, nan=False, fill=None):
        assert dtype in (torch.int64, torch.int32, torch.float32, torch.uint8) and not (nan and dtype != torch.float32)
        assert fill is None or not nan
        self.n, self.dtype, self.off = int(n), dtype, int(off)
        total = self.FRONT + self.off + self.n + self.TAIL
        if nan:
            self.cpu = torch.full((total,), NAN, dtype=dtype)
        elif fill is not None:
            self.cpu = torch.full((total,), fill, dtype=dtype)
        else:
            self.cpu = torch.full((total * torch.empty((), dtype=dtype).element_size(),), BYTE, dtype=torch.uint8).view(dtype)
        self.sentinel = self.cpu.clone()
        self.dev = None

    def view(self, flat):
        return flat[self.FRONT + self.off:self.FRONT + self.off + self.n]

    def put(self, payload, dev):
        payload = torch.as_tensor(payload).reshape(-1)
        assert payload.dtype == self.dtype and payload.numel() == self.n, (payload.dtype, payload.numel(), self.dtype, self.n)
        self.view(self.cpu).copy_(payload)
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
        got = self.view(flat).clone()
        self.view(flat).copy_(self.view(self.sentinel))
        assert torch.equal(flat.view(torch.uint8), self.sentinel.view(torch.uint8)), f"{name}: elements outside the view were written"
        return got

    def unchanged(self, name):
        assert torch.equal(self.dev.cpu().view(torch.uint8), self.cpu.view(torch.uint8)), f"{name}: was written"

"""Guarded device arrays: typed views of exactly the documented length into one torch.uint8 buffer, each on a 256-byte
boundary with a guard band on both sides.  Plain torch; nothing here imports the package.

Why: the parity tests compare the bytes an array is documented to have.  A kernel that writes one row past n, or reads
past the end of an input and lets the value steer a result, is invisible to them when the neighbouring bytes belong to
another tensor.  Here the neighbouring bytes are guards with a known fill: a stray write damages a guard (`damaged`), a
stray read changes an output when the fill changes (`refill`: the same call run under fill A and fill B must return the
same bytes).

The guard of an array is max(4096, its byte length rounded up to 4096) wide on each side, so that a capacity-for-count
mistake or a doubled stride still lands inside it.  Fills per kind of array (A, B):
    "float"  f32 / f64 values and coordinates             bytes 0xFF (NaN)   7.0
    "byte"   u8 flags, masks, images, descriptors         0x00               0xFF
    "index"  i32 / i64 indices, counts, orders, hints     0                  1
The integer fills are legal small values on purpose: a guard read through as an index or a loop bound must show up as a
wrong byte or a damaged guard, never as a wild address."""
import numpy as np
import torch

ALIGN, PAGE = 256, 4096
KINDS = ("float", "byte", "index")


def guard_width(nbytes):
    return max(PAGE, (int(nbytes) + PAGE - 1) // PAGE * PAGE)


def image_length(width, height, step):
    """Documented byte length of an image of rows `step` bytes apart: the last row ends with its last pixel."""
    return (int(height) - 1) * int(step) + int(width) if height > 0 and width > 0 else 0


def fill_bytes(kind, which, dtype, nbytes, device="cpu"):
    """`nbytes` bytes of fill `which` ("A" / "B") of `kind` for elements of `dtype`, as a uint8 tensor."""
    assert kind in KINDS and which in ("A", "B")
    size = torch.empty(0, dtype=dtype).element_size()
    assert nbytes % size == 0
    if kind == "float":
        assert dtype in (torch.float32, torch.float64)
        if which == "A":
            return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=device)
        return torch.full((nbytes // size,), 7.0, dtype=dtype, device=device).view(torch.uint8)
    if kind == "byte":
        assert dtype == torch.uint8
        return torch.full((nbytes,), 0x00 if which == "A" else 0xFF, dtype=torch.uint8, device=device)
    assert dtype in (torch.int32, torch.int64)
    return torch.full((nbytes // size,), 0 if which == "A" else 1, dtype=dtype, device=device).view(torch.uint8)


def _torch_dtype(a):
    return {"float32": torch.float32, "float64": torch.float64, "uint8": torch.uint8, "int32": torch.int32,
            "int64": torch.int64}[str(a.dtype)]


class _Entry:
    __slots__ = ("name", "role", "dtype", "shape", "kind", "off", "nbytes", "guard", "pad", "initial")


class Arena:
    """arena.inp / out / inout hand out the views; see the module text.  `capacity`: bytes of the one buffer."""

    def __init__(self, device, capacity=1 << 24, which="A"):
        self.device = torch.device(device)
        self.raw = torch.zeros(capacity + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.raw.data_ptr()) % ALIGN
        self.capacity, self.cursor, self.which = capacity, 0, which
        self.entries = {}

    # ---- allocation ------------------------------------------------------------------------------------------------------
    def _bytes(self, lo, hi):
        return self.raw[self.base + lo:self.base + hi]

    def _place(self, name, role, dtype, shape, kind, pad=None):
        assert name not in self.entries, name
        e = _Entry()
        e.name, e.role, e.dtype, e.kind = name, role, dtype, kind
        e.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        e.nbytes = int(np.prod(e.shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        e.guard = guard_width(e.nbytes)
        e.off = self.cursor + e.guard                      # cursor and guard are multiples of ALIGN
        end = e.off + e.nbytes + e.guard
        assert end <= self.capacity, "arena exhausted"
        self.cursor = (end + ALIGN - 1) // ALIGN * ALIGN
        e.pad = None if pad is None else torch.as_tensor(pad, dtype=torch.bool).reshape(-1).to(self.device)
        assert e.pad is None or (e.pad.numel() == e.nbytes and dtype == torch.uint8)
        e.initial = None
        self.entries[name] = e
        return e

    def view(self, name):
        e = self.entries[name]
        v = self._bytes(e.off, e.off + e.nbytes).view(e.dtype).view(e.shape)
        assert v.data_ptr() % ALIGN == 0 or e.nbytes == 0
        return v

    def arg(self, name):
        """What to pass to a call: the view -- or, for an array of no elements (torch gives an empty tensor no address), one
        guard byte at the array's address.  Only its data_ptr() is meant to be used."""
        e = self.entries[name]
        return self.view(name) if e.nbytes else self._bytes(e.off, e.off + 1)

    def _fill_guards(self, e, which):
        for lo in (e.off - e.guard, e.off + e.nbytes):
            self._bytes(lo, lo + e.guard).copy_(fill_bytes(e.kind, which, e.dtype, e.guard, self.device))
        if e.pad is not None:
            self._bytes(e.off, e.off + e.nbytes)[e.pad] = 0x00 if which == "A" else 0xFF

    def _fill_payload(self, e, which):
        self._bytes(e.off, e.off + e.nbytes).copy_(fill_bytes(e.kind, which, e.dtype, e.nbytes, self.device))

    def _copy_in(self, e, array):
        t = torch.from_numpy(np.array(array, copy=True, order="C")).to(e.dtype).reshape(-1)   # (a copy: shared inputs are read-only)
        assert t.numel() * t.element_size() == e.nbytes, f"{e.name}: payload is not the documented length"
        raw = t.view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8)   # (an empty tensor has no stride to view)
        e.initial = raw.to(self.device).clone()
        self._bytes(e.off, e.off + e.nbytes).copy_(e.initial)

    def inp(self, name, array, fill, dtype=None):
        """An input: the payload copied in, both guards filled."""
        a = np.ascontiguousarray(array)
        dtype = dtype or _torch_dtype(a)
        e = self._place(name, "in", dtype, a.shape, fill)
        self._copy_in(e, a)
        self._fill_guards(e, self.which)
        return self.view(name)

    def out(self, name, dtype, shape, fill):
        """An output: payload and both guards filled; the payload fill is the sentinel of rows left untouched."""
        e = self._place(name, "out", dtype, shape, fill)
        self._fill_payload(e, self.which)
        self._fill_guards(e, self.which)
        return self.view(name)

    def inout(self, name, array, fill, dtype=None):
        a = np.ascontiguousarray(array)
        dtype = dtype or _torch_dtype(a)
        e = self._place(name, "inout", dtype, a.shape, fill)
        self._copy_in(e, a)
        self._fill_guards(e, self.which)
        return self.view(name)

    def image(self, name, img, step, role="in"):
        """An image of rows `step` bytes apart as one array of image_length bytes: the row padding counts as guard (it takes
        the guard fill and is checked and refilled with the guards).  Returns the flat view; its data_ptr is the image."""
        img = np.ascontiguousarray(img, np.uint8)
        height, width = img.shape
        assert step >= width
        n = image_length(width, height, step)
        flat = np.zeros(n, np.uint8)
        pad = np.ones(n, bool)
        for r in range(height):
            flat[r * step:r * step + width] = img[r]
            pad[r * step:r * step + width] = False
        e = self._place(name, role, torch.uint8, (n,), "byte", pad=pad)
        self._copy_in(e, flat)
        self._fill_guards(e, self.which)
        return self.view(name)

    # ---- the checks ------------------------------------------------------------------------------------------------------
    def sentinel(self, name, which=None):
        """The payload an untouched output `name` holds, as a numpy array of its shape."""
        e = self.entries[name]
        b = fill_bytes(e.kind, which or self.which, e.dtype, e.nbytes)
        return b.view(e.dtype).view(e.shape).numpy().copy()

    def payload(self, name):
        """Copy of the payload on the host (numpy, the array's dtype and shape)."""
        return self.view(name).cpu().numpy().copy()

    def damaged(self):
        """{name: byte offsets relative to the array at which a guard (or an image's row padding) no longer holds its fill}:
        negative in front of the array, >= its length behind it.  Empty when every guard is intact."""
        bad = {}
        for e in self.entries.values():
            offs = []
            for lo in (e.off - e.guard, e.off + e.nbytes):
                ne = self._bytes(lo, lo + e.guard) != fill_bytes(e.kind, self.which, e.dtype, e.guard, self.device)
                if bool(ne.any()):
                    offs += (torch.nonzero(ne).reshape(-1).cpu().numpy() + (lo - e.off)).tolist()
            if e.pad is not None:
                ne = e.pad & (self._bytes(e.off, e.off + e.nbytes) != (0x00 if self.which == "A" else 0xFF))
                if bool(ne.any()):
                    offs += torch.nonzero(ne).reshape(-1).cpu().numpy().tolist()
            if offs:
                bad[e.name] = sorted(offs)
        return bad

    def inputs_unchanged(self):
        """Names of the inputs whose payload is no longer what was copied in (row padding aside)."""
        changed = []
        for e in self.entries.values():
            if e.role != "in":
                continue
            ne = self._bytes(e.off, e.off + e.nbytes) != e.initial
            if e.pad is not None:
                ne = ne & ~e.pad
            if bool(ne.any()):
                changed.append(e.name)
        return changed

    def refill(self, which):
        """Rewrite the guards of all inputs (every array's, so that `damaged` has one fill to compare with) with fill
        `which` of their kind; payloads of inputs stay.  Follow it with reset_outputs before the next run."""
        assert which in ("A", "B")
        self.which = which
        for e in self.entries.values():
            self._fill_guards(e, which)

    def reset_outputs(self):
        """Outputs back to the sentinel of the current fill, in/out arrays back to what was copied in."""
        for e in self.entries.values():
            if e.role == "out":
                self._fill_payload(e, self.which)
            elif e.role == "inout":
                self._bytes(e.off, e.off + e.nbytes).copy_(e.initial)
            if e.role != "in" and e.pad is not None:
                self._fill_guards(e, self.which)

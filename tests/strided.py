"""Framed buffers: operands and outputs with a leading dimension, guard rows and a sentinel around them.

A frame is one allocation of `offset + (guard + rows + guard) x ld` elements.  The logical rows x width window sits at row `guard`,
column 0 of the [guard + rows + guard][ld] matrix that starts `offset` elements into the allocation (offset > 0: a base pointer
that is only element-aligned).  Everything that is not window holds a sentinel:

    float32   a quiet NaN with the payload 0x5A5A5 (0x7FC5A5A5), compared as uint32
    bf16      the quiet NaN 0x7FC5, compared as uint16
    int32     the pattern 0x5AC3A53C, compared as uint32

so a pad value that leaks into a result shows as a NaN (of THIS payload where it was copied, of any payload where it went
through arithmetic -- has_nan() catches both), and a store outside the window shows as a changed bit pattern.  The guards
are at least GUARD = 256 rows, the tallest tile of any kernel: a kernel that over-reads or over-writes a whole tile past the
last row or column still stays inside memory the test owns.

The layout, window() and assert_untouched() work on any flat array of the frame's size (tests/test_strided_frames.py proves on host
arrays that the check fires); upload() / download() move the same image through the binding's DeviceArray, and .ptr / .ld are
what a C-ABI call needs of the window.  The module itself is what the binding's op wrappers take as `frames`: they place every
operand with framed() and every output with out_frame() (tests/test_gpu_strides.py).
"""
import numpy as np

GUARD = 256

SENTINEL = {np.dtype(np.float32): np.uint32(0x7FC5A5A5), np.dtype(np.uint16): np.uint16(0x7FC5),
            np.dtype(np.int32): np.uint32(0x5AC3A53C)}
_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.uint16): np.uint16, np.dtype(np.int32): np.uint32}


def as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_BITS[a.dtype])


def has_sentinel(a):
    """Does `a` hold the sentinel of its type, bit for bit?"""
    return bool((as_bits(a) == SENTINEL[np.asarray(a).dtype]).any())


def has_nan(a):
    """Any NaN at all (float32, or bf16 bit patterns as uint16)?"""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return bool((((a & 0x7F80) == 0x7F80) & ((a & 0x007F) != 0)).any())
    return bool(np.isnan(a).any())


class Frame:
    def __init__(self, rows, width, ld=None, dtype=np.float32, guard=GUARD, offset=0):
        self.rows, self.width = int(rows), int(width)
        self.ld = self.width if ld is None else int(ld)
        self.dtype = np.dtype(dtype)
        self.guard, self.offset = int(guard), int(offset)
        assert self.rows >= 1 and self.width >= 1 and self.ld >= self.width and self.guard >= GUARD and self.offset >= 0
        self.shape = (self.rows, self.width)
        self.total_rows = self.rows + 2 * self.guard
        self.size = self.offset + self.total_rows * self.ld   # elements of the allocation
        self.dev = None

    # ---- the layout, on any flat array of self.size elements --------------------------------------------------------------
    def image(self, data=None):
        """The flat bit image of the frame: sentinel everywhere, `data` (rows x width) in the window."""
        bits = np.full(self.size, SENTINEL[self.dtype], _BITS[self.dtype])
        if data is not None:
            data = np.ascontiguousarray(data, self.dtype).reshape(self.rows, self.width)
            self._matrix(bits)[self.guard:self.guard + self.rows, :self.width] = as_bits(data)
        return bits

    def _matrix(self, arr):
        arr = np.asarray(arr)
        assert arr.shape == (self.size,) and arr.dtype.itemsize == self.dtype.itemsize, (arr.shape, arr.dtype)
        return arr.view(_BITS[self.dtype])[self.offset:].reshape(self.total_rows, self.ld)

    def window(self, arr=None):
        """The logical rows x width result (a copy, in the frame's dtype)."""
        m = self._matrix(self.download() if arr is None else arr)
        return m[self.guard:self.guard + self.rows, :self.width].copy().view(self.dtype)

    def assert_untouched(self, arr=None):
        """Every element outside the window still holds the sentinel, bit for bit; names the first (row, column) that does not
        (window coordinates: guard rows before the window are negative rows, pad columns are columns >= width; the elements
        in front of an offset base are reported as row None)."""
        arr = self.download() if arr is None else arr
        bits = np.asarray(arr).view(_BITS[self.dtype])
        s = SENTINEL[self.dtype]
        head = np.flatnonzero(bits[:self.offset] != s)
        if head.size:
            raise AssertionError(f"frame touched in front of its base: element {int(head[0])} of {self.offset} "
                                 f"(row None, column {int(head[0])}) holds {int(bits[head[0]]):#x}")
        bad = self._matrix(arr) != s
        bad[self.guard:self.guard + self.rows, :self.width] = False
        if bad.any():
            r, c = np.argwhere(bad)[0]
            raise AssertionError(f"frame touched outside its {self.rows} x {self.width} window (ld {self.ld}): (row {int(r) - self.guard}, "
                                 f"column {int(c)}) holds {int(self._matrix(arr)[r, c]):#x}, {int(bad.sum())} elements changed")

    # ---- the device side --------------------------------------------------------------------------------------------------
    def upload(self, data=None):
        from vit_amd import binding as B
        self.dev = B.DeviceArray.from_numpy(self.image(data))
        return self

    @property
    def ptr(self):
        """Device address of the window's element (0, 0)."""
        return self.dev.ptr + (self.offset + self.guard * self.ld) * self.dtype.itemsize

    def download(self):
        return self.dev.numpy()

    def check(self):
        """assert_untouched() and a window free of the sentinel and of any other NaN, from one download; returns the window."""
        arr = self.download()
        self.assert_untouched(arr)
        w = self.window(arr)
        assert not has_sentinel(w), "the window holds the sentinel: an element was not written, or a pad value was copied into it"
        assert self.dtype == np.int32 or not has_nan(w), "the window holds a NaN: a pad value went through the arithmetic"
        return w


def framed(data, ld=None, dtype=None, offset=0):
    """An input frame holding `data` ([rows][width], or [n] as one row) on the device."""
    data = np.asarray(data)
    d2 = data.reshape(1, -1) if data.ndim == 1 else data.reshape(data.shape[0], -1)
    return Frame(d2.shape[0], d2.shape[1], ld, dtype or data.dtype, offset=offset).upload(d2)


def out_frame(rows, width, ld=None, dtype=np.float32, offset=0, preload=None):
    """An output frame on the device: sentinel everywhere (the window too), or `preload` in the window (in-place operands)."""
    return Frame(rows, width, ld, dtype, offset=offset).upload(preload)

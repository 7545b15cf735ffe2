"""Device memory for the tests of the device-pointer entry points (test infrastructure, no torch needed).

`Hip` is hipMalloc / hipMemcpy / hipFree through ctypes on the HIP runtime the library itself uses.  `guarded` /
`guarded_up` place every buffer a `_dev` entry point reads or writes BETWEEN two margins of PAD doubles inside one
allocation, the whole allocation pre-filled with one quiet-NaN bit pattern:

- a store a few elements past the end of an output (the last ragged tile) lands in a margin and `margins_intact` sees it;
- a read past the end of an input returns the NaN, which shows in the result it reaches;
- an output element the library never writes still holds the pattern.

PAD is one full 128 x 128 tile: no tile-granular access of the library steps further, so every access of a correct or a
slightly wrong kernel stays inside the test's own allocation.  Nothing here relies on a fault; no buffer sits at the edge
of an allocation.  The pattern is written and compared as uint64, never through a float comparison (NaN != NaN)."""
import ctypes as C

import numpy as np

PAD = 16384                                       # doubles per margin: one 128 x 128 tile
SENTINEL = np.uint64(0x7FF8C0DEC0DE5EED)          # a quiet NaN with a payload no computation produces

H2D, D2H, D2D = 1, 2, 3


class Hip:
    """hipMalloc / hipMemcpy through ctypes on the HIP runtime the library itself uses (no torch needed)."""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so.7")      # already loaded by libgpslc_hip.so: same instance
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.bufs = []

    def up(self, x):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, order="F"))
        p = self.empty(x.size)
        assert self.rt.hipMemcpy(p, x.ctypes.data_as(C.c_void_p), x.nbytes, H2D) == 0
        return p

    def empty(self, count):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), 8 * count) == 0
        self.bufs.append(p)
        return p

    def down(self, p, count):
        out = np.empty(count)
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, 8 * count, D2H) == 0
        return out

    def put_bits(self, p, words):
        """the uint64 words `words` to device address p"""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.size:
            assert self.rt.hipMemcpy(p, w.ctypes.data_as(C.c_void_p), w.nbytes, H2D) == 0

    def get_bits(self, p, count):
        out = np.empty(count, dtype=np.uint64)
        if count:
            assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, 8 * count, D2H) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.rt.hipFree(p)
        self.bufs = []


class Guarded:
    """One allocation of count + 2 PAD doubles; `ptr` is the interior (base + 8 PAD bytes), `bits` what was uploaded there."""

    def __init__(self, base, count, bits):
        self.base, self.count, self.bits = base, int(count), bits
        self.ptr = C.c_void_p(base.value + 8 * PAD)

    def at(self, offset):
        """device address of interior element `offset`"""
        assert 0 <= offset < max(self.count, 1)
        return C.c_void_p(self.ptr.value + 8 * int(offset))


_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = Hip()
    return _hip


def _bits(array):
    a = np.ascontiguousarray(np.asarray(array, dtype=np.float64).reshape(-1, order="F"))
    return a.view(np.uint64)


def _alloc(interior_bits):
    count = interior_bits.size
    img = np.full(count + 2 * PAD, SENTINEL, dtype=np.uint64)
    img[PAD:PAD + count] = interior_bits
    base = hip().empty(count + 2 * PAD)
    hip().put_bits(base, img)
    return Guarded(base, count, interior_bits.copy())


def guarded(count):
    """`count` doubles between two margins, everything (interior included) holding SENTINEL"""
    return _alloc(np.full(int(count), SENTINEL, dtype=np.uint64))


def guarded_up(array):
    """the array, column-major, between two SENTINEL margins"""
    return _alloc(_bits(array))


def margins_intact(buf):
    """both margins bit for bit what was written"""
    lo = hip().get_bits(buf.base, PAD)
    hi = hip().get_bits(C.c_void_p(buf.ptr.value + 8 * buf.count), PAD)
    return bool(np.all(lo == SENTINEL) and np.all(hi == SENTINEL))


def interior_bits(buf):
    return hip().get_bits(buf.ptr, buf.count)


def interior(buf):
    """the payload as doubles (flat, column-major order)"""
    return interior_bits(buf).view(np.float64)


def untouched(buf):
    """interior and margins bit-identical to what was uploaded (an input the library must not write; an output of a refused
    or empty call)"""
    return margins_intact(buf) and bool(np.array_equal(interior_bits(buf), buf.bits))


def overwrite(buf, array=None):
    """replace the interior: with the array, or (None) with SENTINEL everywhere"""
    bits = np.full(buf.count, SENTINEL, dtype=np.uint64) if array is None else _bits(array)
    assert bits.size == buf.count
    hip().put_bits(buf.ptr, bits)
    buf.bits = bits.copy()


def release():
    """free every buffer handed out so far"""
    if _hip is not None:
        _hip.free()

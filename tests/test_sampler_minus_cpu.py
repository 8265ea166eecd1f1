"""The float32 facts the clamp-free sample5 (csrc/pagk_device.h) rests on, swept in numpy float32.

For 1 <= X the minus-side coordinate X - 1.0f is exact, so its integer part is int(X) - 1 and its fraction and weight are
those of X: the device sampler takes the minus-side taps from the centre's quad index and the centre's fractions and
prepares no coordinate for them.  The plus side is NOT of that kind -- X + 1.0f rounds where it crosses the top of a
binade -- and the second test holds that open: whoever "finishes the job" on the plus side fails it."""
import numpy as np

F = np.float32
ONE = F(1)


def _floats(lo_bits, hi_bits, chunk=1 << 22):
    """Every float32 whose bit pattern lies in [lo_bits, hi_bits), in chunks."""
    for b in range(lo_bits, hi_bits, chunk):
        yield np.arange(b, min(b + chunk, hi_bits), dtype=np.uint32).view(F)


def _bits(v):
    return int(np.array(v, F).view(np.uint32))


def _below_binade_tops(count=4096, top=8192):
    """The `count` floats below each of 2, 4, ..., top."""
    k = 2
    while k <= top:
        b = _bits(k)
        yield np.arange(b - count, b, dtype=np.uint32).view(F)
        k *= 2


def _parts(x):
    """int(x), xx = x - floor(x) and 1 - xx as the sampler forms them (x >= 0)."""
    f = x - np.floor(x)
    return x.astype(np.int64), f, ONE - f


def _sweep():
    yield from _floats(_bits(1), _bits(2048))
    yield from _below_binade_tops()


def test_minus_side_is_the_centre_shifted_by_one_quad():
    n = 0
    for x in _sweep():
        i, f, w = _parts(x)
        im, fm, wm = _parts(x - ONE)
        assert np.array_equal(im, i - 1), "int(X - 1) != int(X) - 1"
        assert np.array_equal(fm.view(np.uint32), f.view(np.uint32)), "fract(X - 1) != fract(X)"
        assert np.array_equal(wm.view(np.uint32), w.view(np.uint32)), "1 - fract(X - 1) != 1 - fract(X)"
        n += x.size
    assert n == _bits(2048) - _bits(1) + 13 * 4096


def test_plus_side_is_not():
    bad = two = 0
    for x in _below_binade_tops():
        i, f, _ = _parts(x)
        ip, fp, _ = _parts(x + ONE)
        bad += int(((ip != i + 1) | (fp.view(np.uint32) != f.view(np.uint32))).sum())
        two += int((ip == i + 2).sum())
    assert bad > 0, "X + 1.0f behaved exactly on every float below a binade top: the sweep is not testing anything"
    assert two > 0, "no X with int(X + 1) == int(X) + 2 found"

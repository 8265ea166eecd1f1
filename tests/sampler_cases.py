"""Images, coordinates and the numpy model of the sampler tests (test_sampler_cpu.py, test_sampler_gpu.py).

The sampler is PatchMatch::GetPixelValue (reference src/patch_match.cpp:391-406): the one routine under every tracking
variant and under the oracle's track.  Everything here runs on the CPU and imports neither the oracle nor the package."""
import functools

import numpy as np

F = np.float32


def _random(rows, cols, seed):
    # 1..255: a tap that wrongly reads a "0 by definition" byte (padding, past the end) never equals the right one
    return np.random.default_rng(seed).integers(1, 256, (rows, cols), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def images():
    """{name: image}: 13 x 7, 2 x 1, 1 x 1 (continuous) and a 13 x 7 view of a buffer with 16 bytes per row whose three
    padding bytes per row are 0xEE.  The view shows the same pixels as the continuous 13 x 7 image."""
    base = _random(7, 13, 0x5A3)
    buf = np.full((7, 16), 0xEE, np.uint8)
    buf[:, :13] = base
    out = {"13x7": base, "2x1": _random(1, 2, 0x5A4), "1x1": _random(1, 1, 0x5A5), "13x7-stride16": buf[:, :13]}
    for a in out.values():
        a.setflags(write=False)
    return out


# frames whose levels 0..L-1 the device test samples: (width, height, levels, (rows, cols) of the top level)
PYRAMIDS = ((52, 28, 3, (7, 13)),    # even parents: the single-launch pyramid packs the taps; 13 x 7 at the top
            (52, 28, 4, (3, 6)),     # ... one level more: the 13 x 7 level is an odd parent, every level is built on its own
            (27, 15, 3, (3, 6)),     # every parent odd: the fixed-point resize; 13 x 7, 6 x 3
            (64, 64, 7, (1, 1)))     # more than four levels; 2 x 2 and 1 x 1 at the top


def frame(width, height):
    return _random(height, width, 0x5B0 + width)


def _neighbours(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def axis(size):
    """The coordinates of one axis of a level `size` pixels long: every multiple of 0.25 in [-2, size + 2]; 0, size - 1,
    size and every integer position with both float neighbours; -0.0, NaN, +-inf, +-1e30."""
    vals = [F(k) * F(0.25) for k in range(-8, 4 * (size + 2) + 1)]
    for v in sorted({0, size - 1, size, *range(size)}):
        vals += _neighbours(v)
    vals += [F(-0.0), F(np.nan), F(np.inf), F(-np.inf), F(1e30), F(-1e30)]
    return np.array(vals, F)


def coordinates(cols, rows):
    """n x 2 float32: the Cartesian product of the two axes' coordinates."""
    xs, ys = axis(cols), axis(rows)
    xy = np.empty((xs.size * ys.size, 2), F)
    xy[:, 0] = np.repeat(xs, ys.size)
    xy[:, 1] = np.tile(ys, xs.size)
    return xy


def five(xy):
    """The coordinates of the five samples of one Gauss-Newton pixel (src/patch_match.cpp:252,259-262), n x 5 x 2: centre,
    x + 1, x - 1, y + 1, y - 1, the +-1 formed in float32."""
    x, y, one = xy[:, 0], xy[:, 1], F(1)
    with np.errstate(invalid="ignore"):
        return np.stack([np.stack([x, y], 1), np.stack([x + one, y], 1), np.stack([x - one, y], 1),
                         np.stack([x, y + one], 1), np.stack([x, y - one], 1)], 1).astype(F)


def inside(xy, cols, rows, margin):
    """Rows of xy inside the domain pagk_selftest_sample validates for its clamp-free modes: margin 0 for one sample
    ([0, cols - 1) x [0, rows - 1)), 1 for the five ([1, cols - 2) x [1, rows - 2))."""
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        return (x >= margin) & (x < cols - 1 - margin) & (y >= margin) & (y < rows - 1 - margin)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def model(img, xy):
    """GetPixelValue (src/patch_match.cpp:391-406) in numpy float32, line by line, on the flat buffer behind `img`
    (img.strides[0] bytes per row).  What the reference leaves open is as oracle/README.md defines it: bytes past the end
    of the buffer and row-padding bytes read as 0, a NaN coordinate is 0."""
    rows, cols = img.shape
    step = img.strides[0]
    # the buffer as the sampler sees it: rows * step bytes, padding zeroed, and zeros behind the end (the farthest tap is
    # data[step + 1] of the last pixel)
    flat = np.zeros(rows * step + step + 2, np.uint8)
    flat[:rows * step].reshape(rows, step)[:, :cols] = img
    x, y = xy[:, 0].astype(F), xy[:, 1].astype(F)
    x = np.where(np.isnan(x), F(0), x)
    y = np.where(np.isnan(y), F(0), y)
    x = np.where(x < 0, F(0), x)                    # :394  if (x < 0) x = 0;
    y = np.where(y < 0, F(0), y)                    # :395
    x = np.where(x >= F(cols), F(cols - 1), x)      # :396  if (x >= img.cols) x = img.cols - 1;
    y = np.where(y >= F(rows), F(rows - 1), y)      # :397
    off = y.astype(np.int64) * step + x.astype(np.int64)   # :399  &img.data[int(y) * img.step + int(x)]
    xx, yy = x - np.floor(x), y - np.floor(y)       # :400
    a, b = F(1) - xx, F(1) - yy                     # :401
    d0, d1 = flat[off].astype(F), flat[off + 1].astype(F)
    d2, d3 = flat[off + step].astype(F), flat[off + step + 1].astype(F)
    return b * (a * d0 + xx * d1) + yy * (a * d2 + xx * d3)   # :402-403

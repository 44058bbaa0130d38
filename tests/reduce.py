"""The box mean of reduced outputs (csrc/reduce_rule.h) restated in numpy float32, and the
cases the host and the device statements of the rule are checked on.

Output pixel (ox, oy) at factor k covers x in [k ox, min(k ox + k, W)), y in [k oy, min(k oy +
k, H)). Per channel: s = 0; for y, then x, ascending: s = float32(s + in[y][x]); the result is
float32(s / float32(count)), count the pixels in the block. Every step below is one float32
operation on whole planes, in that order, so the bits are the rule's."""
import numpy as np

FACTORS = (2, 4, 8)
# 1x1; partial blocks on both edges; full blocks only; one edge partial at 8; both edges partial
SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (19, 13)]
GPU_SIZES = SIZES + [(130, 67)]  # reduced widths 65, 33, 17: a row of more than one wave at factor 2, odd edges


def reduced_shape(h, w, k):
    return -(-h // k), -(-w // k)


def reduce(img, k):
    """(H, W, 4) float32 -> (ceil(H / k), ceil(W / k), 4) float32 by the rule."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape[:2]
    oh, ow = reduced_shape(h, w, k)
    acc = np.zeros((oh, ow, 4), np.float32)
    count = np.zeros((oh, ow), np.float32)
    for dy in range(k):          # a block's rows, top to bottom
        for dx in range(k):      # a row's pixels, left to right
            sub = img[dy::k, dx::k]  # the blocks that have this pixel
            sh, sw = sub.shape[:2]
            acc[:sh, :sw] = acc[:sh, :sw] + sub  # float32 + float32 -> float32, round to nearest
            count[:sh, :sw] += np.float32(1.0)
    assert acc.dtype == np.float32 and np.all(count >= 1)
    return (acc / count[..., None]).astype(np.float32)


def reduce_scalar(img, k):
    """The same, one pixel at a time as the rule is written (slow: for small images)."""
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]
    oh, ow = reduced_shape(h, w, k)
    out = np.zeros((oh, ow, 4), np.float32)
    for oy in range(oh):
        for ox in range(ow):
            s = np.zeros(4, np.float32)
            n = 0
            for y in range(k * oy, min(k * oy + k, h)):
                for x in range(k * ox, min(k * ox + k, w)):
                    s = (s + img[y, x]).astype(np.float32)
                    n += 1
            out[oy, ox] = s / np.float32(n)
    return out


def images(w, h, seed=0):
    """name -> (h, w, 4) float32: random values of both signs, values near the largest half
    (sums of 64 of them stay far below float32's range), a constant image, and small values
    beside large ones, where the order of the sum shows."""
    rng = np.random.default_rng(1000 * w + h + seed)
    out = {
        "noise": rng.standard_normal((h, w, 4)).astype(np.float32) * np.float32(3.0),
        "near_half_max": (65504.0 - rng.random((h, w, 4)) * 64.0).astype(np.float32)
        * rng.choice(np.array([-1.0, 1.0], np.float32), (h, w, 4)),
        "constant": np.full((h, w, 4), np.float32(0.1), np.float32),
        "mixed": (rng.standard_normal((h, w, 4)) * 10.0 ** rng.integers(-6, 7, (h, w, 4))).astype(np.float32),
    }
    return out

"""k_film_reduce on the device (rr_debug_film_reduce with a context) against the numpy
restatement of csrc/reduce_rule.h (tests/reduce.py): bit for bit, at every factor, on the
sizes with full blocks only, partial blocks on one edge and on both, a single pixel, and an
image whose reduced rows take more than one wave."""
import numpy as np
import pytest

import reduce as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", R.FACTORS)
@pytest.mark.parametrize("w,h", R.GPU_SIZES)
def test_device_reduction_is_the_numpy_rule(ctx, rr, w, h, k):
    for name, img in R.images(w, h).items():
        want = R.reduce(img, k)
        got = ctx.film_reduce(img, k)
        assert got.shape == R.reduced_shape(h, w, k) + (4,) and got.dtype == np.float32
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, (name, w, h, k, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])
        assert np.array_equal(rr.native.film_reduce(img, k).view(np.uint32), got.view(np.uint32))  # host = device


def test_factor_one_copies_and_bad_factors_are_refused(ctx, rr):
    img = R.images(19, 13)["noise"]
    assert np.array_equal(ctx.film_reduce(img, 1), img)  # 0 + v, then v / 1
    for bad in (0, 3, 16):
        with pytest.raises(rr.RRError) as e:
            ctx.film_reduce(img, bad)
        assert e.value.code == rr.native.RR_EINVAL

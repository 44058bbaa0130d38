"""View settings without a GPU: the numpy restatement (tests/view_settings.py)
against the frozen oracle's Filmic chain, the display gamma's fixed polynomials
against the library's host function bit for bit and against pow in double, and
the scene file's look / gamma fields."""
import json

import numpy as np
import pytest

import view_settings as V
from conftest import scene_path
from oracle import oracle as O

F32 = np.float32
S04 = scene_path("04_very-simple-standin.rrscene")


@pytest.fixture(scope="module")
def grid():
    """Every multiple of 2^-16 in [0, 1]."""
    return (np.arange(65537, dtype=np.float64) / 65536.0).astype(F32)


@pytest.mark.parametrize("n3,n1", [(17, 1024), (2, 2), (33, 4096)])
def test_restatement_equals_the_oracle(tmp_path, n3, n1):
    """Look None, gamma 1, view Filmic: view8 is orc_filmic on 100k random
    triples and the edge values."""
    V.write_luts(str(tmp_path), n3=n3, n1=n1)
    luts = V.load_luts(str(tmp_path))
    rng = np.random.default_rng(5)
    rgb = np.exp2(rng.uniform(-16.0, 14.0, (100000, 3))).astype(F32)
    rgb[::7] *= F32(rng.uniform(0.0, 2.0))
    rgb[::11, 1] = rgb[::11, 0]  # ties between channels: the tetrahedra's shared faces
    rgb[::13, 2] = rgb[::13, 1]
    e = V.EDGES
    edges = np.array([[a, b, c] for a in e for b in e[::3] for c in e[::4]], F32)
    rgb = np.concatenate([rgb, edges, np.stack([e, e, e], axis=-1)])
    O.set_filmic(luts)
    try:
        want = O.filmic(rgb)
    finally:
        O.set_filmic(None)
    got = V.view8(rgb[None], V.FILMIC, luts)[0, :, :3]
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} mismatches"


def test_medium_contrast_is_the_base_curve(tmp_path):
    V.write_luts(str(tmp_path), looks=["High Contrast"])
    luts = V.load_luts(str(tmp_path))
    img = V.edge_image(64, 15)
    base = V.view8(img, V.FILMIC, luts)
    assert np.array_equal(V.view8(img, V.FILMIC, luts, look="Filmic - Medium Contrast"), base)
    assert not np.array_equal(V.view8(img, V.FILMIC, luts, look="High Contrast"), base)


@pytest.mark.parametrize("g", V.GAMMAS)
def test_gamma_host_function_bit_for_bit(rr, grid, g):
    got = rr.display_gamma(grid, g)
    want = V.display_gamma(grid, g)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))} of {grid.size} differ"
    # and beyond the grid: the edge values, values above 1, tiny ones
    x = np.concatenate([V.EDGES, np.exp2(np.linspace(-130.0, 127.9, 4001)).astype(F32)])
    assert np.array_equal(rr.display_gamma(x, g).view(np.uint32), V.display_gamma(x, g).view(np.uint32))


# The largest error of display_gamma against v ** (1 / g) in double over the
# grid, in 16-bit codes (65535 |approx - exact|), as measured
# (profiles/view_settings.md): 0.00646 code, at g = 0.45 and 0.7 (about 0.1
# ulp-of-a-code: the float32 rounding of the two polynomials, far below the
# half code that would move a sample).
GAMMA_MAX_CODES = 0.00646


def test_gamma_accuracy(rr, grid):
    worst = 0.0
    for g in V.GAMMAS:
        approx = rr.display_gamma(grid, g).astype(np.float64)
        exact = grid.astype(np.float64) ** (1.0 / float(F32(g)))  # the float32 g the function is given
        err = float(np.max(65535.0 * np.abs(approx - exact)))
        print(f"display gamma {g}: max error {err:.4f} 16-bit codes")
        worst = max(worst, err)
    print(f"display gamma: worst {worst:.4f} 16-bit codes")
    assert worst <= 1.25 * GAMMA_MAX_CODES
    assert worst < 0.5


def test_gamma_one_is_not_skipped_by_the_debug_entry(rr, grid):
    """A pass through log2 and exp2 is not the identity, which is why frames
    skip the step at gamma 1; the host function evaluates it as asked."""
    out = rr.display_gamma(grid, 1.0)
    assert np.array_equal(out.view(np.uint32), V.display_gamma(grid, 1.0).view(np.uint32))
    assert np.max(np.abs(out.astype(np.float64) - grid)) < 1e-6


@pytest.mark.parametrize("g", [0.0, -1.0, 5.0001, float("nan")])
def test_gamma_range_of_the_debug_entry(rr, g):
    with pytest.raises(rr.RRError) as e:
        rr.display_gamma(np.zeros(4, F32), g)
    assert e.value.code == -22


def _scene(tmp_path, **render):
    with open(S04) as f:
        sc = json.load(f)
    for k, v in render.items():
        if v is None:
            sc["render"].pop(k, None)
        else:
            sc["render"][k] = v
    p = tmp_path / "scene.rrscene"
    p.write_text(json.dumps(sc))
    return str(p)


@pytest.mark.parametrize("look", V.LOOK_FILES)
@pytest.mark.parametrize("prefix", ["", "Filmic - "])
def test_scene_look_names(rr, tmp_path, look, prefix):
    s = rr.Scene(_scene(tmp_path, view_transform="Filmic", look=prefix + look))
    try:
        assert s.view_settings() == (rr.native.RR_VIEW_FILMIC, look, 1.0)
    finally:
        s.close()


def test_scene_views_and_defaults(rr, tmp_path):
    for name, value in (("Standard", 0), ("Raw", 1), ("Filmic", 2), ("Filmic Log", 3), ("False Color", 4)):
        s = rr.Scene(_scene(tmp_path, view_transform=name, look=None, gamma=None))
        assert s.view_settings() == (value, "None", 1.0)
        assert s.frame_constants(1).render_ints[5] == value
        s.close()
    s = rr.Scene(_scene(tmp_path, view_transform="AgX", look="Punchy", gamma=2.2))
    v, look, g = s.view_settings()  # unknown: Standard, no look (the frame's warning names both)
    assert (v, look) == (0, "None") and g == F32(2.2)
    s.close()
    assert list(rr.native.LOOKS) == list(V.LOOK_FILES)
    assert (rr.native.RR_VIEW_FILMIC_LOG, rr.native.RR_VIEW_FALSE_COLOR) == (3, 4)


@pytest.mark.parametrize("g", [0.0, -0.5, 5.5, 1e9])
def test_scene_gamma_range(rr, tmp_path, g):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene(tmp_path, gamma=g))
    assert e.value.code == -22 and "gamma" in str(e.value)


@pytest.mark.parametrize("g", [0.2, 1.0, 5.0])
def test_scene_gamma_accepted(rr, tmp_path, g):
    s = rr.Scene(_scene(tmp_path, gamma=g))
    assert s.view_settings()[2] == F32(g)
    s.close()


def test_params_view_range(rr):
    s = rr.Scene(S04)
    try:
        for v in (3, 4):
            assert s.frame_constants(1, rr.default_params(view_transform=v)).render_ints[5] == v
        with pytest.raises(rr.RRError):
            s.frame_constants(1, rr.default_params(view_transform=5))
    finally:
        s.close()


def test_runner_passes_look_and_gamma_through(rr, tmp_path):
    calls = []

    class Stub:
        def set_look(self, name):
            calls.append(("look", name))

        def set_display_gamma(self, g):
            calls.append(("gamma", g))

        def close(self):
            pass

    rr.BackendRunner(tmp_path, ctx=Stub(), look="High Contrast", display_gamma=2.2).close()
    assert calls == [("look", "High Contrast"), ("gamma", 2.2)]
    calls.clear()
    rr.BackendRunner(tmp_path, ctx=Stub()).close()
    assert calls == []

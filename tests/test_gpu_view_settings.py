"""View settings on the device: Filmic looks, Filmic Log, False Color and the
display gamma (csrc/view.hip k_view, csrc/png16.hip Png16Sub) against the numpy
restatement of tests/view_settings.py, bit for bit, on synthetic LUTs in
Blender's formats; the fallbacks when a LUT is missing; the setters, their
environment twins and the scene's fields."""
import json
import os

import numpy as np
import pytest

import color_modes as CM
import png16_reader as P
import view_settings as V
from conftest import scene_path
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
S01 = scene_path("01_simple-animation.rrscene")
LOOKS = [k for k, f in V.LOOK_FILES.items() if f]
WAVEFRONT = 4  # RR_FLAG_WAVEFRONT


@pytest.fixture(scope="module")
def lut_sets(tmp_path_factory):
    """a: cubes of edge 17, 1-component curves; b: cubes of edge 2, 3-component
    curves. Every look's curve and the false-colour cube in both."""
    out = {}
    for name, n3, n1, comps in (("a", 17, 1024, 1), ("b", 2, 64, 3)):
        d = str(tmp_path_factory.mktemp("luts_" + name))
        V.write_luts(d, n3=n3, n1=n1, looks=LOOKS, comps=comps, false_color_n3=n3, look_n1=33 if n3 == 2 else 257)
        out[name] = (d, V.load_luts(d))
    return out


@pytest.fixture(scope="module")
def tables(rr):
    return {8: O.srgb_lut(), 16: rr.native.srgb16_table()}


@pytest.fixture()
def vctx(ctx):
    """The session's context, handed back with no LUTs, look or gamma set."""
    yield ctx
    ctx.set_ocio_config(None)
    ctx.set_look(None)
    ctx.set_display_gamma(0.0)


# (view, look, gamma): each look, Filmic Log, False Color, and the two gammas on Standard, Raw and Filmic
CASES = [(V.FILMIC, look, 1.0) for look in V.LOOK_FILES] + [(V.FILMIC_LOG, None, 1.0), (V.FALSE_COLOR, None, 1.0)] + \
    [(v, None, g) for v in (V.STANDARD, V.RAW, V.FILMIC) for g in (0.7, 2.2)] + \
    [(V.FILMIC, "Filmic - Very Low Contrast", 0.7), (V.FILMIC_LOG, None, 2.2), (V.FALSE_COLOR, None, 0.7)]
SIZES = [(1, 1), (255, 1), (257, 1), (64, 15)]


def _case_id(c):
    return f"{['std', 'raw', 'filmic', 'log', 'false'][c[0]]}-{(c[1] or 'none').replace(' ', '')}-g{c[2]}"


def _apply(ctx, look, gamma):
    ctx.set_look(look)
    ctx.set_display_gamma(0.0 if gamma == 1.0 else gamma)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_view_device_bit_exact(vctx, lut_sets, tables, which, case):
    view, look, gamma = case
    d, luts = lut_sets[which]
    vctx.set_ocio_config(d)
    _apply(vctx, look, gamma)
    for k, (w, h) in enumerate(SIZES):
        img = V.edge_image(w, h, seed=k)
        for scale in (1.0, 0.37):
            got = vctx.view_device(img, view, scale)
            want = V.view8(img, view, luts, look or "None", gamma, scale, tables[8])
            bad = np.argwhere((got != want).any(axis=-1))
            assert len(bad) == 0, f"{w}x{h} scale {scale}: {len(bad)} pixels, first {bad[0]}: " \
                                  f"{img[tuple(bad[0])]} -> {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"


def test_view_device_second_grid_trip(vctx, lut_sets, tables):
    """1152 x 912 pixels are more than the 4096 blocks of 256 the pass launches:
    the last 2,048 pixels come from the grid-stride loop's second trip."""
    d, luts = lut_sets["a"]
    vctx.set_ocio_config(d)
    _apply(vctx, "High Contrast", 2.2)
    w, h = 1152, 912
    assert w * h > 4096 * 256
    img = np.zeros((h, w, 4), F32)
    tile = V.edge_image(1024, 57, seed=3)[..., :3].reshape(-1, 3)
    flat = np.resize(tile, (h * w, 3))
    flat[-2048:] = tile[:2048][::-1]  # the second trip's pixels are not a repeat of the first's
    img[..., :3] = flat.reshape(h, w, 3)
    got = vctx.view_device(img, V.FILMIC, 1.0)
    want = V.view8(img, V.FILMIC, luts, "High Contrast", 2.2, 1.0, tables[8])
    assert np.array_equal(got, want), f"{np.count_nonzero((got != want).any(axis=-1))} pixels differ"
    assert np.all(got[..., 3] == 255)


PNG_CASES = [(V.FILMIC, "Medium High Contrast", 2.2), (V.FILMIC, "Low Contrast", 1.0), (V.FILMIC_LOG, None, 1.0),
             (V.FALSE_COLOR, None, 0.7), (V.STANDARD, None, 2.2), (V.RAW, None, 0.7)]


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("case", PNG_CASES, ids=_case_id)
def test_png16_bit_exact(vctx, lut_sets, tables, which, case):
    view, look, gamma = case
    d, luts = lut_sets[which]
    vctx.set_ocio_config(d)
    _apply(vctx, look, gamma)
    for k, (w, h) in enumerate([(1, 1), (3, 17), (333, 33)]):
        img = V.edge_image(w, h, seed=10 + k)
        for mode, c in CM.MODES.items():
            data = vctx.encode_device("PNG", img, 16, mode, view_transform=view, exposure_scale=0.8)
            if c == 4:
                px, _ = P.read_png16(data)
            else:
                px, info = CM.read_png(data)
                assert (info["depth"], info["channels"]) == (16, c)
            want = V.view16(img, c, view, luts, look or "None", gamma, 0.8, tables[16])
            assert np.array_equal(px.reshape(want.shape), want), \
                f"{mode} {w}x{h}: {np.count_nonzero(px.reshape(want.shape) != want)} samples differ"


RENDER_CASES = [(V.FILMIC, "Medium High Contrast", 1.0), (V.FILMIC_LOG, None, 1.0), (V.FALSE_COLOR, None, 1.0),
                (V.FILMIC, None, 2.2), (V.STANDARD, None, 2.2)]


@pytest.mark.parametrize("flags", [0, WAVEFRONT], ids=["tiles", "wavefront"])
def test_rendered_frames(vctx, rr, lut_sets, tables, flags):
    """01 at 96 x 54, 8 spp, both render paths: rgba8 is the restatement of the
    returned film, and the film is the film of the frame without the setting."""
    d, luts = lut_sets["a"]
    vctx.set_ocio_config(d)
    s = vctx.load_scene(S01)
    try:
        base = rr.default_params(width=96, height=54, spp=8, flags=flags)
        film0, rgba0, st0 = vctx.render_to_memory(s, 30, base)
        assert st0.view_transform == V.FILMIC and st0.view_transform_substituted == 0
        scale = float(vctx.frame_state(s, 30, base).render_floats[2])
        assert np.array_equal(rgba0, V.view8(film0, V.FILMIC, luts, "None", 1.0, scale, tables[8]))
        seen = [rgba0]
        for view, look, gamma in RENDER_CASES:
            _apply(vctx, look, gamma)
            p = rr.default_params(width=96, height=54, spp=8, flags=flags, view_transform=view)
            film, rgba, st = vctx.render_to_memory(s, 30, p)
            assert (st.view_transform, st.view_transform_substituted) == (view, 0), vctx.last_warning()
            assert vctx.last_warning() == ""
            assert np.array_equal(film, film0)
            want = V.view8(film, view, luts, look or "None", gamma, scale, tables[8])
            assert np.array_equal(rgba, want), f"{_case_id((view, look, gamma))}: " \
                                               f"{np.count_nonzero((rgba != want).any(axis=-1))} pixels differ"
            assert not any(np.array_equal(rgba, o) for o in seen)  # every setting shows in the picture
            seen.append(rgba)
    finally:
        s.close()


def test_unchanged_bits_without_settings(vctx, rr, lut_sets, tables):
    """Filmic / None / gamma 1 and Standard: the same calls before any setter
    is used, with the setters at "None" and 1, and handed back to the scene."""
    d, luts = lut_sets["a"]
    vctx.set_ocio_config(d)
    s = vctx.load_scene(S01)
    img = V.edge_image(333, 33, seed=2)

    def run(views=(V.FILMIC, V.STANDARD)):
        out = []
        for view in views:
            p = rr.default_params(width=96, height=54, spp=8, view_transform=view)
            film, rgba, st = vctx.render_to_memory(s, 30, p)
            assert (st.view_transform, st.view_transform_substituted) == (view, 0)
            out += [film, rgba, vctx.view_device(img, view, 1.0)]
            for mode in CM.MODES:
                out.append(np.frombuffer(vctx.encode_device("PNG", img, 16, mode, view_transform=view), np.uint8))
            out.append(np.frombuffer(vctx.png16_device(img, view, 1.0), np.uint8))
        return out

    try:
        before = run()
        vctx.set_look("None")
        vctx.set_display_gamma(1.0)
        explicit = run()
        vctx.set_look("Medium Contrast")  # the base curve: the bits of None (Filmic only: Standard takes no look)
        medium = run((V.FILMIC,))
        vctx.set_look(None)
        vctx.set_display_gamma(0.0)
        after = run()
        for other in (explicit, medium, after):
            assert len(other) in (len(before), len(before) // 2)
            assert all(np.array_equal(a, b) for a, b in zip(before, other))
        # and what those bits are: the Filmic chain and Standard, at gamma 1
        assert np.array_equal(before[2], V.view8(img, V.FILMIC, luts, table=tables[8]))
        px, _ = P.read_png16(before[5].tobytes())
        assert np.array_equal(px, V.view16(img, 4, V.FILMIC, luts, table=tables[16]))
        n = len(before) // 2
        assert np.array_equal(before[n + 2], V.view8(img, V.STANDARD, table=tables[8]))
        px, _ = P.read_png16(before[n + 5].tobytes())
        assert np.array_equal(px, P.front_end(img, 0, 1.0, tables[16]))
    finally:
        s.close()


def test_fallbacks(vctx, rr, tmp_path, tables):
    s = vctx.load_scene(S01)
    try:
        std = rr.default_params(width=64, height=36, spp=4, view_transform=V.STANDARD)
        _, rgba_std, st = vctx.render_to_memory(s, 30, std)
        assert st.view_transform_substituted == 0 and vctx.last_warning() == ""
        # no LUTs at all: False Color and Filmic Log are Standard, flagged and named
        for view, name in ((V.FALSE_COLOR, "False Color"), (V.FILMIC_LOG, "Filmic Log")):
            p = rr.default_params(width=64, height=36, spp=4, view_transform=view)
            _, rgba, st = vctx.render_to_memory(s, 30, p)
            assert (st.view_transform, st.view_transform_substituted) == (0, 1)
            assert name in vctx.last_warning() and "Standard" in vctx.last_warning()
            assert np.array_equal(rgba, rgba_std)
        # the base pair alone: a look renders as base Filmic, False Color as Standard, each naming its file
        V.write_luts(str(tmp_path))
        vctx.set_ocio_config(str(tmp_path))
        fil = rr.default_params(width=64, height=36, spp=4, view_transform=V.FILMIC)
        _, rgba_fil, st = vctx.render_to_memory(s, 30, fil)
        assert (st.view_transform, st.view_transform_substituted) == (2, 0) and vctx.last_warning() == ""
        vctx.set_look("High Contrast")
        _, rgba, st = vctx.render_to_memory(s, 30, fil)
        w = vctx.last_warning()
        assert (st.view_transform, st.view_transform_substituted) == (2, 1)
        assert "High Contrast" in w and V.LOOK_FILES["High Contrast"] in w, w
        assert np.array_equal(rgba, rgba_fil)
        # the same look in a 16-bit PNG frame: the file of the frame without it
        vctx.set_png_depth(16)
        t, st = vctx.render_frame(s, 30, fil, str(tmp_path / "look"), "PNG")
        assert st.view_transform_substituted == 1
        vctx.set_look(None)
        t, st = vctx.render_frame(s, 30, fil, str(tmp_path / "none"), "PNG")
        assert st.view_transform_substituted == 0
        assert (tmp_path / "look.png").read_bytes() == (tmp_path / "none.png").read_bytes()
        vctx.set_png_depth(0)
        # a look with a view that takes none is ignored and said so
        vctx.set_look("Medium Contrast")
        _, rgba, st = vctx.render_to_memory(s, 30, std)
        assert st.view_transform_substituted == 1 and "Medium Contrast" in vctx.last_warning()
        assert np.array_equal(rgba, rgba_std)
        vctx.set_look(None)
        _, rgba, st = vctx.render_to_memory(s, 30, rr.default_params(width=64, height=36, spp=4,
                                                                      view_transform=V.FALSE_COLOR))
        w = vctx.last_warning()
        assert (st.view_transform, st.view_transform_substituted) == (0, 1)
        assert "False Color" in w and V.FALSE_COLOR_FILE in w, w
        assert np.array_equal(rgba, rgba_std)
        # the inspection entries substitute nothing
        img = V.edge_image(3, 17)
        vctx.set_look("High Contrast")
        for call in (lambda: vctx.view_device(img, V.FILMIC), lambda: vctx.view_device(img, V.FALSE_COLOR),
                     lambda: vctx.encode_device("PNG", img, 16, "RGB", view_transform=V.FILMIC),
                     lambda: vctx.view_device(img, 5)):
            with pytest.raises(rr.RRError) as e:
                call()
            assert e.value.code == -22
        # a malformed optional file fails the configuration like a malformed base file
        (tmp_path / "luts" / V.LOOK_FILES["Low Contrast"]).write_text("Version 1\nFrom 0 1\nLength 3\nComponents 1\n{\n0\n1\n}\n")
        with pytest.raises(rr.RRError) as e:
            vctx.set_ocio_config(str(tmp_path))
        assert e.value.code == -22
        _, rgba, st = vctx.render_to_memory(s, 30, fil)
        assert (st.view_transform, st.view_transform_substituted) == (0, 1)  # no LUTs were kept
        os.remove(tmp_path / "luts" / V.LOOK_FILES["Low Contrast"])
        (tmp_path / "luts" / V.FALSE_COLOR_FILE).write_text("SPILUT 1.0\n3 3\n2 2 2\n0 0 0 0 0 0\n")
        with pytest.raises(rr.RRError) as e:
            vctx.set_ocio_config(str(tmp_path))
        assert e.value.code == -22
    finally:
        s.close()
        vctx.set_png_depth(0)


def test_frames_in_flight_keep_their_look(vctx, rr, lut_sets, tmp_path):
    d, luts = lut_sets["a"]
    vctx.set_ocio_config(d)
    vctx.set_png_depth(16)
    s = vctx.load_scene(S01)
    p = rr.default_params(width=96, height=54, spp=8)
    settings = [("High Contrast", 0.0), ("Very Low Contrast", 2.2), (None, 0.7)]
    try:
        for k, (look, g) in enumerate(settings):  # one at a time: what each setting's file is
            vctx.set_look(look)
            vctx.set_display_gamma(g)
            vctx.render_frame(s, 30, p, str(tmp_path / f"alone{k}"), "PNG")
        tickets = []
        for k, (look, g) in enumerate(settings):
            vctx.set_look(look)
            vctx.set_display_gamma(g)
            tickets.append(vctx.submit_frame(s, 30, p, str(tmp_path / f"flight{k}"), "PNG"))
        vctx.set_look("Low Contrast")  # after the submits: none of the three may take it
        vctx.set_display_gamma(5.0)
        for t in tickets:
            _, st = vctx.complete_frame(t)
            assert st.view_transform == V.FILMIC and st.view_transform_substituted == 0
        files = [(tmp_path / f"flight{k}.png").read_bytes() for k in range(3)]
        for k in range(3):
            assert files[k] == (tmp_path / f"alone{k}.png").read_bytes(), k
        assert len(set(files)) == 3
    finally:
        s.close()
        vctx.set_png_depth(0)


def test_scene_setter_environment(rr, lut_sets, tables, tmp_path, monkeypatch):
    """The context's look and gamma (setter, or RR_LOOK / RR_DISPLAY_GAMMA read
    by rr_create) come before the scene's render.look / render.gamma."""
    d, luts = lut_sets["a"]
    with open(S01) as f:
        sc = json.load(f)
    sc["render"]["look"] = "Filmic - Low Contrast"
    sc["render"]["gamma"] = 1.5
    path = str(tmp_path / "look.rrscene")
    with open(path, "w") as f:
        json.dump(sc, f)
    p = rr.default_params(width=64, height=36, spp=4)

    def check(c, look, gamma):
        s = c.load_scene(path)
        try:
            film, rgba, st = c.render_to_memory(s, 30, p)
            assert (st.view_transform, st.view_transform_substituted) == (V.FILMIC, 0), c.last_warning()
            scale = float(c.frame_state(s, 30, p).render_floats[2])
            assert np.array_equal(rgba, V.view8(film, V.FILMIC, luts, look, gamma, scale, tables[8])), (look, gamma)
        finally:
            s.close()

    monkeypatch.delenv("RR_LOOK", raising=False)
    monkeypatch.delenv("RR_DISPLAY_GAMMA", raising=False)
    monkeypatch.setenv("RR_OCIO_DIR", d)
    with rr.RenderContext(0) as c:
        check(c, "Low Contrast", 1.5)  # the scene's
        c.set_look("None")
        check(c, "None", 1.5)
        c.set_display_gamma(1.0)
        check(c, "None", 1.0)
        c.set_look("Filmic - High Contrast")
        c.set_display_gamma(2.2)
        check(c, "High Contrast", 2.2)
        c.set_look("")
        c.set_display_gamma(0)
        check(c, "Low Contrast", 1.5)
        for bad in ("Punchy", "Filmic - ", "high contrast"):
            with pytest.raises(rr.RRError) as e:
                c.set_look(bad)
            assert e.value.code == -22
        for bad in (-1.0, 5.5, float("nan")):
            with pytest.raises(rr.RRError) as e:
                c.set_display_gamma(bad)
            assert e.value.code == -22
        check(c, "Low Contrast", 1.5)  # a refused value changes nothing
    monkeypatch.setenv("RR_LOOK", "Very High Contrast")
    monkeypatch.setenv("RR_DISPLAY_GAMMA", "0.7")
    with rr.RenderContext(0) as c:
        check(c, "Very High Contrast", 0.7)
        c.set_look(None)  # back to the scene's
        check(c, "Low Contrast", 0.7)
    monkeypatch.setenv("RR_LOOK", "")
    monkeypatch.setenv("RR_DISPLAY_GAMMA", "")
    with rr.RenderContext(0, look="Medium Low Contrast", display_gamma=2.2) as c:
        check(c, "Medium Low Contrast", 2.2)
    for name, bad in (("RR_LOOK", "Punchy"), ("RR_DISPLAY_GAMMA", "7"), ("RR_DISPLAY_GAMMA", "two")):
        monkeypatch.setenv(name, bad)
        with pytest.raises(rr.RRError) as e:
            rr.RenderContext(0)
        assert e.value.code == -22 and name in str(e.value)
        monkeypatch.setenv(name, "")

"""k_tiles' camera masks drop triangles that another one hides over the whole
tile (tiles.hip tile_mask). The closest hit must not change:
film and RGBA8 equal the oracle's, which brute-forces every camera ray, at
tolerance 0 (as test_gpu_parity.py), on small scenes placed where the rule
could go wrong. Triangles are given in camera space (x right, y up, z = depth
along the view axis) and written in world space into a copy of the 04vs
stand-in whose mesh object sits at the origin without animation.

Counting frames (RR_FLAG_COUNT_TRAVERSAL) give the camera rays' triangle
tests, trav_tris[0]: with two triangles larger than the screen every traced ray
tests both unless the rule drops one, so the counts say whether it fired.
"""
import json

import numpy as np
import pytest

import soups
from conftest import scene_path
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
SIZES = [(64, 64), (72, 40)]  # the second has partial tiles at the right and bottom edge


def big(z, s=1.0):
    """A triangle at depth z that contains the whole screen with room to spare
    (the sensor's half extents are 0.36 and less: +-1.8 s at z = 5 s)."""
    return [(-6.0 * s, -4.0 * s, z), (6.0 * s, -4.0 * s, z), (0.0, 8.0 * s, z)]


def tilted(s=1.0):
    """big() tilted about the vertical: depth 5 + x / 2, about 4 to 7 across the frame."""
    return [(-6.0 * s, -4.0 * s, 2.0), (6.0 * s, -4.0 * s, 8.0), (0.0, 8.0 * s, 5.0)]


FRONT, BACK = big(5.0), big(8.0, 2.0)
COPLANAR = [(-7.0, -5.0, 5.0), (7.0, -5.0, 5.0), (0.0, 9.0, 5.0)]
# its plane x = y passes through the camera: edge-on, no inverse-depth plane
GRAZING = [(-1.0, -1.0, 6.0), (1.0, 1.0, 6.0), (0.0, 0.0, 9.0)]


def cube_around_camera(h=3.0):
    c = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, cc, d in quads:
        tris += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    rot = soups._rotation(np.random.default_rng(5))  # no face parallel to the sensor
    return (np.array(tris) @ rot.T).tolist()


def _render(ctx, rr, tmp_path, name, cam_tris, w, h, spp, clip=None, flags=0):
    """Renders the triangles (camera space) and the oracle's frame of the same
    state; returns (film, rgba, oracle film, oracle rgba, counting frame's stats)."""
    p = rr.default_params(width=w, height=h, spp=spp, flags=flags)
    base = ctx.load_scene(S04)
    try:
        cam = ctx.frame_state(base, 1, p).camera.astype(np.float64)
    finally:
        base.close()
    pos, right, up, back = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    t = np.array(cam_tris, np.float64).reshape(-1, 3, 3)
    world = pos + t[..., 0:1] * right + t[..., 1:2] * up - t[..., 2:3] * back
    scene = soups.soup_scene_dict(S04, 0, tris=world.astype(np.float32))
    obj = scene["objects"][1]
    obj.pop("animation", None)
    obj["location"] = [0.0, 0.0, 0.0]
    obj["matrix_world_saved"] = [float(x) for x in np.eye(4).reshape(-1)]
    if clip:
        scene["objects"][0]["camera"]["clip_start"], scene["objects"][0]["camera"]["clip_end"] = clip
    path = str(tmp_path / f"{name}.rrscene")
    with open(path, "w") as f:
        json.dump(scene, f)
    s = ctx.load_scene(path)
    try:
        film, rgba, _ = ctx.render_to_memory(s, 1, p)
        st = ctx.frame_state(s, 1, p)
        assert int(st.render_ints[7]) == (4 if flags & rr.native.RR_FLAG_WAVEFRONT else 2)
        pc = rr.default_params(width=w, height=h, spp=spp, flags=flags | rr.native.RR_FLAG_COUNT_TRAVERSAL)
        cfilm, _, cst = ctx.render_to_memory(s, 1, pc)
        assert np.array_equal(cfilm, film)
    finally:
        s.close()
    of, orgba = O.render_state(st)
    return film, rgba, of, orgba, cst


def _check(film, rgba, of, orgba, lit=True):
    nbad = int(np.count_nonzero(rgba != orgba))
    assert nbad == 0, f"{nbad} 8-bit mismatches"
    assert np.array_equal(film, of), f"{np.count_nonzero(film != of)} film mismatches"
    if lit:  # something is visible
        assert len(np.unique(orgba.reshape(-1, 4), axis=0)) > 1


def _tests_per_ray(st):
    print(f"camera rays traced {st.camera_rays_traced}, triangle tests {st.trav_tris[0]}")
    return st.trav_tris[0], st.camera_rays_traced


@pytest.mark.parametrize("w,h,spp", [(64, 64, 8), (72, 40, 33)])
@pytest.mark.parametrize("front_first", [True, False])
def test_one_hiding_triangle(ctx, rr, tmp_path, w, h, spp, front_first):
    """A triangle larger than the screen in front of another: one test per
    traced ray (two without the rule), so a rule that drops nothing fails."""
    tris = [FRONT, BACK] if front_first else [BACK, FRONT]
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "hiding", tris, w, h, spp)
    _check(film, rgba, of, orgba)
    tests, rays = _tests_per_ray(st)
    assert rays == w * h * spp
    assert tests == rays


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("first", [0, 1])
def test_coplanar_triangles_both_stay(ctx, rr, tmp_path, w, h, first):
    """Two coplanar triangles, both orders of original id (closer's tie rule
    picks the smaller id): nothing is dropped, two tests per traced ray."""
    tris = [FRONT, COPLANAR] if first == 0 else [COPLANAR, FRONT]
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "coplanar", tris, w, h, 8)
    _check(film, rgba, of, orgba)
    tests, rays = _tests_per_ray(st)
    assert rays == w * h * 8
    assert tests == 2 * rays


@pytest.mark.parametrize("w,h", SIZES)
def test_interpenetrating_triangles(ctx, rr, tmp_path, w, h):
    """Two triangles that cross inside the frame: each is the nearer one on its side."""
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "crossing", [tilted(), FRONT], w, h, 8)
    _check(film, rgba, of, orgba)
    _tests_per_ray(st)
    assert len(np.unique(orgba.reshape(-1, 4), axis=0)) > 2


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("clip", [(5.0, 100.0), (0.1, 5.0)])
def test_front_triangle_crosses_a_clip_plane(ctx, rr, tmp_path, w, h, clip):
    """The front triangle crosses clip_start (its near part is clipped and the
    far triangle shows through), then clip_end (its far part and the far
    triangle are clipped)."""
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "clip", [tilted(), BACK], w, h, 8, clip=clip)
    _check(film, rgba, of, orgba)
    _tests_per_ray(st)


@pytest.mark.parametrize("w,h", SIZES)
def test_camera_inside_the_cube(ctx, rr, tmp_path, w, h):
    """Every face seen from its inner side, vertices behind the camera. The
    closed cube keeps the light and the world out: the frame is black, and the
    check is that every camera ray still finds a face (it is absorbed there;
    a ray through a wrongly emptied mask would return the world's colour)."""
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "inside", cube_around_camera(), w, h, 8)
    _check(film, rgba, of, orgba, lit=False)
    tests, rays = _tests_per_ray(st)
    assert rays == w * h * 8 and tests >= rays


@pytest.mark.parametrize("w,h", SIZES)
def test_grazing_plane_behind_a_covering_triangle(ctx, rr, tmp_path, w, h):
    """A triangle whose plane passes through the camera position, behind a
    covering one: it has no inverse depth to compare and stays in the masks of
    the tiles its rectangle meets."""
    film, rgba, of, orgba, st = _render(ctx, rr, tmp_path, "grazing", [FRONT, GRAZING], w, h, 8)
    _check(film, rgba, of, orgba)
    tests, rays = _tests_per_ray(st)
    assert rays < tests < 2 * rays


def test_04vs_cube_corner_view(ctx, rr):
    """The 04vs cube at 64 x 64: silhouette, diagonal and interior tiles in one frame."""
    s = ctx.load_scene(S04)
    try:
        p = rr.default_params(width=64, height=64, spp=8)
        film, rgba, _ = ctx.render_to_memory(s, 30, p)
        of, orgba = O.render_state(ctx.frame_state(s, 30, p))
        _check(film, rgba, of, orgba)
        pc = rr.default_params(width=64, height=64, spp=8, flags=rr.native.RR_FLAG_COUNT_TRAVERSAL)
        _tests_per_ray(ctx.render_to_memory(s, 30, pc)[2])
    finally:
        s.close()


def test_wavefront_path_gives_the_same_bits(ctx, rr, tmp_path):
    """The split path (RR_FLAG_WAVEFRONT) has no tile masks: the same frame."""
    film, rgba, of, orgba, _ = _render(ctx, rr, tmp_path, "hiding_wf", [FRONT, BACK], 72, 40, 8,
                                       flags=rr.native.RR_FLAG_WAVEFRONT)
    _check(film, rgba, of, orgba)
    tfilm, trgba, _, _, _ = _render(ctx, rr, tmp_path, "hiding_t", [FRONT, BACK], 72, 40, 8)
    assert np.array_equal(film, tfilm) and np.array_equal(rgba, trgba)

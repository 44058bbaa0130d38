"""k_tiles' sample loop has a second body for tiles that one triangle covers
(tiles.hip tile_mask / tiles_body, paths.hpp shade_covered): no
cull test, no lane predicates, no mask loop, the triangle's, material's and
light's records read at wave-uniform addresses. It must compute what the
general body computes: film and RGBA8 equal the oracle's bit for bit, and the
ray counters equal those of the same frame rendered with the body compiled
out (RR_TILES_COVERED=0, which compiles to the parent commit's instructions),
recorded in tests/golden/tile_covered_counters.json by
tools/record_tile_covered.py.

Which body ran is observed, not assumed: a counting launch adds, per screen
tile, the samples its covered body ran to the second half of the tile cost
buffer that rr_debug_tile_costs hands out (tiles.hip tiles_body); every case
states what that must show (`covered`).

Triangles are given in camera space (x right, y up, z = depth along the view
axis), the light too, and written in world space into a copy of the 04vs
stand-in, as tests/test_gpu_tile_occlusion.py does.
"""
import json
import os

import numpy as np
import pytest

import soups
from conftest import GOLDEN, scene_path
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
COUNTERS = os.path.join(GOLDEN, "tile_covered_counters.json")
FIELDS = ("camera_rays", "camera_rays_traced", "extension_rays", "shadow_rays", "extension_rays_escaped",
          "shadow_rays_escaped")


def big(z, s=1.0):
    """A triangle at depth z that contains the whole screen with room to spare
    (the sensor's half extents are 0.36 and less: +-1.8 s at z = 5 s)."""
    return [(-6.0 * s, -4.0 * s, z), (6.0 * s, -4.0 * s, z), (0.0, 8.0 * s, z)]


FRONT = big(5.0)
BACKSIDE = [FRONT[1], FRONT[0], FRONT[2]]  # the other winding: seen from behind, shade() flips the normal
TILTED = [(-6.0, -4.0, 2.0), (6.0, -4.0, 8.0), (0.0, 8.0, 5.0)]  # depth 5 + x / 2
QUAD = [[(-6.0, -4.0, 5.0), (6.0, -4.0, 5.0), (6.0, 8.0, 5.0)], [(-6.0, -4.0, 5.0), (6.0, 8.0, 5.0), (-6.0, 8.0, 5.0)]]
# a floor 0.05 below the camera: its plane passes the camera at 0.03 degrees, below
# tri_inv_depth_plane's threshold, so it has no inverse-depth plane and never counts as covering
GRAZING = [(-100.0, -0.05, 0.5), (100.0, -0.05, 0.5), (0.0, -0.05, 200.0)]
MID = [(0.0, -1.0, 5.0), (0.0, 1.0, 5.0)]  # the frame's middle column at depth 5
BEHIND = [(-6.0, -4.0, 5.0), (6.0, -4.0, 5.0), (0.0, 8.0, -1.0)]  # one vertex behind the camera plane


def lit_cube(half=1.2, z=4.5):
    """A cube like 04vs', near enough that its front face about fills a 64 x 64 frame: turned 15 degrees about
    the vertical and 10 about the horizontal axis, so two more faces show at the rim. The tiles inside one of
    the front face's two triangles are covered; those on its diagonal, on the cube's edges and the silhouette
    are not."""
    c = np.array([[x, y, w] for x in (-half, half) for y in (-half, half) for w in (-half, half)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    a, b = np.radians(15.0), np.radians(10.0)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    c = c @ (rx @ ry).T + np.array([0.0, 0.0, z])
    return [[c[i], c[j], c[k]] for q in quads for i, j, k in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]


LIGHT = (0.5, 0.6, 2.0)  # camera space: between the camera and the triangles

# name: tris (None: the 04vs cube itself), w, h, spp and what differs from the default scene.
# covered: the tiles whose samples the covered body must have run, all of them (spp per tile) — "all": every
# tile, "none": no tile, "interior": the tiles wholly inside the image and no other, "some": at least one tile
# and not every tile (which ones follows from the geometry; the bits and counters are checked on all of them)
CASES = {
    "full_front": dict(tris=[FRONT], w=64, h=64, spp=37, covered="all"),
    "full_back": dict(tris=[BACKSIDE], w=64, h=64, spp=5, covered="all"),
    "cube_lit": dict(tris=lit_cube(), w=64, h=64, spp=33, covered="some"),
    "cube_04vs": dict(tris=None, w=64, h=64, spp=8, frame=30, covered="none"),  # faces smaller than a tile + margins
    "light_disk": dict(tris=[TILTED], w=48, h=32, spp=7, light=("POINT", 0.25), covered="all"),
    "light_point": dict(tris=[TILTED], w=48, h=32, spp=7, light=("POINT", 0.0), covered="all"),
    "light_sun": dict(tris=[TILTED], w=48, h=32, spp=7, light=("SUN", 0.0), covered="all"),
    "emissive": dict(tris=[FRONT], w=32, h=32, spp=9, mat=dict(emission=[1.0, 0.5, 0.25], emission_strength=2.0),
                     covered="all"),
    "specular": dict(tris=[TILTED], w=48, h=32, spp=40, mat=dict(metallic=0.75, roughness=0.2), covered="all"),
    "bounces_1": dict(tris=[FRONT], w=32, h=32, spp=5, max_bounces=1, covered="all"),
    "bounces_12": dict(tris=[TILTED, big(8.0, 2.0)], w=48, h=32, spp=11, max_bounces=12, covered="all"),
    "no_light": dict(tris=[FRONT], w=32, h=32, spp=5, n_lights=0, covered="all"),
    "edge_tiles_61x45": dict(tris=[FRONT], w=61, h=45, spp=35, covered="interior"),
    # split: a line (two camera-space points a, b) that cuts the frame in two, and the triangle that alone covers
    # the side left of a -> b on screen, then the one for the right side (None: nothing does, the triangle is
    # clipped there); expected_tiles() turns it into tiles
    "coplanar_quad": dict(tris=QUAD, w=64, h=64, spp=6, covered="some",  # the diagonal's tiles hold two
                          split=(QUAD[0][0], QUAD[0][2], QUAD[1], QUAD[0])),
    # TILTED is at depth 5 on the frame's middle column, nearer on its left
    "clip_start": dict(tris=[TILTED], w=64, h=64, spp=6, clip=(5.0, 100.0), covered="some",
                       split=(MID[0], MID[1], None, TILTED)),
    "clip_end": dict(tris=[TILTED], w=64, h=64, spp=6, clip=(0.1, 5.0), covered="some",
                     split=(MID[0], MID[1], TILTED, None)),
    "grazing": dict(tris=[GRAZING], w=64, h=64, spp=6, covered="none"),
    "behind_camera": dict(tris=[BEHIND], w=64, h=64, spp=6, covered="none"),
    "two_lights": dict(tris=[FRONT], w=32, h=32, spp=9, n_lights=2, covered="none"),
    "three_lights": dict(tris=[FRONT], w=32, h=32, spp=9, n_lights=3, covered="none"),
    "interpenetrating": dict(tris=[TILTED, FRONT], w=64, h=64, spp=6, covered="some",  # they cross on that column
                             split=(MID[0], MID[1], TILTED, FRONT)),
}


def scene_dict(ctx, rr, case):
    """The case's scene (parsed JSON) and its frame number."""
    if case["tris"] is None:
        with open(S04) as f:
            return json.load(f), case.get("frame", 1)
    p = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"])
    base = ctx.load_scene(S04)
    try:
        cam = ctx.frame_state(base, 1, p).camera.astype(np.float64)
    finally:
        base.close()
    pos, right, up, back = cam[0:3], cam[3:6], cam[6:9], cam[9:12]

    def world(q):
        q = np.asarray(q, np.float64)
        return pos + q[..., 0:1] * right + q[..., 1:2] * up - q[..., 2:3] * back

    t = np.array(case["tris"], np.float64).reshape(-1, 3, 3)
    scene = soups.soup_scene_dict(S04, 0, tris=world(t).astype(np.float32))
    obj = scene["objects"][1]
    obj.pop("animation", None)
    obj["location"] = [0.0, 0.0, 0.0]
    obj["matrix_world_saved"] = [float(x) for x in np.eye(4).reshape(-1)]
    if "clip" in case:
        scene["objects"][0]["camera"]["clip_start"], scene["objects"][0]["camera"]["clip_end"] = case["clip"]
    if "max_bounces" in case:
        scene["render"]["max_bounces"] = case["max_bounces"]
    if "mat" in case:
        for m in scene["materials"]:
            m.update(case["mat"])
    lamp = scene["objects"].pop(2)
    for k in range(case.get("n_lights", 1)):
        lo = json.loads(json.dumps(lamp))
        lo["name"] = f"Light{k}"
        at = world(np.array([LIGHT[0] - 0.7 * k, LIGHT[1], LIGHT[2] + 0.5 * k]))
        lo["location"] = [float(x) for x in at]
        lo["matrix_world_saved"][12:15] = [float(x) for x in at]
        if "light" in case:
            lo["light"]["type"], lo["light"]["radius"] = case["light"]
            if case["light"][0] == "SUN":
                lo["light"]["energy"] = 3.0
        scene["objects"].append(lo)
    return scene, 1


def load_case(ctx, rr, tmp_path, name):
    case = CASES[name]
    scene, frame = scene_dict(ctx, rr, case)
    path = str(tmp_path / f"{name}.rrscene")
    with open(path, "w") as f:
        json.dump(scene, f)
    return ctx.load_scene(path), frame


def expected_tiles(case, camera):
    """For a case with a `split`: (tiles that must be covered, tiles that must not), from the geometry in
    float64. A tile the line passes through must not be (it sees both sides); a tile on a side nothing covers
    must not be; a tile at least 5 px clear of the line (filter reach 2.5 px + tile_mask's pixel + slack) and
    5 px inside every edge of its side's triangle must be. The tiles in between are left open."""
    w, h = case["w"], case["h"]
    half_w, half_h = float(camera[12]), float(camera[13])

    def px(p):
        p = np.asarray(p, np.float64)
        return np.array([(p[0] / p[2] / half_w + 1.0) * (w * 0.5), (1.0 - p[1] / p[2] / half_h) * (h * 0.5)])

    def dist(a, b, q):  # signed distance of q from the line a -> b
        n = np.array([-(b[1] - a[1]), b[0] - a[0]])
        return float(n @ (q - a)) / float(np.hypot(*n))

    a, b, neg, pos = case["split"]
    a, b = px(a), px(b)
    sides = {False: neg and [px(v) for v in neg], True: pos and [px(v) for v in pos]}
    must = np.zeros(((h + 7) // 8, (w + 7) // 8), bool)
    must_not = np.zeros_like(must)
    for ty in range(must.shape[0]):
        for tx in range(must.shape[1]):
            corners = [np.array([8.0 * tx + dx, 8.0 * ty + dy]) for dx in (0.0, 8.0) for dy in (0.0, 8.0)]
            d = [dist(a, b, q) for q in corners]
            if min(d) <= 0.0 <= max(d):
                must_not[ty, tx] = True
                continue
            tri = sides.get(d[0] > 0.0)
            if tri is None:
                must_not[ty, tx] = True
                continue
            centre = np.mean(tri, axis=0)
            inside = min(abs(x) for x in d)
            for k in range(3):
                sgn = 1.0 if dist(tri[k], tri[(k + 1) % 3], centre) > 0.0 else -1.0
                inside = min(inside, min(sgn * dist(tri[k], tri[(k + 1) % 3], q) for q in corners))
            must[ty, tx] = inside >= 5.0
    return must, must_not


def counters(st):
    return {k: int(getattr(st, k)) for k in FIELDS}


def render_case(ctx, rr, tmp_path, name):
    """A lone frame (the sample-group variant of k_tiles) and its counting
    launch: (film, rgba, frame state, stats, counting stats, per tile the
    samples the counting launch's covered body ran, shape (tiles y, tiles x))."""
    case = CASES[name]
    s, frame = load_case(ctx, rr, tmp_path, name)
    try:
        p = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"])
        film, rgba, st = ctx.render_to_memory(s, frame, p)
        state = ctx.frame_state(s, frame, p)
        assert int(state.render_ints[7]) == 2  # the tile path
        assert len(state.lights) == case.get("n_lights", 1)
        pc = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"],
                               flags=rr.native.RR_FLAG_COUNT_TRAVERSAL)
        cfilm, crgba, cst = ctx.render_to_memory(s, frame, pc)
        assert np.array_equal(cfilm, film) and np.array_equal(crgba, rgba)
        tx, ty = (case["w"] + 7) // 8, (case["h"] + 7) // 8
        costs = ctx.tile_costs(units=0, raw=True)[0]
        cov = costs[tx * ty:2 * tx * ty].astype(np.int64).reshape(ty, tx)
    finally:
        s.close()
    return film, rgba, state, st, cst, cov


@pytest.fixture(scope="module")
def golden():
    with open(COUNTERS) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_and_counters(ctx, rr, tmp_path, golden, name):
    """Film and RGBA8 equal the oracle's at tolerance 0; the ray counters of
    the timed and of the counting launch equal the recorded ones of the build
    without the covered body."""
    film, rgba, state, st, cst, cov = render_case(ctx, rr, tmp_path, name)
    of, orgba = O.render_state(state)
    nbad = int(np.count_nonzero(rgba != orgba))
    print(name, counters(st), "triangle tests", int(cst.trav_tris[0]))
    assert nbad == 0, f"{nbad} 8-bit mismatches"
    assert np.array_equal(film, of), f"{np.count_nonzero(film != of)} film mismatches"
    assert float(np.ptp(of[..., :3])) > 0.0  # something is visible
    assert counters(st) == golden[name]["timed"]
    assert counters(cst) == golden[name]["counting"]
    assert int(cst.trav_tris[0]) == golden[name]["camera_triangle_tests"]
    # which body ran: a tile is run by one body, every sample of it
    case = CASES[name]
    print(cov)
    assert np.isin(cov, (0, case["spp"])).all()
    ran = cov == case["spp"]
    if case["covered"] == "all":
        assert ran.all()
    elif case["covered"] == "none":
        assert not ran.any()
    elif case["covered"] == "interior":
        inside = np.zeros_like(ran)
        inside[:case["h"] // 8, :case["w"] // 8] = True
        assert np.array_equal(ran, inside)
    else:
        assert ran.any() and not ran.all()
        if "split" in case:  # which tiles, from the geometry
            must, must_not = expected_tiles(case, state.camera)
            print(must.astype(int), must_not.astype(int), sep="\n")
            assert must.any() and must_not.any()
            assert ran[must].all() and not ran[must_not].any()


def test_full_frame_triangle_is_covered_everywhere(ctx, rr, tmp_path):
    """With one triangle over the whole frame every tile takes the covered
    body (the counting launch's tally says so), which traces all 64 lanes of
    every sample with one triangle test each. The input is checked first: every
    sample position (pixel centre + filter offset, below 2 px) lies inside the
    triangle's projection by more than the pixel of margin tile_mask asks for."""
    for name in ("full_front", "full_back"):
        case = CASES[name]
        w, h, spp = case["w"], case["h"], case["spp"]
        _, _, state, st, cst, cov = render_case(ctx, rr, tmp_path, name)
        assert (cov == spp).all()
        cam = state.camera.astype(np.float64)
        pos, right, up, back, half_w, half_h = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12], cam[13]
        v = state.tris.astype(np.float64).reshape(3, 3) - pos
        depth = -(v @ back)
        assert depth.min() > 1.0
        fx = ((v @ right) / depth / half_w + 1.0) * (w * 0.5)
        fy = (1.0 - (v @ up) / depth / half_h) * (h * 0.5)
        m = 4.0  # filter reach (< 2 px + a pixel of slack) + tile_mask's pixel
        corners = [(-m, -m), (w + m, -m), (-m, h + m), (w + m, h + m)]
        area = (fx[1] - fx[0]) * (fy[2] - fy[0]) - (fy[1] - fy[0]) * (fx[2] - fx[0])
        for a in range(3):
            b = (a + 1) % 3
            nx, ny = -(fy[b] - fy[a]) * np.sign(area), (fx[b] - fx[a]) * np.sign(area)
            ln = np.hypot(nx, ny)
            for cx, cy in corners:
                assert (nx * (cx - fx[a]) + ny * (cy - fy[a])) / ln >= 1.0
        assert st.camera_rays == w * h * spp
        assert cst.camera_rays_traced == w * h * spp
        assert int(cst.trav_tris[0]) == w * h * spp  # exactly one triangle test per traced ray


LEAD = "full_front"  # submitted first in every batch: a lone first frame runs sliced, the ones behind it whole
BATCHES = [list(CASES)[k:k + 6] for k in range(0, len(CASES), 6)]


@pytest.mark.parametrize("names", BATCHES, ids=[b[0] for b in BATCHES])
def test_whole_tile_variant(ctx, rr, tmp_path, golden, names):
    """Frames submitted behind a pending one overlap on the device and run
    k_tiles' whole-tile variant (one unit per tile, tile_slices == 1), the
    flagship's instantiation; every case goes through it. Their files equal the
    files of the same frames rendered one at a time (whose pixels the test
    above compares with the oracle), byte for byte, in a float and an 8-bit
    format, and their counters equal the recorded ones."""
    names = [LEAD] + list(names)
    scenes = [load_case(ctx, rr, tmp_path, n) for n in names]
    params = [rr.default_params(width=CASES[n]["w"], height=CASES[n]["h"], spp=CASES[n]["spp"]) for n in names]
    try:
        for fmt, ext in (("OPEN_EXR", "exr"), ("PNG", "png")):
            serial = []
            for i, (s, frame) in enumerate(scenes):
                ctx.render_frame(s, frame, params[i], str(tmp_path / f"s{i}"), fmt, 90)
                serial.append((tmp_path / f"s{i}.{ext}").read_bytes())
            pending, stats = [], []
            for i, (s, frame) in enumerate(scenes):
                if len(pending) == rr.native.RR_MAX_FRAMES_IN_FLIGHT:
                    stats.append(ctx.complete_frame(pending.pop(0))[1])
                pending.append(ctx.submit_frame(s, frame, params[i], str(tmp_path / f"p{i}"), fmt, 90))
            stats += [ctx.complete_frame(t)[1] for t in pending]
            for i, n in enumerate(names):
                assert (tmp_path / f"p{i}.{ext}").read_bytes() == serial[i], f"{n}: {fmt} file differs"
                assert counters(stats[i]) == golden[n]["timed"], n
            # every frame submitted while another was pending took the whole-tile variant
            assert all(st.tile_slices == 1 for st in stats[1:])
    finally:
        for s, _ in scenes:
            s.close()

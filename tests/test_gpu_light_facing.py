"""k_tiles' shading of the tiles one triangle covers (paths.hpp shade_covered)
skips the draw of a point on a point / disk light where light_behind
(csrc/rr_device.h) says the light lies wholly behind the hit's surface
(DESIGN.md §4). A skipped draw must be one whose `cosN > 0` test would have
failed: film and RGBA8 equal the oracle's bit for bit (the oracle draws at
every hit), and the ray counters equal those of the same frame rendered with
the rule compiled out (RR_LIGHT_FACING=0, which compiles tiles.hip to the
parent commit's instructions), recorded in
tests/golden/light_facing_counters.json by tools/record_light_facing.py.

Where the rule is asked: the single-triangle cases (sections 1 to 4, 7, the
odd frame's interior tiles) run the covered body in every tile, and the cubes
in the tiles inside one triangle. Their silhouette and edge tiles, the
two-light cases (no tile runs the covered body with two lights) and the later
bounces of bounces_12* and pingpong_* run shade(), which does not ask the
rule: those cases are regression checks of the code around it, and they are
the cases a rule in shade() would have to pass (it was built, measured slower
and removed: profiles/light_facing.md).

Triangles and lights are given in camera space (x right, y up, z = depth along
the view axis) and written in world space into a copy of the 04vs stand-in, as
tests/test_gpu_tile_covered.py does; its triangles are reused. A screen-filling
triangle at depth 5 is seen from its camera side whichever its winding, so
"behind its plane" is z > 5 and a light's height over the plane is 5 - z.
"""
import json
import os

import numpy as np
import pytest

import soups
import test_gpu_tile_covered as TC
from conftest import GOLDEN
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S04 = TC.S04
COUNTERS = os.path.join(GOLDEN, "light_facing_counters.json")
R = 0.25  # the disk light's radius


def at_height(hgt, x=0.5, y=0.6):
    """A light position whose centre is `hgt` above the plane z = 5 (towards the camera)."""
    return (x, y, 5.0 - hgt)


def cube3(half=1.0, z=4.5):
    """TC.lit_cube's cube turned 35 degrees about the vertical and 30 about the horizontal axis: three faces
    (quads 1, 2 and 4) show about equally; edge, corner and silhouette tiles run the general body."""
    c = np.array([[x, y, w] for x in (-half, half) for y in (-half, half) for w in (-half, half)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    a, b = np.radians(35.0), np.radians(30.0)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    c = c @ (rx @ ry).T + np.array([0.0, 0.0, z])
    return [[c[i], c[j], c[k]] for q in quads for i, j, k in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]


def face_sides(tris, light, centre):
    """Per quad of a cube (two triangles each): (faces the camera at the origin, the light's height over it)."""
    out = []
    for k in range(0, len(tris), 2):
        a, b, c = (np.asarray(x, np.float64) for x in tris[k])
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        if n @ (a - np.asarray(centre)) < 0.0:
            n = -n
        out.append((bool(n @ -a > 0.2), float(n @ (np.asarray(light, np.float64) - a))))
    return out


CUBE3_LIGHT = (-3.0, 2.5, 3.6)      # behind two of cube3's three visible faces, in front of the third
LIT_CUBE_LIGHT = (3.0, 2.5, 3.6)    # behind TC.lit_cube's front face (the one with covered tiles)
BIG_FAR = TC.big(1000.0, 200.0)     # the screen-filling triangle at depth 1e3
DISK = "POINT"

# name: tris, w, h, spp, lights [(kind, radius, camera-space position)], and what differs from the default scene.
# shadow: "none" no shadow ray may be counted (every draw skipped or discarded), "all" one per camera hit at
# bounce 0 and more, None: the recorded counters decide alone.
CASES = {
    # 1. all skipped / none skipped, both windings
    "behind_front": dict(tris=[TC.FRONT], w=32, h=32, spp=8, lights=[(DISK, R, at_height(-3.0))], shadow="none"),
    "behind_back": dict(tris=[TC.BACKSIDE], w=32, h=32, spp=8, lights=[(DISK, R, at_height(-3.0))], shadow="none"),
    "infront_front": dict(tris=[TC.FRONT], w=32, h=32, spp=8, lights=[(DISK, R, at_height(3.0))], shadow="all"),
    "infront_back": dict(tris=[TC.BACKSIDE], w=32, h=32, spp=8, lights=[(DISK, R, at_height(3.0))], shadow="all"),
    # 5. general body: cubes, an odd frame, two lights
    "cube3_two_dark": dict(tris=cube3(), w=64, h=64, spp=9, lights=[(DISK, R, CUBE3_LIGHT)]),
    "lit_cube_front_dark": dict(tris=TC.lit_cube(), w=64, h=64, spp=9, lights=[(DISK, R, LIT_CUBE_LIGHT)]),
    "edge_tiles_61x45": dict(tris=[TC.FRONT], w=61, h=45, spp=7, lights=[(DISK, R, at_height(-3.0))], shadow="none"),
    "edge_tiles_61x45_cube": dict(tris=cube3(), w=61, h=45, spp=7, lights=[(DISK, R, CUBE3_LIGHT)]),
    "two_lights": dict(tris=[TC.FRONT], w=32, h=32, spp=16,
                       lights=[(DISK, R, at_height(3.0)), (DISK, R, at_height(-3.0, x=-0.2))]),
    "two_lights_cube": dict(tris=cube3(), w=48, h=48, spp=8, lights=[(DISK, R, CUBE3_LIGHT), ("POINT", 0.0, (3.0, -2.5, 3.6))]),
    # 6. later bounces (tiles_continue): TC's bounces_12 pair, the light behind the far triangle
    "bounces_12": dict(tris=[TC.TILTED, TC.big(8.0, 2.0)], w=48, h=32, spp=11, max_bounces=12,
                       lights=[(DISK, R, (0.5, 0.6, 9.0))]),
    "bounces_12_between": dict(tris=[TC.TILTED, TC.big(8.0, 2.0)], w=48, h=32, spp=11, max_bounces=12,
                               lights=[(DISK, R, (4.0, 0.6, 7.5))]),
    # ... and a pair that faces each other across the camera (the second lies behind it, unseen): paths bounce
    # between the two up to the cap; the light behind the rear one, and between them
    "pingpong_behind": dict(tris=[TC.FRONT, TC.big(-2.0, 3.0)], w=32, h=32, spp=6, max_bounces=12,
                            lights=[(DISK, R, (0.5, 0.6, -4.0))]),
    "pingpong_between": dict(tris=[TC.FRONT, TC.big(-2.0, 3.0)], w=32, h=32, spp=6, max_bounces=12,
                             lights=[(DISK, R, (0.5, 0.6, 1.0))]),
    # 7. nothing to skip
    "sun": dict(tris=[TC.TILTED], w=48, h=32, spp=7, lights=[("SUN", 0.0, at_height(-3.0))]),
    "no_light": dict(tris=[TC.FRONT], w=32, h=32, spp=5, lights=[], shadow="none"),
    "emissive": dict(tris=[TC.FRONT], w=32, h=32, spp=9, lights=[(DISK, R, at_height(-3.0))],
                     mat=dict(emission=[1.0, 0.5, 0.25], emission_strength=2.0), shadow="none"),
}
# 2. the disk straddling the plane: centre at k radii over it (the rule's own threshold on these coordinates lies
# near -1.12: +-1.25 is the nearest pair it separates)
for k in (0.5, 0.99, 1.01, 1.1, 1.25):
    for sgn, tag in ((1.0, "p"), (-1.0, "m")):
        CASES[f"straddle_{tag}{k}"] = dict(tris=[TC.FRONT if k != 0.99 else TC.BACKSIDE], w=32, h=32, spp=10,
                                           lights=[(DISK, R, at_height(sgn * k * R, x=1.5))],
                                           shadow="none" if sgn * k <= -1.01 else None)
# 3. the plain point light, at +-1e-6 of its distance over the plane and in it
for tag, hgt in (("p", 3.0e-6), ("m", -3.0e-6), ("0", 0.0)):
    CASES[f"point_{tag}"] = dict(tris=[TC.FRONT], w=32, h=32, spp=10, lights=[("POINT", 0.0, at_height(hgt, x=3.0))])
CASES["point_behind"] = dict(tris=[TC.FRONT], w=32, h=32, spp=6, lights=[("POINT", 0.0, at_height(-3.0))],
                             shadow="none")
# a negative radius (the loader passes it on) is the plain point light, for the rule too
CASES["neg_radius_infront"] = dict(tris=[TC.FRONT], w=32, h=32, spp=6, lights=[(DISK, -1.0, at_height(0.5))],
                                   shadow="all")
CASES["neg_radius_behind"] = dict(tris=[TC.BACKSIDE], w=32, h=32, spp=6, lights=[(DISK, -1.0, at_height(-3.0))],
                                  shadow="none")
CASES["point_infront"] = dict(tris=[TC.BACKSIDE], w=32, h=32, spp=6, lights=[("POINT", 0.0, at_height(3.0))],
                              shadow="all")
# 4. large coordinates: the grazing set-ups with the light 1e4 away, and at depth 1e3 at scale 1e3 (radius 50)
for tag, k in (("p1.01", 1.01), ("m1.01", -1.01), ("m0.5", -0.5), ("m50", -50.0)):
    CASES[f"far_light_{tag}"] = dict(tris=[TC.FRONT], w=32, h=32, spp=8,
                                     lights=[(DISK, R, at_height(k * R, x=1.0e4))])
CASES["far_point_m"] = dict(tris=[TC.FRONT], w=32, h=32, spp=8, lights=[("POINT", 0.0, at_height(-1.0e-2, x=1.0e4))])
CASES["far_point_p"] = dict(tris=[TC.FRONT], w=32, h=32, spp=8, lights=[("POINT", 0.0, at_height(1.0e-2, x=1.0e4))])
for tag, k in (("p1.01", 1.01), ("m1.01", -1.01), ("m1.1", -1.1), ("m2", -2.0)):
    CASES[f"deep_{tag}"] = dict(tris=[BIG_FAR], w=32, h=32, spp=8, clip=(0.1, 1.0e5),
                                lights=[(DISK, 50.0, (100.0, 120.0, 1000.0 - k * 50.0))])


def scene_dict(ctx, rr, case):
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
    for k, (kind, radius, where) in enumerate(case["lights"]):
        lo = json.loads(json.dumps(lamp))
        lo["name"] = f"Light{k}"
        at = world(np.array(where))
        lo["location"] = [float(x) for x in at]
        lo["matrix_world_saved"][12:15] = [float(x) for x in at]
        lo["light"]["type"], lo["light"]["radius"] = kind, radius
        if kind == "SUN":
            lo["light"]["energy"] = 3.0
        elif max(abs(x) for x in where) > 100.0:  # far lights: enough energy that a lit sample is not 0 in float
            lo["light"]["energy"] = lo["light"]["energy"] * 1.0e6
        scene["objects"].append(lo)
    return scene


def load_case(ctx, rr, tmp_path, name):
    path = str(tmp_path / f"{name}.rrscene")
    with open(path, "w") as f:
        json.dump(scene_dict(ctx, rr, CASES[name]), f)
    return ctx.load_scene(path)


def render_case(ctx, rr, tmp_path, name, flags=0):
    """A lone frame (the sample-group variant of k_tiles) and its counting launch: (film, rgba, frame state,
    stats, counting stats)."""
    case = CASES[name]
    s = load_case(ctx, rr, tmp_path, name)
    try:
        p = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"], flags=flags)
        film, rgba, st = ctx.render_to_memory(s, 1, p)
        state = ctx.frame_state(s, 1, p)
        assert int(state.render_ints[7]) == (4 if flags & rr.native.RR_FLAG_WAVEFRONT else 2)
        assert len(state.lights) == len(case["lights"])
        pc = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"],
                               flags=flags | rr.native.RR_FLAG_COUNT_TRAVERSAL)
        cfilm, crgba, cst = ctx.render_to_memory(s, 1, pc)
        assert np.array_equal(cfilm, film) and np.array_equal(crgba, rgba)
    finally:
        s.close()
    return film, rgba, state, st, cst


@pytest.fixture(scope="module")
def golden():
    with open(COUNTERS) as f:
        return json.load(f)


def test_case_geometry():
    """The inputs are what the case names say (float64, camera space)."""
    sides = face_sides(cube3(), CUBE3_LIGHT, (0.0, 0.0, 4.5))
    seen = [h for vis, h in sides if vis]
    assert len(seen) == 3 and sum(h < -1.0 for h in seen) == 2 and sum(h > 1.0 for h in seen) == 1
    sides = face_sides(TC.lit_cube(), LIT_CUBE_LIGHT, (0.0, 0.0, 4.5))
    assert [h < -0.5 for vis, h in sides if vis] == [True]  # its front face, away from the light


@pytest.mark.parametrize("name", list(CASES))
def test_bits_and_counters(ctx, rr, tmp_path, golden, name):
    """Film and RGBA8 equal the oracle's at tolerance 0; the ray counters of the timed and of the counting launch
    equal the recorded ones of the build without the rule."""
    film, rgba, state, st, cst = render_case(ctx, rr, tmp_path, name)
    of, orgba = O.render_state(state)
    nbad = int(np.count_nonzero(rgba != orgba))
    print(name, TC.counters(st))
    assert nbad == 0, f"{nbad} 8-bit mismatches"
    assert np.array_equal(film, of), f"{np.count_nonzero(film != of)} film mismatches"
    assert TC.counters(st) == golden[name]["timed"]
    assert TC.counters(cst) == golden[name]["counting"]
    case = CASES[name]
    hits = case["w"] * case["h"] * case["spp"]  # the triangle fills the screen: every camera ray hits
    if case.get("shadow") == "none":
        assert st.shadow_rays == 0
    elif case.get("shadow") == "all":
        assert st.camera_rays == hits and st.shadow_rays >= hits


def test_split_path_same_frame(ctx, rr, tmp_path):
    """The split path (RR_FLAG_WAVEFRONT), whose shading does not ask the rule, renders the same frame and writes
    the same file as k_tiles."""
    for name in ("cube3_two_dark", "straddle_m1.25"):
        film, rgba, state, _, _ = render_case(ctx, rr, tmp_path, name)
        wfilm, wrgba, wstate, _, _ = render_case(ctx, rr, tmp_path, name, flags=rr.native.RR_FLAG_WAVEFRONT)
        assert np.array_equal(wfilm, film) and np.array_equal(wrgba, rgba)
        of, orgba = O.render_state(wstate)
        assert np.array_equal(wfilm, of) and np.array_equal(wrgba, orgba)
        case = CASES[name]
        s = load_case(ctx, rr, tmp_path, name)
        try:
            for tag, flags in (("t", 0), ("w", rr.native.RR_FLAG_WAVEFRONT)):
                p = rr.default_params(width=case["w"], height=case["h"], spp=case["spp"], flags=flags)
                ctx.render_frame(s, 1, p, str(tmp_path / f"{name}_{tag}"), "OPEN_EXR", 90)
        finally:
            s.close()
        assert (tmp_path / f"{name}_t.exr").read_bytes() == (tmp_path / f"{name}_w.exr").read_bytes()


LEAD = "infront_front"  # submitted first in every batch: a lone first frame runs sliced, the ones behind it whole
BATCHES = [list(CASES)[k:k + 11] for k in range(0, len(CASES), 11)]


@pytest.mark.parametrize("names", BATCHES, ids=[b[0] for b in BATCHES])
def test_whole_tile_variant(ctx, rr, tmp_path, golden, names):
    """Frames submitted behind a pending one run k_tiles' whole-tile variant, the flagship's instantiation: every
    case goes through it. Their files equal the files of the same frames rendered one at a time (whose pixels
    the test above compares with the oracle), byte for byte, and their counters equal the recorded ones."""
    names = [LEAD] + list(names)
    scenes = [load_case(ctx, rr, tmp_path, n) for n in names]
    params = [rr.default_params(width=CASES[n]["w"], height=CASES[n]["h"], spp=CASES[n]["spp"]) for n in names]
    try:
        serial = []
        for i, s in enumerate(scenes):
            ctx.render_frame(s, 1, params[i], str(tmp_path / f"s{i}"), "OPEN_EXR", 90)
            serial.append((tmp_path / f"s{i}.exr").read_bytes())
        pending, stats = [], []
        for i, s in enumerate(scenes):
            if len(pending) == rr.native.RR_MAX_FRAMES_IN_FLIGHT:
                stats.append(ctx.complete_frame(pending.pop(0))[1])
            pending.append(ctx.submit_frame(s, 1, params[i], str(tmp_path / f"p{i}"), "OPEN_EXR", 90))
        stats += [ctx.complete_frame(t)[1] for t in pending]
        for i, n in enumerate(names):
            assert (tmp_path / f"p{i}.exr").read_bytes() == serial[i], f"{n}: file differs"
            assert TC.counters(stats[i]) == golden[n]["timed"], n
        assert all(st.tile_slices == 1 for st in stats[1:])
    finally:
        for s in scenes:
            s.close()

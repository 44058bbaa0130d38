"""Device hierarchy build (bvh.hip) and walks on degenerate and boundary-size
scenes (tests/degenerate.py), against the CPU oracle at tolerance 0: both sides
run the same uncontracted fp32 op sequence. The oracle's own walks are pinned
against brute force on the same cases and rays in test_oracle.py
(test_degenerate_cases_walks_equal_brute_force), which is also where the hit
fractions asserted here were settled.

What each case exists for (bvh.hip unless said otherwise):

  n1            no internal node; nodes/children sized n > 1 ? n - 1 : 1; k_refit's
                and k_build_small's n == 1 root (both children = leaf 0); the
                collapse's one-slot root (qw_set: S.m = 1)
  n2            never PLOC (want_ploc && n > 2): Karras at hier 3 and under the collapse
  n3            the smallest PLOC build (ctl next index n - 2 = 1)
  same50        all Morton keys equal: delta()'s index tie-break 32 + clz(i ^ j);
                k_build_small's rank-by-(key, i) sort must be stable; equal t:
                the smallest original id wins (rr_device.h / wavefront.hip walks)
  same600       the same above kSmallBuild: the radix scatter's stability with one
                digit in every pass; PLOC with every merge area equal (ties: the
                lower position, one merge per round, a chain of 599 nodes)
  coplanar700   one zero-extent axis in k_morton (s = ext > 0 ? 1024 / ext : 0),
                multi-kernel build; zero-extent boxes in the 6-wide node's
                per-axis scale (q4_exponent of 0)
  coplanar40    the same through k_build_small
  line40        two zero-extent axes, every triangle zero-area, zero-volume boxes
                everywhere; the watertight test on collinear triangles
  point20       three zero-extent axes: every key 0, every box a point
  zeroarea300   zero-area leaves (two or three equal vertices) among real ones
  outlier1500   one far triangle: every other centroid in one Morton cell
  rand15/16/17  around the PLOC search radius kPlocR = 16 (n < 16: every cluster
                sees every other)
  rand31/32/33  2 kPlocR (+ 1): the window clipped at both ends / at neither
  rand63/64/65  the scatter's 64-key rounds: a full round, one key into the next
                (partial ballot, ok[r])
  rand511/512/513  kSmallBuild = 512: the last one-workgroup builds and the first
                multi-kernel LBVH (hier 2); 513 also renders through the split path
  rand1023/1024/1025  the radix sort tile kSortTile = 1024 and the scan tile
                kScanTile = 1024 (PLOC and collapse scans over bound + 1 entries:
                1024 -> a second scan tile)
  rand2049      three sort tiles, the third with one key
  rand4096/4097 exclusive_scan over m = 256 * cdiv(n, 1024) histogram words:
                1024 (one scan tile) and 1280 (the first second tile)
  rand20000     collapse levels and PLOC rounds whose scans span many scan tiles
                (build and 6-wide checks only)

Builders: on cases of 3 <= n <= 512 triangles hier=2 is built by the
one-workgroup k_build_small and hier=3 (PLOC forced) and the 6-wide collapse by
the multi-kernel path (k_transform .. k_radix_scatter, build_ploc); below 3
triangles hier=3 is k_build_small's Karras tree too and only the collapse takes
the multi-kernel path; above 512 everything is multi-kernel.
"""
import numpy as np
import pytest

import degenerate
from conftest import qbvh_leaf_positions, scene_path, walk_lbvh
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
FRAMES_LDS = ("n1", "same50", "coplanar40", "line40", "rand33")           # LDS-resident: k_tiles
FRAMES_SPLIT = ("rand513", "coplanar700", "outlier1500", "rand4097")      # split path, 6-wide hierarchy


def _load(ctx, tmp_path, name):
    path = str(tmp_path / f"{name}.rrscene")
    n = len(degenerate.scene(S04, name, path))
    s = ctx.load_scene(path)
    assert s.counts()["triangles"] == n
    return s


def _check_bvh2_boxes(children, boxes, order, tris):
    """Every child box of every BVH2 node contains the triangles below it, in
    float64 from the world triangles (leaf refs index the sorted order)."""
    t = tris.astype(np.float64)[order.astype(np.int64)]
    leaf_lo, leaf_hi = t.min(axis=1), t.max(axis=1)
    sub = {}
    stack = [(0, False)]
    while stack:
        v, done = stack.pop()
        if not done:
            stack.append((v, True))
            stack += [(int(c), False) for c in children[v] if c >= 0]
            continue
        lo, hi = [], []
        for side in range(2):
            c = int(children[v, side])
            if c < 0:
                first, count = (~c) & 0x0FFFFFFF, ((~c) >> 28) + 1
                lo_c, hi_c = leaf_lo[first:first + count].min(0), leaf_hi[first:first + count].max(0)
            else:
                lo_c, hi_c = sub.pop(c)
            b = boxes[v, 6 * side:6 * side + 6].astype(np.float64)
            assert np.all(b[0:3] <= lo_c) and np.all(hi_c <= b[3:6]), (v, side)
            lo.append(lo_c)
            hi.append(hi_c)
        sub[v] = (np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1]))


@pytest.mark.parametrize("name", degenerate.CASES)
def test_build_equals_oracle(ctx, tmp_path, name):
    """Frames 1 and 30: the LBVH (hier 2), PLOC (hier 3) and the quantised
    6-wide collapse equal the oracle's node for node (keys, order, children,
    boxes), and hold on their own: the BVH2 walk covers every leaf once, every
    child box contains its triangles, the 6-wide leaves are a permutation of
    the triangles and every 6-wide node but the root is referenced once. (Which
    builder runs for which hier and size: the module docstring.)"""
    s = _load(ctx, tmp_path, name)
    try:
        for frame in (1, 30):
            st = ctx.frame_state(s, frame)
            n = st.tris.shape[0]
            degenerate.check_property(name, st.tris)
            for hier in (2, 3):
                keys, order, children, boxes = ctx.bvh(s, frame, hier=hier)
                ok, oo, oc, ob = O.build_lbvh(st.tris, hier=hier)
                assert np.array_equal(keys, ok), (frame, hier)
                assert np.array_equal(order, oo), (frame, hier)
                assert np.array_equal(children, oc), (frame, hier, int(np.count_nonzero(children != oc)))
                assert np.array_equal(boxes, ob), (frame, hier, int(np.count_nonzero(boxes != ob)))
                assert np.all(np.diff(keys.astype(np.int64)) >= 0) and sorted(order.tolist()) == list(range(n))
                if name.startswith("same") or name == "point20":  # equal keys: the sort is stable
                    assert np.array_equal(order, np.arange(n))
                leaves, inner, _ = walk_lbvh(children)
                if n == 1:
                    assert children.tolist() == [[~0, ~0]]
                else:
                    assert sorted(leaves) == list(range(n)) and sorted(inner) == list(range(n - 1))
                _check_bvh2_boxes(children, boxes, order, st.tris)
            ch, bx, qorder = ctx.qbvh(s, frame, with_order=True)
            och, obx, oorder = O.build_qbvh(st.tris, with_order=True)
            assert ch.shape == och.shape and np.array_equal(ch, och), frame
            assert np.array_equal(bx, obx), (frame, int(np.count_nonzero(bx != obx)))
            assert np.array_equal(qorder, oorder), frame
            assert sorted(qbvh_leaf_positions(ch)) == list(range(n))
            assert sorted(qorder.tolist()) == list(range(n))
            inner = ch[(ch >= 0) & (ch != 0x7FFFFFFF)]
            assert np.array_equal(np.sort(inner), np.arange(1, ch.shape[0]))
    finally:
        s.close()


@pytest.mark.parametrize("name", degenerate.TRACE_CASES)
def test_trace_equals_oracle_and_brute_force(ctx, tmp_path, name):
    """4,096 rays (half aimed at the case from outside, half from inside its
    box) through the LBVH, PLOC, the 6-wide hierarchy and its one-LDS-entry
    walk (widths 2, 3, 4, 6): hits, ids and any-hit answers equal the oracle's
    walk of the same hierarchy, ids and t equal brute force. Then 64 packets of
    8x8 rays sharing an origin through the packet and beam walks (widths 5, 7).
    Not vacuous: more than a tenth of the rays hit wherever a triangle has
    area, none where none has, and identical triangles answer with id 0."""
    s = _load(ctx, tmp_path, name)
    try:
        st = ctx.frame_state(s, 1)
        degenerate.check_property(name, st.tris)
        rays = degenerate.rays(name, st.tris)
        assert rays.shape == (4096, 8)
        bh, bp = O.trace_brute(st.tris, rays)
        O.stack_drops(reset=True)
        for width in (2, 3, 4, 6):
            hits, prims, occ = ctx.trace(s, 1, rays, width=width)
            oh, op, oo = O.trace(st.tris, rays, width=min(width, 4))
            assert np.array_equal(prims, op), (width, int(np.count_nonzero(prims != op)))
            assert np.array_equal(hits, oh), (width, int(np.count_nonzero(hits != oh)))
            assert np.array_equal(occ, oo), (width, int(np.count_nonzero(occ != oo)))
            assert np.array_equal(prims, bp), (width, int(np.count_nonzero(prims != bp)))
            assert np.array_equal(hits[:, 0], bh[:, 0]), width
        frac = float((bp >= 0).mean())
        print(f"{name}: hit fraction {frac:.3f}")
        assert frac == 0.0 if name in degenerate.NO_AREA else frac > 0.10
        if name.startswith("same"):
            assert np.all(bp[bp >= 0] == 0)
        pk = degenerate.packet_rays(name, st.tris)
        assert pk.shape == (4096, 8) and np.all(pk[:, 0:3] == pk[0, 0:3])
        oh, op, _ = O.trace(st.tris, pk, width=4)
        assert O.stack_drops() == 0
        assert name in degenerate.NO_AREA or np.count_nonzero(op >= 0) >= 32
        for width in (5, 7):
            hits, prims, occ = ctx.trace(s, 1, pk, width=width)
            assert np.array_equal(prims, op), (width, int(np.count_nonzero(prims != op)))
            assert np.array_equal(hits, oh), (width, int(np.count_nonzero(hits != oh)))
            assert (occ == 255).all()
    finally:
        s.close()


@pytest.mark.parametrize("name", ["rand64", "coplanar40"])
def test_ray_edges_equal_oracle(ctx, tmp_path, name):
    """degenerate.edge_rays: +0.0 / -0.0 and subnormal direction components,
    rays in the plane z = const (coplanar40's own plane), origins exactly on a
    vertex, an edge and in a triangle with tmin = 0, rays along the faces of
    the root box, tmax = inf, tmin == tmax at an exact hit distance and
    tmin > tmax: the device's BVH2 and 6-wide walks answer as the oracle's."""
    s = _load(ctx, tmp_path, name)
    try:
        st = ctx.frame_state(s, 1)
        degenerate.check_property(name, st.tris)
        rays = degenerate.edge_rays(name, st.tris, O.trace_brute)
        for width in (2, 4):
            hits, prims, occ = ctx.trace(s, 1, rays, width=width)
            oh, op, oo = O.trace(st.tris, rays, width=width)
            print(f"{name}: {len(rays)} edge rays, width {width}: {int((op >= 0).sum())} hits")
            bad = np.nonzero((prims != op) | (occ != oo) | np.any(hits != oh, axis=1))[0]
            assert bad.size == 0, (width, bad.tolist(), rays[bad[:4]].tolist())
            assert (op >= 0).any() and (op < 0).any()
    finally:
        s.close()


@pytest.mark.parametrize("name", FRAMES_LDS + FRAMES_SPLIT)
def test_frames_equal_oracle(ctx, rr, tmp_path, name):
    """64 x 36 at 4 spp: film and RGBA equal the oracle's frame of the same
    state; the first group renders LDS-resident through k_tiles (hierarchy 2),
    the second through the split path (hierarchy 4); no traversal-stack push
    is dropped and every camera ray is accounted for."""
    s = _load(ctx, tmp_path, name)
    try:
        p = rr.default_params(width=64, height=36, spp=4)
        film, rgba, stats = ctx.render_to_memory(s, 1, p)
        st = ctx.frame_state(s, 1, p)
        degenerate.check_property(name, st.tris)
        assert int(st.render_ints[7]) == (2 if name in FRAMES_LDS else 4)
        assert stats.stack_drops == 0
        assert stats.camera_rays == 64 * 36 * 4
        O.stack_drops(reset=True)
        of, orgba = O.render_state(st)
        assert O.stack_drops() == 0
        assert np.array_equal(film, of), f"{np.count_nonzero(film != of)} film mismatches"
        assert np.array_equal(rgba, orgba), f"{np.count_nonzero(rgba != orgba)} 8-bit mismatches"
        seen = len(np.unique(orgba.reshape(-1, 4), axis=0)) > 1
        print(f"{name}: geometry {'visible' if seen else 'not visible'} in the frame")
        assert seen == (name not in degenerate.NO_AREA)
    finally:
        s.close()

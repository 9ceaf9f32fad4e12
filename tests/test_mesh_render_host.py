"""Host (-m "not gpu"): the numpy restatement of the mesh rasteriser (visualize.py, DESIGN.md "Mesh images") against an oracle that shares none
of its code -- point-in-triangle and depth by barycentric coordinates in fractions.Fraction -- and evaluate.vis_selection against a literal
transcription of eval.py:1054-1066.

Everything is rendered at S = 17 from the front: S - 1 = 16 is a power of two, so a vertex placed at the pixel position (px, py), multiples of
1/256, has the fixed-point coordinates (256 px, 256 py) exactly, and the sample of pixel (X, Y) sits at (X + 1/2, Y + 1/2)."""
import os
from fractions import Fraction

import numpy as np
import pytest

from garmentnets_amd import evaluate as E, visualize as V
from garmentnets_amd.io import zarr_store
from test_evaluate_host import AABB, CpuBackend, make_store

S = 17
NONE = 0xFFFFFFFF


def vert(px, py, depth=0.5):
    """the fp32 point the front camera (x, 1 - z, y) puts at the pixel position (px, py) with that depth; exact for the dyadic values used here"""
    return [px / 16, depth, 1 - py / 16]


def render(verts, faces, side="front"):
    return V._render_mesh_idx_numpy(np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3), side, S)


def barycentric(tri, X, Y):
    """the exact barycentric coordinates of the sample of pixel (X, Y) in the triangle of pixel positions `tri`; None for a zero area"""
    (ax, ay), (bx, by), (cx, cy) = [(Fraction(x), Fraction(y)) for x, y in tri]
    px, py = Fraction(2 * X + 1, 2), Fraction(2 * Y + 1, 2)
    det = (by - cy) * (ax - cx) + (cx - bx) * (ay - cy)
    if det == 0:
        return None
    la = ((by - cy) * (px - cx) + (cx - bx) * (py - cy)) / det
    lb = ((cy - ay) * (px - cx) + (ax - cx) * (py - cy)) / det
    return la, lb, 1 - la - lb


def classify(tri, X, Y):
    """'in' (strictly inside), 'out' (strictly outside) or 'edge'"""
    l = barycentric(tri, X, Y)
    if min(l) > 0:
        return "in"
    return "out" if min(l) < 0 else "edge"


def pixels():
    return [(X, Y) for Y in range(S) for X in range(S)]


# ------------------------------------------------------------------------------------------------ coverage
def test_samples_strictly_inside_are_covered_and_strictly_outside_are_not():
    rng = np.random.default_rng(0)
    seen = {"in": 0, "out": 0, "edge": 0}
    for t in range(40):
        tri = [(Fraction(int(a), 256), Fraction(int(b), 256)) for a, b in rng.integers(-2 * 256, 19 * 256, (3, 2))]
        if t % 4 == 0:                              # some vertices on samples, so that edges pass through samples
            tri = [(Fraction(int(a), 2), Fraction(int(b), 2)) for a, b in rng.integers(-3, 37, (3, 2))]
        if barycentric(tri, 0, 0) is None:
            continue
        img = render([vert(float(x), float(y)) for x, y in tri], [[0, 1, 2] if t % 2 else [0, 2, 1]])
        for X, Y in pixels():
            kind = classify(tri, X, Y)
            seen[kind] += 1
            if kind == "in":
                assert img[Y, X] == 0, (tri, X, Y)
            elif kind == "out":
                assert img[Y, X] == NONE, (tri, X, Y)
    assert seen["in"] > 500 and seen["out"] > 500 and seen["edge"] > 10


QUAD = [(2.5, 2.5), (12.5, 2.5), (12.5, 12.5), (2.5, 12.5)]        # pixel positions on samples; the diagonal 0 - 2 passes through 11 samples


@pytest.mark.parametrize("first", [[0, 1, 2], [0, 2, 1], [1, 2, 0], [2, 1, 0]])
@pytest.mark.parametrize("second", [[0, 2, 3], [0, 3, 2], [3, 0, 2], [2, 0, 3]])
def test_a_sample_on_a_shared_edge_belongs_to_exactly_one_face_in_every_stored_orientation(first, second):
    verts = [vert(x, y) for x, y in QUAD]
    alone = [render(verts, [first]), render(verts, [second])]
    both = render(verts, [first, second])
    on_edge = 0
    for X, Y in pixels():
        kinds = [classify([QUAD[i] for i in f], X, Y) for f in (first, second)]
        if kinds == ["edge", "edge"]:
            owners = [k for k in (0, 1) if alone[k][Y, X] == 0]
            if (X, Y) in ((2, 2), (12, 12)):        # the edge's end points lie on the quad's outline too: one owner at the most
                assert len(owners) <= 1
                continue
            on_edge += 1
            assert len(owners) == 1, (X, Y, owners)
            assert both[Y, X] == owners[0]
    assert on_edge == 9
    # the two faces tile the quad: its 11 x 11 samples less one owned side in each direction (hand count: half-open in x and in y)
    assert np.count_nonzero(both != NONE) == 10 * 10


def test_the_centre_of_a_closed_fan_on_a_sample_is_covered_by_exactly_one_face():
    rim = [(2.5, 3.5), (13.5, 2.5), (14.5, 13.5), (3.5, 14.5)]
    verts = [vert(8.5, 8.5)] + [vert(x, y) for x, y in rim]
    rng = np.random.default_rng(1)
    for trial in range(8):
        faces = [[0, 1 + k, 1 + (k + 1) % 4] for k in range(4)]
        faces = [f if rng.random() < 0.5 else [f[0], f[2], f[1]] for f in faces]            # any mix of stored orientations
        faces = [faces[i] for i in rng.permutation(4)]
        covering = [k for k in range(4) if render(verts, [faces[k]])[8, 8] == 0]
        assert len(covering) == 1, (faces, covering)
        assert render(verts, faces)[8, 8] == covering[0]


def test_an_axis_aligned_rectangle_covers_the_hand_count():
    for (x0, y0, x1, y1), count in (((2, 3, 9, 11), 7 * 8),             # corners between samples: the samples X = 2..8, Y = 3..10
                                    ((2.5, 3.5, 9.5, 11.5), 7 * 8),     # edges on samples: 8 x 9 samples less one owned column and one owned row
                                    ((-4, 5, 30, 6.25), 17 * 1),        # wider than the image: Y = 5 alone (5.5 is inside, 6.5 is not)
                                    ((3, 3, 3.25, 9), 0)):              # between two columns of samples
        verts = [vert(x0, y0), vert(x1, y0), vert(x1, y1), vert(x0, y1)]
        for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 2, 3]], [[1, 2, 3], [3, 0, 1]]):
            img = render(verts, faces)
            assert np.count_nonzero(img != NONE) == count, ((x0, y0, x1, y1), faces)
    # the owned column and row, stated: the edge walked downwards in the image (dy > 0 in positive orientation) and the horizontal one walked
    # towards smaller x
    img = render([vert(2.5, 3.5), vert(9.5, 3.5), vert(9.5, 11.5), vert(2.5, 11.5)], [[0, 1, 2], [0, 2, 3]])
    cols, rows = np.flatnonzero((img != NONE).any(axis=0)), np.flatnonzero((img != NONE).any(axis=1))
    assert (len(cols), len(rows)) == (7, 8)
    assert (cols[0], cols[-1]) in ((2, 8), (3, 9)) and (rows[0], rows[-1]) in ((3, 10), (4, 11))


def test_faces_that_are_never_drawn():
    tri = [vert(2, 2), vert(12, 3), vert(5, 13)]
    base = render(tri, [[0, 1, 2]])
    assert np.count_nonzero(base != NONE) > 30
    far = 16 * (2.0 ** 24 / 4096) * 1.01                                 # a camera coordinate whose fixed-point value passes 2^24
    verts = tri + [[np.nan, 0.5, 0.5], [far, 0.5, 0.5], vert(7, 7)]
    for bad in ([0, 1, 6], [0, -1, 2], [0, 1, 3], [0, 1, 4], [0, 0, 1], [0, 5, 5]):
        img = render(verts, [bad, [0, 1, 2]])
        assert np.array_equal(img == 1, base == 0) and not (img == 0).any(), bad


# ------------------------------------------------------------------------------------------------ depth
def test_depth_on_a_plane_within_the_bound_of_its_roundings():
    """z = ((w_a z_a + w_b z_b) + w_c z_c) / area2: the weights are exact, so a term goes through at most 4 roundings (its product, two sums, the
    division) and the weights are positive and sum to area2: |z - exact| <= ((1 + u)^4 - 1) max|z_i| < 5 u max|z_i|, u = 2^-53."""
    p, q, r = Fraction(1, 2), Fraction(-1, 4), Fraction(3, 8)            # depth = p * cam_x + q * cam_y + r, dyadic: every vertex depth is exact in fp32
    rng = np.random.default_rng(2)
    pos = [(Fraction(int(a), 256), Fraction(int(b), 256)) for a, b in rng.integers(0, 17 * 256, (12, 2))]
    depth = [p * x / 16 + q * y / 16 + r for x, y in pos]
    verts = np.array([vert(float(x), float(y), float(d)) for (x, y), d in zip(pos, depth)], np.float32)
    assert all(Fraction(float(v[1])) == d for v, d in zip(verts, depth))
    faces = np.array([[0, 1, 2], [3, 5, 4], [6, 7, 8], [9, 11, 10], [0, 4, 8], [2, 6, 10]], np.int32)
    idx, z = V._render_mesh_numpy(verts, faces, "front", S)
    covered = 0
    for X, Y in pixels():
        if idx[Y, X] == NONE:
            assert z[Y, X] == np.inf
            continue
        covered += 1
        exact = p * Fraction(2 * X + 1, 32) + q * Fraction(2 * Y + 1, 32) + r
        zmax = max(abs(depth[v]) for v in faces[idx[Y, X]])
        assert abs(Fraction(float(z[Y, X])) - exact) <= 5 * Fraction(1, 2 ** 53) * zmax, (X, Y)
    assert covered > 60


def test_the_nearer_face_wins_and_equal_depths_go_to_the_lowest_index():
    a = [vert(1, 1, 0.5), vert(15, 1, 0.5), vert(1, 15, 0.5)]
    b = [vert(1, 1, 0.25), vert(15, 1, 0.25), vert(1, 15, 0.25)]
    img = render(a + b, [[0, 1, 2], [3, 4, 5]])
    assert set(np.unique(img)) == {1, NONE}
    img = render(a + a, [[3, 4, 5], [0, 1, 2]])
    assert set(np.unique(img)) == {0, NONE}
    # an interpenetrating pair: each wins where the oracle's interpolated depth is smaller
    c = [vert(1, 1, 0.125), vert(15, 1, 0.75), vert(1, 15, 0.75)]
    tri = [(1, 1), (15, 1), (1, 15)]
    img = render(a + c, [[0, 1, 2], [3, 4, 5]])
    for X, Y in pixels():
        if classify(tri, X, Y) == "in":
            la, lb, lc = barycentric(tri, X, Y)
            zc = la * Fraction(1, 8) + (lb + lc) * Fraction(3, 4)
            if zc != Fraction(1, 2):
                assert img[Y, X] == (1 if zc < Fraction(1, 2) else 0)


def test_colour_is_the_shaded_barycentric_mix():
    verts = np.array([vert(1, 1, 0.5), vert(15, 1, 0.5), vert(1, 15, 0.5), vert(15, 15, 0.0)], np.float32)
    colors = np.array([[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 1, 1]], np.float32)
    flat, tilted = V.render_mesh_batch([V.mesh_spec(verts, [[0, 1, 2]], colors, ambient=0.25, default_color=(0, 0, 0, 0.5)),
                                        V.mesh_spec(verts, [[1, 3, 2]], colors, ambient=0.25)], S, backend="numpy")
    assert np.array_equal(flat[16, 16], np.float32([0, 0, 0, 0.5])) and np.array_equal(tilted[0, 0], np.float32([1, 1, 1, 0]))
    for X, Y in pixels():
        if classify([(1, 1), (15, 1), (1, 15)], X, Y) == "in":           # facing the camera: shade 1, the colour is the barycentric coordinates
            l = barycentric([(1, 1), (15, 1), (1, 15)], X, Y)
            assert np.allclose(flat[Y, X], [float(v) for v in l] + [1.0], rtol=0, atol=2 ** -22)
    # the tilted face: n = (B - A) x (C - A) in camera space, shade = 0.25 + 0.75 |n_z| / |n|
    A, B, C = (np.array(V.to_camera(verts[[i]], "front")[0]) for i in (1, 3, 2))
    n = np.cross(B - A, C - A)
    shade = 0.25 + 0.75 * abs(n[2]) / np.linalg.norm(n)
    assert 0.3 < shade < 0.95
    l = barycentric([(15, 1), (15, 15), (1, 15)], 12, 12)
    want = shade * (float(l[0]) * colors[1, :3] + float(l[1]) * colors[3, :3] + float(l[2]) * colors[2, :3])
    assert np.allclose(tilted[12, 12, :3], want, rtol=0, atol=2 ** -21) and tilted[12, 12, 3] == 1


# ------------------------------------------------------------------------------------------------ selection
def transcription(rank, samples_per_instance, num_normal, num_best):
    """eval.py:1054-1066 line for line, pandas' sort_values (ascending, NaNs last) written out for a column without equal values"""
    index = sorted((i for i in range(len(rank)) if rank[i] == rank[i]), key=lambda i: rank[i]) + [i for i in range(len(rank)) if rank[i] != rank[i]]
    best_idxs = index[:num_best]
    worst_idxs = index[-num_best:][::-1]
    vis_idxs = np.arange(num_normal) * samples_per_instance
    vis_idx_dict = dict()
    for i, idx in enumerate(vis_idxs):
        vis_idx_dict[idx] = "regular_{0:02d}".format(i)
    for i, idx in enumerate(best_idxs):
        vis_idx_dict[idx] = "best_{0:02d}".format(i)
    for i, idx in enumerate(worst_idxs):
        vis_idx_dict[idx] = "worst_{0:02d}".format(i)
    return {i: vis_idx_dict[i] for i in range(len(rank)) if i in vis_idx_dict}


NAN = float("nan")


@pytest.mark.parametrize("rank, spi, normal, best", [
    ([0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.8, 0.4], 2, 3, 2),          # best 1 5, worst 2 6, regular 0 2 4: row 2 is regular and worst
    ([0.5, NAN, 0.9, 0.3, NAN, 0.2], 1, 2, 2),                   # NaNs sort last: they are the worst
    ([0.3, 0.1], 4, 10, 3),                                      # fewer rows than labels: best and worst overlap, worst written last
    ([0.1, 0.2, 0.3, 0.4], 1, 4, 1),                             # best and regular overlap
    ([0.4, 0.2, 0.3], 1, 1, 0),                                  # num_best = 0: index[-0:] is every row
    ([NAN, NAN, NAN], 1, 1, 1),
    ([], 1, 2, 2),
])
def test_selection_restates_eval_py(rank, spi, normal, best):
    got = E.vis_selection(rank, spi, num_normal=normal, num_best=best, num_worst=7)
    assert got == transcription(rank, spi, normal, best)
    assert all(0 <= row < len(rank) for row in got)


def test_selection_hand_cases():
    assert E.vis_selection([0.5, 0.1, 0.9, 0.3, 0.7, 0.2, 0.8, 0.4], 2, 3, 2, 2) == \
        {0: "regular_00", 1: "best_00", 2: "worst_00", 4: "regular_02", 5: "best_01", 6: "worst_01"}
    assert E.vis_selection([0.3, 0.1], 4, 10, 3, 3) == {0: "worst_00", 1: "worst_01"}
    assert E.vis_selection([0.5, NAN, 0.9], 1, 0, 1, 1) == {0: "best_00", 1: "worst_00"}
    assert E.vis_selection([0.2, 0.2, 0.2], 1, 0, 1, 1) == {0: "best_00", 2: "worst_00"}          # equal values: a stable sort


# ------------------------------------------------------------------------------------------------ evaluate's visualisation section
def _vis_store(tmp_path, null=()):
    store, ds = str(tmp_path / "prediction.zarr"), str(tmp_path / "dataset.zarr")
    keys = make_store(store, 3, null=null)
    rng = np.random.default_rng(5)
    samples = zarr_store.open_group(store, create=False)["samples"]
    for k in keys:
        pc = samples[k].require_group("point_cloud")
        pc.array("pred_nocs_confidence", rng.random((50, 3 if k == keys[0] else 1)).astype(np.float32))    # per axis, as predict writes it; or one
        pc.array("input_points", (rng.random((50, 3)) * 0.5 - 0.25).astype(np.float32))
        pc.array("input_rgb", rng.integers(0, 256, (50, 3)).astype(np.uint8))
    summ = zarr_store.open_group(ds).require_group("summary")
    summ.array("cloth_canonical_aabb_union", AABB)
    summ.array("cloth_aabb_union", np.array([[-0.1, -0.1, -0.2], [1.7, 1.7, 0.3]], dtype=np.float32))
    return store, ds


def test_rank_metric_outside_the_enabled_columns_is_refused_before_any_metric(tmp_path):
    store, ds = _vis_store(tmp_path)

    class Never(CpuBackend):
        def nearest_neighbor(self, pairs):
            raise AssertionError("a metric ran")

    with pytest.raises(ValueError, match="vis_rank_metric"):
        E.evaluate_store(store, AABB, output_dir=str(tmp_path / "o"), metrics=("pc",), backend=Never(), vis_samples_per_instance=1,
                         sim_aabb=AABB)
    assert not os.path.exists(tmp_path / "o")


def test_vis_section_writes_the_panel_grids_and_leaves_the_metrics_alone(tmp_path):
    store, ds = _vis_store(tmp_path, null=(1,))
    sim_aabb = np.asarray(zarr_store.open_group(ds, create=False)["summary"]["cloth_aabb_union"])
    kw = dict(num_points=300, backend=CpuBackend())
    E.evaluate_store(store, AABB, output_dir=str(tmp_path / "plain"), **kw)
    out = E.evaluate_store(store, AABB, output_dir=str(tmp_path / "vis"), vis_samples_per_instance=1, vis_num_normal=1, vis_num_best=1,
                           vis_num_worst=1, vis_img_size=24, vis_sides=("top", "left"), sim_aabb=sim_aabb, vis_backend="numpy", **kw)
    assert not os.path.exists(tmp_path / "plain" / "vis")
    for f in ("all_metrics.csv", "all_metrics_agg.csv", "summary.json"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "vis" / f, "rb").read()
    rank = out["table"][E.DEFAULT_RANK_METRIC]
    assert np.isnan(rank[1])                                             # the null sample sorts last: it is the worst
    labels = E.vis_selection(rank, 1, 1, 1, 1)
    assert labels[1] == "worst_00" and set(labels.values()) == {"best_00", "worst_00"} | ({"regular_00"} if len(labels) == 3 else set())
    want = sorted(f"{func}_{label}.png" for func in E.VIS_FUNCS for label in labels.values())
    assert sorted(os.listdir(tmp_path / "vis" / "vis")) == want and sorted(os.path.basename(f) for f in out["vis_files"]) == want
    panels = {"task_mesh_vis": 3, "nocs_mesh_vis": 2, "nocs_pc_vis": 3}
    for func, n in panels.items():
        for row, label in labels.items():
            img = V.read_png(str(tmp_path / "vis" / "vis" / f"{func}_{label}.png"))
            assert img.shape == (2 * 24, n * 24, 4)
            drawn = [bool((img[:24, 24 * k:24 * (k + 1), 3] > 0).any()) for k in range(n)]      # the first row: seen from the top
            if func == "nocs_pc_vis":
                assert drawn == [True, True, True]
            elif func == "nocs_mesh_vis":                                # the null sample's predicted mesh panel is background
                assert drawn == [True, row != 1], (label, drawn)
            else:                                                        # (how many predicted faces pass the threshold is the store's matter)
                assert drawn[0] and drawn[2] and not (row == 1 and drawn[1]), (label, drawn)

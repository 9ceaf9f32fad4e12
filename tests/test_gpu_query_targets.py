"""GPU (-m gpu): gn_query_targets_batch (csrc/query_targets.hip, ops.query_targets_batch) and the resident dataset's exact targets
(ResidentDataset(exact_targets=True), --exact_targets) -- DESIGN.md "Exact volume targets".

What is held, per case and for all five volume groups:
  * (d2, face_idx) are torch.equal to ops.point_mesh_sqdist_batch at the widened queries and vertices, for every F;
  * w is torch.equal to ops.winding_number_batch when F <= QT_FACE_CHUNK, and within F * 2**-50 of targets.query_targets_reference for every F (the
    project's bound for a sum whose atan2 or order differs; tests/test_query_targets_host.py and DESIGN.md derive it for the chunked order);
  * every float32 target equals targets.target_from applied in numpy to the DEVICE's own fp64 w and d2, bit for bit (NaN where NaN): this holds the
    formula without making a case depend on which side of 0.5 or of a float32 rounding boundary an atan2 ulp puts w.  No case is excluded;
  * a repeated call gives the same bits; the same queries alone and inside a larger batch at another slot are torch.equal.
The shapes are the smallest at which the kernel can go wrong: F around one and two chunks, M around one workgroup's QT_SPAN = 1024 queries.
"""
import csv
import ctypes
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, ops  # noqa: E402
from garmentnets_amd import targets as TG  # noqa: E402
from garmentnets_amd import train_pipeline as TP  # noqa: E402
from garmentnets_amd.io.dataset import TASK_SPACE_VOLUME_GROUP, GarmentInputDataset  # noqa: E402
from garmentnets_amd.io.resident import ResidentDataset, held_arrays, host_sample  # noqa: E402
from test_gpu_resident import BASE, ORDER, write_awkward_store  # noqa: E402
from test_gpu_winding import sheet_mesh  # noqa: E402
from test_winding_host import box_mesh  # noqa: E402

DEV = "cuda:0"
CHUNK = TG.face_chunk()
Q = 1024                                                            # QT_SPAN: the queries of one workgroup (WN_BLOCK * QT_QPT)
FACE_COUNTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
QUERY_COUNTS = (1, Q - 1, Q, Q + 1)
WINDING = "nocs_winding_number_field"
SIGNED = "nocs_signed_distance_field"


def tol(nf):
    return nf * 2.0 ** -50


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _mesh32(v, f):
    return _t(v, torch.float32), _t(f, torch.int32)


def _same_bits(a, b):
    """float arrays equal bit for bit, a NaN matching a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    view = np.int32 if a.dtype == np.float32 else np.int64
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(view), b[~nan].view(view)))


def check_case(q, meshes, tag, w_ref=None, tsdf_clip_value=None, absolute=False):
    """q (B, M, 3) float32 numpy, meshes [(verts float32, faces)] numpy: every property of the module docstring, for the five groups.
    w_ref: per mesh, the numpy reference's w (None: the chunked sum is held to the device's other entries only).  -> {kind: target}"""
    B, M = q.shape[:2]
    qd = _t(q, torch.float32)
    dev_meshes = [_mesh32(v, f) for v, f in meshes]
    q64 = [qd[b].double() for b in range(B)]
    m64 = [(v.double(), f) for v, f in dev_meshes]
    sq = ops.point_mesh_sqdist_batch(q64, m64)
    wn = ops.winding_number_batch(q64, m64)
    out, w_first = {}, None
    for kind in TG.KINDS:
        target, w, d2, face_idx = ops.query_targets_batch(qd, dev_meshes, kind, tsdf_clip_value, absolute, return_fp64=True)
        assert target.shape == (B, M) and target.dtype == torch.float32, (tag, kind)
        assert (w is not None) == TG.needs_w(kind) and (d2 is not None) == TG.needs_d2(kind) == (face_idx is not None), (tag, kind)
        again = ops.query_targets_batch(qd, dev_meshes, kind, tsdf_clip_value, absolute, return_fp64=True)
        for a, b in zip((target, w, d2, face_idx), again):
            assert a is None or torch.equal(a.view(torch.int32 if a.dtype != torch.float64 else torch.int64),
                                            b.view(torch.int32 if b.dtype != torch.float64 else torch.int64)), (tag, kind, "repeated call")
        plain = ops.query_targets_batch(qd, dev_meshes, kind, tsdf_clip_value, absolute)
        assert _same_bits(plain.cpu().numpy(), target.cpu().numpy()), (tag, kind, "return_fp64 changes the target")
        if d2 is not None:
            for b in range(B):
                assert d2.dtype == torch.float64 and face_idx.dtype == torch.int32
                assert torch.equal(face_idx[b], sq[b][0]), (tag, kind, b, "face_idx")
                assert _same_bits(d2[b].cpu().numpy(), sq[b][1].cpu().numpy()), (tag, kind, b, "d2")
        if w is not None:
            if w_first is None:
                w_first = w
            assert torch.equal(w.view(torch.int64), w_first.view(torch.int64)), (tag, kind, "w depends on the kind")
            for b, (v, f) in enumerate(meshes):
                if len(f) <= CHUNK:
                    assert _same_bits(w[b].cpu().numpy(), wn[b].cpu().numpy()), (tag, kind, b, "w against winding_number_batch")
                if w_ref is not None:
                    got, want = w[b].cpu().numpy(), w_ref[b][:M]
                    fin = ~np.isnan(want)
                    err = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
                    assert np.array_equal(np.isnan(got), ~fin) and err <= tol(len(f)), (tag, kind, b, err, tol(len(f)))
        want = TG.target_from(None if w is None else w.cpu().numpy(), None if d2 is None else d2.cpu().numpy(), kind, tsdf_clip_value, absolute)
        assert _same_bits(target.cpu().numpy(), want), (tag, kind, "target against target_from of the device's own w, d2")
        out[kind] = target
    return out


@pytest.fixture(scope="module")
def sheet():
    """the 1922-face sheet with float32 vertices, Q + 1 seeded queries (some outside the unit cube) and the numpy reference's w per face count"""
    v, f = sheet_mesh()
    v = v.astype(np.float32)
    assert len(f) >= 2 * CHUNK + 1
    q = (np.random.default_rng(13).random((Q + 1, 3)) * 1.3 - 0.15).astype(np.float32)
    assert (q < 0).any() and (q > 1).any()
    ref = {nf: TG.query_targets_reference(q, v, f[:nf], WINDING)[1] for nf in FACE_COUNTS}
    assert np.abs(ref[2 * CHUNK + 1]).max() > 0.3
    return dict(v=v, f=f, q=q, ref=ref)


@pytest.mark.parametrize("nq", QUERY_COUNTS)
@pytest.mark.parametrize("nf", FACE_COUNTS)
def test_every_face_and_query_count(sheet, nf, nq):
    out = check_case(sheet["q"][None, :nq], [(sheet["v"], sheet["f"][:nf])], f"F={nf} M={nq}", w_ref=[sheet["ref"][nf]])
    if nf == 0:                                                          # an empty mesh: w = 0, d2 = +inf
        assert torch.equal(out[WINDING], torch.zeros_like(out[WINDING])) and bool(torch.isinf(out["nocs_distance_field"]).all())
        assert bool(torch.isinf(out[SIGNED]).all()) and torch.equal(out["nocs_occupancy_grid"], torch.zeros_like(out[WINDING]))


def test_three_ragged_meshes_in_one_launch_and_alone(sheet):
    bv, bf = box_mesh()
    meshes = [(sheet["v"], sheet["f"][:2 * CHUNK + 1]), (sheet["v"], sheet["f"][700:701]), (bv.astype(np.float32), bf)]
    M = 300
    q = np.stack([sheet["q"][:M], sheet["q"][100:100 + M], sheet["q"][300:300 + M]])
    refs = [TG.query_targets_reference(q[b], *meshes[b], WINDING)[1] for b in range(3)]
    batch = check_case(q, meshes, "ragged batch", w_ref=refs)
    for b in (2, 0, 1):                                                  # alone; and at another slot of another batch, with other neighbours
        alone = check_case(q[b:b + 1], meshes[b:b + 1], f"alone {b}")
        order = [(b + 1) % 3, b]
        moved = {k: ops.query_targets_batch(_t(q[order], torch.float32), [_mesh32(*meshes[i]) for i in order], k) for k in TG.KINDS}
        for kind in TG.KINDS:
            assert torch.equal(alone[kind][0].view(torch.int32), batch[kind][b].view(torch.int32)), (kind, b, "alone against the batch")
            assert torch.equal(moved[kind][1].view(torch.int32), batch[kind][b].view(torch.int32)), (kind, b, "another slot")


def test_degenerate_faces_and_special_queries(sheet):
    """zero-area and repeated faces; a query on a vertex, in a face's plane (the box's z = lo side, inside the face and outside it), a NaN query"""
    bv, bf = box_mesh()
    bv = bv.astype(np.float32)
    v = np.concatenate([bv, sheet["v"][:200]])
    f = np.concatenate([bf, sheet["f"][:150][sheet["f"][:150].max(axis=1) < 200] + 8]).astype(np.int32)
    f[14:18] = f[13]                                                     # repeated faces
    f[20:24, 2] = f[20:24, 0]                                            # (v0, v1, v0)
    f[25] = f[25, 0]                                                     # a point
    lo, hi = bv.min(axis=0), bv.max(axis=0)
    special = np.array([bv[0], bv[7], v[f[21, 0]], [0.5, 0.5, lo[2]], [0.05, 0.9, lo[2]], [lo[0], 0.4, 0.6], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nan],
                        [-3.0, 2.0, 7.0], [1.5, 1.5, 1.5]], dtype=np.float32)
    q = np.concatenate([special, sheet["q"][:90]])[None]
    ref = TG.query_targets_reference(q[0], v, f, WINDING)[1]
    out = check_case(q, [(v, f)], "degenerate faces, special queries", w_ref=[ref])
    for kind in TG.KINDS:                                                # a NaN query: NaN, except occupancy
        t = out[kind][0, 6:8].cpu()
        assert bool((t == 0).all()) if kind == "nocs_occupancy_grid" else bool(torch.isnan(t).all()), kind
        assert bool(torch.isfinite(out[kind][0, :6]).all()) and bool(torch.isfinite(out[kind][0, 8:]).all()), kind
    assert torch.equal(out["nocs_distance_field"][0, :3].cpu(), torch.zeros(3))      # on a vertex: distance 0
    check_case(q, [(v, f)], "tsdf clip, absolute", w_ref=[ref], tsdf_clip_value=0.05, absolute=True)
    check_case(q, [(v, f)], "tsdf clip", tsdf_clip_value=0.3)


def test_refusals_are_raised_by_name(sheet):
    qd = _t(sheet["q"][None, :5], torch.float32)
    v, f = _mesh32(sheet["v"], sheet["f"][:40])
    csr = torch.tensor([[0, 0], [v.shape[0], f.shape[0]]], dtype=torch.int64, device=DEV)
    target = torch.empty((1, 5), dtype=torch.float32, device=DEV)
    bad = torch.zeros(2, dtype=torch.int64, device=DEV)
    nbytes = _lib.load().gn_query_targets_workspace_bytes(1, 5, 40, 2)
    assert nbytes == 1 * 1 * 5 * 20 and _lib.load().gn_query_targets_workspace_bytes(2, 5, CHUNK + 1, 0) == 2 * 2 * 5 * 8
    assert _lib.load().gn_query_targets_workspace_bytes(1, 5, 40, 9) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(query=qd, verts=v, faces=f, table=csr, B=1, M=5, max_nf=40, kind=2, work=ws, work_bytes=nbytes, out=target, flags=bad):
        return _lib.call("gn_query_targets_batch", p(query), p(verts), p(faces), p(table), B, M, max_nf, kind, 0, 0.0, 0, p(work), work_bytes, p(out), None, None,
                         None, p(flags), None)
    assert call() == _lib.GN_OK
    for kw, words in ((dict(query=None), "null pointer"), (dict(out=None), "null pointer"), (dict(table=None), "null pointer"), (dict(flags=None), "null pointer"),
                      (dict(verts=None), "null pointer"), (dict(faces=None), "null pointer"), (dict(kind=4), "unknown kind 4"), (dict(kind=-1), "unknown kind"),
                      (dict(work_bytes=nbytes - 1), "short workspace"), (dict(work=None), "short workspace"), (dict(B=65536), "bad sizes"),
                      (dict(M=2 ** 31), "bad sizes"), (dict(max_nf=65536 * CHUNK), "bad sizes")):
        with pytest.raises(ValueError, match="gn_query_targets_batch: .*" + words):
            call(**kw)
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0]
    with pytest.raises(ValueError, match="unknown kind 'marching_cube_mesh'"):
        ops.query_targets_batch(qd, [(v, f)], "marching_cube_mesh")
    with pytest.raises(ValueError):
        ops.query_targets_batch(qd, [(v, f), (v, f)], WINDING)
    with pytest.raises(TypeError):
        ops.query_targets_batch(qd.double(), [(v, f)], WINDING)
    with pytest.raises(TypeError):
        ops.query_targets_batch(qd, [(v.double(), f)], WINDING)
    # a workspace sized for fewer faces than a mesh has: flagged, not walked
    with pytest.raises(_lib.GarmentNetsHipError, match="max_nf"):
        call(max_nf=CHUNK, faces=_t(sheet["f"][:CHUNK + 1], torch.int32), table=torch.tensor([[0, 0], [v.shape[0], CHUNK + 1]], dtype=torch.int64, device=DEV),
             work=torch.empty(200, dtype=torch.uint8, device=DEV), work_bytes=200)
        ops._qt_bad(bad, "query_targets")


def test_bad_face_index_raises_and_leaves_the_next_call_alone(sheet):
    qd = _t(sheet["q"][None, :63], torch.float32)
    mesh = _mesh32(sheet["v"], sheet["f"][:CHUNK + 40])
    before = ops.query_targets_batch(qd, [mesh], SIGNED)
    for kind in (WINDING, "nocs_distance_field", SIGNED):
        for where, value in ((3, len(sheet["v"])), (CHUNK + 7, -1)):         # in the first chunk, in the second
            faces = sheet["f"][:CHUNK + 40].copy()
            faces[where, 1] = value
            with pytest.raises(IndexError):
                ops.query_targets_batch(qd, [(mesh[0], _t(faces, torch.int32))], kind)
    with pytest.raises(IndexError):                                       # no queries: the faces are still checked
        ops.query_targets_batch(qd[:, :0], [(mesh[0], _t(faces, torch.int32))], WINDING)
    assert torch.equal(before, ops.query_targets_batch(qd, [mesh], SIGNED))


# ------------------------------------------------------------------------------------------------ the resident dataset
@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """two awkward 5-sample stores of the same meshes and clouds: one with 5^3 volumes, one with no `volume` group at all"""
    root = tmp_path_factory.mktemp("exact")
    out = {"volume": str(root / "v5.zarr"), "bare": str(root / "bare.zarr")}
    write_awkward_store(out["volume"], 5, seed=5)
    shutil.copytree(out["volume"], out["bare"])
    removed = [shutil.rmtree(sample / "volume") for sample in (root / "bare.zarr" / "samples").iterdir() if sample.is_dir()]
    assert len(removed) == 5
    return out


def _dataset(path, **kw):
    return GarmentInputDataset(path, volume_size=5, **{**BASE, **kw})


RES_CASES = {
    "winding": (dict(surface_sample_ratio=0.5, surface_sample_std=0.5), ORDER),
    "task_space_aug": (dict(volume_group=TASK_SPACE_VOLUME_GROUP, surface_sample_ratio=0.25, surface_sample_std=0.5, enable_augumentation=True), ORDER),
    "task_space_no_surface": (dict(volume_group=TASK_SPACE_VOLUME_GROUP, num_surface_sample=0, enable_augumentation=True), [1, 3]),
    "signed_tsdf_abs": (dict(volume_group=SIGNED, tsdf_clip_value=0.05, volume_absolute_value=True, enable_augumentation=True), [2, 3, 4]),
    "distance": (dict(volume_group="nocs_distance_field", tsdf_clip_value=0.5), [0, 1]),
    "occupancy_mc": (dict(volume_group="nocs_occupancy_grid", surface_sample_ratio=0.5, num_mc_surface_sample=50), [1, 4, 0]),
}


@pytest.mark.parametrize("name", list(RES_CASES))
def test_resident_exact_targets(stores, name):
    kw, chunk = RES_CASES[name]
    ds = _dataset(stores["volume"], **kw)
    # (the awkward store holds no distance volume: its other fields do not depend on the group, so the winding group's batch stands in for them)
    with_volume = ResidentDataset(ds if ds.volume_group != "nocs_distance_field" else _dataset(stores["volume"], **{**kw, "volume_group": WINDING}), ORDER, DEV)
    stored = with_volume.batch(chunk)
    res = ResidentDataset(_dataset(stores["bare"], **kw), ORDER, DEV, exact_targets=True)     # (marching_cube_mesh is still stored: unaffected by the flag)
    assert res.exact_targets and "volume" not in res.names and "volume" not in res.arrays and res.volume_shape == (0, 0, 0)
    assert ("task_verts" in res.names) == ds.volume_task_space
    assert res.nbytes == sum(t.numel() * t.element_size() for t in res.arrays.values())
    extra = sum(res.arrays[k].numel() * res.arrays[k].element_size() for k in set(res.names) - set(with_volume.names))      # task_verts, when only the field reads them
    assert with_volume.nbytes - res.nbytes == 5 * 5 ** 3 * 4 - extra and (extra > 0) == (name == "task_space_no_surface")
    got = res.batch(chunk)
    assert set(got.keys) == set(stored.keys)
    for k in stored.keys:                                                 # every other field, and the queries: the exact_targets=False batch, bit for bit
        if k != "gt_volume_value":
            assert torch.equal(getattr(got, k), getattr(stored, k)), (name, k)
    again = res.batch(chunk)
    assert torch.equal(got.gt_volume_value.view(torch.int32), again.gt_volume_value.view(torch.int32))
    # the values: ops.query_targets_batch at the queries BEFORE the pivot turn (the same seeded dataset without augmentation forms them un-turned)
    plain_q = got.volume_query_points
    if ds.volume_task_space and ds.enable_augumentation:
        plain_q = ResidentDataset(_dataset(stores["bare"], **{**kw, "enable_augumentation": False}), ORDER, DEV, exact_targets=True).batch(chunk).volume_query_points
        assert not torch.equal(plain_q, got.volume_query_points)
    meshes = []
    for idx in chunk:
        sample, _ = host_sample(res.dataset, idx, held_arrays(num_volume_sample=1, volume_task_space=ds.volume_task_space, exact_targets=True))
        meshes.append((sample["task_verts" if ds.volume_task_space else "nocs_verts"], sample["faces"]))
    want = ops.query_targets_batch(plain_q.contiguous(), [_mesh32(v, f) for v, f in meshes], ds.volume_group, ds.tsdf_clip_value, ds.volume_absolute_value)
    assert torch.equal(got.gt_volume_value.view(torch.int32), want.view(torch.int32)), name
    # and the host restatement: the same formula in numpy at those queries.  d2 is the same bits on both sides; the two sides' w differ by at most
    # F * 2**-50 (atan2), so their float32 roundings w32 differ by at most dw = F * 2**-50 + ulp32(w), ulp32(w) <= 2**-23 * max(1, |w|).  Hence: the winding
    # groups differ by at most dw; the signed distance by 2 dw sqrt(d2) (the sign factor 1 - 2 w32, clipped: 1-Lipschitz) plus one rounding; occupancy is
    # equal wherever |w - 0.5| > dw; the distance is equal.  tsdf_clip_value scales by 1 / tsdf (one more rounding), clip and abs are 1-Lipschitz.
    q_host = plain_q.cpu().numpy()
    for b, (v, f) in enumerate(meshes):
        ref, w, d2, _ = TG.query_targets_reference(q_host[b], v, f, ds.volume_group, ds.tsdf_clip_value, ds.volume_absolute_value)
        dev = got.gt_volume_value[b].cpu().numpy()
        dw = tol(len(f)) + 2.0 ** -23 * np.maximum(1.0, np.abs(w)) if w is not None else 0.0
        if ds.volume_group == "nocs_occupancy_grid":
            away = np.abs(w - 0.5) > dw
            assert away.sum() > len(away) // 2 and np.array_equal(dev[away], ref[away]), (name, b)
        elif ds.volume_group == "nocs_distance_field":
            assert _same_bits(dev, ref), (name, b)
        else:
            moved = 2 * dw * np.sqrt(d2) if ds.volume_group == SIGNED else dw
            slack = moved / (ds.tsdf_clip_value or 1.0) + 2.0 ** -22 * np.maximum(1.0, np.abs(ref))
            err = np.abs(dev.astype(np.float64) - ref)
            assert bool((err <= slack).all()), (name, b, float(err.max()), float(slack.max()))


def test_unknown_group_is_refused_in_the_constructor(stores):
    ds = _dataset(stores["bare"], volume_group="marching_cube_mesh")
    with pytest.raises(ValueError, match="marching_cube_mesh"):
        ResidentDataset(ds, ORDER, DEV, exact_targets=True)
    with pytest.raises(Exception):                                        # without the flag the bare store has no volume to hold
        ResidentDataset(_dataset(stores["bare"]), ORDER, DEV)
    no_queries = ResidentDataset(_dataset(stores["bare"], num_volume_sample=0, volume_group="marching_cube_mesh"), ORDER, DEV, exact_targets=True)
    assert not no_queries.exact_targets and "gt_volume_value" not in no_queries.batch([0, 1]).keys


def test_resident_entries_refuse_by_name(stores):
    res = ResidentDataset(_dataset(stores["bare"], volume_group=SIGNED), ORDER, DEV, exact_targets=True)
    B, M = 2, 7
    slots = torch.tensor([0, 3], dtype=torch.int32, device=DEV)
    query, value = torch.rand((B, M, 3), device=DEV), torch.empty((B, M), device=DEV)
    bad = torch.zeros(2, dtype=torch.int64, device=DEV)
    nbytes = _lib.load().gn_query_targets_workspace_bytes(B, M, res.max_faces, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    total = int(res.layout.offsets["verts"][-1])

    def call(sl=slots, q=query, out=value, flags=bad, kind=2, task=0, work=ws, work_bytes=nbytes, max_nf=res.max_faces, B=B):
        return _lib.call("gn_resident_query_targets", ctypes.byref(res.store), p(sl), B, M, task, total, max_nf, kind, 0, 0.0, 0, p(q), p(work), work_bytes, p(out),
                         p(flags), None)
    assert call() == _lib.GN_OK
    for kw, words in ((dict(sl=None), "null pointer"), (dict(q=None), "null pointer"), (dict(out=None), "null pointer"), (dict(flags=None), "null pointer"),
                      (dict(kind=5), "unknown kind 5"), (dict(task=1), "no task-space vertices"), (dict(work_bytes=nbytes - 1), "short workspace"),
                      (dict(work=None), "short workspace"), (dict(max_nf=0), "1 <= max_nf"), (dict(B=0), "1 <= B")):
        with pytest.raises(ValueError, match="gn_resident_query_targets: .*" + words):
            call(**kw)
    uniform = torch.rand((B, M, 3), device=DEV)

    def queries(sl=slots, u=uniform, plain=None, out=query, n_uniform=M):
        return _lib.call("gn_resident_volume_queries", ctypes.byref(res.store), p(sl), B, M, n_uniform, p(u), None, None, None, None, p(plain), p(out), None)
    assert queries() == _lib.GN_OK
    for kw, words in ((dict(sl=None), "null pointer"), (dict(out=None), "null pointer"), (dict(plain=query), "plain == query"), (dict(u=None), "uniform points"),
                      (dict(n_uniform=M - 1), "near-surface queries need"), (dict(n_uniform=M + 1), "0 <= n_uniform <= M")):
        with pytest.raises(ValueError, match="gn_resident_volume_queries: .*" + words):
            queries(**kw)
    torch.cuda.synchronize()
    assert bad.tolist() == [0, 0] and torch.equal(query, uniform)


# ------------------------------------------------------------------------------------------------ end to end
def _ckpt_equal(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_ckpt_equal(v, b[k]) for k, v in a.items())
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_ckpt_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_train_pipeline_exact_targets_run_repeats_bit_for_bit(tmp_path):
    from test_validate_host import VOLUME_SIZE, write_validation_store
    store = tmp_path / "bare.zarr"
    write_validation_store(str(store), 20, volume_groups=())              # no `volume` group at all
    common = ["--zarr_in", str(store), "--volume_size", str(VOLUME_SIZE), "--epochs", "2", "--batch_size", "2", "--num_pc_sample", "400", "--num_batches", "2",
              "--static_epoch_seed", "--no_augmentation", "--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8", "--resident", "--exact_targets"]
    runs = [TP.main(common + ["--output_dir", str(tmp_path / name)]) for name in ("a", "b")]
    keep = lambda rows: [{k: v for k, v in r.items() if k.startswith(("train_", "val_"))} for r in rows]
    assert keep(runs[0]["train_rows"]) == keep(runs[1]["train_rows"]) and len(runs[0]["train_rows"]) == 4
    assert keep(runs[0]["val_epochs"]) == keep(runs[1]["val_epochs"]) and len(runs[0]["val_epochs"]) == 2
    assert all(np.isfinite(v) for r in keep(runs[0]["train_rows"]) for v in r.values())
    rows = [list(csv.DictReader(open(tmp_path / name / "train_metrics.csv"))) for name in ("a", "b")]
    strip = lambda rs: [{k: v for k, v in r.items() if k.startswith("train_")} for r in rs]
    assert strip(rows[0]) == strip(rows[1]) and len(rows[0]) == 4
    assert all(r["exact_targets"] == "True" and r["resident"] == "True" for r in rows[0])
    assert runs[0]["resident"].exact_targets and runs[0]["val_resident"].exact_targets and "volume" not in runs[0]["resident"].arrays
    ck = [torch.load(str(tmp_path / name / "checkpoints" / "last.ckpt"), map_location="cpu", weights_only=False) for name in ("a", "b")]
    assert _ckpt_equal(ck[0]["state_dict"], ck[1]["state_dict"]) and _ckpt_equal(ck[0]["optimizer_states"], ck[1]["optimizer_states"])
    assert "exact_targets" not in ck[0]["hyper_parameters"]

"""The second stage's gt_volume_value at a query point, from the garment's mesh alone (DESIGN.md "Exact volume targets"): the numpy restatement of
csrc/query_targets.hip (gn_query_targets_batch, ops.query_targets_batch, ResidentDataset(exact_targets=True)).

Definition (normative).  A query's float32 coordinates and the float32 vertices are widened exactly to fp64.

    w         winding.py's sum with one change of order: the faces are cut into chunks of QT_FACE_CHUNK consecutive faces; each chunk's solid angles are
              added in face order from 0 (winding.solid_angle_sum_reference of the chunk); the chunk sums are added in ascending chunk order from 0; the
              total is divided by 4 pi.  A mesh of at most QT_FACE_CHUNK faces has winding_number_reference's very bits.
    d2, face  distance.py's strict-`<` minimum in face order (point_mesh_sqdist_reference): taking it per chunk and then over ascending chunks keeps the
              "lowest face index wins" rule, so the chunks do not show.

The float32 target of the dataset's volume_group (`kind`), with w32 = float32(w) -- distance.py's rules at a point instead of a lattice node:

    nocs_winding_number_field, sim_nocs_winding_number_field    w32
    nocs_distance_field                                         float32(sqrt(d2)), the root in fp64
    nocs_signed_distance_field                                  float32(clip(1 - 2*float64(w32), -1, 1) * sqrt(d2))
    nocs_occupancy_grid                                         float32(w32 > 0.5)

then the dataset's data_io steps in their order: with tsdf_clip_value, clip(v / tsdf_clip_value, -1, 1) (numpy divides a float32 array by a Python float in
float32); with absolute, abs(v).  An empty mesh gives w = 0, d2 = +inf; a NaN query gives NaN targets, except occupancy, which gives 0.

QT_FACE_CHUNK is GN_QT_FACE_CHUNK of include/garmentnets_hip.h, read from the built library (gn_query_targets_face_chunk): the one place both sides read.
"""
import numpy as np

from . import _lib
from .distance import DISTANCE_GROUP, OCCUPANCY_GROUP, SIGNED_DISTANCE_GROUP, derived_volume, point_mesh_sqdist_reference
from .winding import FOUR_PI, _mesh_arrays, solid_angle_sum_reference

WINDING_GROUPS = ("nocs_winding_number_field", "sim_nocs_winding_number_field")
KINDS = WINDING_GROUPS + (DISTANCE_GROUP, SIGNED_DISTANCE_GROUP, OCCUPANCY_GROUP)       # the keys of _lib.QT_KINDS


def face_chunk():
    """QT_FACE_CHUNK of the built library"""
    return int(_lib.load().gn_query_targets_face_chunk())


def __getattr__(name):
    if name == "QT_FACE_CHUNK":
        return face_chunk()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f"exact targets: volume_group {kind!r} has no definition on a mesh; expected one of {list(KINDS)}")
    return kind


def needs_w(kind):
    return check_kind(kind) != DISTANCE_GROUP


def needs_d2(kind):
    return check_kind(kind) in (DISTANCE_GROUP, SIGNED_DISTANCE_GROUP)


def target_from(w64, d2, kind, tsdf_clip_value=None, absolute=False):
    """the float32 target of `kind` from the fp64 winding number and squared distance (either may be None where `kind` does not read it): the table
    above, then data_io's tsdf_clip_value and volume_absolute_value steps"""
    check_kind(kind)
    with np.errstate(all="ignore"):
        w32 = np.asarray(w64, dtype=np.float64).astype(np.float32) if needs_w(kind) else None
        v = w32 if kind in WINDING_GROUPS else derived_volume(kind, d2, w32)
        if tsdf_clip_value is not None:
            v = np.clip(v / tsdf_clip_value, -1, 1)
        if absolute:
            v = np.abs(v)
    assert v.dtype == np.float32
    return v


def query_targets_reference(queries, verts, faces, kind, tsdf_clip_value=None, absolute=False, chunk=None):
    """-> (target float32 (M,), w float64 (M,), d2 float64 (M,), face_idx int32 (M,)) of the definition above for every row of `queries` (M, 3) float32
    against the mesh (verts float32, faces); w, or d2 and face_idx, are None where `kind` does not read them.  chunk: QT_FACE_CHUNK by default."""
    check_kind(kind)
    chunk = face_chunk() if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk {chunk}: at least one face per chunk")
    queries, verts = np.asarray(queries), np.asarray(verts)
    if queries.dtype != np.float32 or verts.dtype != np.float32:
        raise TypeError(f"queries and verts are float32 (widened exactly), got {queries.dtype} and {verts.dtype}")
    if queries.ndim != 2 or queries.shape[1] != 3:
        raise ValueError(f"queries: expected an (M, 3) array, got {queries.shape}")
    verts, faces = _mesh_arrays(verts, faces)
    q64 = queries.astype(np.float64)
    w = d2 = face_idx = None
    with np.errstate(all="ignore"):
        if needs_w(kind):
            total = np.zeros(len(q64), dtype=np.float64)
            for c0 in range(0, len(faces), chunk):
                total = total + solid_angle_sum_reference(q64, verts, faces[c0:c0 + chunk])
            w = total / FOUR_PI
        if needs_d2(kind):
            face_idx, d2 = point_mesh_sqdist_reference(q64, verts, faces)
    return target_from(w, d2, kind, tsdf_clip_value, absolute), w, d2, face_idx

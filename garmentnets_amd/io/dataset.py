"""Input side of the hot path: one garment sample of the dataset store -> the point cloud the network sees.

What the reference's ConvImplicitWNFDataset does for inference (/root/reference/datasets/conv_implicit_wnf_dataset.py: data_io
134-181, get_base_data 183-229, rotation_augumentation 370-406, noise_augumentation 408-423, __getitem__ 431-461) and what its
data module does to pick the samples of a subset (prepare_data 478-529), re-built around three pieces of this module's own:

  SeededDraws        the random contract in one place.  Every stage (point selection, noise, rotation) draws from a FRESH
                     numpy RandomState seeded with the sample's dataset index when ``static_epoch_seed`` (None = OS entropy
                     otherwise), in a fixed order: [views kept] -> [points kept]; [noise]; [angle].  Bit-identical samples
                     for a given (idx, static_epoch_seed=True) are pinned by tests/golden/ref_dataset.npz.
                     Its methods return the DRAWS of each sampler without the arithmetic (point_selection, volume_draws, mesh_draws, noise,
                     z_rotation); the samplers below are expressed through them, and io/resident.py uploads them to assemble batches on the device.
  visible_points     view sub-sampling as index arithmetic (np.repeat owner table + np.isin), no per-view loop.
  FIELD tables       which stored arrays feed which output fields, and which fields a rotation touches, as data.

The training / validation targets (get_volume_sample 231-281, get_surface_sample 283-334, get_mc_surface_sample 336-368) are drawn when
their sample counts are > 0 (all 0 by default: the inference samples above are unchanged), with the same random contract: each stage a
fresh RandomState(idx if static_epoch_seed else None), in the reference's order [volume]; [surface]; [mc surface] between the base data and the
noise.  Their fields come out (1, M), (1, M, 3) and (1, M, 1) per sample, (B, M, ...) after collate(), as PyG batches them.
Stores are read through garmentnets_amd.io.zarr_store (Zarr v2; uncompressed / zlib natively, anything else through numcodecs
when that package is importable).
"""
import numpy as np
import torch
from scipy.spatial.transform import Rotation

from ..batch import Batch
from ..common.metrics import barycentric_interpolation, doublearea
from . import zarr_store

# stored array (group, name) -> key of the raw sample dict
RAW_ARRAYS = {
    "cloth_sim_verts": ("mesh", "cloth_verts"),
    "cloth_nocs_verts": ("mesh", "cloth_nocs_verts"),
    "cloth_faces_tri": ("mesh", "cloth_faces_tri"),
    "pc_nocs": ("point_cloud", "nocs"),
    "pc_sim": ("point_cloud", "point"),
    "pc_sim_rgb": ("point_cloud", "rgb"),
    "pc_sizes": ("point_cloud", "sizes"),
}
RAW_ATTRS = ("scale", "grip_vertex_idx")
# per-point output field <- (raw array, divisor applied after the float32 cast)
POINT_FIELDS = {"x": ("pc_sim_rgb", 255), "y": ("pc_nocs", None), "pos": ("pc_sim", None)}
# fields a z-rotation acts on: simulation-space points always; in task space the query points turn about the NOCS cube's axis instead
SIM_SPACE_FIELDS = ("pos", "sim_grip_point", "gt_sim_points")
TASK_SPACE_SIM_FIELDS = ("pos", "sim_grip_point")
TASK_SPACE_QUERY_FIELDS = ("volume_query_points", "surf_query_points")
TASK_SPACE_PIVOT = np.array([0.5, 0.5, 0.0], dtype=np.float32)
SUBSETS = ("train", "val", "test")
# the target fields of the three samplers, float32 after collate()
TARGET_FIELDS = ("volume_query_points", "gt_volume_value", "surf_query_points", "gt_sim_points", "mc_surf_query_points", "is_query_point_on_surf")
# the volume group whose queries live in task space (the reference's dataset derives volume_task_space from it)
TASK_SPACE_VOLUME_GROUP = "sim_nocs_winding_number_field"


class SeededDraws:
    """the per-sample random streams; one fresh RandomState per stage, as the reference seeds them"""

    def __init__(self, idx, static_epoch_seed):
        self.seed = int(idx) if static_epoch_seed else None

    def fresh(self):
        return np.random.RandomState(seed=self.seed)

    def point_selection(self, view_sizes, num_views, num_points, num_stored=None):
        """-> indices (into the stored cloud) of the points kept: `num_views` of the views (only drawn when there are more), then
        `num_points` of their points without replacement.  RandomState.choice(array, n, replace=False) IS array[permutation(len)[:n]],
        which is how the pool is indexed here."""
        rs = self.fresh()
        total_views = len(view_sizes)
        if num_views < total_views:
            kept = rs.choice(total_views, size=num_views, replace=False)
            pool = visible_points(view_sizes, kept)
        else:
            pool = np.arange(int(np.sum(view_sizes)) if num_stored is None else num_stored)
        return pool[rs.choice(len(pool), size=num_points, replace=False)]

    def noise(self, std, shape):
        return self.fresh().normal(loc=np.zeros(3), scale=np.full(3, std), size=shape)

    def mesh_draws(self, num_samples):
        """-> (face uniforms (n,), uv (n, 2)), float64: what mesh_sample_barycentric draws from its fresh RandomState.  RandomState.choice(F, n,
        replace=True, p=w) IS searchsorted(face_cdf, random_sample(n), side="right"), which is how the faces are found here (sample_faces)."""
        rs = self.fresh()
        return rs.random_sample(num_samples), rs.uniform(0, 1, size=(num_samples, 2))

    def volume_draws(self, num_volume_sample, surface_sample_ratio=0, surface_sample_std=0.05):
        """the draws of get_volume_sample -> {"uniform": (n_uniform, 3) float32 query points} and, when surface_sample_ratio != 0, "face_u" / "uv"
        (mesh_draws of the n_surface near-surface points, a RandomState of their own) and "noise" (n_surface, 3) float64, drawn after the uniform
        points from their stream"""
        rs = self.fresh()
        if surface_sample_ratio == 0:
            return {"uniform": rs.uniform(low=0, high=1, size=(num_volume_sample, 3)).astype(np.float32)}
        n_uniform = int(num_volume_sample * surface_sample_ratio)
        n_surface = num_volume_sample - n_uniform
        uniform = rs.uniform(low=0, high=1, size=(n_uniform, 3)).astype(np.float32)
        face_u, uv = self.mesh_draws(n_surface)
        noise = rs.normal(loc=(0,) * 3, scale=(surface_sample_std,) * 3, size=(n_surface, 3))
        return {"uniform": uniform, "face_u": face_u, "uv": uv, "noise": noise}

    def z_angle(self, lo, hi):
        return self.fresh().uniform(lo, hi)

    def z_rotation(self, lo, hi):
        angle = self.z_angle(lo, hi)
        return Rotation.from_euler("z", angle, degrees=True).as_matrix().astype(np.float32)


def visible_points(view_sizes, kept_views):
    """ascending indices of the stored points that belong to one of `kept_views` (views are stored back to back, view_sizes[v] points each)"""
    owner = np.repeat(np.arange(len(view_sizes)), np.asarray(view_sizes, dtype=np.int64))
    return np.flatnonzero(np.isin(owner, kept_views))


def face_cdf(verts, faces):
    """the float64 table RandomState.choice(len(faces), p=area share) searches: cumsum of the normalised doubled areas, divided by its last entry"""
    w = doublearea(verts, faces)
    cdf = np.cumsum(w / np.sum(w))
    cdf /= cdf[-1]
    if np.isnan(cdf[-1]):
        raise ValueError("probabilities contain NaN")                       # (RandomState.choice's refusal of a mesh without area)
    return cdf


def sample_faces(cdf, face_u, uv, index_dtype=np.int64):
    """mesh_sample_barycentric's arithmetic on given draws -> (barycentric float64 (n, 3), face index (n,)): the face is the upper bound of its
    uniform in the CDF; u, v reflected when u + v >= 1; w = 1 - (u + v)"""
    face_idx = np.searchsorted(cdf, face_u, side="right").astype(index_dtype)
    uv = np.array(uv, dtype=np.float64)
    flip = np.sum(uv, axis=1) >= 1
    uv[flip] = 1 - uv[flip]
    bc = np.empty((len(uv), 3), dtype=uv.dtype)
    bc[:, :2] = uv
    bc[:, 2] = 1 - np.sum(uv, axis=1)
    return bc, face_idx


def _mesh_sample(draws, verts, faces, num_samples):
    return sample_faces(face_cdf(verts, faces), *draws.mesh_draws(num_samples), index_dtype=np.asarray(faces).dtype)


def data_io(sample_group):
    """one sample group of the store -> raw sample dict (data_io: 134-160, the inference subset)"""
    raw = {key: sample_group[grp][name][:] for key, (grp, name) in RAW_ARRAYS.items()}
    attrs = sample_group.attrs
    raw.update({k: attrs[k] for k in RAW_ATTRS})
    return raw


def read_volume(sample_group, volume_group="nocs_winding_number_field", volume_size=128, tsdf_clip_value=None, volume_absolute_value=False):
    """samples/<key>/volume/<volume_group>/<volume_size> -> (1, 1, D, H, W) float32 (data_io: 163-179): divided by tsdf_clip_value and clipped
    to [-1, 1] when that is set, then absolute values when volume_absolute_value"""
    volume = np.expand_dims(sample_group["volume"][volume_group][str(volume_size)][:], (0, 1)).astype(np.float32)
    if tsdf_clip_value is not None:
        volume = np.clip(volume / tsdf_clip_value, -1, 1)
    if volume_absolute_value:
        volume = np.abs(volume)
    return volume


def read_mc_mesh(sample_group):
    """the marching-cubes mesh of a sample and its per-vertex on-surface flags (data_io: 156-161)"""
    g = sample_group["marching_cube_mesh"]
    return {k: g[k][:] for k in ("marching_cube_verts", "marching_cube_faces", "is_vertex_on_surface")}


def nocs_grid_sample(volume, query_points):
    """trilinear sample of a (D, H, W) volume (any leading 1-axes) at (M, 3) points of the unit cube -> (M,) float32: the reference's
    nocs_grid_sample (components/gridding.py:45-98) = grid_sample(align_corners=True, padding_mode='border') with the zyx flip, i.e. point
    (x, y, z) reads volume[x * (D-1), y * (H-1), z * (W-1)].  fp32 in ATen's CPU order: coordinate ((2q - 1) + 1) / 2 * (size - 1) clipped
    to [0, size - 1]; corner weight (w_W * w_H) * w_D; the eight corners added to 0 in (D, H, W) bit order, those past the far face skipped."""
    vol = np.asarray(volume, dtype=np.float32)
    vol = vol.reshape(vol.shape[-3:])
    q = np.asarray(query_points, dtype=np.float32)
    one, two = np.float32(1), np.float32(2)
    lo, frac = [], []
    for ax in range(3):
        n = vol.shape[ax]
        c = np.minimum(np.float32(n - 1), np.maximum((((two * q[:, ax] - one) + one) / two) * np.float32(n - 1), np.float32(0)))
        f0 = np.floor(c)
        lo.append(f0)
        frac.append(((f0 + one) - c, c - f0))                                # weights of the low and the high corner
    out = np.zeros(len(q), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for corner in range(8):
            bit = [(corner >> 2) & 1, (corner >> 1) & 1, corner & 1]
            w = (frac[2][bit[2]] * frac[1][bit[1]]) * frac[0][bit[0]]
            idx = [lo[ax] + np.float32(bit[ax]) for ax in range(3)]
            inb = np.ones(len(q), dtype=bool)
            for ax in range(3):
                inb &= (idx[ax] >= 0) & (idx[ax] <= vol.shape[ax] - 1)
            ii = [np.where(inb, idx[ax], 0).astype(np.int64) for ax in range(3)]
            out = np.where(inb, out + vol[ii[0], ii[1], ii[2]] * w, out)
    return out


class AABBGripNormalizer:
    """task-space normaliser (common/geometry_util.py:100-123): the simulation-space box (2, 3) into the unit NOCS cube, x / y centred on 0.5,
    the top of z at 1 - padding; the same numpy operations in the same order"""

    def __init__(self, aabb, padding=0.05):
        nocs_radius = 0.5 - padding
        radius = np.max(np.abs(aabb), axis=0)[:2]
        radius_scale = np.min(nocs_radius / radius)
        z_scale = (nocs_radius * 2) / (aabb[1, 2] - aabb[0, 2])
        self.scale = min(radius_scale, z_scale)
        self.offset = np.array([0.5, 0.5, 1 - padding - aabb[1, 2] * self.scale], dtype=aabb.dtype)

    def __call__(self, data):
        return (data * self.scale) + self.offset


def _for_batching(data):
    return {k: v.reshape((1,) + v.shape) for k, v in data.items()}


def get_volume_sample(idx, data_in, volume, num_volume_sample, surface_sample_ratio=0, surface_sample_std=0.05, static_epoch_seed=False,
                      volume_group="nocs_winding_number_field"):
    """volume query points and the volume's values there (get_volume_sample: 231-281).  surface_sample_ratio == 0: uniform points of the unit
    cube; otherwise int(num_volume_sample * surface_sample_ratio) UNIFORM points (the reference sizes the uniform part by the ratio) followed
    by points of the NOCS mesh plus N(0, surface_sample_std) noise, all clipped to [0, 1].  Occupancy grids threshold the value at > 0.1."""
    d = SeededDraws(idx, static_epoch_seed).volume_draws(num_volume_sample, surface_sample_ratio, surface_sample_std)
    if surface_sample_ratio == 0:
        query = d["uniform"]
    else:
        verts, faces = data_in["cloth_nocs_verts"], data_in["cloth_faces_tri"]
        bc, face_idx = sample_faces(face_cdf(verts, faces), d["face_u"], d["uv"], index_dtype=np.asarray(faces).dtype)
        on_mesh = barycentric_interpolation(bc, verts, faces[face_idx])
        query = np.clip(np.concatenate([d["uniform"], on_mesh + d["noise"]], axis=0).astype(np.float32), 0, 1)
    values = nocs_grid_sample(volume, query)
    if volume_group == "nocs_occupancy_grid":
        values = (values > 0.1).astype(np.float32)
    return _for_batching({"volume_query_points": query, "gt_volume_value": values})


def check_surface_normal_noise(surface_normal_noise_ratio):
    if surface_normal_noise_ratio != 0:
        raise NotImplementedError("surface_normal_noise_ratio != 0 needs libigl's per-vertex normals, which this package does not carry "
                                  "(the shipped configs set surface_normal_noise_ratio: 0)")


def get_surface_sample(idx, data_in, num_surface_sample, static_epoch_seed=False, volume_task_space=False, cloth_sim_aabb=None,
                       surface_normal_noise_ratio=0):
    """points of the garment mesh in the decoder's query space and their simulation-space positions (get_surface_sample: 283-334); in
    task space the roles swap: queries are the AABBGripNormalizer'd simulation vertices' points, targets the NOCS ones"""
    check_surface_normal_noise(surface_normal_noise_ratio)
    nocs_verts, sim_verts, faces = data_in["cloth_nocs_verts"], data_in["cloth_sim_verts"], data_in["cloth_faces_tri"]
    if volume_task_space:
        nocs_verts, sim_verts = AABBGripNormalizer(cloth_sim_aabb)(sim_verts), nocs_verts
    bc, face_idx = _mesh_sample(SeededDraws(idx, static_epoch_seed), nocs_verts, faces, num_surface_sample)
    sampled_faces = faces[face_idx]
    return _for_batching({"surf_query_points": barycentric_interpolation(bc, nocs_verts, sampled_faces),
                          "gt_sim_points": barycentric_interpolation(bc, sim_verts, sampled_faces)})


def get_mc_surface_sample(idx, data_in, num_surface_sample, static_epoch_seed=False):
    """points of the marching-cubes mesh and whether each lies on the garment's surface (get_mc_surface_sample: 336-368): the interpolated
    per-vertex flag > 0.5.  The reference draws num_surface_sample points here, not num_mc_surface_sample; so does this."""
    verts, faces = data_in["marching_cube_verts"], data_in["marching_cube_faces"]
    flags = np.expand_dims(data_in["is_vertex_on_surface"].astype(np.float32), axis=-1)
    bc, face_idx = _mesh_sample(SeededDraws(idx, static_epoch_seed), verts, faces, num_surface_sample)
    sampled_faces = faces[face_idx]
    on_surface = barycentric_interpolation(bc, flags, sampled_faces)
    return _for_batching({"mc_surf_query_points": barycentric_interpolation(bc, verts, sampled_faces),
                          "is_query_point_on_surf": (on_surface > 0.5).astype(np.float32)})


def get_base_data(idx, data_in, num_pc_sample=6000, num_views=4, static_epoch_seed=False, cloth_sim_aabb=None):
    """raw sample -> the un-augmented network input (get_base_data: 183-229): colour / NOCS label / position of the selected points
    (float32; colours / 255), the grip vertex in both spaces, the selected point nearest to it, bookkeeping fields"""
    sel = SeededDraws(idx, static_epoch_seed).point_selection(data_in["pc_sizes"], num_views, num_pc_sample, len(data_in["pc_sim"]))
    out = {}
    for field, (src, divisor) in POINT_FIELDS.items():
        v = data_in[src][sel].astype(np.float32)
        out[field] = v if divisor is None else v / np.float32(divisor)
    g = data_in["grip_vertex_idx"]
    grip = {"sim_grip_point": data_in["cloth_sim_verts"][g][None, :], "nocs_grip_point": data_in["cloth_nocs_verts"][g][None, :]}
    nearest = int(np.argmin(np.linalg.norm(out["pos"] - grip["sim_grip_point"][0], axis=1)))
    out["scale"] = np.array([data_in["scale"]])
    out.update(grip)
    out["grip_pc_idx"] = np.array([nearest])
    out["dataset_idx"] = np.array([idx])
    if cloth_sim_aabb is not None:
        out["cloth_sim_aabb"] = np.asarray(cloth_sim_aabb)[None]
    return out


def noise_augmentation(idx, data, pc_noise_std, static_epoch_seed=False):
    """isotropic Gaussian jitter of the input positions (noise_augumentation: 408-423); float64 out, as numpy promotes it"""
    jitter = SeededDraws(idx, static_epoch_seed).noise(pc_noise_std, data["pos"].shape)
    return {**data, "pos": data["pos"] + jitter}


def rotation_augmentation(idx, data, random_rot_range=(-90, 90), static_epoch_seed=False, volume_task_space=False):
    """random rotation about z of everything that lives in simulation space (rotation_augumentation: 370-406); the matrix is recorded as
    `input_aug_rot_mat` (1,3,3) because predict / eval rotate the ground-truth mesh with it"""
    lo, hi = random_rot_range
    if lo > hi:
        raise AssertionError("random_rot_range must be (low, high)")
    R = SeededDraws(idx, static_epoch_seed).z_rotation(lo, hi)
    turned = dict(data)
    plain = TASK_SPACE_SIM_FIELDS if volume_task_space else SIM_SPACE_FIELDS
    pivoted = TASK_SPACE_QUERY_FIELDS if volume_task_space else ()
    turned.update({k: (data[k] @ R.T).astype(np.float32) for k in plain if k in data})
    turned.update({k: ((data[k] - TASK_SPACE_PIVOT) @ R.T + TASK_SPACE_PIVOT).astype(np.float32) for k in pivoted if k in data})
    turned["input_aug_rot_mat"] = R[None]
    return turned


def instance_split(sample_ids, dataset_split=(8, 1, 1), split_seed=0):
    """the data module's seeded train / val / test split (prepare_data: 478-529; predict.py:63-66 iterates `prediction.subset`).

    Samples sharing a `sample_id` are one garment INSTANCE and never straddle two subsets.  Instances are ordered by sorted id; with
    n instances the subset sizes are trunc(n * share) with the remainder given to train; a RandomState(split_seed) permutation of the
    instance order is cut in that order (train, val, test); a subset's samples = the ascending dataset indices of its instances.
    -> {"train": idx array, "val": ..., "test": ...}"""
    if len(dataset_split) != len(SUBSETS):
        raise AssertionError("dataset_split = (train, val, test) shares")
    uniq, inst_of_sample = np.unique(np.asarray(sample_ids), return_inverse=True)      # sorted ids, like the reference's group-by
    n = len(uniq)
    share = np.asarray(dataset_split, dtype=np.float64)
    counts = (share / share.sum() * n).astype(np.int64)
    counts[0] += n - counts.sum()
    order = np.random.RandomState(seed=split_seed).permutation(n)
    cuts = np.concatenate([[0], np.cumsum(counts)])
    return {name: np.flatnonzero(np.isin(inst_of_sample, order[cuts[i]:cuts[i + 1]])) for i, name in enumerate(SUBSETS)}


class GarmentInputDataset:
    """dataset[idx] -> dict of numpy arrays (the fields of the reference's Data object that the inference path and predict.py
    read); collate() -> Batch.  Constructor arguments carry the reference's names and defaults.  ``subset_indices(name)`` gives the
    dataset indices predict iterates for ``prediction.subset = name``."""

    def __init__(self, zarr_path, num_pc_sample=6000, enable_augumentation=True, random_rot_range=(-90, 90), num_views=4,
                 pc_noise_std=0, static_epoch_seed=False, volume_task_space=False, dataset_split=(8, 1, 1), split_seed=0,
                 num_volume_sample=0, num_surface_sample=0, num_mc_surface_sample=0, surface_sample_ratio=0, surface_sample_std=0.05,
                 surface_normal_noise_ratio=0, surface_normal_std=0, volume_size=128, volume_group="nocs_winding_number_field",
                 tsdf_clip_value=None, volume_absolute_value=False, **kwargs):
        if num_views <= 0:
            raise AssertionError("num_views > 0")
        if num_surface_sample > 0:
            check_surface_normal_noise(surface_normal_noise_ratio)
        if volume_group == TASK_SPACE_VOLUME_GROUP:
            volume_task_space = True
            if num_mc_surface_sample != 0:
                raise AssertionError("num_mc_surface_sample must be 0 for task-space volumes")
        self.num_volume_sample, self.num_surface_sample, self.num_mc_surface_sample = num_volume_sample, num_surface_sample, num_mc_surface_sample
        self.surface_sample_ratio, self.surface_sample_std = surface_sample_ratio, surface_sample_std
        self.surface_normal_noise_ratio, self.surface_normal_std = surface_normal_noise_ratio, surface_normal_std
        self.volume_size, self.volume_group, self.tsdf_clip_value, self.volume_absolute_value = volume_size, volume_group, tsdf_clip_value, volume_absolute_value
        root = zarr_store.open_group(zarr_path, create=False)
        self.samples_group = root["samples"]
        self.keys = sorted(self.samples_group.keys())
        self.num_pc_sample, self.enable_augumentation, self.random_rot_range = num_pc_sample, enable_augumentation, tuple(random_rot_range)
        self.num_views, self.pc_noise_std, self.static_epoch_seed, self.volume_task_space = num_views, pc_noise_std, static_epoch_seed, volume_task_space
        self.dataset_split, self.split_seed = tuple(dataset_split), split_seed
        self.cloth_sim_aabb = root["summary"]["cloth_aabb_union"][:].astype(np.float32)
        self._split = None

    def __len__(self):
        return len(self.keys)

    def sample_ids(self):
        """`sample_id` attribute of every sample, in dataset order (a store without the attribute: every sample its own instance)"""
        return [self.samples_group[k].attrs.get("sample_id", k) for k in self.keys]

    def subset_indices(self, subset):
        if subset not in SUBSETS:
            raise KeyError(f"subset {subset!r}: expected one of {SUBSETS}")
        if self._split is None:
            self._split = instance_split(self.sample_ids(), self.dataset_split, self.split_seed)
        return self._split[subset]

    def __getitem__(self, idx):
        idx = int(idx)
        group = self.samples_group[self.keys[idx]]
        data_in = data_io(group)
        sample = get_base_data(idx, data_in, self.num_pc_sample, self.num_views, self.static_epoch_seed, self.cloth_sim_aabb)
        if self.num_volume_sample > 0:
            volume = read_volume(group, self.volume_group, self.volume_size, self.tsdf_clip_value, self.volume_absolute_value)
            sample.update(get_volume_sample(idx, data_in, volume, self.num_volume_sample, self.surface_sample_ratio, self.surface_sample_std,
                                            self.static_epoch_seed, self.volume_group))
        if self.num_surface_sample > 0:
            sample.update(get_surface_sample(idx, data_in, self.num_surface_sample, self.static_epoch_seed, self.volume_task_space,
                                             self.cloth_sim_aabb, self.surface_normal_noise_ratio))
        if self.num_mc_surface_sample > 0:
            sample.update(get_mc_surface_sample(idx, {**data_in, **read_mc_mesh(group)}, self.num_surface_sample, self.static_epoch_seed))
        sample["input_aug_rot_mat"] = np.eye(3, dtype=np.float32)[None]
        if self.pc_noise_std > 0:
            sample = noise_augmentation(idx, sample, self.pc_noise_std, self.static_epoch_seed)
        if self.enable_augumentation:
            sample = rotation_augmentation(idx, sample, self.random_rot_range, self.static_epoch_seed, self.volume_task_space)
        return sample

    @staticmethod
    def collate(samples):
        """PyG-style batching: every field concatenated along dim 0, plus the `batch` vector of the per-point fields; the target fields
        (1, M[, C]) per sample -> (B, M[, C]) float32"""
        sizes = [len(s["pos"]) for s in samples]
        cat = {k: torch.from_numpy(np.concatenate([np.asarray(s[k]) for s in samples], axis=0)) for k in samples[0]}
        cat["pos"], cat["x"] = cat["pos"].float(), cat["x"].float()
        cat.update({k: cat[k].float() for k in TARGET_FIELDS if k in cat})
        batch = torch.repeat_interleave(torch.arange(len(samples)), torch.tensor(sizes))
        return Batch(sizes=sizes, batch=batch, **cat)

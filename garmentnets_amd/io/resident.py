"""A subset of a dataset store held in device memory, and its batches assembled there (DESIGN.md "Resident dataset").

  ResidentDataset(dataset, indices, device)   reads every sample of `indices` ONCE through the host dataset's own readers (dataset.data_io / read_volume /
                                              read_mc_mesh: the codecs and the tsdf_clip_value / volume_absolute_value handling are theirs) and packs them
                                              into a few device arrays, ragged parts back to back with CSR offsets (plan()).  What depends on the stored
                                              sample alone -- the fp64 face-area CDFs RandomState.choice searches, the task-space vertices -- is computed at
                                              load by the host code (dataset.face_cdf, AABBGripNormalizer) and stored beside it: its bits are the host's.
  resident.batch(chunk) -> Batch              on the device, with the keys, shapes and dtypes of GarmentInputDataset.collate([dataset[k] for k in chunk])
                                              .to(device).  The random contract does not move: every draw comes from dataset.SeededDraws on the host, a fresh
                                              RandomState per stage; the chunk's draws go into one pinned buffer (draw_sections()) and up in one async copy;
                                              at most five gn_resident_* launches (csrc/resident.hip) do the selection, the target sampling, the ground-truth
                                              lookup and the augmentation.  Nothing is read back and the stream is not synchronised.
  ResidentDataset(..., exact_targets=True)    holds no volume: gt_volume_value is the field of the garment's own resident mesh at the same query points
                                              (targets.py; gn_resident_volume_queries + gn_resident_query_targets), so a store without a `volume` group trains.

Not here: a device RNG (it would break the seeded contract validation relies on), fp16 volumes, eviction.
"""
import time
from collections import namedtuple

import numpy as np
import torch

from .. import _lib, ops, targets
from ..batch import Batch
from . import dataset as D

# resident array -> (the per-sample count it is ragged in, floats / ints per row, dtype)
ARRAY_SPECS = {
    "pc_sim": ("points", 3, np.float32), "pc_nocs": ("points", 3, np.float32), "pc_rgb": ("points", 3, np.uint8),
    "sim_verts": ("verts", 3, np.float32), "nocs_verts": ("verts", 3, np.float32), "task_verts": ("verts", 3, np.float32),
    "faces": ("faces", 3, np.int32), "cdf_nocs": ("faces", 1, np.float64), "cdf_task": ("faces", 1, np.float64),
    "mc_verts": ("mc_verts", 3, np.float32), "mc_flags": ("mc_verts", 1, np.float32), "mc_faces": ("mc_faces", 3, np.int32),
    "cdf_mc": ("mc_faces", 1, np.float64), "volume": ("voxels", 1, np.float32),
}
COUNTS = ("points", "verts", "faces", "mc_verts", "mc_faces", "voxels")
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}
_SCALE_TORCH = {"f": torch.float64, "i": torch.int64, "u": torch.int64}     # the batch's `scale` field: the 8 bytes of np.array([attrs["scale"]])
DRAW_RING = 3                                   # pinned draw buffers in flight: a buffer is reused only after its own upload has finished

Layout = namedtuple("Layout", "arrays offsets nbytes staging_bytes")
DrawLayout = namedtuple("DrawLayout", "sections nbytes")


def held_arrays(num_volume_sample=0, num_surface_sample=0, num_mc_surface_sample=0, surface_sample_ratio=0, volume_task_space=False, exact_targets=False):
    """the names of ARRAY_SPECS a dataset with these sampler settings needs resident.  exact_targets: gt_volume_value comes from the mesh
    (targets.py), so no volume is held; in task space the field is the one of the task-space vertices, which are then held."""
    near = num_volume_sample > 0 and surface_sample_ratio != 0
    surf = num_surface_sample > 0
    names = ["pc_sim", "pc_nocs", "pc_rgb", "sim_verts", "nocs_verts", "faces"]
    if near or (surf and not volume_task_space):
        names.append("cdf_nocs")
    if surf and volume_task_space:
        names += ["task_verts", "cdf_task"]
    elif exact_targets and num_volume_sample > 0 and volume_task_space:
        names.append("task_verts")
    if num_mc_surface_sample > 0:
        names += ["mc_verts", "mc_flags", "mc_faces", "cdf_mc"]
    if num_volume_sample > 0 and not exact_targets:
        names.append("volume")
    return tuple(names)


def _align8(n):
    return (n + 7) // 8 * 8


def plan(counts, names):
    """counts: one {points, verts, faces, mc_verts, mc_faces, voxels} per sample (array SHAPES only) -> Layout: arrays {name: (rows, width, dtype)}, offsets
    {count: int64 (n + 1,) CSR table}, nbytes (the device footprint: the arrays, the meta and grip tables, the bounding box) and the pinned staging bytes
    (the largest sample, every array 8-byte aligned).  Nothing is read or allocated."""
    n = len(counts)
    offsets = {c: np.concatenate([[0], np.cumsum([int(s[c]) for s in counts], dtype=np.int64)]).astype(np.int64) for c in COUNTS}
    arrays = {k: (int(offsets[ARRAY_SPECS[k][0]][-1]), ARRAY_SPECS[k][1], np.dtype(ARRAY_SPECS[k][2])) for k in names}
    nbytes = sum(rows * width * dt.itemsize for rows, width, dt in arrays.values())
    nbytes += n * len(_lib.RESIDENT_META) * 8 + n * 6 * 4 + 6 * 4
    staging = max((sum(_align8(int(s[ARRAY_SPECS[k][0]]) * ARRAY_SPECS[k][1] * np.dtype(ARRAY_SPECS[k][2]).itemsize) for k in names) for s in counts), default=0)
    return Layout(arrays, offsets, int(nbytes), int(staging))


def draw_sections(B, num_pc_sample, num_volume_sample=0, n_uniform=0, num_surface_sample=0, mc=False, near=False, pc_noise=False, rotation=False):
    """the layout of one batch's draw buffer -> DrawLayout(sections {name: (byte offset, numpy dtype, shape)}, nbytes): fp64 sections first, then fp32, then
    int32, so every section is aligned to its type"""
    P, n_surface, Ms = num_pc_sample, num_volume_sample - n_uniform, num_surface_sample
    want = []
    if near:
        want += [("vol_face_u", np.float64, (B, n_surface)), ("vol_uv", np.float64, (B, n_surface, 2)), ("vol_noise", np.float64, (B, n_surface, 3))]
    if Ms > 0:
        want += [("surf_face_u", np.float64, (B, Ms)), ("surf_uv", np.float64, (B, Ms, 2))]
    if mc:
        want += [("mc_face_u", np.float64, (B, Ms)), ("mc_uv", np.float64, (B, Ms, 2))]
    if pc_noise:
        want.append(("pc_noise", np.float64, (B, P, 3)))
    if num_volume_sample > 0:
        want.append(("vol_uniform", np.float32, (B, n_uniform, 3)))
    if rotation:
        want.append(("rot", np.float32, (B, 3, 3)))
    want += [("sel", np.int32, (B, P)), ("slots", np.int32, (B,))]
    sections, off = {}, 0
    for name, dt, shape in want:
        sections[name] = (off, np.dtype(dt), shape)
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    return DrawLayout(sections, _align8(off))


def sample_counts(dataset, idx, names):
    """the counts of one sample from the arrays' metadata alone"""
    group = dataset.samples_group[dataset.keys[int(idx)]]
    shape = lambda grp, name: group[grp].array_meta(name)[0]
    out = {"points": shape("point_cloud", "point")[0], "verts": shape("mesh", "cloth_verts")[0], "faces": shape("mesh", "cloth_faces_tri")[0],
           "mc_verts": 0, "mc_faces": 0, "voxels": 0, "volume_shape": (0, 0, 0)}
    if "mc_verts" in names:
        mc = group["marching_cube_mesh"]
        out["mc_verts"], out["mc_faces"] = mc.array_meta("marching_cube_verts")[0][0], mc.array_meta("marching_cube_faces")[0][0]
    if "volume" in names:
        vs = tuple(group["volume"][dataset.volume_group].array_meta(str(dataset.volume_size))[0])
        if len(vs) != 3:
            raise ValueError(f"sample {idx}: volume of shape {vs}, expected (D, H, W)")
        out["volume_shape"], out["voxels"] = vs, int(np.prod(vs))
    return out


def _f32_verts(a, name, idx):
    if a.dtype != np.float32:
        raise TypeError(f"sample {idx}: {name} is {a.dtype}; the resident kernels interpolate float32 vertices (as the shipped stores hold them)")
    return a


def _faces(faces, num_verts, name, idx):
    f = np.asarray(faces)
    if len(f) == 0 or f.min() < 0 or f.max() >= num_verts:
        raise ValueError(f"sample {idx}: {name} is empty or names a vertex outside [0, {num_verts})")
    return f.astype(np.int32)


def host_sample(dataset, idx, names):
    """one sample read through the host dataset's readers -> ({resident array name: numpy array}, extras): the arrays as they go to the device, the
    CDFs and the task-space vertices computed by the host code"""
    idx = int(idx)
    group = dataset.samples_group[dataset.keys[idx]]
    raw = D.data_io(group)
    if raw["pc_sim_rgb"].dtype != np.uint8:
        raise TypeError(f"sample {idx}: point_cloud/rgb is {raw['pc_sim_rgb'].dtype}, expected uint8")
    sim, nocs = _f32_verts(raw["cloth_sim_verts"], "cloth_verts", idx), _f32_verts(raw["cloth_nocs_verts"], "cloth_nocs_verts", idx)
    faces = _faces(raw["cloth_faces_tri"], len(sim), "cloth_faces_tri", idx)
    out = {"pc_sim": raw["pc_sim"].astype(np.float32), "pc_nocs": raw["pc_nocs"].astype(np.float32), "pc_rgb": raw["pc_sim_rgb"],
           "sim_verts": sim, "nocs_verts": nocs, "faces": faces}
    if "cdf_nocs" in names:
        out["cdf_nocs"] = D.face_cdf(nocs, raw["cloth_faces_tri"])
    if "task_verts" in names:
        out["task_verts"] = _f32_verts(D.AABBGripNormalizer(dataset.cloth_sim_aabb)(sim), "the task-space normalised cloth_verts", idx)
    if "cdf_task" in names:
        out["cdf_task"] = D.face_cdf(out["task_verts"], raw["cloth_faces_tri"])
    if "mc_verts" in names:
        mc = D.read_mc_mesh(group)
        out["mc_verts"] = _f32_verts(mc["marching_cube_verts"], "marching_cube_verts", idx)
        out["mc_flags"] = mc["is_vertex_on_surface"].astype(np.float32)
        out["mc_faces"] = _faces(mc["marching_cube_faces"], len(out["mc_verts"]), "marching_cube_faces", idx)
        out["cdf_mc"] = D.face_cdf(out["mc_verts"], mc["marching_cube_faces"])
    if "volume" in names:
        out["volume"] = D.read_volume(group, dataset.volume_group, dataset.volume_size, dataset.tsdf_clip_value, dataset.volume_absolute_value)[0, 0]
    g = raw["grip_vertex_idx"]
    scale = np.array([raw["scale"]])
    if scale.dtype.itemsize != 8:
        raise TypeError(f"sample {idx}: scale attribute of dtype {scale.dtype}")
    extras = {"grip": np.concatenate([sim[g], nocs[g]]).astype(np.float32), "scale": scale, "pc_sizes": np.asarray(raw["pc_sizes"]),
              "pc_len": len(raw["pc_sim"])}
    return out, extras


class ResidentDataset:
    def __init__(self, dataset, indices, device, max_bytes=None, exact_targets=False):
        """exact_targets: gt_volume_value is the field of the garment's own mesh at the query points (targets.py, gn_resident_query_targets) instead
        of a trilinear sample of a stored volume: the store needs no `volume` group and none is read or held"""
        t0 = time.time()
        self.dataset, self.device = dataset, torch.device(device)
        self.indices = [int(k) for k in indices]
        ds = dataset
        if ds.enable_augumentation and ds.random_rot_range[0] > ds.random_rot_range[1]:
            raise AssertionError("random_rot_range must be (low, high)")
        if ds.num_mc_surface_sample > 0 and ds.num_surface_sample <= 0:
            raise ValueError("ResidentDataset: the mc-surface sampler draws num_surface_sample points; it is 0")
        self.exact_targets = bool(exact_targets) and ds.num_volume_sample > 0
        if self.exact_targets:
            targets.check_kind(ds.volume_group)                      # ValueError naming the group
        self.names = held_arrays(ds.num_volume_sample, ds.num_surface_sample, ds.num_mc_surface_sample, ds.surface_sample_ratio, ds.volume_task_space,
                                 self.exact_targets)
        self.near = ds.num_volume_sample > 0 and ds.surface_sample_ratio != 0
        self.n_uniform = int(ds.num_volume_sample * ds.surface_sample_ratio) if self.near else ds.num_volume_sample
        counts = [sample_counts(ds, k, self.names) for k in self.indices]
        shapes = {c["volume_shape"] for c in counts}
        if len(shapes) > 1:
            raise ValueError(f"ResidentDataset: the samples' volumes differ in shape: {sorted(shapes)}")
        self.volume_shape = shapes.pop() if shapes else (0, 0, 0)
        self.layout = plan(counts, self.names)
        self.nbytes = self.layout.nbytes
        budget = max_bytes if max_bytes is not None else torch.cuda.mem_get_info(self.device)[0] // 2
        if self.nbytes > budget:
            raise ValueError(f"ResidentDataset: {len(self.indices)} samples need {self.nbytes} bytes of device memory, the budget is {int(budget)} bytes")
        self.max_faces = max((int(c["faces"]) for c in counts), default=0)
        self._load(counts)
        self._slot = {k: i for i, k in enumerate(self.indices)}       # (a repeated index keeps its last copy)
        self._ring = [[None, None] for _ in range(DRAW_RING)]        # [pinned buffer, the event behind its last upload]
        self._turn = 0
        self.load_seconds = time.time() - t0

    def __len__(self):
        return len(self.indices)

    # ------------------------------------------------------------------------------------------------ load
    def _load(self, counts):
        n, lay, dev = len(self.indices), self.layout, self.device
        self.arrays = {k: torch.empty(rows * width, dtype=_TORCH[dt], device=dev) for k, (rows, width, dt) in lay.arrays.items()}
        staging = torch.empty(max(lay.staging_bytes, 8), dtype=torch.uint8).pin_memory()
        host = staging.numpy()
        meta = np.zeros((n, len(_lib.RESIDENT_META)), dtype=np.int64)
        grip = np.zeros((n, 6), dtype=np.float32)
        col = {name: i for i, name in enumerate(_lib.RESIDENT_META)}
        self.pc_sizes, self.pc_len, self.scale_dtype = [], [], None
        stream = torch.cuda.current_stream(dev)
        for i, idx in enumerate(self.indices):
            sample, extras = host_sample(self.dataset, idx, self.names)
            off = 0
            for k in self.names:
                count_key, width, dt = ARRAY_SPECS[k]
                a = np.ascontiguousarray(sample[k], dtype=dt).reshape(-1)
                if a.size != int(counts[i][count_key]) * width:
                    raise ValueError(f"sample {idx}: {k} holds {a.size} values, its metadata promised {int(counts[i][count_key]) * width}")
                nb = a.nbytes
                host[off:off + nb] = a.view(np.uint8)
                start = int(lay.offsets[count_key][i]) * width * a.itemsize
                self.arrays[k].view(torch.uint8)[start:start + nb].copy_(staging[off:off + nb], non_blocking=True)
                off += _align8(nb)
            stream.synchronize()                                       # the staging buffer is free again: host memory stays flat
            if self.scale_dtype not in (None, extras["scale"].dtype):
                raise TypeError(f"sample {idx}: scale is {extras['scale'].dtype}, earlier samples' {self.scale_dtype}")
            self.scale_dtype = extras["scale"].dtype
            o = lay.offsets
            row = {"pc_off": o["points"][i], "pc_len": extras["pc_len"], "vert_off": o["verts"][i], "face_off": o["faces"][i], "num_faces": counts[i]["faces"],
                   "mc_vert_off": o["mc_verts"][i], "mc_face_off": o["mc_faces"][i], "num_mc_faces": counts[i]["mc_faces"], "dataset_idx": idx,
                   "scale_bits": extras["scale"].view(np.int64)[0]}
            for name, v in row.items():
                meta[i, col[name]] = v
            grip[i] = extras["grip"]
            self.pc_sizes.append(extras["pc_sizes"])
            self.pc_len.append(extras["pc_len"])
        self.arrays["meta"] = torch.from_numpy(meta).to(dev)
        self.arrays["grip"] = torch.from_numpy(grip).to(dev)
        self.arrays["aabb"] = torch.from_numpy(np.ascontiguousarray(self.dataset.cloth_sim_aabb, dtype=np.float32).reshape(6)).to(dev)
        self.store = ops.resident_store(self.arrays, self.volume_shape)
        # gn_resident_query_targets' flags: never read back (host_sample refuses a face index outside its mesh at load), not counted in nbytes
        self._qt_bad = torch.zeros(2, dtype=torch.int64, device=dev) if self.exact_targets else None

    # ------------------------------------------------------------------------------------------------ draws
    def draw_layout(self, B):
        ds = self.dataset
        return draw_sections(B, ds.num_pc_sample, ds.num_volume_sample, self.n_uniform, ds.num_surface_sample, ds.num_mc_surface_sample > 0, self.near,
                             ds.pc_noise_std > 0, ds.enable_augumentation)

    def fill_draws(self, views, b, idx, slot):
        """the draws of garment `idx` into row b of the section views: SeededDraws' stages, as GarmentInputDataset.__getitem__ consumes them"""
        ds = self.dataset
        draws = D.SeededDraws(idx, ds.static_epoch_seed)
        views["slots"][b] = slot
        views["sel"][b] = draws.point_selection(self.pc_sizes[slot], ds.num_views, ds.num_pc_sample, self.pc_len[slot])
        if ds.num_volume_sample > 0:
            v = draws.volume_draws(ds.num_volume_sample, ds.surface_sample_ratio, ds.surface_sample_std)
            views["vol_uniform"][b] = v["uniform"]
            if self.near:
                views["vol_face_u"][b], views["vol_uv"][b], views["vol_noise"][b] = v["face_u"], v["uv"], v["noise"]
        if ds.num_surface_sample > 0:
            views["surf_face_u"][b], views["surf_uv"][b] = draws.mesh_draws(ds.num_surface_sample)
        if ds.num_mc_surface_sample > 0:
            views["mc_face_u"][b], views["mc_uv"][b] = draws.mesh_draws(ds.num_surface_sample)
        if ds.pc_noise_std > 0:
            views["pc_noise"][b] = draws.noise(ds.pc_noise_std, (ds.num_pc_sample, 3))
        if ds.enable_augumentation:
            views["rot"][b] = draws.z_rotation(*ds.random_rot_range)

    def _pinned(self, nbytes):
        entry = self._ring[self._turn]
        self._turn = (self._turn + 1) % DRAW_RING
        if entry[1] is not None:
            entry[1].synchronize()                                     # this buffer's upload of DRAW_RING batches ago (long done)
        if entry[0] is None or entry[0].numel() < nbytes:
            entry[0] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return entry

    # ------------------------------------------------------------------------------------------------ batch
    def batch(self, chunk):
        chunk = [int(k) for k in chunk]
        slots = [self._slot[k] for k in chunk]                         # KeyError: not resident
        ds, dev, B = self.dataset, self.device, len(chunk)
        if B == 0:
            raise ValueError("ResidentDataset.batch: empty chunk")
        lay = self.draw_layout(B)
        entry = self._pinned(lay.nbytes)
        host = entry[0].numpy()
        views = {k: host[off:off + int(np.prod(shape)) * dt.itemsize].view(dt).reshape(shape) for k, (off, dt, shape) in lay.sections.items()}
        for b, (idx, slot) in enumerate(zip(chunk, slots)):
            self.fill_draws(views, b, idx, slot)
        with torch.cuda.device(dev):
            up = entry[0][:lay.nbytes].to(dev, non_blocking=True)     # the one upload of the batch
            entry[1] = torch.cuda.Event()
            entry[1].record(torch.cuda.current_stream(dev))
            d = {k: up[off:off + int(np.prod(shape)) * dt.itemsize].view(_TORCH.get(dt, torch.int32)).view(shape) for k, (off, dt, shape) in lay.sections.items()}
            new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
            P, rot = ds.num_pc_sample, d.get("rot")
            task = ds.volume_task_space
            out = {"x": new(B * P, 3), "y": new(B * P, 3), "pos": new(B * P, 3)}
            batch_vec = new(B * P, dtype=torch.int64)
            ops.resident_points(self.store, d["slots"], d["sel"], d.get("pc_noise"), rot, out["x"], out["y"], out["pos"], batch_vec)
            scale_bits = new(B, dtype=torch.int64)
            out["scale"] = scale_bits.view(_SCALE_TORCH[self.scale_dtype.kind])
            out.update(sim_grip_point=new(B, 3), nocs_grip_point=new(B, 3), grip_pc_idx=new(B, dtype=torch.int64), dataset_idx=new(B, dtype=torch.int64),
                       cloth_sim_aabb=new(B, 2, 3))
            rot_out = new(B, 3, 3)
            ops.resident_garment(self.store, d["slots"], d["sel"], rot, out["grip_pc_idx"], out["sim_grip_point"], out["nocs_grip_point"], scale_bits,
                                 out["dataset_idx"], out["cloth_sim_aabb"], rot_out)
            if ds.num_volume_sample > 0:
                M = ds.num_volume_sample
                out.update(volume_query_points=new(B, M, 3), gt_volume_value=new(B, M))
                turn = rot if task else None
                if self.exact_targets:                                 # the same queries; the values from the mesh, taken before the queries turn
                    plain = new(B, M, 3) if turn is not None else None
                    ops.resident_volume_queries(self.store, d["slots"], d["vol_uniform"], d.get("vol_face_u"), d.get("vol_uv"), d.get("vol_noise"), turn,
                                                plain, out["volume_query_points"])
                    ops.resident_query_targets(self.store, d["slots"], out["volume_query_points"] if plain is None else plain, task,
                                               int(self.layout.offsets["verts"][-1]), self.max_faces, ds.volume_group, ds.tsdf_clip_value,
                                               ds.volume_absolute_value, out["gt_volume_value"], self._qt_bad)
                else:
                    ops.resident_volume(self.store, d["slots"], d["vol_uniform"], d.get("vol_face_u"), d.get("vol_uv"), d.get("vol_noise"), turn,
                                        ds.volume_group == "nocs_occupancy_grid", out["volume_query_points"], out["gt_volume_value"])
            if ds.num_surface_sample > 0:
                M = ds.num_surface_sample
                out.update(surf_query_points=new(B, M, 3), gt_sim_points=new(B, M, 3))
                ops.resident_surface(self.store, d["slots"], d["surf_face_u"], d["surf_uv"], task, rot, out["surf_query_points"], out["gt_sim_points"])
            if ds.num_mc_surface_sample > 0:
                M = ds.num_surface_sample
                out.update(mc_surf_query_points=new(B, M, 3), is_query_point_on_surf=new(B, M, 1))
                ops.resident_mc_surface(self.store, d["slots"], d["mc_face_u"], d["mc_uv"], out["mc_surf_query_points"], out["is_query_point_on_surf"])
            out["input_aug_rot_mat"] = rot_out
        return Batch(sizes=[P] * B, batch=batch_vec, **out)

    def batches(self, indices, batch_size):
        """-> (dataset indices, device Batch) per batch of `indices`, in order: validate.host_batches' contract"""
        for i in range(0, len(indices), batch_size):
            chunk = [int(k) for k in indices[i:i + batch_size]]
            yield chunk, self.batch(chunk)


"""python -m garmentnets_amd.prepare: complete a dataset store with the training targets that are computed from its garment meshes.

Reads, per sample, mesh/{cloth_verts, cloth_nocs_verts, cloth_faces_tri} (and summary/cloth_aabb_union for the task-space group) and writes
through io.zarr_store, with default_compressor():

  volume/nocs_winding_number_field/<size>       the generalised winding number (winding.py) of the NOCS mesh at every node of the
                                                size^3 lattice over the unit cube, float32
  volume/sim_nocs_winding_number_field/<size>   the same of AABBGripNormalizer(cloth_aabb_union)(cloth_verts): the task-space vertices
                                                io.dataset.get_surface_sample queries
  volume/nocs_distance_field/<size>             (--derived_groups) the distance from every node of that lattice to the NOCS mesh, float32
  volume/nocs_signed_distance_field/<size>      (--derived_groups) clip(1 - 2 w, -1, 1) times that distance, w the stored nocs_winding_number_field of the
                                                same size: minus the distance inside, plus outside, zero on the garment and where w crosses 0.5
  volume/nocs_occupancy_grid/<size>             (--derived_groups) float32(w > 0.5)
  marching_cube_mesh/ (--marching_cubes)        marching_cube_verts float32 (V, 3), marching_cube_faces int32 (F, 3): common.marching_cubes_util.
                                                marching_cubes(NOCS field, 0.5, spacing 1/(size-1)); is_vertex_on_surface bool (V,)

  point_cloud/ (--point_clouds)                 point float32 (N, 3), nocs float32 (N, 3), rgb uint8 (N, 3), sizes int64 (views,): the simulation mesh seen by
                                                --pc_views pinhole cameras on a ring around cloth_aabb_union, the covered pixels of every view in raster
                                                order (point_cloud.py; DESIGN.md "Point clouds from meshes"); the cameras go into the group's attributes

The on-surface rule is THIS PACKAGE'S OWN (the reference ships the flag, not how it was made): a marching-cubes vertex is on the surface
when its distance to the NOCS mesh, sqrt(ops.point_mesh_sqdist), is <= tau.  The default tau = 1/(size-1) is derived, not tuned: a
marching-cubes vertex lies on a lattice edge that the 0.5 level crosses, and where the garment's surface makes that crossing the surface
passes through the same edge, within one edge length of the vertex; a vertex farther away than that closes the field over an opening.

The derived groups (distance.py has their definitions, this package's own as well) are built after --groups, a chunk of --batch_size garments
per launch; the signed field and the occupancy grid read the stored winding field, so it has to be there or be built in the same run.

A field whose range does not contain 0.5 has no isosurface: its marching_cube_mesh arrays are written empty and the group's attributes
say why ("empty": the reason).  Existing arrays are kept unless --overwrite is given.  Marching cubes and the on-surface distances run on the device
whatever --backend says (the package has no host marching cubes); --backend picks who computes the winding numbers and the lattice distances.
"""
import argparse
import json
import time

import numpy as np

from . import distance, point_cloud, winding
from .io import zarr_store
from .io.dataset import TASK_SPACE_VOLUME_GROUP, AABBGripNormalizer

NOCS_GROUP = "nocs_winding_number_field"
GROUPS = (NOCS_GROUP, TASK_SPACE_VOLUME_GROUP)
DERIVED_GROUPS = (distance.DISTANCE_GROUP, distance.SIGNED_DISTANCE_GROUP, distance.OCCUPANCY_GROUP)
MESH_ARRAYS = ("cloth_verts", "cloth_nocs_verts", "cloth_faces_tri")
MC_ARRAYS = ("marching_cube_verts", "marching_cube_faces", "is_vertex_on_surface")
ISO_LEVEL = 0.5


def build_parser():
    ap = argparse.ArgumentParser(description="complete a garmentnets dataset store: winding-number volumes and the marching-cubes mesh of "
                                             "every sample, computed from its garment mesh")
    ap.add_argument("--zarr_in", required=True, help="garmentnets dataset store (Zarr v2); completed in place")
    ap.add_argument("--volume_size", type=int, default=128)
    ap.add_argument("--groups", nargs="*", default=list(GROUPS), help=f"volume groups to build, of {GROUPS}")
    ap.add_argument("--derived_groups", nargs="*", default=[], choices=DERIVED_GROUPS,
                    help="volume groups to derive from the NOCS mesh's distance field and the stored NOCS winding field; default none")
    ap.add_argument("--marching_cubes", action="store_true", help="build the marching_cube_mesh group from the NOCS field (on the device)")
    ap.add_argument("--on_surface_distance", type=float, default=None, help="tau of the on-surface rule; default 1/(volume_size-1)")
    ap.add_argument("--batch_size", type=int, default=4, help="garments per launch")
    ap.add_argument("--overwrite", action="store_true", help="rebuild arrays that the store already holds")
    ap.add_argument("--backend", default="hip", choices=("hip", "numpy"),
                    help="who computes the winding numbers, the lattice distances and the point clouds")
    ap.add_argument("--point_clouds", action="store_true", help="render point_cloud/{point, nocs, rgb, sizes} from the garment mesh (point_cloud.py)")
    ap.add_argument("--pc_views", type=int, default=4, help="cameras on the ring")
    ap.add_argument("--pc_img_size", type=int, default=256, help="pixels per image side: a view holds at most its square in points")
    ap.add_argument("--pc_fov", type=float, default=point_cloud.DEFAULT_FOV, help="field of view, degrees (a look)")
    ap.add_argument("--pc_elevation", type=float, default=point_cloud.DEFAULT_ELEVATION, help="degrees above the xy plane (a look)")
    ap.add_argument("--pc_azimuth0", type=float, default=0.0, help="azimuth of the first camera, degrees about z")
    ap.add_argument("--pc_distance", type=float, default=None, help="camera distance; default r / sin(fov / 2), r the half-diagonal of cloth_aabb_union")
    ap.add_argument("--pc_color", type=float, nargs=3, default=list(point_cloud.DEFAULT_BASE_COLOR), metavar=("R", "G", "B"),
                    help="the base colour the headlight shades, in [0, 1]")
    return ap


def sample_mesh(sample_group, group, aabb):
    """(verts float64, faces) of the mesh whose field `group` holds"""
    mesh = sample_group["mesh"]
    faces = mesh["cloth_faces_tri"][:]
    if group == NOCS_GROUP:
        return mesh["cloth_nocs_verts"][:].astype(np.float64), faces
    return np.asarray(AABBGripNormalizer(aabb)(mesh["cloth_verts"][:]), dtype=np.float64), faces


def marching_cube_group(volume, nocs_verts, faces, tau):
    """the three arrays of marching_cube_mesh for one NOCS field (device work) -> (dict of numpy arrays, None or why they are empty)"""
    import torch

    from . import ops
    from .common import marching_cubes_util
    dev = torch.device("cuda", torch.cuda.current_device())
    size = volume.shape[-1]
    try:
        verts64, mc_faces, _, _, _ = marching_cubes_util.marching_cubes(torch.from_numpy(volume).to(dev), ISO_LEVEL, (1.0 / (size - 1),) * 3)
    except (ValueError, RuntimeError) as e:
        return {"marching_cube_verts": np.zeros((0, 3), np.float32), "marching_cube_faces": np.zeros((0, 3), np.int32),
                "is_vertex_on_surface": np.zeros((0,), bool)}, str(e)
    verts = verts64.float()                                  # what the store holds; the flag is measured from these
    _, d2 = ops.point_mesh_sqdist(verts.double(), torch.from_numpy(np.ascontiguousarray(nocs_verts, dtype=np.float64)).to(dev),
                                  torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int64)).to(dev))
    return {"marching_cube_verts": verts.cpu().numpy(), "marching_cube_faces": mc_faces.to(torch.int32).cpu().numpy(),
            "is_vertex_on_surface": (torch.sqrt(d2) <= tau).cpu().numpy()}, None


def build_derived_groups(samples, chunk, derived, size, overwrite, backend, comp):
    """write the missing (or, with overwrite, all) `derived` volumes of the samples `chunk`; the distances of the whole chunk come from one
    launch -> [(sample, group)] written"""
    todo = {k: [g for g in derived if overwrite or f"volume/{g}/{size}" not in samples[k]] for k in chunk}
    todo = {k: gs for k, gs in todo.items() if gs}
    meshes, wnf = {}, {}
    for k, gs in todo.items():
        if any(g != distance.DISTANCE_GROUP for g in gs):
            if f"volume/{NOCS_GROUP}/{size}" not in samples[k]:
                raise ValueError(f"sample {k}: --derived_groups {' '.join(g for g in gs if g != distance.DISTANCE_GROUP)} reads "
                                 f"volume/{NOCS_GROUP}/{size}; build it in the same run (--groups)")
            wnf[k] = samples[k]["volume"][NOCS_GROUP][str(size)][:]
        if any(g != distance.OCCUPANCY_GROUP for g in gs):
            meshes[k] = sample_mesh(samples[k], NOCS_GROUP, None)
            if len(meshes[k][1]) == 0:
                raise ValueError(f"sample {k}: its mesh has no faces, so its distance to every lattice node is infinite: no target volume")
    d2 = dict(zip(meshes, distance.distance_field(list(meshes.values()), (size,) * 3, backend=backend)[0])) if meshes else {}
    done = []
    for k, gs in todo.items():
        for g in gs:
            samples[k].require_group("volume").require_group(g).array(str(size), distance.derived_volume(g, d2.get(k), wnf.get(k)), compressor=comp)
            done.append((k, g))
    return done


def build_point_clouds(samples, chunk, cameras, img_size, color, overwrite, backend, comp):
    """write point_cloud/{point, nocs, rgb, sizes} of the samples of `chunk` that lack one of them (or, with overwrite, of all): the simulation mesh
    seen from `cameras`, every garment times every view in one launch set -> [sample] written"""
    todo = [k for k in chunk if overwrite or not all(f"point_cloud/{a}" in samples[k] for a in point_cloud.CLOUD_ARRAYS)]
    if not todo:
        return []
    meshes = [(samples[k]["mesh"]["cloth_verts"][:].astype(np.float32), samples[k]["mesh"]["cloth_nocs_verts"][:].astype(np.float32),
               samples[k]["mesh"]["cloth_faces_tri"][:].astype(np.int32)) for k in todo]
    clouds = point_cloud.render_point_clouds(meshes, cameras, img_size, color, backend="numpy" if backend == "numpy" else "device")
    for k, cloud in zip(todo, clouds):
        if cloud["sizes"].sum() == 0:
            raise ValueError(f"sample {k}: no camera sees its mesh (no covered pixel in any of {len(cameras)} views): no point cloud")
        pc = samples[k].require_group("point_cloud")
        for a in point_cloud.CLOUD_ARRAYS:
            pc.array(a, cloud[a], compressor=comp)
        pc.put_attrs({"cameras": point_cloud.camera_attrs(cameras), "img_size": int(img_size), "base_color": [float(c) for c in color],
                      "ambient": point_cloud.DEFAULT_AMBIENT})
    return todo


def prepare_store(zarr_in, volume_size=128, groups=GROUPS, marching_cubes=False, on_surface_distance=None, batch_size=4, overwrite=False,
                  backend="hip", log=print, derived_groups=(), point_clouds=False, pc_views=4, pc_img_size=256, pc_fov=point_cloud.DEFAULT_FOV,
                  pc_elevation=point_cloud.DEFAULT_ELEVATION, pc_azimuth0=0.0, pc_distance=None, pc_color=point_cloud.DEFAULT_BASE_COLOR):
    """-> summary dict {"samples", "written": {what: count}, "seconds"}; log gets one dict per sample"""
    groups = list(groups)
    unknown = [g for g in groups if g not in GROUPS]
    if unknown:
        raise ValueError(f"unknown volume group(s) {unknown}: this command builds {list(GROUPS)}")
    derived = list(derived_groups)
    unknown = [g for g in derived if g not in DERIVED_GROUPS]
    if unknown:
        raise ValueError(f"unknown derived group(s) {unknown}: this command derives {list(DERIVED_GROUPS)}")
    size = int(volume_size)
    if size < 2:
        raise ValueError(f"volume_size {size}: a lattice needs at least 2 nodes per axis")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size} < 1")
    tau = 1.0 / (size - 1) if on_surface_distance is None else float(on_surface_distance)
    root = zarr_store.open_group(zarr_in, create=False)
    if "samples" not in root:
        raise ValueError(f"{zarr_in}: no samples group")
    samples = root["samples"]
    keys = sorted(samples.keys())
    for k in keys:
        missing = [a for a in MESH_ARRAYS if f"mesh/{a}" not in samples[k]]
        if missing:
            raise ValueError(f"{zarr_in}: sample {k} has no mesh/{missing[0]}: the targets are computed from the garment meshes")
    aabb = None
    if TASK_SPACE_VOLUME_GROUP in groups:
        if "summary/cloth_aabb_union" not in root:
            raise ValueError(f"{zarr_in}: no summary/cloth_aabb_union, which {TASK_SPACE_VOLUME_GROUP} is normalised with")
        aabb = root["summary"]["cloth_aabb_union"][:].astype(np.float32)          # the dtype GarmentInputDataset normalises with
    cameras = None
    if point_clouds:
        if "summary/cloth_aabb_union" not in root:
            raise ValueError(f"{zarr_in}: no summary/cloth_aabb_union, which the cameras of --point_clouds are placed around")
        cameras = point_cloud.camera_ring(root["summary"]["cloth_aabb_union"][:], pc_views, pc_img_size, pc_fov, pc_elevation, pc_azimuth0, pc_distance)
        if not 1 <= int(pc_img_size) <= 4096:
            raise ValueError(f"pc_img_size {pc_img_size} outside [1, 4096]")
    comp = zarr_store.default_compressor()
    written = {g: 0 for g in groups + derived}
    if point_clouds:
        written["point_cloud"] = 0
    if marching_cubes:
        written["marching_cube_mesh"] = 0
    t_all = time.perf_counter()
    for s in range(0, len(keys), batch_size):
        chunk = keys[s:s + batch_size]
        t0 = time.perf_counter()
        did = {k: [] for k in chunk}
        for g in groups:
            todo = [k for k in chunk if overwrite or f"volume/{g}/{size}" not in samples[k]]
            if not todo:
                continue
            fields = winding.winding_field([sample_mesh(samples[k], g, aabb) for k in todo], (size,) * 3, backend=backend)
            for k, field in zip(todo, fields):
                samples[k].require_group("volume").require_group(g).array(str(size), field, compressor=comp)
                did[k].append(g)
                written[g] += 1
        if derived:
            for k, g in build_derived_groups(samples, chunk, derived, size, overwrite, backend, comp):
                did[k].append(g)
                written[g] += 1
        if point_clouds:
            for k in build_point_clouds(samples, chunk, cameras, int(pc_img_size), pc_color, overwrite, backend, comp):
                did[k].append("point_cloud")
                written["point_cloud"] += 1
        if marching_cubes:
            for k in chunk:
                sg = samples[k]
                if not overwrite and all(f"marching_cube_mesh/{a}" in sg for a in MC_ARRAYS):
                    continue
                if f"volume/{NOCS_GROUP}/{size}" not in sg:
                    raise ValueError(f"sample {k}: --marching_cubes reads volume/{NOCS_GROUP}/{size}; build it in the same run (--groups)")
                nocs_verts, faces = sample_mesh(sg, NOCS_GROUP, None)
                arrays, empty = marching_cube_group(sg["volume"][NOCS_GROUP][str(size)][:], nocs_verts, faces, tau)
                mc = sg.require_group("marching_cube_mesh")
                for name in MC_ARRAYS:
                    mc.array(name, arrays[name], compressor=comp)
                mc.put_attrs({"empty": empty or False, "on_surface_distance": tau, "volume_size": size})
                did[k].append("marching_cube_mesh")
                written["marching_cube_mesh"] += 1
        dt = time.perf_counter() - t0
        for k in chunk:
            log({"sample": k, "written": did[k], "seconds": dt / len(chunk)})
    summary = {"samples": len(keys), "written": written, "seconds": time.perf_counter() - t_all}
    log(summary)
    return summary


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        return prepare_store(a.zarr_in, a.volume_size, a.groups, a.marching_cubes, a.on_surface_distance, a.batch_size, a.overwrite, a.backend,
                             log=lambda row: print(json.dumps(row)), derived_groups=a.derived_groups, point_clouds=a.point_clouds,
                             pc_views=a.pc_views, pc_img_size=a.pc_img_size, pc_fov=a.pc_fov, pc_elevation=a.pc_elevation, pc_azimuth0=a.pc_azimuth0,
                             pc_distance=a.pc_distance, pc_color=a.pc_color)
    except ValueError as e:
        ap.error(str(e))


if __name__ == "__main__":
    main()

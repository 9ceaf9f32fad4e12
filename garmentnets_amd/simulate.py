"""python -m garmentnets_amd.simulate: hang the garments of a dataset store from their grip vertices (cloth.py) and write mesh/cloth_verts.

Reads, per sample, mesh/{cloth_nocs_verts, cloth_faces_tri}, the attribute grip_vertex_idx (drawn with RandomState(seed + dataset index) and written
back where it is absent) and summary/cloth_canonical_aabb_union (whose longest edge is the rest scale; --rest_scale where the store has none), and
writes through io.zarr_store, with default_compressor():

  samples/<key>/mesh/cloth_verts       float32 (V, 3): the garment after --duration seconds of cloth.py's solver in the gripper frame (grip vertex at the
                                       origin, z up); the mesh group's attributes get {"cloth_simulation": the parameters, the substep count and the
                                       diagnostics of the final state (kinetic energy, largest stretch strain, massless vertices)}
  summary/cloth_aabb_union             float32 (2, 3): the union box of every cloth_verts of the store, when the store has none or with --update_summary

--self_collision turns the vertex-vertex contacts of cloth.py on: --collision_thickness (default: cloth.DEFAULT_COLLISION_THICKNESS_FACTOR times the
garment's mean stretch rest length, cloth.mean_stretch_rest_length, so it differs from garment to garment), --collision_margin (default: the thickness),
--collision_rebuild, --collision_max_list, --collision_relax.  The five parameters and the four contact diagnostics of the sample then join
"cloth_simulation", and a sample with contact_overflow > 0 or contact_travel > 1 is named in a printed warning (a contact may have been cut off or
missed).  Without the flag the store is byte for byte what it was.

--face_contacts (only with --self_collision) turns the vertex-face contacts of cloth.py on as well: --face_thickness (default:
cloth.DEFAULT_FACE_THICKNESS_FACTOR times the garment's mean stretch rest length), --face_max_list.  The two parameters and the three face-contact
diagnostics then join "cloth_simulation", and face_contact_overflow > 0 joins the warning.  Without the flag nothing changes.

An existing cloth_verts is kept unless --overwrite is given.  --backend hip runs --batch_size garments per call of ops.cloth_simulate_batch (one workgroup
each); --backend numpy runs the restatement, which gives the same bits.  After this command `prepare` can build every other group: simulate -> prepare ->
train -> predict -> evaluate runs from canonical meshes alone.
"""
import argparse
import dataclasses
import json
import time

import numpy as np

from . import cloth
from .io import zarr_store

MESH_INPUTS = ("cloth_nocs_verts", "cloth_faces_tri")


def build_parser():
    ap = argparse.ArgumentParser(description="hang the garments of a garmentnets dataset store: mesh/cloth_verts from the canonical meshes")
    ap.add_argument("--zarr_in", required=True, help="garmentnets dataset store (Zarr v2); completed in place")
    ap.add_argument("--overwrite", action="store_true", help="simulate samples that already hold mesh/cloth_verts again")
    ap.add_argument("--update_summary", action="store_true", help="rewrite summary/cloth_aabb_union from the store's cloth_verts")
    ap.add_argument("--batch_size", type=int, default=16, help="garments per call (one workgroup each)")
    ap.add_argument("--backend", default="hip", choices=("hip", "numpy"))
    ap.add_argument("--seed", type=int, default=0, help="a missing grip_vertex_idx is drawn with RandomState(seed + dataset index)")
    ap.add_argument("--rest_scale", type=float, default=None, help="rest shape = (nocs - 0.5) * rest_scale, for a store without "
                                                                    "summary/cloth_canonical_aabb_union")
    ap.add_argument("--gravity", type=float, default=cloth.DEFAULT_GRAVITY, help="m / s^2 along -z")
    ap.add_argument("--h", type=float, default=cloth.DEFAULT_H, help="seconds per substep")
    ap.add_argument("--duration", type=float, default=cloth.DEFAULT_DURATION, help="seconds simulated")
    ap.add_argument("--damping", type=float, default=cloth.DEFAULT_DAMPING, help="1 / s")
    ap.add_argument("--alpha_stretch", type=float, default=cloth.DEFAULT_ALPHA_STRETCH, help="stretch compliance, m / N")
    ap.add_argument("--alpha_bend", type=float, default=cloth.DEFAULT_ALPHA_BEND, help="bend compliance, m / N")
    ap.add_argument("--density", type=float, default=cloth.DEFAULT_DENSITY, help="kg / m^2")
    ap.add_argument("--self_collision", action="store_true", help="vertex-vertex self-collision (cloth.py); off by default")
    ap.add_argument("--collision_thickness", type=float, default=None,
                    help=f"metres; default {cloth.DEFAULT_COLLISION_THICKNESS_FACTOR} x the garment's mean stretch rest length")
    ap.add_argument("--collision_margin", type=float, default=None,
                    help=f"metres beyond the thickness at which a pair enters a contact list; default {cloth.DEFAULT_COLLISION_MARGIN_FACTOR} x the thickness")
    ap.add_argument("--collision_rebuild", type=int, default=cloth.DEFAULT_COLLISION_REBUILD, help="substeps between two contact-list builds")
    ap.add_argument("--collision_max_list", type=int, default=cloth.DEFAULT_COLLISION_MAX_LIST, help="entries a contact list can hold, at most 64")
    ap.add_argument("--collision_relax", type=float, default=cloth.DEFAULT_COLLISION_RELAX, help="in (0, 1]: the share of a contact correction applied")
    ap.add_argument("--face_contacts", action="store_true", help="vertex-face contacts (cloth.py) beside the vertex-vertex ones; needs --self_collision")
    ap.add_argument("--face_thickness", type=float, default=None,
                    help=f"metres; default {cloth.DEFAULT_FACE_THICKNESS_FACTOR} x the garment's mean stretch rest length")
    ap.add_argument("--face_max_list", type=int, default=cloth.DEFAULT_FACE_MAX_LIST, help="entries a face-contact list can hold, at most 32")
    return ap


def grip_index(sample_group, dataset_idx, num_verts, seed):
    """the sample's grip_vertex_idx; where absent, drawn with RandomState(seed + dataset index) and written back"""
    attrs = sample_group.attrs
    if "grip_vertex_idx" in attrs:
        return int(attrs["grip_vertex_idx"])
    grip = int(np.random.RandomState(int(seed) + int(dataset_idx)).randint(0, num_verts))
    sample_group.put_attrs({"grip_vertex_idx": grip})
    return grip


def collision_params(params, g, collision):
    """`params` with the contacts of `collision` ({"thickness", "margin" (None: the defaults from the garment g), "rebuild", "max_list", "relax"}) on;
    with the key "face" ({"thickness" (None: the default from g), "max_list"}) the vertex-face contacts too"""
    t = collision.get("thickness")
    if t is None:
        t = cloth.DEFAULT_COLLISION_THICKNESS_FACTOR * cloth.mean_stretch_rest_length(g)
    m = collision.get("margin")
    if m is None:
        m = cloth.DEFAULT_COLLISION_MARGIN_FACTOR * t
    if not t > 0:
        raise ValueError(f"collision thickness {t}: expected a positive number (a garment without a stretch constraint has no default)")
    on = dataclasses.replace(params, collision_thickness=float(t), collision_margin=float(m), collision_rebuild=int(collision["rebuild"]),
                             collision_max_list=int(collision["max_list"]), collision_relax=float(collision["relax"]))
    face = collision.get("face")
    if face is None:
        return on
    tf = face.get("thickness")
    if tf is None:
        tf = cloth.DEFAULT_FACE_THICKNESS_FACTOR * cloth.mean_stretch_rest_length(g)
    if not tf > 0:
        raise ValueError(f"face thickness {tf}: expected a positive number (a garment without a stretch constraint has no default)")
    return dataclasses.replace(on, face_thickness=float(tf), face_max_list=int(face["max_list"]))


def run_batch(garments, substeps, backend):
    """-> ([(x, v)] numpy, [the contact diagnostics]) of `garments`, those that share their collision and face-contact constants in one call each"""
    groups = {}
    for n, g in enumerate(garments):
        groups.setdefault(json.dumps([g.collision, g.face_collision], sort_keys=True), []).append(n)
    states, stats = [None] * len(garments), [None] * len(garments)
    for idx in groups.values():
        gs = [garments[n] for n in idx]
        if backend == "numpy":
            res = [cloth.simulate_reference(g, substeps, stats=True) for g in gs]
            got, st = [r[:2] for r in res], [r[2] for r in res]
        else:
            from . import ops
            got, st = ops.cloth_simulate_batch(gs, substeps, stats=True)
            got = [(x.cpu().numpy(), v.cpu().numpy()) for x, v in got]
        for n, state, d in zip(idx, got, st):
            states[n], stats[n] = state, d
    return states, stats


def simulate_store(zarr_in, params=None, duration=cloth.DEFAULT_DURATION, rest_scale=None, batch_size=16, overwrite=False, update_summary=False,
                   backend="hip", seed=0, log=print, collision=None):
    """-> summary dict {"samples", "written", "substeps", "seconds"}; log gets one dict per sample.  collision: None (no contacts; `params` must then
    have them off too) or the dict collision_params reads"""
    params = cloth.ClothParams() if params is None else params
    if params.contacts:
        raise ValueError("simulate_store: give the contacts through `collision`, not through params")
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size} < 1")
    substeps = cloth.substeps_of(duration, params.h)
    if substeps < 0:
        raise ValueError(f"duration {duration} < 0")
    root = zarr_store.open_group(zarr_in, create=False)
    if "samples" not in root:
        raise ValueError(f"{zarr_in}: no samples group")
    if "summary/cloth_canonical_aabb_union" in root:
        scale = cloth.rest_scale_of(root["summary"]["cloth_canonical_aabb_union"][:])
    elif rest_scale is not None:
        scale = float(rest_scale)
    else:
        raise ValueError(f"{zarr_in}: no summary/cloth_canonical_aabb_union to take the rest scale from: give --rest_scale")
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f"rest scale {scale}: expected a positive number")
    samples = root["samples"]
    keys = sorted(samples.keys())
    for k in keys:
        missing = [a for a in MESH_INPUTS if f"mesh/{a}" not in samples[k]]
        if missing:
            raise ValueError(f"{zarr_in}: sample {k} has no mesh/{missing[0]}: the garment is simulated from its canonical mesh")
    todo = [(i, k) for i, k in enumerate(keys) if overwrite or "mesh/cloth_verts" not in samples[k]]
    comp = zarr_store.default_compressor()
    record = dict({k: v for k, v in dataclasses.asdict(params).items() if k not in cloth.COLLISION_FIELDS + cloth.FACE_COLLISION_FIELDS},
                  duration=float(duration),
                  substeps=substeps, rest_scale=scale)
    warned = []
    t_all = time.perf_counter()
    for s in range(0, len(todo), batch_size):
        chunk = todo[s:s + batch_size]
        t0 = time.perf_counter()
        garments, extra = [], []
        for i, k in chunk:
            mesh = samples[k]["mesh"]
            nocs = mesh["cloth_nocs_verts"][:]
            g = cloth.garment_from_nocs(nocs, mesh["cloth_faces_tri"][:], grip_index(samples[k], i, len(nocs), seed), scale, params)
            if collision is not None:
                on = collision_params(params, g, collision)
                g = dataclasses.replace(g, collision=cloth.collision_constants(on), face_collision=cloth.face_collision_constants(on))
                extra.append({f: getattr(on, f) for f in cloth.COLLISION_FIELDS + (cloth.FACE_COLLISION_FIELDS if on.face_contacts else ())})
            garments.append(g)
        states, stats = run_batch(garments, substeps, backend)
        dt = time.perf_counter() - t0
        for n, ((i, k), g, (x, v)) in enumerate(zip(chunk, garments, states)):
            diag = cloth.diagnostics(g, x, v)
            if collision is not None:
                diag = dict(diag, **extra[n], **stats[n])
                face_cut = stats[n].get("face_contact_overflow", 0)
                if stats[n]["contact_overflow"] > 0 or stats[n]["contact_travel"] > 1 or face_cut > 0:
                    warned.append(k)
                    face_note = f", face_contact_overflow {face_cut}" if "face_contact_overflow" in stats[n] else ""
                    face_hint = "; for the face lists raise --face_max_list or lower --collision_margin" if face_cut > 0 else ""
                    log({"warning": f"sample {k}: contact_overflow {stats[n]['contact_overflow']}, contact_travel {stats[n]['contact_travel']:.3g}"
                                    f"{face_note}: a contact may have been cut off or missed (raise --collision_max_list or "
                                    f"--collision_margin, or lower --collision_rebuild{face_hint})"})
            mesh = samples[k].require_group("mesh")
            mesh.array("cloth_verts", x.astype(np.float32), compressor=comp)
            mesh.put_attrs({"cloth_simulation": dict(record, grip_vertex_idx=g.grip, **diag)})
            log(dict({"sample": k, "seconds": dt / len(chunk)}, **diag))
    wrote_summary = False
    if keys and (update_summary or "summary/cloth_aabb_union" not in root) and all("mesh/cloth_verts" in samples[k] for k in keys):
        lo = np.min([samples[k]["mesh"]["cloth_verts"][:].min(axis=0) for k in keys], axis=0)
        hi = np.max([samples[k]["mesh"]["cloth_verts"][:].max(axis=0) for k in keys], axis=0)
        root.require_group("summary").array("cloth_aabb_union", np.stack([lo, hi]).astype(np.float32))
        wrote_summary = True
    summary = {"samples": len(keys), "written": len(todo), "substeps": substeps, "summary_written": wrote_summary,
               "seconds": time.perf_counter() - t_all}
    if collision is not None:
        summary["contact_warnings"] = warned
    log(summary)
    return summary


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.face_contacts and not a.self_collision:
        ap.error("--face_contacts needs --self_collision: the face contacts share the vertex contacts' margin, rebuild interval and relaxation")
    try:
        params = cloth.ClothParams(gravity=a.gravity, h=a.h, damping=a.damping, alpha_stretch=a.alpha_stretch, alpha_bend=a.alpha_bend,
                                   density=a.density)
        collision = None
        if a.self_collision:
            collision = {"thickness": a.collision_thickness, "margin": a.collision_margin, "rebuild": a.collision_rebuild,
                         "max_list": a.collision_max_list, "relax": a.collision_relax}
            if a.face_contacts:
                collision["face"] = {"thickness": a.face_thickness, "max_list": a.face_max_list}
        return simulate_store(a.zarr_in, params, a.duration, a.rest_scale, a.batch_size, a.overwrite, a.update_summary, a.backend, a.seed,
                              log=lambda row: print(json.dumps(row)), collision=collision)
    except ValueError as e:
        ap.error(str(e))


if __name__ == "__main__":
    main()

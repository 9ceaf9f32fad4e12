"""Chamfer metrics on the GPU -- the definitions of /root/reference/eval.py:259-271 (chamfer) and
:381-402 (hybrid chamfer: nearest neighbours in NOCS space, distances in simulation space), with the two cKDTree queries
replaced by the exact brute-force gn_nearest_neighbor kernel."""
import torch

from .. import ops


def chamfer(pred_points, gt_points):
    """-> dict(chamfer_forward, chamfer_backward, chamfer_symmetrical) (means of Euclidean NN distances)"""
    _, d2f = ops.nearest_neighbor(pred_points, gt_points)
    _, d2b = ops.nearest_neighbor(gt_points, pred_points)
    fwd = torch.sqrt(d2f.double()).mean()
    bwd = torch.sqrt(d2b.double()).mean()
    return {"chamfer_forward": fwd, "chamfer_backward": bwd, "chamfer_symmetrical": 0.5 * (fwd + bwd)}


def hybrid_chamfer(pred_nocs_points, gt_nocs_points, pred_sim_points, gt_sim_points):
    fi, _ = ops.nearest_neighbor(pred_nocs_points, gt_nocs_points)
    bi, _ = ops.nearest_neighbor(gt_nocs_points, pred_nocs_points)
    fwd = torch.norm(pred_sim_points.double() - gt_sim_points.double()[fi.long()], dim=1).mean()
    bwd = torch.norm(gt_sim_points.double() - pred_sim_points.double()[bi.long()], dim=1).mean()
    return {"hybrid_chamfer_forward": fwd, "hybrid_chamfer_backward": bwd, "hybrid_chamfer_symmetrical": 0.5 * (fwd + bwd)}


# ================================================================================================================================
# The metric stage of eval.py (compute_* at eval.py:58-580), one function per metric.  Host work (sampling, interpolation, the
# decision stump, means) is numpy with the reference's dtype rules; the all-pairs searches go to a backend -- by default the fp64
# kernels of csrc/eval_dist.hip (DeviceBackend).  Every function is split in two: a plan that prepares the host arrays and lists the
# searches it needs, and a finish that turns their results into the metric dict, so that evaluate.py can send one sample's searches of
# several metrics to the device in one launch.
import numpy as np

from . import marching_cubes_util as _mcu

PC_COLUMNS = ("nocs_pc_error_distance", "nocs_pc_mirror_error_distance", "nocs_pc_min_agg_error_distance", "nocs_pc_agg_min_error_distance",
              "nocs_pc_diff_std_x", "nocs_pc_diff_std_y", "nocs_pc_diff_std_z", "nocs_pc_error_x", "nocs_pc_error_y", "nocs_pc_error_z")
THRESHOLD_COLUMNS = ("optimal_wnf_gradient_threshold",)


def grip_point_columns():
    # eval.py:173-178 -- 'distanc' is the reference's spelling, kept so that the columns line up with its outputs
    return tuple(f"grip_point_{m}_{k}" for k in ("pc", "global") for m in ("error_distance", "mirror_error_distanc", "min_error_distanc"))


def _hole_categories(predict_holes):
    return (("nocs", "sim") if predict_holes else ()) + ("nocs_no_hole", "sim_no_hole", "nocs_mc")


def chamfer_columns(predict_holes=True):
    return tuple(f"chamfer_symmetrical_{c}" for c in _hole_categories(predict_holes))


def hybrid_chamfer_columns(predict_holes=True):
    cats = (("regular",) if predict_holes else ()) + ("no_hole",)
    return tuple(f"hybrid_chamfer_{k}_{c}_{a}" for c in cats for a in ("pred", "mirror", "min") for k in ("forward", "backward", "symmetrical"))


def hausdorff_columns(predict_holes=True):
    return tuple(f"hausdorff_{c}" for c in _hole_categories(predict_holes))


class DeviceBackend:
    """the searches on the GPU: ops.nearest_neighbor_f64_batch / ops.point_mesh_sqdist_batch (one launch per call, whatever the number of
    pairs) and the connected components of csrc/mesh_cc.hip.  Inputs and outputs are numpy arrays."""

    def __init__(self, device=None):
        import torch
        self.torch = torch
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

    def _dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)

    def _host(self, res):
        if not res:
            return []
        idx = self.torch.cat([r[0] for r in res]).cpu().numpy()
        d2 = self.torch.cat([r[1] for r in res]).cpu().numpy()
        out, o = [], 0
        for r in res:
            n = r[0].shape[0]
            out.append((idx[o:o + n], d2[o:o + n]))
            o += n
        return out

    def nearest_neighbor(self, pairs):
        """pairs: [(query (n,3), ref (m,3))] -> [(idx int32 (n,), d2 float64 (n,))] (empty ref: +inf, -1)"""
        cache = {}

        def dev(a):                         # a set used by several pairs goes over once (ops stores a repeated REFERENCE set once too)
            if id(a) not in cache:
                cache[id(a)] = self._dev(a, np.float64)
            return cache[id(a)]
        return self._host(ops.nearest_neighbor_f64_batch([dev(q) for q, _ in pairs], [dev(r) for _, r in pairs]))

    def point_mesh_sqdist(self, pairs):
        """pairs: [(query (n,3), verts (v,3), faces (f,3))] -> [(face_idx int32 (n,), d2 float64 (n,))]"""
        cache = {}

        def dev(a, dt):
            if id(a) not in cache:
                cache[id(a)] = self._dev(a, dt)
            return cache[id(a)]
        return self._host(ops.point_mesh_sqdist_batch([dev(q, np.float64) for q, _, _ in pairs],
                                                      [(dev(v, np.float64), dev(f, np.int64)) for _, v, f in pairs]))

    def largest_connected_component(self, faces, num_verts):
        return _mcu.largest_connected_component(self._dev(faces, np.int64), int(num_verts)).cpu().numpy()


def default_backend():
    return DeviceBackend()


class Plan:
    """what one metric of one sample needs from the backend: nn = [(query, ref)], pm = [(query, verts, faces)]; finish(nn_results,
    pm_results) -> metric dict"""

    def __init__(self, finish, nn=(), pm=()):
        self.finish, self.nn, self.pm = finish, list(nn), list(pm)


def run_plans(plans, backend):
    """every search of `plans` in ONE backend call per kind -> [metric dict or the exception its finish raised] (one per plan).  An error of
    the backend itself is raised."""
    nn = backend.nearest_neighbor([p for pl in plans for p in pl.nn]) if any(pl.nn for pl in plans) else []
    pm = backend.point_mesh_sqdist([p for pl in plans for p in pl.pm]) if any(pl.pm for pl in plans) else []
    out, i, j = [], 0, 0
    for pl in plans:
        a, b = nn[i:i + len(pl.nn)], pm[j:j + len(pl.pm)]
        i, j = i + len(pl.nn), j + len(pl.pm)
        try:
            with np.errstate(all="ignore"):
                out.append(pl.finish(a, b))
        except Exception as e:          # noqa: BLE001 -- one (metric, sample) fails alone, as the reference's parallel_map
            out.append(e)
    return out


def _run(plan, backend):
    r = run_plans([plan], backend if backend is not None else default_backend())[0]
    if isinstance(r, Exception):
        raise r
    return r


# ---------------------------------------------------------------------------------------------------------------- host helpers
def aabb_inverse(aabb, data):
    """AABBNormalizer(aabb).inverse(data) (common/geometry_util.py:73-98), numpy's dtype rules: float32 in, float32 out under numpy 2"""
    aabb = np.asarray(aabb)
    center = np.mean(aabb, axis=0)
    scale = 1 / np.max(aabb[1] - aabb[0])
    half = np.ones((3,), dtype=aabb.dtype) / 2
    return (data - half) / scale + center


def doublearea(verts, faces):
    """twice the triangle areas, fp64: the root of the summed squares of the doubled areas of the triangle projected onto the (x,y), (y,z)
    and (z,x) planes, edges taken from the third vertex (libigl's doublearea; its precision on float32 input is not pinned here)"""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces)
    r, s = v[f[:, 0]] - v[f[:, 2]], v[f[:, 1]] - v[f[:, 2]]
    acc = np.zeros(len(f), dtype=np.float64)
    for x in range(3):
        y = (x + 1) % 3
        p = r[:, x] * s[:, y] - r[:, y] * s[:, x]
        acc = acc + p * p
    return np.sqrt(acc)


def mesh_sample_barycentric(verts, faces, num_samples, seed=0):
    """(barycentric float64 (n,3), face index (n,) in the faces' dtype) -- common/geometry_util.py:184-223: faces drawn by area from a FRESH
    RandomState(seed), then u, v uniform in [0,1), reflected when u + v >= 1, w = 1 - u - v"""
    w = doublearea(verts, faces)
    w = w / np.sum(w)
    rs = np.random.RandomState(seed=seed)
    face_idx = rs.choice(len(faces), size=num_samples, replace=True, p=w).astype(np.asarray(faces).dtype)
    uv = rs.uniform(0, 1, size=(num_samples, 2))
    flip = np.sum(uv, axis=1) >= 1
    uv[flip] = 1 - uv[flip]
    bc = np.empty((num_samples, 3), dtype=uv.dtype)
    bc[:, :2] = uv
    bc[:, 2] = 1 - np.sum(uv, axis=1)
    return bc, face_idx


def barycentric_interpolation(bc, verts, faces):
    """(n, C) in the VERTICES' dtype (common/geometry_util.py:165-182): the terms bc[:, i] * verts[faces[:, i]] are added in the order
    i = 0, 1, 2 into a zero array of that dtype, each partial sum rounded to it"""
    out = np.zeros((len(bc), verts.shape[1]), dtype=verts.dtype)
    for i in range(bc.shape[1]):
        np.add(out, bc[:, i:i + 1] * verts[faces[:, i]], out=out, casting="same_kind")
    return out


def _delete_invalid_verts(verts, faces, keep):
    import torch
    v, f = _mcu.delete_invalid_verts(torch.from_numpy(np.ascontiguousarray(verts)), torch.from_numpy(np.ascontiguousarray(faces)),
                                     torch.from_numpy(np.ascontiguousarray(keep)))
    return v.numpy(), f.numpy()


def _remove_holes(verts, faces, keep, backend, extra=None):
    """eval.py:497-503 / :529-548 -- the faces whose vertices are all kept, then the largest connected component of those (the vertices of
    `extra` travel along); no surviving face raises ValueError, as np.argmax(cc_sizes) does there"""
    v1, f1 = _delete_invalid_verts(verts, faces, keep)
    e1 = _delete_invalid_verts(extra, faces, keep)[0] if extra is not None else None
    cc = backend.largest_connected_component(f1, v1.shape[0])
    v2, f2 = _delete_invalid_verts(v1, f1, cc)
    e2 = _delete_invalid_verts(e1, f1, cc)[0] if extra is not None else None
    return v2, f2, e2


def _get(sample, path):
    return np.asarray(sample[path])


def _pred_mesh(sample, volume_task_space):
    v, f, sim = _get(sample, "marching_cubes_mesh/verts"), _get(sample, "marching_cubes_mesh/faces"), _get(sample, "marching_cubes_mesh/warp_field")
    if volume_task_space:                   # eval.py:209-213: verts in simulation space, warp field in NOCS space
        v, sim = sim, v
    return v, f, sim


def _gt_mesh(sample):
    return _get(sample, "gt_mesh/cloth_faces_tri"), _get(sample, "gt_mesh/cloth_nocs_verts"), _get(sample, "gt_mesh/cloth_verts")


def _gt_mc(sample):
    g = "gt_marching_cubes_mesh/"
    return _get(sample, g + "marching_cube_verts"), _get(sample, g + "marching_cube_faces"), _get(sample, g + "is_vertex_on_surface")


def _sampled_points(verts, faces, num_points, seed, *others):
    """points sampled on (verts, faces) and the same barycentric points interpolated in each of `others` (per-vertex arrays)"""
    bc, fi = mesh_sample_barycentric(verts, faces, int(num_points), seed=seed)
    ff = faces[fi]
    return bc, ff, [barycentric_interpolation(bc, verts, ff)] + [barycentric_interpolation(bc, o, ff) for o in others]


def _valid_samples(sample, value_key, bc, ff, value_threshold):
    value = _get(sample, value_key)
    return np.squeeze(barycentric_interpolation(bc, np.expand_dims(value, axis=1), ff)) > value_threshold


# ---------------------------------------------------------------------------------------------------------------- metrics
def plan_optimal_gradient_threshold(sample, precision_weight=0.85, **_):
    """eval.py:58-102"""
    gt_mc_verts = _get(sample, "gt_marching_cubes_mesh/marching_cube_verts")
    on_surface = _get(sample, "gt_marching_cubes_mesh/is_vertex_on_surface")
    pred_verts = _get(sample, "marching_cubes_mesh/verts")
    gm = _get(sample, "marching_cubes_mesh/volume_gradient_magnitude")

    def finish(nn, _pm):
        nn_idx = nn[0][0]
        if len(gt_mc_verts) == 0 and len(nn_idx):
            raise IndexError("index 0 is out of bounds for axis 0 with size 0")     # cKDTree on no points answers index 0
        return {"optimal_wnf_gradient_threshold": decision_stump_threshold(gm, on_surface[nn_idx], precision_weight)}
    return Plan(finish, nn=[(pred_verts, gt_mc_verts)])


def decision_stump_threshold(gm, nn_is_on_surface, precision_weight):
    """the gradient value that maximises precision_weight * precision + (1 - precision_weight) * recall of "on surface iff gm >= value"
    (eval.py:82-100); min(gm) when no score is finite"""
    order = np.argsort(gm)
    s = nn_is_on_surface[order]
    fn = np.cumsum(s)
    tp = np.cumsum(s[::-1])[::-1]
    fp = np.cumsum(~s[::-1])[::-1]
    with np.errstate(all="ignore"):
        precision = tp / (tp + fp)
        recall = tp / (tp + fn)
        score = precision * precision_weight + recall * (1 - precision_weight)
    if np.any(np.isfinite(score)):
        return gm[order[np.argmax(score)]]
    return gm.min()


def optimal_gradient_threshold(sample, precision_weight=0.85, backend=None):
    return _run(plan_optimal_gradient_threshold(sample, precision_weight), backend)


def pc_metrics(sample, nocs_aabb, **_):
    """eval.py:105-143 (host only)"""
    gt = aabb_inverse(nocs_aabb, _get(sample, "point_cloud/gt_nocs"))
    pred = aabb_inverse(nocs_aabb, _get(sample, "point_cloud/pred_nocs"))
    diff = pred - gt
    err_per_dim = np.mean(np.abs(diff), axis=0)
    std_per_dim = np.std(diff, axis=0)
    mirror_gt = gt.copy()
    mirror_gt[:, 0] = -mirror_gt[:, 0]
    dist = np.linalg.norm(diff, axis=1)
    mirror_dist = np.linalg.norm(pred - mirror_gt, axis=1)
    out = {"nocs_pc_error_distance": np.mean(dist), "nocs_pc_mirror_error_distance": np.mean(mirror_dist),
           "nocs_pc_min_agg_error_distance": np.mean(np.minimum(dist, mirror_dist)),
           "nocs_pc_agg_min_error_distance": np.minimum(np.mean(dist), np.mean(mirror_dist))}
    for name, v in (("nocs_pc_diff_std", std_per_dim), ("nocs_pc_error", err_per_dim)):
        for i, ax in enumerate("xyz"):
            out[f"{name}_{ax}"] = v[i]
    return out


def grip_point_metrics(sample, nocs_aabb, **_):
    """eval.py:146-182 (host only)"""
    gt = aabb_inverse(nocs_aabb, _get(sample, "misc/gt_nocs_grip_point"))
    preds = (("pc", aabb_inverse(nocs_aabb, _get(sample, "misc/pred_nocs_grip_point"))),
             ("global", aabb_inverse(nocs_aabb, _get(sample, "misc/pred_global_nocs_grip_point"))))
    out = {}
    for key, p in preds:
        mirror = p.copy()
        mirror[0] = -mirror[0]
        e, me = np.linalg.norm(p - gt), np.linalg.norm(mirror - gt)
        out[f"grip_point_error_distance_{key}"] = e
        out[f"grip_point_mirror_error_distanc_{key}"] = me
        out[f"grip_point_min_error_distanc_{key}"] = min(e, me)
    return out


def plan_sampled_chamfer(sample, nocs_aabb, num_points=1e4, value_threshold=0.13, value_key="marching_cubes_mesh/volume_gradient_magnitude",
                         seed=0, predict_holes=True, volume_task_space=False, **_):
    """eval.py:185-317: symmetric chamfer distance between points sampled on the predicted and the ground-truth surfaces, per category"""
    pv, pf, psim = _pred_mesh(sample, volume_task_space)
    gf, gnocs, gsim = _gt_mesh(sample)
    mv, mf, mon = _gt_mc(sample)
    gnocs, pv, mv = aabb_inverse(nocs_aabb, gnocs), aabb_inverse(nocs_aabb, pv), aabb_inverse(nocs_aabb, mv)
    pbc, pff, (p_nocs, p_sim) = _sampled_points(pv, pf, num_points, seed, psim)
    _, _, (g_nocs, g_sim) = _sampled_points(gnocs, gf, num_points, seed, gsim)
    sv, sf = _delete_invalid_verts(mv, mf, mon)
    _, _, (g_mc,) = _sampled_points(sv, sf, num_points, seed)
    cats = {"nocs_no_hole": (p_nocs, g_nocs), "sim_no_hole": (p_sim, g_sim), "nocs_mc": (g_mc, g_nocs)}
    if predict_holes:
        ok = _valid_samples(sample, value_key, pbc, pff, value_threshold)
        cats.update(nocs=(p_nocs[ok], g_nocs), sim=(p_sim[ok], g_sim))
    order = [c for c in _hole_categories(predict_holes)]
    nn = [pair for c in order for pair in (cats[c], cats[c][::-1])]

    def finish(res, _pm):
        out = {}
        for k, c in enumerate(order):
            fwd = np.mean(np.sqrt(res[2 * k][1]))
            bwd = np.mean(np.sqrt(res[2 * k + 1][1]))
            out[f"chamfer_symmetrical_{c}"] = np.mean([fwd, bwd])
        return out
    return Plan(finish, nn=nn)


def sampled_chamfer(sample, nocs_aabb, backend=None, **kw):
    return _run(plan_sampled_chamfer(sample, nocs_aabb, **kw), backend)


def plan_sampled_hybrid_chamfer(sample, nocs_aabb, num_points=1e4, value_threshold=0.13,
                                value_key="marching_cubes_mesh/volume_gradient_magnitude", seed=0, predict_holes=True, volume_task_space=False,
                                **_):
    """eval.py:320-456: nearest neighbours found in NOCS space, distances measured between the matched points in simulation space; with
    the prediction's NOCS mirrored in x ("mirror") and the smaller of the two ("min")"""
    pv, pf, psim = _pred_mesh(sample, volume_task_space)
    gf, gnocs, gsim = _gt_mesh(sample)
    gnocs, pv = aabb_inverse(nocs_aabb, gnocs), aabb_inverse(nocs_aabb, pv)
    pbc, pff, (p_nocs, p_sim) = _sampled_points(pv, pf, num_points, seed, psim)
    _, _, (g_nocs, g_sim) = _sampled_points(gnocs, gf, num_points, seed, gsim)
    cats = [("no_hole", p_nocs, p_sim)]
    if predict_holes:
        ok = _valid_samples(sample, value_key, pbc, pff, value_threshold)
        cats.insert(0, ("regular", p_nocs[ok], p_sim[ok]))
    nn, jobs = [], []
    for c, pn, ps in cats:
        mirror = pn.copy()
        mirror[:, 0] = -mirror[:, 0]
        for aug, q in (("pred", pn), ("mirror", mirror)):
            nn += [(q, g_nocs), (g_nocs, q)]
            jobs.append((c, aug, ps))

    def finish(res, _pm):
        out = {}
        for k in range(0, len(jobs), 2):
            c = jobs[k][0]
            per = {}
            for aug, ps, (fwd_r, bwd_r) in ((jobs[k][1], jobs[k][2], res[2 * k:2 * k + 2]), (jobs[k + 1][1], jobs[k + 1][2], res[2 * k + 2:2 * k + 4])):
                f = np.mean(np.linalg.norm(ps - g_sim[fwd_r[0]], axis=1))
                b = np.mean(np.linalg.norm(g_sim - ps[bwd_r[0]], axis=1))
                per[aug] = {"forward": f, "backward": b, "symmetrical": np.mean([f, b])}
            per["min"] = {m: min(per["pred"][m], per["mirror"][m]) for m in per["pred"]}
            for aug in ("pred", "mirror", "min"):
                for m in ("forward", "backward", "symmetrical"):
                    out[f"hybrid_chamfer_{m}_{c}_{aug}"] = per[aug][m]
        return out
    return Plan(finish, nn=nn)


def sampled_hybrid_chamfer(sample, nocs_aabb, backend=None, **kw):
    return _run(plan_sampled_hybrid_chamfer(sample, nocs_aabb, **kw), backend)


def plan_hausdorff(sample, nocs_aabb, value_threshold=0.13, value_key="marching_cubes_mesh/volume_gradient_magnitude", predict_holes=True,
                   volume_task_space=False, backend=None, **_):
    """eval.py:458-580: igl.hausdorff between the ground-truth cloth mesh and the predicted / ground-truth marching-cubes meshes"""
    backend = backend if backend is not None else default_backend()
    pv, pf, psim = _pred_mesh(sample, volume_task_space)
    gf, gnocs, gsim = _gt_mesh(sample)
    mv, mf, mon = _gt_mc(sample)
    gnocs, pv, mv = aabb_inverse(nocs_aabb, gnocs), aabb_inverse(nocs_aabb, pv), aabb_inverse(nocs_aabb, mv)
    cv, cf, _ = _remove_holes(mv, mf, mon, backend)
    cats = {"nocs_no_hole": (gnocs, gf, pv, pf), "sim_no_hole": (gsim, gf, psim, pf), "nocs_mc": (gnocs, gf, cv, cf)}
    if predict_holes:
        hv, hf, hsim = _remove_holes(pv, pf, _get(sample, value_key) > value_threshold, backend, extra=psim)
        cats.update(nocs=(gnocs, gf, hv, hf), sim=(gsim, gf, hsim, hf))
    order = list(_hole_categories(predict_holes))
    pm = [p for c in order for p in mesh_hausdorff_pairs(*cats[c])]

    def finish(_nn, res):
        return {f"hausdorff_{c}": _hausdorff_from(res[2 * k], res[2 * k + 1]) for k, c in enumerate(order)}
    return Plan(finish, pm=pm)


def mesh_hausdorff_pairs(va, fa, vb, fb):
    """the two point-to-mesh searches of igl.hausdorff(va, fa, vb, fb): the vertices of B against mesh A, those of A against mesh B"""
    return [(vb, va, fa), (va, vb, fb)]


def _hausdorff_from(ba, ab):
    return np.sqrt(max(np.max(ba[1]), np.max(ab[1])))


def mesh_hausdorff(va, fa, vb, fb, backend=None):
    """igl.hausdorff(va, fa, vb, fb): sqrt of the larger of the two largest squared vertex-to-mesh distances (fp64)"""
    plan = Plan(lambda _nn, res: _hausdorff_from(res[0], res[1]), pm=mesh_hausdorff_pairs(va, fa, vb, fb))
    return _run(plan, backend)


def hausdorff(sample, nocs_aabb, backend=None, **kw):
    return _run(plan_hausdorff(sample, nocs_aabb, backend=backend, **kw), backend)

"""The cases of tests/golden/ref_render.npz (make_golden_render.py) as calls of garmentnets_amd.visualize: shared by the host test (numpy backend) and the
GPU test (device backend), so both backends answer the same questions."""
import os

import numpy as np

from garmentnets_amd import visualize as V

SIDES = ("front", "top", "left")
KERNELS = (1, 4, 5, 8)


def load_golden(golden_dir):
    with np.load(os.path.join(golden_dir, "ref_render.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_pairs(g, backend):
    """-> [(name, ours, the reference's)] over every image of the golden file"""
    out = []

    def nocs(name):
        p, side, k, S = g[name + "/points"], str(g[name + "/side"]), int(g[name + "/k"]), int(g[name + "/S"])
        return (V.render_points_idx(p, img_size=S, kernel_size=k, side=side, backend=backend),
                V.render_nocs(p, side=side, img_size=S, kernel_size=k, backend=backend))

    for name in [f"cloud_{s}_k{k}" for s in SIDES for k in KERNELS] + ["nonfinite", "empty"]:
        idx, img = nocs(name)
        out += [(name + "/idx", idx, g[name + "/idx"]), (name + "/img", img, g[name + "/img"])]
    idx, img = nocs("big")
    out += [("big/idx", idx, g["big/idx"]), ("big/img_sub", img[::8, ::8], g["big/img_sub"])]
    q, wnf, pred = g["wnf/query"], g["wnf/values"], g["wnf_pair/pred"]
    out.append(("wnf/img", V.render_wnf_points(q, wnf, img_size=32, backend=backend), g["wnf/img"]))
    out.append(("wnf_pair/img", V.render_wnf_points_pair(q, wnf, pred, img_size=32, backend=backend), g["wnf_pair/img"]))
    out.append(("wnf_none/img", V.render_wnf_points(g["wnf_none/query"], wnf, img_size=32, backend=backend), g["wnf_none/img"]))
    gt, pr, grips, conf = g["pair/gt"], g["pair/pred"], g["pair/grips"], g["pair/confidence"]
    out.append(("pair/img", V.render_nocs_pair(gt, pr, grips[0], grips[1], grips[2], img_size=32, kernel_size=4, backend=backend), g["pair/img"]))
    out.append(("pair/img_two_grips", V.render_nocs_pair(gt, pr, grips[0], grips[1], img_size=32, kernel_size=5, backend=backend),
                g["pair/img_two_grips"]))
    out.append(("pair/confidence_img", V.render_confidence_pair(gt, pr, conf, img_size=32, backend=backend), g["pair/confidence_img"]))
    out.append(("pair/overlay_img", V.overlay_grip(g["cloud_front_k4/img"], grips[0], color=(0, 1, 0, 1), kernel_size=8, backend=backend),
                g["pair/overlay_img"]))
    return out


def equal(a, b):
    """np.array_equal of two arrays of one shape and dtype"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)

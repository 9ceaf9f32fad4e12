"""The torch restatements of the training step (tests/test_gpu_train.py, tests/test_train_host.py): the losses, PointNet2NOCS's forward, Adam's inputs.
Plain torch at any dtype on the CPU; a plain module, imported by its siblings; it holds no test.  The indices (FPS, ball tables as gn_sa_gather's slot
table, kNN neighbours) and the ReLU masks are taken from the HIP forward -- `record_forward` captures them -- so both sides differentiate the same
piecewise-linear map; the max winners are each side's own, as in the other gradient suites."""
import contextlib

import torch
import torch.nn.functional as F

from garmentnets_amd.components.gridding import VirtualGrid
from grad_reference import r_sa_gather, r_segment_max


# ------------------------------------------------------------------------------------------------ losses
def mirror(p, axis):
    """components/symmetry.py on one axis: fp32, each step rounded"""
    if axis is None:
        return p
    q = p.clone()
    q[:, axis] = (q[:, axis] - 0.5) * -1 + 0.5
    return q


def target_bins(gt, bins):
    """VirtualGrid.get_points_grid_idxs over the unit cube (tests/test_gpu_validate.py::bin_restatement forms them the same way)"""
    return VirtualGrid(grid_shape=(bins,) * 3, batch_size=1, device=gt.device).get_points_grid_idxs(gt.float())


def r_bin_loss(sets, bins, weights, targets):
    """sum_s w_s * CrossEntropyLoss(logits_s viewed (n, bins, 3), targets_s (n, 3)); logits of any dtype"""
    total = 0
    for (lg, _), w, t in zip(sets, weights, targets):
        total = total + w * F.cross_entropy(lg[:, :bins * 3].reshape(lg.shape[0], bins, 3), t)
    return total


VALUE_LOSS = {"l2": F.mse_loss, "smooth_l1": F.smooth_l1_loss, "bce_logits": F.binary_cross_entropy_with_logits}


def mirror_x(t):
    """MirrorMSELoss's target: x of (M, 3) rows mirrored about 0.5, fp32"""
    q = t.reshape(-1, 3).clone()
    q[:, 0] = (q[:, 0] - 0.5) * -1 + 0.5
    return q.reshape(t.shape)


# ------------------------------------------------------------------------------------------------ what the HIP forward decided
@contextlib.contextmanager
def record_forward():
    """while active: every gn_linear call with a ReLU leaves its output r (the masks, in execution order), every gn_sa_gather call its centre indices
    and slot table"""
    from garmentnets_amd import ops
    rec = {"r": [], "sa": []}
    linear, sa_gather = ops.linear, ops.sa_gather

    def rec_linear(x, w, bias=None, bn_scale=None, bn_shift=None, relu=False, out=None, K=None):
        y = linear(x, w, bias, bn_scale, bn_shift, relu=relu, out=out, K=K)
        if relu:
            assert bn_scale is None                                   # r itself, before any affine
            rec["r"].append(y.detach().clone())
        return y

    def rec_sa_gather(x, pos, centre_idx, nbr, self_loops=True, self_src=None):
        res = sa_gather(x, pos, centre_idx, nbr, self_loops=self_loops, self_src=self_src)
        rec["sa"].append((centre_idx.cpu().long(), res[1].cpu(), res[2], nbr.shape[0]))
        return res
    ops.linear, ops.sa_gather = rec_linear, rec_sa_gather
    try:
        yield rec
    finally:
        ops.linear, ops.sa_gather = linear, sa_gather


# ------------------------------------------------------------------------------------------------ PointNet2NOCS
def r_knn(x, nbr, d2, n_sources):
    """nbr / d2 (Nq, k) shared data -> the interpolation matrix (no gradient through it) @ x"""
    valid = nbr >= 0
    w = valid.to(x.dtype) / d2.to(x.dtype).clamp(min=1e-16)
    coef = w / w.sum(1, keepdim=True)
    mat = torch.zeros((nbr.shape[0], n_sources), dtype=x.dtype)
    mat.scatter_add_(1, nbr.clamp(min=0).long(), coef)
    return mat @ x


def r_global_max(h, sizes):
    out, s = [], 0
    for n in sizes:
        out.append(h[s:s + n].max(0).values)
        s += n
    return torch.stack(out)


class Restated:
    """PointNet2NOCS.forward in plain torch at `dtype`.  P: name -> parameter (leaf, dtype); buffers: name -> running statistic (fp32 data);
    rec: record_forward's capture of the HIP forward; gmask: the HIP forward's global_feature > 0; knn: level -> (nbr, d2) on the CPU; training: BatchNorm on batch statistics over the rows the
    stack sees (the SA stacks: real edges only)"""

    def __init__(self, model, P, buffers, rec, knn, sizes, gmask, dtype, training):
        self.model, self.P, self.B, self.dtype, self.training = model, P, buffers, dtype, training
        self.masks = iter([(r > 0).cpu() for r in rec["r"]])
        self.sa = iter(rec["sa"])
        self.knn, self.sizes, self.gmask = knn, sizes, gmask

    def mlp(self, prefix, stack, h):
        for i, block in enumerate(stack):
            p = f"{prefix}.{i}"
            h = F.linear(h, self.P[p + ".0.weight"], self.P[p + ".0.bias"]) * next(self.masks).to(self.dtype)
            if len(block) > 2:
                bn = block[2]
                if self.training:
                    h = F.batch_norm(h, None, None, self.P[p + ".2.weight"], self.P[p + ".2.bias"], True, 0.0, bn.eps)
                else:
                    h = F.batch_norm(h, self.B[p + ".2.running_mean"].to(self.dtype), self.B[p + ".2.running_var"].to(self.dtype), self.P[p + ".2.weight"],
                                     self.P[p + ".2.bias"], False, 0.0, bn.eps)
        return h

    def conv(self, name, module, x, pos):
        cidx, slot, S, M = next(self.sa)
        edges = r_sa_gather(x, pos, cidx, slot, S)
        rows = (slot >= 0).nonzero().squeeze(1)
        hc = self.mlp(f"{name}.conv.local_nn", module.conv.local_nn, edges[rows])
        h = torch.zeros((M * S, hc.shape[1]), dtype=self.dtype).index_copy(0, rows, hc)
        return r_segment_max(h, slot, M, S), pos[cidx]

    def forward(self, x, pos):
        m, P, dt = self.model, self.P, self.dtype
        x0, p0 = x.to(dt), pos.to(dt)
        x1, p1 = self.conv("sa1_module", m.sa1_module, x0, p0)
        x2, p2 = self.conv("sa2_module", m.sa2_module, x1, p1)
        x3 = r_global_max(self.mlp("sa3_module.nn", m.sa3_module.nn, torch.cat((x2, p2), 1)), self.sizes[2])
        h = self.mlp("fp3_module.nn", m.fp3_module.nn, torch.cat((r_knn(x3, *self.knn[3], x3.shape[0]), x2), 1))
        h = self.mlp("fp2_module.nn", m.fp2_module.nn, torch.cat((r_knn(h, *self.knn[2], h.shape[0]), x1), 1))
        h = self.mlp("fp1_module.nn", m.fp1_module.nn, torch.cat((r_knn(h, *self.knn[1], h.shape[0]), x0), 1))
        h = F.linear(h, P["lin1.weight"], P["lin1.bias"]) * next(self.masks).to(dt)
        features = F.linear(h, P["lin2.weight"], P["lin2.bias"])
        logits = F.linear(features, P["lin3.weight"], P["lin3.bias"])
        g = F.linear(x3 * self.gmask.to(dt), P["global_lin1.weight"], P["global_lin1.bias"])
        return logits, F.linear(g, P["global_lin2.weight"], P["global_lin2.bias"])

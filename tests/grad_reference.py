"""What the GPU suites share (test_gpu_autograd*.py, test_gpu_unet_grad.py, test_gpu_mlp_grad.py, test_*pointnet2_forward*.py): the error rule and the
plain restatements that more than one of them uses.  A plain module, imported by its siblings; it holds no test."""
import numpy as np
import torch
import torch.nn.functional as F


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(name, ref64, t32, ours, factor=4):
    """THE rule: ours against fp64 <= factor x (torch-fp32 against fp64) + 1 fp32 ulp of the largest gradient, every element finite; prints the figures
    before it asserts; returns the ratio ours / torch-fp32 (0 for an empty tensor, which passes)"""
    ref64, t32, ours = ref64.double().cpu(), t32.double().cpu(), ours.double().cpu()
    assert ref64.shape == ours.shape, (name, ref64.shape, ours.shape)
    if ref64.numel() == 0:
        return 0.0
    assert bool(torch.isfinite(ours).all()), name
    e32 = float((t32 - ref64).abs().max())
    eo = float((ours - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max())))
    print(f"[grad-error] {name}: torch-fp32 {e32:.3e}  hip {eo:.3e}  ulp(max |g|) {ulp:.3e}  bound {factor * e32 + ulp:.3e}  ratio {eo / max(e32, 1e-300):.2f}")
    assert eo <= factor * e32 + ulp, (name, eo, e32, ulp)
    return eo / max(e32, 1e-300)


# ------------------------------------------------------------------------------------------------ restatements (plain torch, any dtype, any device)
def _first_max(vals, mask, dim):
    """one-hot (same shape) of the FIRST maximum of vals along dim among mask (all False where mask is empty): written out, no reliance on argmax"""
    neg = torch.where(mask, vals, torch.full_like(vals, -float("inf")))
    eq = (neg == neg.max(dim=dim, keepdim=True).values) & mask
    return eq & (eq.cumsum(dim) == 1)


def r_segment_max(h, slot_src, M, S):
    hv = h.reshape(M, S, -1)
    sel = _first_max(hv, (slot_src.reshape(M, S) >= 0)[:, :, None].expand_as(hv), 1)
    return (hv * sel.to(h.dtype)).sum(1)


def r_sa_gather(x, pos, centre_idx, slot_src, S):
    """edge rows [x_j, pos_j - pos_i] (x None: the positions alone); an empty slot is a zero row.  x through a one-hot matrix (differentiable),
    positions are data"""
    rows, n = slot_src.numel(), pos.shape[0]
    valid = slot_src >= 0
    j = slot_src.clamp(min=0).long()
    onehot = ((j[:, None] == torch.arange(n, device=pos.device)[None, :]) & valid[:, None]).to(pos.dtype)
    ci = centre_idx.long()[torch.arange(rows, device=pos.device) // S]
    rel = (pos[j] - pos[ci]) * valid[:, None].to(pos.dtype)
    return torch.cat((onehot @ x, rel), 1) if x is not None else rel


def r_sample(volume, query):
    """volume (N, C, D, H, W), query (N, M, 3) in [0, 1] -> (N, M, C): the reference's call of F.grid_sample"""
    n, m = query.shape[:2]
    s = F.grid_sample(volume, (2.0 * query - 1.0).view(n, m, 1, 1, 3), mode="bilinear", padding_mode="border", align_corners=True)
    return s.view(n, volume.shape[1], m).permute(0, 2, 1)


def r_layer(x0, x1, w, gamma, beta, groups, eps, mask=None):
    """one 'gcr' layer over the virtual concat [x0, x1 nearest-upsampled] (NCDHW); mask: the ReLU's selection handed in, None: its own"""
    x = x0 if x1 is None else torch.cat((x0, F.interpolate(x1, scale_factor=2, mode="nearest")), 1)
    h = F.conv3d(F.group_norm(x, groups, gamma, beta, eps), w, padding=1)
    return F.relu(h) if mask is None else h * mask


def r_unet(model, P, x, selections=None, record=None, prefix=""):
    """model: the module (structure); P: its parameters by name, each under `prefix`, in x's dtype.
    selections: (ReLU masks per layer in execution order, pool winner indices per level) taken from the HIP forward: the restatement then differentiates
    the same piecewise-linear map as the HIP run, whatever the dtype; None: it forms its own, and appends them to the two lists of record when that is
    given (shared selections without a GPU)"""
    masks, winners = (None, None) if selections is None else (iter(selections[0]), iter(selections[1]))

    def double_conv(name, dc, x0, x1=None):
        for k, sc in (("SingleConv1", dc.SingleConv1), ("SingleConv2", dc.SingleConv2)):
            n = f"{prefix}{name}.basic_module.{k}"
            x0 = r_layer(x0, x1, P[n + ".conv.weight"], P[n + ".groupnorm.weight"], P[n + ".groupnorm.bias"], sc.groupnorm.num_groups, sc.groupnorm.eps,
                         mask=None if masks is None else next(masks).to(x0.dtype))
            x1 = None
            if record is not None:
                record[0].append(x0.detach() > 0)
        return x0
    feats = []
    for i, enc in enumerate(model.encoders):
        if i > 0 and winners is not None:
            idx = next(winners)
            x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
        elif i > 0 and record is not None:
            x, idx = F.max_pool3d(x, 2, return_indices=True)
            record[1].append(idx)
        elif i > 0:
            x = F.max_pool3d(x, 2)
        x = double_conv(f"encoders.{i}", enc.basic_module, x)
        feats.insert(0, x)
    for i, dec in enumerate(model.decoders):
        x = double_conv(f"decoders.{i}", dec.basic_module, feats[i + 1], x)
    return F.conv3d(x, P[prefix + "final_conv.weight"], P[prefix + "final_conv.bias"])


def _randomise_norms(module, g):
    """the affine parameters of every GroupNorm and BatchNorm1d, and the running statistics of the BatchNorms; in the first BatchNorm a negative gamma
    and one that is exactly 0"""
    first = True
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.GroupNorm, torch.nn.BatchNorm1d)):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.2 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
                if first:
                    m.weight[0] = -0.8
                    if m.weight.numel() > 1:
                        m.weight[1] = 0.0
                    first = False


# ------------------------------------------------------------------------------------------------ PointNet++ forward (tests/test_*pointnet2_forward*.py)
def point_conv_slots(nbr, cnt, self_loops, self_src=None):
    """(M, S) int64 source point of every edge of every centre, -1 = no edge, formed here in numpy from the ball-query table alone: the first cnt[c]
    entries of row c; with self_loops the entries equal to "node c" (self_src[c], or the centre's own number c) are dropped and node c is appended
    (PyG: remove_self_loops, then add_self_loops over the M targets).  S = K, + 1 with self_loops."""
    nbr, cnt = np.asarray(nbr, np.int64), np.asarray(cnt, np.int64)
    M, K = nbr.shape
    node = np.arange(M, dtype=np.int64) if self_src is None else np.asarray(self_src, np.int64)
    slots = np.where(np.arange(K)[None, :] < cnt[:, None], nbr, -1)
    if self_loops:
        slots = np.concatenate((np.where(slots == node[:, None], -1, slots), node[:, None]), 1)
    return slots


def r_point_conv(x, pos, centre_idx, nbr, cnt, self_loops, self_src, blocks, dtype):
    """PointConv(local_nn, aggr = max) restated in plain torch at `dtype`: rows [x_j, pos_j - pos_i] of every edge (x None: the positions alone)
    through the three blocks (w, b, sc, sh) = Linear -> ReLU -> folded eval-BatchNorm affine (sc None: no BatchNorm), the maximum over a centre's
    edges, 0 for a centre without any.  Inputs are fp32 data (CPU); the relative position is formed at `dtype`."""
    slots = torch.from_numpy(point_conv_slots(nbr, cnt, self_loops, self_src))
    M, S = slots.shape
    valid = slots >= 0
    j = slots.clamp(min=0).reshape(-1)
    ci = centre_idx.long().repeat_interleave(S)
    p = pos.to(dtype)
    h = p[j] - p[ci]
    if x is not None:
        h = torch.cat((x.to(dtype)[j], h), 1)
    for w, b, sc, sh in blocks:
        h = torch.relu(h @ w.to(dtype).t() + b.to(dtype))
        if sc is not None:
            h = h * sc.to(dtype) + sh.to(dtype)
    h = torch.where(valid.reshape(-1, 1), h, torch.full_like(h, -float("inf"))).reshape(M, S, -1).max(1).values
    return torch.where(torch.isinf(h) & (h < 0), torch.zeros_like(h), h)


def ball_query_loop(pos, ptr, centre_idx, centre_ptr, r, K):
    """the radius query as a numpy loop: per centre the first K points of its own example, in ascending index, whose squared distance -- float32,
    ((dx dx + dy dy) + dz dz), every operation rounded -- is strictly below float32(r r); -> (nbr (M, K) int32, -1 from cnt on; cnt (M) int32)"""
    pos = np.ascontiguousarray(pos, np.float32)
    r2 = np.float32(float(r) * float(r))
    M = len(centre_idx)
    nbr, cnt = np.full((M, K), -1, np.int32), np.zeros(M, np.int32)
    for b in range(len(ptr) - 1):
        s, e = int(ptr[b]), int(ptr[b + 1])
        for c in range(int(centre_ptr[b]), int(centre_ptr[b + 1])):
            d = pos[s:e] - pos[int(centre_idx[c])][None, :]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert d2.dtype == np.float32
            hit = s + np.nonzero(d2 < r2)[0][:K]
            nbr[c, :len(hit)], cnt[c] = hit, len(hit)
    return nbr, cnt

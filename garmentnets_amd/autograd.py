"""Differentiable bindings of the point and grid operators, under the third-party call shapes INTEGRATION.md section B documents.

The reference's dense layers (nn.Linear, BatchNorm1d, Conv3d, GroupNorm, ...) have torch's own backward on ROCm.  The third-party operators
between them (torch_cluster.fps / radius, PointConv's gather + max, global_max_pool, knn_interpolate, torch_scatter.scatter, F.grid_sample) are
the ones this package restates in HIP; here each gets a ``torch.autograd.Function`` whose forward is the existing op, unchanged, and whose backward
is a kernel of csrc/grad.hip.  A reference-side module that binds these functions can take gradients on an MI355X.

What this is NOT: a training loop, an optimiser, train-mode BatchNorm, or a backward for the conv / MLP kernels of the inference path (DESIGN.md
section 9).  The inference modules do not import this file; ``gn_sa_fused`` stays inference-only (``point_conv_max`` is the unfused chain).

Selections (max / min) hand the gradient to ONE element per (slot, channel): among equal values the lowest point / edge index (torch_scatter's CUDA
choice is whichever thread wins an atomic: parity unpinned).  Every sum is ordered: identical calls give identical bits.
"""
import torch

from . import ops
from .components.pointnet2 import Segments, _example_self_src

__all__ = ["fps", "radius", "ball_table", "point_conv_max", "global_max_pool", "knn_interpolate", "scatter", "grid_sample_points"]


def _rows(t):
    """fp32 rows the C ABI can read in place (unit column stride), else a contiguous copy"""
    if t.dtype != torch.float32:
        raise TypeError(f"expected torch.float32 features, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"expected (rows, channels), got shape {tuple(t.shape)}")
    return t if (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= t.shape[1] else t.contiguous()


# ------------------------------------------------------------------------------------------------ index results (no gradient)
def fps(pos, batch, ratio=0.5, random_start=False):
    """torch_cluster.fps(pos, batch, ratio): int64 indices of the sampled points.  random_start=False (the first point of each example) is this
    package's pinned choice; an index result, not differentiable."""
    seg = Segments.of(batch)
    with torch.no_grad():
        cseg = Segments([ops.fps_count(n, ratio) for n in seg.sizes], pos.device)
        start = None
        if random_start:
            start = torch.tensor([int(torch.randint(0, max(n, 1), (1,))) for n in seg.sizes], dtype=torch.int32).to(pos.device)
        idx = ops.fps(pos.detach().contiguous(), seg.ptr, cseg.ptr, max(seg.sizes) if seg.sizes else 0, cseg.total, start)
    return idx.long()


def ball_table(x, y_idx, r, batch_x, batch_y, max_num_neighbors=32):
    """The radius graph as gn_ball_query's table: (nbr int32 [M][K] -- the first K points within r of centre x[y_idx[c]], ascending index, -1 padded --
    and cnt int32 [M]).  ``point_conv_max`` takes this form."""
    seg, cseg = Segments.of(batch_x), Segments.of(batch_y)
    with torch.no_grad():
        return ops.ball_query(x.detach().contiguous(), seg.ptr, y_idx.to(torch.int32), cseg.ptr, r, int(max_num_neighbors))


def radius(x, y_idx, r, batch_x, batch_y, max_num_neighbors=32):
    """torch_cluster.radius(x, x[y_idx], r, batch_x, batch_y, max_num_neighbors) -> edge_index (2, E) int64: row = centre, col = point of x."""
    nbr, _ = ball_table(x, y_idx, r, batch_x, batch_y, max_num_neighbors)
    row, col = (nbr >= 0).nonzero(as_tuple=True)
    return torch.stack((row, nbr[row, col].long()))


# ------------------------------------------------------------------------------------------------ PointConv(local_nn, aggr='max')
class _SaGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, centre_idx, nbr, self_loops, self_src):
        edges, slot_src, _ = ops.sa_gather(x, pos, centre_idx, nbr, self_loops=self_loops, self_src=self_src)
        ctx.save_for_backward(slot_src)
        ctx.x_shape = tuple(x.shape)
        ctx.mark_non_differentiable(slot_src)
        return edges, slot_src

    @staticmethod
    def backward(ctx, grad_edges, _):
        (slot_src,) = ctx.saved_tensors
        n, c = ctx.x_shape
        gx = ops.sa_gather_bwd(grad_edges, slot_src, c, n) if ctx.needs_input_grad[0] else None
        return gx, None, None, None, None, None


class _SegmentMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, slot_src, M, S):
        out = ops.segment_max(h, slot_src, M, S)
        ctx.save_for_backward(h, out, slot_src)
        ctx.ms = (M, S)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, out, slot_src = ctx.saved_tensors
        return ops.segment_max_bwd(grad_out, out, h, slot_src, *ctx.ms), None, None, None


def point_conv_max(x, pos, centre_idx, nbr, local_nn, add_self_loops=True, self_loop_scope="batch", batch=None, batch_centre=None):
    """PointConv(local_nn, aggr='max') over the radius graph ``nbr`` (``ball_table``): edge rows [x_j, pos_j - pos_i] -> ``local_nn`` (any
    nn.Module, torch's own backward) -> max per centre.  Differentiable in x and in local_nn's parameters; positions are data.  The unfused chain
    gn_sa_gather + local_nn + gn_segment_max.  self_loop_scope="example" (needs batch / batch_centre): the self-loop rule per example, as
    components.pointnet2.SAModule applies it."""
    centre_idx = centre_idx.to(torch.int32)
    M, K = nbr.shape
    S = K + (1 if add_self_loops else 0)
    self_src = None
    if add_self_loops and self_loop_scope == "example":
        seg, cseg = Segments.of(batch), Segments.of(batch_centre)
        if seg.num > 1:
            self_src = _example_self_src(seg.sizes, cseg.sizes, pos.device)
    pos = pos.detach().contiguous()
    if x is None:
        edges, slot_src, _ = ops.sa_gather(None, pos, centre_idx, nbr, self_loops=add_self_loops, self_src=self_src)
    else:
        edges, slot_src = _SaGather.apply(_rows(x), pos, centre_idx, nbr, add_self_loops, self_src)
    h = local_nn(edges) if local_nn is not None else edges
    return _SegmentMax.apply(_rows(h), slot_src, M, S)


# ------------------------------------------------------------------------------------------------ global_max_pool
class _GlobalMaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, ptr, B):
        out = ops.global_max_pool(h, ptr, B)
        ctx.save_for_backward(h, out, ptr)
        ctx.B = B
        return out

    @staticmethod
    def backward(ctx, grad_out):
        h, out, ptr = ctx.saved_tensors
        return ops.global_max_pool_bwd(grad_out, out, h, ptr, ctx.B), None, None


def global_max_pool(x, batch):
    """torch_geometric.nn.global_max_pool(x, batch) -> (B, C)"""
    seg = Segments.of(batch)
    return _GlobalMaxPool.apply(_rows(x), seg.ptr, seg.num)


# ------------------------------------------------------------------------------------------------ knn_interpolate
class _KnnInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos_x, ptr_x, pos_y, ptr_y, k):
        out = ops.knn_interpolate(x, pos_x, ptr_x, pos_y, ptr_y, k)
        ctx.save_for_backward(pos_x, ptr_x, pos_y, ptr_y)
        ctx.k, ctx.n = k, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_y):
        pos_x, ptr_x, pos_y, ptr_y = ctx.saved_tensors
        # the forward keeps no index tensor: the same search again (ascending (d2, index), the forward kernels' order)
        nbr, d2 = ops.knn_neighbours(pos_x, ptr_x, pos_y, ptr_y, ctx.k)
        return ops.knn_interpolate_bwd(grad_y, nbr, d2, ctx.n), None, None, None, None, None


def knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k=3):
    """torch_geometric.nn.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k): gradient to the features x only -- the neighbour search and the
    weights sit under no_grad in torch_geometric too."""
    seg_x, seg_y = Segments.of(batch_x), Segments.of(batch_y)
    return _KnnInterpolate.apply(_rows(x), pos_x.detach().contiguous(), seg_x.ptr, pos_y.detach().contiguous(), seg_y.ptr, int(k))


# ------------------------------------------------------------------------------------------------ torch_scatter.scatter
class _GridScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, flat_idx, cells, reduce):
        vol = ops.grid_scatter(rows, flat_idx, 1, (cells,), reduce).view(cells, rows.shape[1])
        if reduce in ("max", "min"):
            ctx.save_for_backward(flat_idx, vol, rows)       # the winner test reads the stored output and the input
        else:
            ctx.save_for_backward(flat_idx)                  # mean: the cell counts are counted again from flat_idx (one int32 per cell)
        ctx.reduce, ctx.n = reduce, rows.shape[0]
        return vol

    @staticmethod
    def backward(ctx, grad_vol):
        flat_idx, *rest = ctx.saved_tensors
        vol, rows = rest if rest else (None, None)
        return ops.grid_scatter_bwd(grad_vol.contiguous(), flat_idx, ctx.n, ctx.reduce, vol=vol, src=rows), None, None, None


def scatter(src, index, dim=-1, dim_size=None, reduce="mean"):
    """torch_scatter.scatter(src (C, N), index (N,), dim=-1, dim_size, reduce) -> (C, dim_size), the call of networks/conv_implicit_wnf.py:92-94.
    Empty cells hold 0 (1 under 'mul').  'mul' runs forward-only: asking for its gradient is a ValueError."""
    if reduce not in ops.REDUCE_CODES:
        raise ValueError(f"scatter: reduce={reduce!r} is not one of {sorted(ops.REDUCE_CODES)}")
    if src.dim() != 2 or dim not in (-1, 1) or index.dim() != 1 or index.numel() != src.shape[1]:
        raise ValueError("scatter: this binding takes src (C, N), index (N,) and dim=-1")
    if dim_size is None:
        dim_size = int(index.max().item()) + 1 if index.numel() else 0
    if reduce == "mul" and torch.is_grad_enabled() and src.requires_grad:
        raise ValueError("scatter: reduce='mul' has no gradient here (nobody trains with it; it divides by zero at a zero factor)")
    rows = _rows(src.t())
    return _GridScatter.apply(rows, index.to(torch.int32).contiguous(), int(dim_size), reduce).t()


# ------------------------------------------------------------------------------------------------ F.grid_sample
class _TrilinearSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vol, query):
        out = ops.trilinear_sample_batch(vol, query)
        ctx.save_for_backward(vol, query)
        return out

    @staticmethod
    def backward(ctx, grad_rows):
        vol, query = ctx.saved_tensors
        return ops.trilinear_sample_bwd(grad_rows, vol, query, want_vol=ctx.needs_input_grad[0], want_query=ctx.needs_input_grad[1])


def grid_sample_points(volume, query):
    """ImplicitWNFDecoder.forward's sampling: F.grid_sample(volume (N, C, D, H, W), 2 * query - 1, mode='bilinear', padding_mode='border',
    align_corners=True) at query (N, M, 3) in [0, 1] -> features (N, M, C).  Differentiable in the volume and in the query (a coordinate clamped
    at the border gets gradient 0, F.grid_sample's rule).  The volume gradient is an ordered sum per voxel: no float atomics."""
    if volume.dim() != 5 or query.dim() != 3 or query.shape[0] != volume.shape[0] or query.shape[2] != 3:
        raise ValueError("grid_sample_points: volume must be (N, C, D, H, W) and query (N, M, 3)")
    if volume.dtype != torch.float32 or query.dtype != torch.float32:
        raise TypeError("grid_sample_points: volume and query must be torch.float32")
    return _TrilinearSample.apply(volume.permute(0, 2, 3, 4, 1).contiguous(), query.contiguous())

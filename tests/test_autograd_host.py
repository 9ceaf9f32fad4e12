"""CPU: the operator gradients' host side -- argument checks raised before any launch, header / prototypes in step, imports without a GPU -- and
the SPARSE restatements of the six operators (s_*: index_add_ / scatter_reduce / gather, memory linear in the input) that
tests/test_gpu_autograd_edges.py uses as its fp64 yardstick at sizes the dense restatements of tests/test_gpu_autograd.py (masks of cells x N,
one-hot matrices of rows x n) cannot hold.  The licence for that use is at the end of this file: on inputs small enough for the dense forms, each
sparse form gives the same forward and the same gradient in fp64, exactly, planted ties included."""
import os
import re

import pytest
import torch

from garmentnets_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWD = ["gn_grid_scatter_bwd", "gn_segment_max_bwd", "gn_global_max_pool_bwd", "gn_sa_gather_bwd", "gn_knn_interpolate_bwd", "gn_trilinear_sample_bwd",
       "gn_knn_neighbours", "gn_grid_scatter_bwd_workspace_bytes", "gn_sa_gather_bwd_workspace_bytes", "gn_knn_interpolate_bwd_workspace_bytes",
       "gn_trilinear_sample_bwd_workspace_bytes"]


def test_autograd_imports_without_a_gpu():
    from garmentnets_amd import autograd as A
    for name in ("fps", "radius", "point_conv_max", "global_max_pool", "knn_interpolate", "scatter", "grid_sample_points"):
        assert callable(getattr(A, name)), name
        assert name in A.__all__


def test_inference_modules_do_not_import_autograd():
    pkg = os.path.join(REPO, "garmentnets_amd")
    for rel in ("predict.py", "validate.py", "evaluate.py", "components", "networks"):
        path = os.path.join(pkg, rel)
        files = [path] if path.endswith(".py") else [os.path.join(path, f) for f in os.listdir(path) if f.endswith(".py")]
        for f in files:
            assert "autograd" not in open(f).read().replace("torch.autograd", ""), f


def test_header_declares_every_gradient_entry():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    declared = set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in BWD:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_workspace_sizes():
    lib = _lib.load()
    assert lib.gn_grid_scatter_bwd_workspace_bytes(100, 8, 64, ops.REDUCE_CODES["sum"]) == 0
    assert lib.gn_grid_scatter_bwd_workspace_bytes(100, 8, 64, ops.REDUCE_CODES["mean"]) == 64 * 4
    assert lib.gn_grid_scatter_bwd_workspace_bytes(100, 8, 64, ops.REDUCE_CODES["max"]) == (64 + 100 + 800) * 4
    assert lib.gn_sa_gather_bwd_workspace_bytes(1000, 50) == (3 * 50 + 1 + 2 * 1000) * 4
    assert lib.gn_knn_interpolate_bwd_workspace_bytes(10, 3, 7) == (3 * 7 + 1 + 2 * 30) * 4 + 30 * 4
    assert lib.gn_trilinear_sample_bwd_workspace_bytes(2, 5, 3, 3, 3) == (3 * 54 + 1 + 2 * 80) * 4 + 80 * 8


def test_c_abi_refuses_bad_arguments_before_any_launch():
    with pytest.raises(ValueError, match="mul"):
        _lib.call("gn_grid_scatter_bwd", None, None, None, 0, None, 4, 8, 8, 16, ops.REDUCE_CODES["mul"], None, 0, None, 8, None)
    with pytest.raises(ValueError, match="bad reduce"):
        _lib.call("gn_grid_scatter_bwd", None, None, None, 0, None, 4, 8, 8, 16, 7, None, 0, None, 8, None)
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.call("gn_grid_scatter_bwd", None, None, None, 0, None, 4, 8, 8, 16, ops.REDUCE_CODES["mean"], None, 0, None, 8, None)
    with pytest.raises(ValueError, match="c_real"):
        _lib.call("gn_grid_scatter_bwd", None, None, None, 0, None, 4, 8, 9, 16, ops.REDUCE_CODES["sum"], None, 0, None, 8, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("gn_segment_max_bwd", None, 4, None, 4, None, 4, None, 3, 0, 4, None, 4, None)            # S == 0
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("gn_global_max_pool_bwd", None, 4, None, 4, None, 2, None, 1, 4, None, 4, None)           # ldi < C
    with pytest.raises(ValueError, match="workspace too small"):
        _lib.call("gn_sa_gather_bwd", None, 4, None, 10, 4, 5, None, 0, None, 4, None)
    with pytest.raises(ValueError, match="k must be"):
        _lib.call("gn_knn_neighbours", None, None, None, None, 1, 4, 0, None, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("gn_knn_interpolate_bwd", None, None, 4, 0, None, 4, 4, 4, None, 0, None, 4, None)        # k == 0
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("gn_trilinear_sample_bwd", None, 2, None, 1, 4, 4, 4, 4, None, 8, None, 0, None, None, None)   # ldg < C


def test_wrappers_refuse_mul_by_name_and_bad_shapes():
    from garmentnets_amd import autograd as A
    gv = torch.zeros(1, 8, 4)
    idx = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="'mul' has no gradient"):
        ops.grid_scatter_bwd(gv, idx, 5, "mul")
    with pytest.raises(ValueError, match="not one of"):
        ops.grid_scatter_bwd(gv, idx, 5, "prod")
    with pytest.raises(ValueError, match="needs the forward's output"):
        ops.grid_scatter_bwd(gv, idx, 5, "max")
    with pytest.raises(ValueError, match="flat_idx has"):
        ops.grid_scatter_bwd(gv, idx, 6, "sum")
    with pytest.raises(TypeError):
        ops.grid_scatter_bwd(gv.double(), idx, 5, "sum")
    with pytest.raises(TypeError):
        ops.grid_scatter_bwd(gv, idx.long(), 5, "sum")
    with pytest.raises(ValueError, match="mul"):
        A.scatter(torch.zeros(4, 5, requires_grad=True), torch.zeros(5, dtype=torch.int64), -1, 8, "mul")
    with pytest.raises(ValueError, match="src \\(C, N\\)"):
        A.scatter(torch.zeros(4, 5), torch.zeros(6, dtype=torch.int64), -1, 8, "mean")
    with pytest.raises(ValueError, match="shapes do not match"):
        ops.segment_max_bwd(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(7, 4), torch.zeros(6, dtype=torch.int32), 3, 2)
    with pytest.raises(TypeError):
        ops.segment_max_bwd(torch.zeros(3, 4).double(), torch.zeros(3, 4), torch.zeros(6, 4), torch.zeros(6, dtype=torch.int32), 3, 2)
    with pytest.raises(ValueError, match="shapes do not match"):
        ops.global_max_pool_bwd(torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(9, 4), torch.zeros(3, dtype=torch.int32), 2)
    with pytest.raises(ValueError, match="does not match"):
        ops.sa_gather_bwd(torch.zeros(6, 2), torch.zeros(6, dtype=torch.int32), 4, 10)
    with pytest.raises(ValueError, match="k must be"):
        ops.knn_neighbours(torch.zeros(4, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(2, dtype=torch.int32), 0)
    with pytest.raises(ValueError, match="do not match nbr"):
        ops.knn_interpolate_bwd(torch.zeros(3, 4), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), 9)
    with pytest.raises(ValueError, match="grad_rows must be"):
        ops.trilinear_sample_bwd(torch.zeros(2, 5, 3), torch.zeros(2, 3, 3, 3, 4), torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="query \\(B, M, 3\\)"):
        ops.trilinear_sample_bwd(torch.zeros(2, 5, 4), torch.zeros(2, 3, 3, 3, 4), torch.zeros(2, 5, 2))
    with pytest.raises(TypeError):
        A.grid_sample_points(torch.zeros(1, 4, 3, 3, 3).double(), torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="volume must be"):
        A.grid_sample_points(torch.zeros(4, 3, 3, 3), torch.zeros(1, 5, 3))


def test_cpu_tensors_are_rejected_after_the_checks():
    with pytest.raises(_lib.GarmentNetsHipError):
        ops.grid_scatter_bwd(torch.zeros(1, 8, 4), torch.zeros(5, dtype=torch.int32), 5, "sum")


# ------------------------------------------------------------------------------------------------ sparse restatements (plain torch, any dtype, CPU)
def s_first_max(v, key, nkeys, valid=None):
    """v (E, C), key (E,) int64: the destination of every element -> bool (E, C), True where the element is the FIRST maximum of its destination
    among `valid` elements.  Written out, no argmax: the maximum per (destination, channel) by scatter_reduce('amax'), then the minimum element
    index among the elements equal to it by scatter_reduce('amin')."""
    E, C = v.shape
    v = v.detach()
    if valid is not None:
        v = torch.where(valid[:, None], v, torch.full_like(v, -float("inf")))
    kx = key[:, None].expand(E, C)
    top = torch.full((nkeys, C), -float("inf"), dtype=v.dtype).scatter_reduce(0, kx, v, "amax", include_self=True)
    eq = v == top.gather(0, kx)
    if valid is not None:
        eq &= valid[:, None]
    idx = torch.arange(E)[:, None].expand(E, C)
    first = torch.full((nkeys, C), E, dtype=torch.int64).scatter_reduce(0, kx, torch.where(eq, idx, E), "amin", include_self=True)
    return idx == first.gather(0, kx)


def _s_select(src, sel, key, nkeys):
    return torch.zeros((nkeys, src.shape[1]), dtype=src.dtype).index_add_(0, key, src * sel.to(src.dtype))


def s_scatter(src, cell, cells, reduce):
    """src (N, C), cell (N,) int64 -> (cells, C)"""
    if reduce in ("max", "min"):
        return _s_select(src, s_first_max(src if reduce == "max" else -src, cell, cells), cell, cells)
    tot = torch.zeros((cells, src.shape[1]), dtype=src.dtype).index_add_(0, cell, src)
    if reduce == "mean":
        tot = tot / torch.bincount(cell, minlength=cells).clamp(min=1).to(src.dtype)[:, None]
    return tot


def s_segment_max(h, slot_src, M, S):
    key = torch.arange(M * S) // S
    return _s_select(h, s_first_max(h, key, M, slot_src >= 0), key, M)


def s_global_max(h, sizes):
    key = torch.repeat_interleave(torch.arange(len(sizes)), torch.as_tensor(sizes, dtype=torch.int64))
    return _s_select(h, s_first_max(h, key, len(sizes)), key, len(sizes))


def s_sa_gather(x, pos, centre_idx, slot_src, S):
    """edge rows [x_j, pos_j - pos_i]; an empty slot is a zero row.  x by row indexing (its gradient is an index_add_), positions are data"""
    valid = (slot_src >= 0)[:, None].to(pos.dtype)
    j = slot_src.clamp(min=0).long()
    ci = centre_idx.long()[torch.arange(slot_src.numel()) // S]
    rel = (pos[j] - pos[ci]) * valid
    return torch.cat((x[j] * valid.to(x.dtype), rel), 1) if x is not None else rel


def s_knn(x, nbr, d2):
    """nbr / d2 (Nq, k) shared data: the k weighted rows gathered and summed per query (no gradient through the weights)"""
    valid = nbr >= 0
    w = valid.to(x.dtype) / d2.to(x.dtype).clamp(min=1e-16)
    coef = w / w.sum(1, keepdim=True)
    return (coef[:, :, None] * x[nbr.clamp(min=0).long()]).sum(1)


# the sampler's restatement is F.grid_sample itself, linear in its input already: tests/test_gpu_autograd.py::r_sample serves both roles.


# ------------------------------------------------------------------------------------------------ sparse == dense, forward and gradient, in fp64
# Inputs are multiples of 2^-6 below 2^6 in magnitude and every weight is a power of two, so each sum and product of either form is exact in
# fp64: the equalities below cannot depend on the order in which a GEMM or an index_add_ happens to add, and "equal" means equal bits.
def _quant(shape, seed):
    return torch.randint(-2 ** 12, 2 ** 12, shape, generator=torch.Generator().manual_seed(seed)).double() / 64


def _both(dense, sparse, x, gout):
    outs = []
    for fn in (dense, sparse):
        leaf = x.clone().requires_grad_(True)
        out = fn(leaf)
        outs.append((out.detach(), torch.autograd.grad(out, [leaf], gout)[0]))
    (fd, gd), (fs, gs) = outs
    assert fd.dtype == torch.float64 and fd.shape == fs.shape
    assert torch.equal(fd, fs) and torch.equal(gd, gs)
    assert float(gd.abs().max()) > 0
    return fd, gd


@pytest.mark.parametrize("reduce", ["max", "min", "mean", "sum"])
def test_sparse_scatter_equals_dense(reduce):
    from test_gpu_autograd import r_scatter
    n, c, cells = 500, 7, 40
    src = _quant((n, c), 1)
    cell = torch.randint(0, cells, (n,), generator=torch.Generator().manual_seed(2))
    cell[cell == 5] = 6                                        # an empty cell
    src[300:400] = src[100:200]                                # planted ties: equal rows ...
    cell[300:400] = cell[100:200]                              # ... in equal cells
    cell[-30:] = 9
    src[-30:, 0], src[-30:, 1] = 64.0, -64.0                   # thirty points of one cell hold its maximum / minimum
    gout = _quant((cells, c), 3)
    _, g = _both(lambda s: r_scatter(s, cell, cells, reduce), lambda s: s_scatter(s, cell, cells, reduce), src, gout)
    if reduce in ("max", "min"):
        ch = 0 if reduce == "max" else 1
        assert float(g[n - 30, ch]) == float(gout[9, ch]) and float(g[n - 29:, ch].abs().max()) == 0.0


def test_sparse_segment_max_equals_dense():
    from test_gpu_autograd import r_segment_max
    M, S, C = 23, 7, 11
    h = torch.relu(_quant((M * S, C), 4))
    h[1::S] = h[0::S]                                          # slot 1 repeats slot 0
    slot = torch.randint(-1, 30, (M * S,), generator=torch.Generator().manual_seed(5)).to(torch.int32)
    slot[3 * S:4 * S] = -1                                     # a centre without a valid slot
    slot[5 * S] = -1                                           # the first of two tied slots is empty: the second one wins
    gout = _quant((M, C), 6)
    _, g = _both(lambda t: r_segment_max(t, slot, M, S), lambda t: s_segment_max(t, slot, M, S), h, gout)
    assert float(g[3 * S:4 * S].abs().max()) == 0.0 and float(g[5 * S].abs().max()) == 0.0


def test_sparse_global_max_equals_dense():
    from test_gpu_autograd import r_global_max
    sizes, C = [40, 1, 0, 17, 16], 9
    h = torch.relu(_quant((sum(sizes), C), 7))
    h[0] = h[33] = h[:40].max(0).values                        # rows 0 and 33 both hold every channel's maximum
    gout = _quant((len(sizes), C), 8)
    _, g = _both(lambda t: r_global_max(t, sizes), lambda t: s_global_max(t, sizes), h, gout)
    assert torch.equal(g[0], gout[0]) and float(g[33].abs().max()) == 0.0


def test_sparse_sa_gather_equals_dense():
    from test_gpu_autograd import r_sa_gather
    n, Mc, S, C = 60, 25, 6, 5
    g = torch.Generator().manual_seed(9)
    slot = torch.randint(-1, n, (Mc * S,), generator=g).to(torch.int32)
    slot[:S] = 7                                               # one point in every slot of a centre
    slot[S::S] = 11                                            # ... and one point in every centre
    centre = torch.randint(0, n, (Mc,), generator=g)
    pos, x = _quant((n, 3), 10), _quant((n, C), 11)
    gout = _quant((Mc * S, C + 3), 12)
    _both(lambda t: r_sa_gather(t, pos, centre, slot, S), lambda t: s_sa_gather(t, pos, centre, slot, S), x, gout)
    assert torch.equal(r_sa_gather(None, pos, centre, slot, S), s_sa_gather(None, pos, centre, slot, S))


def test_sparse_knn_equals_dense():
    from test_gpu_autograd import r_knn
    ns, C = 30, 6
    # weights 1 / d2 that are powers of two with a power-of-two sum: (1), (1/2, 1/2), (1/4, 1/4, 1/2), (1/4 x 4) and a row with invalid slots
    pat = torch.tensor([[1.0, 0, 0, 0], [2.0, 2.0, 0, 0], [4.0, 4.0, 2.0, 0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0, 0]], dtype=torch.float32)
    use = torch.tensor([[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 0]], dtype=torch.bool)   # the last row: d2 = 0 twice, both clamped: 1/2, 1/2
    g = torch.Generator().manual_seed(13)
    rows = torch.arange(100) % 5
    d2 = pat[rows]
    others = torch.tensor([j for j in range(ns) if j != 3])
    nbr = torch.stack([torch.cat((torch.tensor([3]), others[torch.randperm(ns - 1, generator=g)[:3]])) for _ in range(100)]).to(torch.int32)
    # (source 3 is every query's first neighbour: a hot destination; the other three are distinct)
    nbr = torch.where(use[rows], nbr, torch.full_like(nbr, -1))
    d2 = torch.where(use[rows], d2, torch.zeros_like(d2))
    for r in range(100):
        v = nbr[r][nbr[r] >= 0].tolist()
        assert len(set(v)) == len(v)
    x, gout = _quant((ns, C), 14), _quant((100, C), 15)
    _both(lambda t: r_knn(t, nbr, d2, ns), lambda t: s_knn(t, nbr, d2), x, gout)

"""CPU: the operator gradients' host side -- argument checks raised before any launch, header / prototypes in step, imports without a GPU."""
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

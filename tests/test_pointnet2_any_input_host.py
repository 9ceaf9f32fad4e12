"""CPU: host side of PointNet++ / gridding at any cloud size, kNN k and reduction -- argument checks, workspace sizing, reduction names and the
channel-padded bookkeeping of the volume aggregator (no GPU: everything here is decided before a launch)."""
import pytest
import torch

from garmentnets_amd import _lib, ops
from garmentnets_amd.components import unet3d as U
from garmentnets_amd.networks.conv_implicit_wnf import VolumeFeatureAggregator, agg_stored_channels


def test_fps_workspace_bytes():
    lib = _lib.load()
    assert lib.gn_fps_workspace_bytes(4, 36864) == 0            # the LDS-resident kernels need none
    assert lib.gn_fps_workspace_bytes(4, 6000) == 0
    assert lib.gn_fps_workspace_bytes(3, 36865) == 3 * 36865 * 16   # one (x, y, z, d) record per point
    assert lib.gn_fps_workspace_bytes(0, 100000) == 0


def test_fps_past_the_limit_needs_a_workspace():
    with pytest.raises(ValueError, match="workspace"):
        _lib.call("gn_fps_nested", None, None, None, None, 1, 40000, None, None, None, None)
    with pytest.raises(ValueError, match="gn_fps_workspace_bytes"):
        _lib.call("gn_fps_nested_ws", None, None, None, None, 1, 40000, None, None, None, None, 0, None)
    with pytest.raises(ValueError, match="gn_fps_workspace_bytes"):
        _lib.call("gn_fps_nested_ws", None, None, None, None, 2, 40000, None, None, None, None, 16 * 40000, None)


def test_knn_any_k_argument_checks():
    with pytest.raises(ValueError, match="k must be"):
        _lib.call("gn_knn_interpolate_any", None, 4, None, None, None, None, 1, 1, 4, 0, None, 4, None)
    with pytest.raises(ValueError, match="bad sizes"):
        _lib.call("gn_knn_interpolate_any", None, 4, None, None, None, None, 1, 1, 0, 33, None, 4, None)


def test_scatter_workspace_bytes_per_reduction():
    lib = _lib.load()
    N, C = 1000, 40
    fp64 = N * C * 8 + 2 * N * 4
    assert lib.gn_grid_scatter_workspace_bytes(N, C, ops.REDUCE_CODES["max"]) == 0
    assert lib.gn_grid_scatter_workspace_bytes(N, C, ops.REDUCE_CODES["min"]) == 0
    assert lib.gn_grid_scatter_workspace_bytes(N, C, ops.REDUCE_CODES["mean"]) == fp64
    assert lib.gn_grid_scatter_workspace_bytes(N, C, ops.REDUCE_CODES["sum"]) == fp64
    assert lib.gn_grid_scatter_workspace_bytes(N, C, ops.REDUCE_CODES["mul"]) == (6 * N + 1) * 4
    with pytest.raises(ValueError, match="bad arguments"):
        _lib.call("gn_grid_scatter_ex", None, C, None, N, C, C, 8, 5, None, None, None, 0, 0, None)
    with pytest.raises(ValueError, match="c_real"):
        _lib.call("gn_grid_scatter_ex", None, C, None, N, C, C + 1, 8, 0, None, None, None, 0, 0, None)


def test_reduction_names():
    assert set(ops.REDUCE_CODES) == {"max", "mean", "sum", "add", "min", "mul"}
    assert ops.REDUCE_CODES["sum"] == ops.REDUCE_CODES["add"]
    for r in ops.REDUCE_CODES:
        assert VolumeFeatureAggregator(nn_channels=[9, 16], reduce_method=r).reduce_method == r
    with pytest.raises(ValueError, match="reduce_method='prod'"):
        VolumeFeatureAggregator(nn_channels=[9, 16], reduce_method="prod")
    src = torch.zeros(4, 16)
    with pytest.raises(ValueError, match="not one of"):
        ops.grid_scatter(src, torch.zeros(4, dtype=torch.int32), 1, (2, 2, 2), "prod")
    with pytest.raises(ValueError, match="mul"):
        ops.grid_scatter(src, torch.zeros(4, dtype=torch.int32), 1, (2, 2, 2), "mul", with_stats=True)


def test_aggregator_stored_width():
    assert [agg_stored_channels(c) for c in (128, 48, 16, 100, 40, 7, 137)] == [128, 48, 16, 128, 64, 32, 160]
    # the UNet takes the padded storage of any width, and refuses an unpadded input it cannot read by name
    net = U.Abstract3DUNet(in_channels=100, out_channels=8, f_maps=32, num_groups=4, num_levels=2)
    net.check_input(torch.empty(1, 8, 8, 8, agg_stored_channels(100)))
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        net.check_input(torch.empty(1, 8, 8, 8, 100))
    lay = net.encoders[0].basic_module.SingleConv1._layout(torch.empty(1, 1, 1, 1, 128), None)
    assert lay == ((100,), (128,), 128)

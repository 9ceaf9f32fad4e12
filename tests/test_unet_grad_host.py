"""Host-side checks of the UNet gradients (csrc/unet_grad.hip, garmentnets_amd/autograd.py): no GPU needed -- run with `-m "not gpu"`."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from garmentnets_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gn_conv3d_bwd_weight", "gn_conv3d_bwd_weight_workspace_bytes", "gn_relu_mask", "gn_groupnorm_bwd_stats", "gn_groupnorm_bwd_stats_workspace_bytes",
           "gn_groupnorm_bwd_coef", "gn_groupnorm_bwd_apply", "gn_maxpool3d_2_bwd"]


def test_header_declares_every_unet_gradient_entry():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    declared = set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_no_float_atomics_in_the_source():
    src = open(os.path.join(REPO, "garmentnets_amd", "csrc", "unet_grad.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic", code, re.I)


def test_workspace_sizes():
    lib = _lib.load()
    # chains x 27 x round_up(Cin, 32) x Cout floats: tiles = B * ceil(D/4) * ceil(H/8) * ceil(W/8), blocks = ceil(Cin/32) * Cout / (64 or 32),
    # chains = ceil(tiles / ceil(tiles / min(tiles, ceil(512 / blocks))))
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(2, 16, 16, 16, 32, 64) == 32 * 27 * 32 * 64 * 4          # 32 tiles, 1 block: a chain per tile
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(2, 128, 128, 128, 128, 128) == 64 * 27 * 128 * 128 * 4   # 16384 tiles, 8 blocks: 64 chains of 256
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(1, 8, 8, 8, 16, 32) == 2 * 27 * 32 * 32 * 4              # Cin 16 rounds up to one 32-slice
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(3, 12, 8, 8, 96, 96) == 9 * 27 * 96 * 96 * 4             # 9 tiles, 9 blocks (32-wide columns)
    # 15 tiles (5 per sample), 48 blocks: 8 chains of 2 -- chain 2 spans samples 0 / 1, chain 7 holds one tile (the GPU suite's direct weight-gradient case)
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(3, 4, 8, 40, 384, 256) == 8 * 27 * 384 * 256 * 4
    assert lib.gn_conv3d_bwd_weight_workspace_bytes(1, 8, 8, 8, 16, 48) == 0                                 # refused shape
    assert lib.gn_groupnorm_bwd_stats_workspace_bytes(2, 4096, 64) == 2 * 8 * 2 * 64 * 8
    assert lib.gn_groupnorm_bwd_stats_workspace_bytes(3, 513, 32) == 3 * 2 * 2 * 32 * 8


def test_c_abi_refuses_bad_arguments_before_any_launch():
    c = _lib.call
    with pytest.raises(ValueError, match="multiple of 32"):
        c("gn_conv3d_bwd_weight", None, 16, None, 0, None, None, None, None, 1, 8, 8, 8, 48, None, 0, None, None)
    with pytest.raises(ValueError, match="multiples of 4"):
        c("gn_conv3d_bwd_weight", None, 6, None, 0, None, None, None, None, 1, 8, 8, 8, 32, None, 0, None, None)
    with pytest.raises(ValueError, match="even dims"):
        c("gn_conv3d_bwd_weight", None, 16, None, 16, None, None, None, None, 1, 8, 7, 8, 32, None, 0, None, None)
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_conv3d_bwd_weight", None, 16, None, 0, None, None, None, None, 1, 8, 8, 8, 32, None, 0, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_conv3d_bwd_weight", None, 16, None, 0, None, None, None, None, 1, 8, 8, 8, 32, None, 1 << 30, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_relu_mask", None, None, 6, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_relu_mask", None, None, 8, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_groupnorm_bwd_stats", None, 32, 0, None, 1, 4, 4, 4, 30, 0, None, 0, None, None, None)          # C % 4
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_groupnorm_bwd_stats", None, 32, 16, None, 1, 4, 4, 4, 32, 0, None, 0, None, None, None)         # ldg < goff + C
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_groupnorm_bwd_stats", None, 32, 0, None, 1, 4, 4, 4, 32, 0, None, 0, None, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_groupnorm_bwd_coef", None, None, None, None, 30, 32, 64, None, None, None, None, 0, 0, 0, 1, 1, 8, 1e-5, None, None, None, None, None, None,
          None)                                                                                              # 30 channels in 8 groups
    with pytest.raises(ValueError, match="same voxels"):
        c("gn_groupnorm_bwd_coef", None, None, None, None, 32, 32, 64, None, None, None, None, 32, 32, 9, 8, 1, 8, 1e-5, None, None, None, None, None, None,
          None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_groupnorm_bwd_coef", None, None, None, None, 32, 32, 64, None, None, None, None, 0, 0, 0, 1, 1, 8, 1e-5, None, None, None, None, None, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_groupnorm_bwd_apply", None, 32, 0, None, 1, 4, 4, 4, 32, 0, None, None, None, 32, 8, 0, None, None)   # cs < coff + C
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_groupnorm_bwd_apply", None, 32, 0, None, 1, 4, 4, 4, 32, 0, None, None, None, 32, 0, 0, None, None)
    with pytest.raises(ValueError, match="even dims"):
        c("gn_maxpool3d_2_bwd", None, None, 1, 4, 5, 4, 32, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_maxpool3d_2_bwd", None, None, 1, 4, 4, 4, 30, None, None)


@pytest.mark.parametrize("cin,cout", [(32, 64), (16, 32), (48, 32), (96, 160)])
def test_pack_conv_weight_bwd_data_is_the_transposed_convolution(cin, cout):
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g, dtype=torch.float64)
    pack = ops.pack_conv_weight_bwd_data(w.float())
    cin_p = -(-cin // 32) * 32
    assert pack.dtype == torch.float32 and tuple(pack.shape) == (27, cout // 16, cin_p, 16)
    # the documented forward pack layout [27 taps][in/16][out][16], in = Cout and out = Cin (padded) here -> an nn.Conv3d weight (out, in, 3, 3, 3)
    wt = pack.permute(2, 1, 3, 0).reshape(cin_p, cout, 3, 3, 3)
    assert torch.equal(wt[cin:], torch.zeros_like(wt[cin:]))                   # the extra output columns are zero rows
    w32 = w.float().double()                                                   # (the pack holds the fp32 weight)
    x = torch.randn((2, cin, 5, 6, 7), generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn((2, cout, 5, 6, 7), generator=g, dtype=torch.float64)
    (ref,) = torch.autograd.grad(F.conv3d(x, w32, padding=1), x, gy)
    got = F.conv3d(gy, wt.double(), padding=1)[:, :cin]
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_autograd_imports_without_a_gpu_and_refuses_other_layer_orders_by_name():
    from garmentnets_amd import autograd as A
    from garmentnets_amd.components.unet3d import Abstract3DUNet, SingleConv
    for name in ("conv3d_gcr", "max_pool3d_2", "unet3d"):
        assert callable(getattr(A, name)), name
        assert name in A.__all__
    model = Abstract3DUNet(16, 4, f_maps=(32, 64), layer_order="cr", num_groups=8)
    with pytest.raises(NotImplementedError, match="'cr'"):
        A.unet3d(model, torch.zeros(1, 16, 8, 8, 8, requires_grad=True))
    with pytest.raises(NotImplementedError, match="'crg'"):
        A.conv3d_gcr(SingleConv(16, 32, order="crg"), torch.zeros(1, 8, 8, 8, 16))

"""CPU: argument checks of the any-width GroupNorm entries and the UNet's channel-padding plan (no GPU needed)."""
import pytest
import torch

from garmentnets_amd import _lib
from garmentnets_amd.components import unet3d as U


def test_new_groupnorm_entries_refuse_bad_arguments():
    # more channels than the workgroup's LDS holds (16 B per channel + 8 B per group, 160 KB)
    with pytest.raises(ValueError):
        _lib.call("gn_groupnorm_affine_map", None, None, 12000, 12000, 64, None, None, 0, 0, 0, 1, 1, 8, 1e-5, None, None, None, None, None, None)
    assert "LDS" in _lib.load().gn_last_error().decode()
    with pytest.raises(ValueError):      # stored stride below the real channel count
        _lib.call("gn_groupnorm_affine_map", None, None, 48, 32, 64, None, None, 0, 0, 0, 1, 1, 8, 1e-5, None, None, None, None, None, None)
    with pytest.raises(ValueError):      # groups do not divide the real channels
        _lib.call("gn_groupnorm_affine_map", None, None, 20, 32, 64, None, None, 0, 0, 0, 1, 1, 8, 1e-5, None, None, None, None, None, None)
    with pytest.raises(ValueError):      # source 1 must cover the same voxels after replication
        _lib.call("gn_groupnorm_affine_map", None, None, 32, 32, 64, None, None, 16, 32, 16, 8, 1, 8, 1e-5, None, None, None, None, None, None)
    with pytest.raises(ValueError):
        _lib.call("gn_channel_stats_any", None, 1, 64, 6, None, None, None)
    # the narrow entries keep their limits
    with pytest.raises(ValueError):
        _lib.call("gn_groupnorm_affine", None, None, 1024, 64, None, None, 512, 8, 8, 1, 8, 1e-5, None, None, None, None, None, None)
    with pytest.raises(ValueError):
        _lib.call("gn_channel_stats", None, 1, 64, 96, None, None, None)


def test_unet_refuses_what_stays_out_of_scope():
    net = U.Abstract3DUNet(in_channels=24, out_channels=8, f_maps=32, num_levels=2)
    with pytest.raises(NotImplementedError, match="multiple of 16"):
        net.run(torch.zeros(1, 8, 8, 8, 24))
    net = U.Abstract3DUNet(in_channels=32, out_channels=8, f_maps=16, num_levels=4)
    with pytest.raises(NotImplementedError, match="halve evenly"):
        net.run(torch.zeros(1, 12, 16, 16, 32))


def _layouts(net, G, in_channels):
    """(real, stored, cout) of every SingleConv call of a forward pass, from the shapes alone"""
    out, x, feats = [], G, []
    c = in_channels

    def lay(conv, s0, s1=None):
        src0 = torch.empty(1, 1, 1, 1, s0)
        src1 = None if s1 is None else torch.empty(1, 1, 1, 1, s1)
        r = conv._layout(src0, src1)
        out.append(r)
        return U.stored_channels(conv.conv.out_channels)
    for enc in net.encoders:
        c = lay(enc.basic_module.SingleConv1, c)
        c = lay(enc.basic_module.SingleConv2, c)
        feats.insert(0, c)
    for dec, skip in zip(net.decoders, feats[1:]):
        c = lay(dec.basic_module.SingleConv1, skip, c)
        c = lay(dec.basic_module.SingleConv2, c)
    return out


def test_shipped_widths_take_the_unpadded_path():
    """every layer of the shipped UNet (and of other multiple-of-32 widths) runs exactly the unpadded code"""
    for f_maps, levels in ((32, 4), (64, 5), (128, 4), (32, 6)):
        net = U.Abstract3DUNet(in_channels=128, out_channels=128, f_maps=f_maps, num_levels=levels)
        assert all(r is None for r in _layouts(net, 32, 128))
        assert torch.equal(net.final_conv.stored_weight(), net.final_conv.weight.detach().reshape(128, f_maps))


def test_padded_layout_and_weights():
    net = U.Abstract3DUNet(in_channels=16, out_channels=8, f_maps=[24, 48, 96], num_levels=3)
    lays = _layouts(net, 16, 16)
    # encoders.0: 16 -> 24 (stored 32) -> 24; encoders.1: 24 -> 24 -> 48 (64); encoders.2: 48 -> 48 -> 96; decoders.0: (48 | 96) -> 48 ...
    assert lays[0] == ((16,), (16,), 32)
    assert lays[2] == ((24,), (32,), 32) and lays[3] == ((24,), (32,), 64)
    assert lays[6] == ((48, 96), (64, 96), 64)
    conv = net.decoders[0].basic_module.SingleConv1
    wp = conv._padded_weight(lays[6])
    w = conv.conv.weight.detach()
    assert wp.shape == (64, 160, 3, 3, 3)
    assert torch.equal(wp[:48, :48], w[:, :48]) and torch.equal(wp[:48, 64:160], w[:, 48:])
    assert int(torch.count_nonzero(wp[48:])) == 0 and int(torch.count_nonzero(wp[:, 48:64])) == 0
    fw = net.final_conv.stored_weight()
    assert fw.shape == (8, 32) and torch.equal(fw[:, :24], net.final_conv.weight.detach().reshape(8, 24)) and int(torch.count_nonzero(fw[:, 24:])) == 0

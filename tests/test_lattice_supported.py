"""ops.lattice_split_supported: which volumes, decoder packs and lattices the lattice form of the split-operand decoder takes (no GPU needed)."""
import torch

from garmentnets_amd import arith as AR, ops


def _pack(out_channels=1, hidden=256):
    return ops.DecodeSplitPack(torch.zeros(1, dtype=torch.int16), torch.zeros(1), 1.0, out_channels, hidden)


def test_lattice_split_supported_with_and_without_the_lattice_size():
    vol = torch.zeros(8, 12, 16, 32)
    assert ops.lattice_split_supported(vol, _pack())                    # the volume and the pack alone
    assert ops.lattice_split_supported(vol, _pack(), 16)                # Q equals the largest axis
    assert ops.lattice_split_supported(vol, _pack(), 128)
    assert not ops.lattice_split_supported(vol, _pack(), 15)            # coarser than the volume along one axis: the sampler + decoder pair
    assert not ops.lattice_split_supported(vol, _pack(), 12)
    assert not ops.lattice_split_supported(vol, _pack(), 2048)          # beyond the lattice sizes the kernels index
    assert not ops.lattice_split_supported(torch.zeros(8, 8, 8, 128), _pack(), 16)       # the unfolded 128-channel volume
    assert not ops.lattice_split_supported(vol, _pack(out_channels=3), 16)
    assert not ops.lattice_split_supported(vol, _pack(hidden=512), 16)
    assert not ops.lattice_split_supported(vol.permute(1, 0, 2, 3), _pack(), 16)         # not contiguous


def test_fused_lattice_is_the_default_and_can_be_turned_off():
    assert AR.Arith().fused_lattice is True
    assert AR.Arith().replace(fused_lattice=False).fused_lattice is False

"""GPU (-m gpu): the lattice form of the split-operand decoder (csrc/decode_split.hip, LAT: bricks of 4 x 8 x 8 lattice points sampled out of an
LDS voxel box inside the decoder kernel) against the two-kernel path it replaces by default (gn_trilinear_sample + gn_implicit_decode_split),
through ImplicitWNFDecoder._decode_rows with Arith.fused_lattice on and off: bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import arith as AR, ops  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import DecoderPack, ImplicitWNFDecoder  # noqa: E402

DEV = "cuda:0"
FUSED, PAIR = AR.DEFAULT.replace(decode_mode="f16x2", fused_lattice=True), AR.DEFAULT.replace(decode_mode="f16x2", fused_lattice=False)


@pytest.fixture(scope="module")
def decoder():
    """a folded [32, 256, 256, 1] decoder: its fp32 layers and its split-operand pack, as ImplicitWNFDecoder.folded_pack lays them out"""
    g = torch.Generator().manual_seed(7)
    raw = []
    for i, (n, k) in enumerate(((256, 32), (256, 256), (1, 256))):
        raw.append((torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5, torch.randn(n, generator=g) * 0.1,
                    (torch.rand(n, generator=g) + 0.5) if i < 2 else None, torch.randn(n, generator=g) * 0.1 if i < 2 else None))
    dev = lambda v: None if v is None else v.contiguous().to(DEV)
    layers = tuple((dev(ops.pack_kpair(w) if i < 2 else w), dev(b), dev(sc), dev(sh), w.shape[0]) for i, (w, b, sc, sh) in enumerate(raw))
    return ImplicitWNFDecoder((32, 256, 256, 1)), DecoderPack(layers, ops.pack_decode_split(raw).to(DEV), 32)


def _volume(dims, seed):
    return (torch.randn(*dims, 32, generator=torch.Generator().manual_seed(seed)) * 1.5).to(DEV)


def _scale(vol, pack):
    D, H, W, C = vol.shape
    return ops.decoder_input_scale((vol.double() ** 2).sum(dim=(0, 1, 2)).view(1, C), D * H * W, pack.smax)[0]


def _decode(decoder, vol, Q, arith, xscale):
    dec, layers = decoder
    out = torch.full((Q * Q * Q, 1), float("nan"), device=DEV)
    dec._decode_rows(dec._plan(arith, vol[None], layers, Q, Q * Q * Q), vol, out, layers, Q=Q, xscale=xscale)
    return out


# 8^3 / 8: the smallest Q == G, every brick touches a face; 8^3 / 16: spacing 1/2; 12^3 / 18: ragged bricks on all axes; 8 x 12 x 16 / 16: non-cubic,
# Q equals only the largest axis; 16^3 / 12: Q < G -- the lattice form does not apply, the call must fall back to the pair and still match
@pytest.mark.parametrize("dims,Q", [((8, 8, 8), 8), ((8, 8, 8), 16), ((12, 12, 12), 18), ((8, 12, 16), 16), ((16, 16, 16), 12)])
def test_fused_lattice_equals_sampler_plus_decoder(decoder, dims, Q):
    vol = _volume(dims, Q + dims[2])
    assert ops.lattice_split_supported(vol, decoder[1].split, Q) == (Q >= max(dims))
    for xs in (None, _scale(vol, decoder[1].split)):
        want = _decode(decoder, vol, Q, PAIR, xs)
        got = _decode(decoder, vol, Q, FUSED, xs)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), (dims, Q, xs is not None)


def test_fused_lattice_propagates_nan_and_inf_voxels_like_the_pair(decoder):
    vol = _volume((8, 8, 8), 3)
    xs = _scale(vol, decoder[1].split)
    vol[2, 3, 4, 5] = float("nan")
    vol[5, 1, 6, 0] = float("inf")
    want = _decode(decoder, vol, 16, PAIR, xs)
    got = _decode(decoder, vol, 16, FUSED, xs)
    assert torch.isnan(want).any() and torch.isfinite(want).any()
    assert torch.allclose(got, want, rtol=0.0, atol=0.0, equal_nan=True)
    assert torch.equal(torch.isnan(got), torch.isnan(want))


def test_fused_lattice_per_garment_scale_and_unsafe_garment(decoder):
    """two garments, each with its own input scale; the second is flagged unsafe: the lattice kernel leaves it alone and the gated fp32 kernel
    computes its rows"""
    dec, layers = decoder
    Q = 16
    vols = [_volume((8, 8, 8), 11), _volume((8, 8, 8), 12) * 0.01]
    xs = [_scale(v, layers.split) for v in vols]
    assert float(xs[0][0]) != float(xs[1][0]) and float(xs[0][2]) == 0.0
    xs[1] = xs[1].clone()
    xs[1][2] = 1.0
    for b in range(2):
        want = _decode(decoder, vols[b], Q, PAIR, xs[b])
        got = _decode(decoder, vols[b], Q, FUSED, xs[b])
        assert torch.equal(got, want), b
    fp32 = ops.implicit_decode(vols[1], layers.fp32, Q=Q, m0=0, M=Q * Q * Q)
    assert torch.equal(got, fp32)


def test_fused_lattice_repeats_bit_for_bit(decoder):
    vol = _volume((12, 12, 12), 5)
    xs = _scale(vol, decoder[1].split)
    first = _decode(decoder, vol, 18, FUSED, xs)
    assert torch.equal(_decode(decoder, vol, 18, FUSED, xs), first)

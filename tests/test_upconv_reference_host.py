"""CPU: the restatements of tests/upconv_reference.py are what they claim to be -- the literal definition of the polyphase partial equals the
2x2x2-tap formulation behind ops.polyphase_weights, the deliberately wrong padding differs from it at the border and nowhere else, and the case table
puts every kind of grid the XCD remap of gn_upconv_partial tells apart in front of each kernel template."""
import torch
import torch.nn.functional as F

import upconv_reference as R
from garmentnets_amd import ops
from test_gpu_conv_variants import _upsampled_partial


def _small(dims, C1, Cout, B, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(B, *dims, C1, generator=g, dtype=torch.float64) * 1.5 + 0.2
    w = torch.randn(Cout, R.C0 + C1, 3, 3, 3, generator=g, dtype=torch.float64) / (27 * C1) ** 0.5
    a1, d1 = R.affine_reference(x1, torch.rand(C1, generator=g) + 0.5, torch.randn(C1, generator=g) + 1.0, groups=1)
    return x1, a1, d1, w


def test_deinterleave_round_trip():
    """R.deinterleave is the inverse of the layout the conv epilogues read (_upsampled_partial of test_gpu_conv_variants.py)"""
    B, (Dc, Hc, Wc), Cout = 2, (3, 5, 2), 4
    fine = torch.arange(B * 8 * Dc * Hc * Wc * Cout, dtype=torch.float64).reshape(B, 2 * Dc, 2 * Hc, 2 * Wc, Cout)
    part = R.deinterleave(fine).contiguous()
    assert part.shape == (B, Dc, Hc, Wc, 8 * Cout)
    assert torch.equal(_upsampled_partial(part, (2 * Dc, 2 * Hc, 2 * Wc)), fine)
    # entry (4 pz + 2 py + px) * Cout + n of coarse voxel (i, j, k) is fine voxel (2i + pz, 2j + py, 2k + px)
    for (i, j, k, pz, py, px, n) in ((0, 0, 0, 0, 0, 0, 0), (2, 4, 1, 1, 0, 1, 3), (1, 3, 0, 0, 1, 1, 2)):
        assert part[1, i, j, k, (4 * pz + 2 * py + px) * Cout + n] == fine[1, 2 * i + pz, 2 * j + py, 2 * k + px, n]


def test_definition_equals_the_two_tap_formulation():
    """partial_reference == conv3d(g_coarse, polyphase_weights(w, c0)[1], padding=1) reshaped as test_polyphase_weights_algebra does, at an odd,
    non-cubic coarse shape with d1 != 0: to 1e-5 * max|ref| (wm is stored in fp32)"""
    dims, C1, Cout, B = (3, 5, 2), 5, 32, 2
    x1, a1, d1, w = _small(dims, C1, Cout, B, 3)
    assert float(d1.abs().min()) > 1e-3
    ref = R.partial_reference(x1, a1, d1, w[:, R.C0:])
    wm = ops.polyphase_weights(w, R.C0)[1]
    g = (x1 * a1[:, None, None, None, :] + d1[:, None, None, None, :]).permute(0, 4, 1, 2, 3)
    part = F.conv3d(g, wm.double(), None, padding=1)                    # (B, 8 * Cout, Dc, Hc, Wc), channel (class, n)
    got = part.permute(0, 2, 3, 4, 1)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # and interleaved back it is the literal fine convolution
    fine = F.conv3d(F.interpolate(g, scale_factor=2, mode="nearest"), w[:, R.C0:], None, padding=1).permute(0, 2, 3, 4, 1)
    assert torch.equal(_upsampled_partial(ref.contiguous(), tuple(2 * n for n in dims)), fine)


def test_padding_before_affine_has_teeth():
    """with the module's d1 the wrong padding differs from the definition by more than 1e-2 at border voxels and is exactly equal away from every face"""
    case = ((5, 6, 5), 16, 32, 2)
    inp = R.make_inputs(case)
    a1, d1 = R.affine_reference(inp["x1"], inp["gamma"], inp["beta"])
    assert float(d1.abs().max()) > 0.5
    ref = R.partial_reference(inp["x1"], a1, d1, inp["w1"])
    bad = R.padding_before_affine(inp["x1"], a1, d1, inp["w1"])
    diff = (bad - ref).abs()
    inner = diff[:, 2:-2, 2:-2, 2:-2]                                    # coarse voxels two or more away from every face ...
    assert inner.numel() > 0 and float(inner.max()) == 0.0
    assert torch.equal(bad[:, 1:-1, 1:-1, 1:-1], ref[:, 1:-1, 1:-1, 1:-1])  # ... and already one away: no fine voxel of theirs sees the pad
    for face in (diff[:, 0], diff[:, -1], diff[:, :, 0], diff[:, :, -1], diff[:, :, :, 0], diff[:, :, :, -1]):
        assert float(face.max()) > 1e-2
    # every case of the table has a border: the (3, 9, 5) ones are where the GPU module looks
    inp = R.make_inputs(R.CASES[4])
    a1, d1 = R.affine_reference(inp["x1"], inp["gamma"], inp["beta"])
    assert float((R.padding_before_affine(inp["x1"], a1, d1, inp["w1"]) - R.partial_reference(inp["x1"], a1, d1, inp["w1"])).abs().max()) > 1e-2


def test_inputs_are_what_the_cases_need():
    for case in R.CASES:
        (Dc, Hc, Wc), C1, Cout, B = case
        inp = R.make_inputs(case)
        x1 = inp["x1"]
        assert x1.shape == (B, Dc, Hc, Wc, C1) and inp["w1"].shape == (Cout, C1, 3, 3, 3) and torch.equal(inp["w"][:, R.C0:], inp["w1"])
        zeros = x1 == 0
        assert int(zeros.sum()) > 0 and int((zeros & torch.signbit(x1)).sum()) > 0 and int((zeros & ~torch.signbit(x1)).sum()) > 0
        if B > 1:
            assert float(x1[R.BIG].abs().max()) > 256 * max(float(x1[b].abs().max()) for b in range(B) if b != R.BIG)
        a1, d1 = R.affine_reference(x1, inp["gamma"], inp["beta"])
        assert bool(torch.isfinite(a1).all()) and bool(torch.isfinite(d1).all()) and float(d1.abs().max()) > 0.5
        # the affine is GroupNorm's
        want = F.group_norm(x1.double().permute(0, 4, 1, 2, 3), R.GROUPS, inp["gamma"].double(), inp["beta"].double(), eps=R.EPS).permute(0, 2, 3, 4, 1)
        got = x1.double() * a1[:, None, None, None, :] + d1[:, None, None, None, :]
        assert float((got - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def test_grid_table_covers_every_kind_of_grid_for_each_template():
    """the launch rule of gn_upconv_partial restated over the case table: for EACH template one workgroup, fewer than 8, a multiple of 8, and more
    than 8 that is no multiple of 8; three column blocks under either template"""
    seen = {1: set(), 2: set()}
    for case in R.CASES:
        (Dc, Hc, Wc), C1, Cout, B = case
        NT, TZC, ncb, nblk = R.launch_rule(case)
        assert C1 % 16 == 0 and 16 <= C1 <= 384 and Cout % 32 == 0
        assert NT == (2 if Cout % 64 == 0 else 1) and TZC == (2 if NT == 1 else 1) and ncb * 32 * NT == Cout
        assert nblk == -(-Dc // TZC) * -(-Hc // 8) * -(-Wc // 8) * (Cout // (32 * NT))
        seen[NT].add(R.nblk_class(nblk))
    for NT in (1, 2):
        assert seen[NT] == set(R.NBLK_CLASSES), (NT, seen[NT])
        assert any(R.launch_rule(c)[0] == NT and R.launch_rule(c)[2] == 3 for c in R.CASES), NT
    rule = {R.case_id(c): R.launch_rule(c) for c in R.CASES}
    assert rule["3x9x5-48to32-B3"] == (1, 2, 1, 4) and rule["3x9x5-48to96-B1"] == (1, 2, 3, 12) and rule["16x8x8-16to32-B1"] == (1, 2, 1, 8)
    assert rule["3x9x5-16to64-B3"] == (2, 1, 1, 6) and rule["3x9x5-32to192-B1"] == (2, 1, 3, 18) and rule["4x8x16-16to64-B1"] == (2, 1, 1, 8)
    assert rule["5x10x17-32to64-B2"] == (2, 1, 1, 30) and rule["2x3x5-384to128-B1"] == (2, 1, 2, 4)
    # what the cases are there for: the single slice, the odd slice count, the full a / d table
    c1s = {c[1] for c in R.CASES}
    assert {16, 48, 384} <= c1s


def test_wrapper_refuses_by_name_before_it_looks_for_a_device():
    """ops.upconv_partial's checks of dtype, contiguity and shape come before anything touches a device: they fire on CPU tensors too (the GPU module
    runs the same refusals against a patched-out launch); the conforming call then fails for want of a GPU, never silently"""
    import pytest
    from garmentnets_amd import _lib
    case = R.CASES[4]
    (Dc, Hc, Wc), C1, Cout, B = case
    inp = R.make_inputs(case)
    a, d = [t.float() for t in R.affine_reference(inp["x1"], inp["gamma"], inp["beta"])]
    inv = torch.ones(B)
    pack = ops.pack_upconv_weight(ops.polyphase_weights(inp["w"], R.C0)[1], Cout, ops.SPLIT_F16X2)
    assert pack.tensor.numel() * 2 == _lib.load().gn_weight_pack_upconv_bytes(C1, Cout) and pack.out_scale.shape == (8 * Cout,)
    full_a = torch.cat((torch.ones(B, R.C0), a), dim=1)
    good = dict(src1=inp["x1"], a1=a, d1=d, pack=pack, cout=Cout, act_inv=inv)
    SP = ops.SplitPack
    for over, exc, msg in [
            (dict(src1=inp["x1"].double()), TypeError, "src1"),
            (dict(src1=inp["x1"].transpose(2, 3)), ValueError, "src1.*contiguous"),
            (dict(src1=inp["x1"][0]), ValueError, "src1: expected"),
            (dict(a1=full_a), ValueError, "a: expected"),
            (dict(d1=full_a[:, R.C0:]), ValueError, "d.*contiguous"),
            (dict(act_inv=inv[:1]), ValueError, "act_inv: expected"),
            (dict(pack=SP(pack.tensor[:-8], pack.mode, pack.out_scale)), ValueError, "pack: "),
            (dict(pack=SP(pack.tensor, pack.mode, pack.out_scale[:Cout])), ValueError, "pack.out_scale: expected"),
            (dict(pack=SP(pack.tensor, ops.SPLIT_BF16X3, pack.out_scale)), ValueError, "two-plane modes only")]:
        with pytest.raises(exc, match=msg):
            ops.upconv_partial(**dict(good, **over))
    with pytest.raises(_lib.GarmentNetsHipError, match="no CPU fallback"):
        ops.upconv_partial(**good)


def test_xcd_remap_is_a_bijection():
    """the remap of blockIdx.x restated: a permutation of range(nblk) for every grid from 1 to 64 workgroups (one that is not leaves tiles unwritten),
    each XCD on a contiguous range"""
    for nblk in range(1, 65):
        logical = [R.xcd_logical(b, nblk) for b in range(nblk)]
        assert sorted(logical) == list(range(nblk)), nblk
        for xcd in range(min(8, nblk)):
            mine = [logical[b] for b in range(xcd, nblk, 8)]
            assert mine == list(range(mine[0], mine[0] + len(mine))), (nblk, xcd)

"""Host-side checks of the f16x2 backward of the UNet convolutions (arith.Arith.conv_grad_mode, unet3d.conv_grad_plan, the data gradient's pack, the C
ABI's declarations, the command line): no GPU needed -- run with `-m "not gpu"`."""
import os
import re

import pytest
import torch

from garmentnets_amd import _lib, arith as AR, ops
from garmentnets_amd.components import unet3d as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gn_conv3d_bwd_weight_split", "gn_conv3d_bwd_weight_split_workspace_bytes", "gn_relu_mask_max", "gn_relu_mask_max_workspace_bytes"]


# ------------------------------------------------------------------------------------------------ Arith
def test_arith_field(monkeypatch):
    monkeypatch.delenv("GARMENTNETS_CONV_GRAD_MODE", raising=False)
    assert AR.Arith().conv_grad_mode == "fp32" and AR.Arith.from_env().conv_grad_mode == "fp32"
    with pytest.raises(ValueError, match="conv_grad_mode"):
        AR.Arith(conv_grad_mode="bf16")
    with pytest.raises(ValueError, match="conv_grad_mode"):
        AR.Arith().replace(conv_grad_mode=None)
    on = AR.Arith().replace(conv_grad_mode="f16x2")
    assert on.conv_grad_mode == "f16x2" and on != AR.Arith() and hash(on) != hash(AR.Arith())
    assert on.strict_fp32().conv_grad_mode == "fp32" and on.strict_fp32() == AR.Arith().strict_fp32()
    # nothing else moves with the field
    assert on.replace(conv_grad_mode="fp32") == AR.Arith()
    assert AR.Arith.from_env().replace(conv_grad_mode="f16x2").replace(conv_grad_mode="fp32") == AR.Arith.from_env()
    for f in ("conv_mode", "decode_mode", "device_packs", "winograd"):
        assert getattr(on, f) == getattr(AR.Arith(), f)
    assert "conv_grad_mode" in AR.__doc__


def test_arith_reads_the_environment(monkeypatch):
    monkeypatch.setenv("GARMENTNETS_CONV_GRAD_MODE", "f16x2")
    assert AR.Arith.from_env().conv_grad_mode == "f16x2"
    monkeypatch.setenv("GARMENTNETS_CONV_GRAD_MODE", "fp32")
    assert AR.Arith.from_env().conv_grad_mode == "fp32"
    monkeypatch.setenv("GARMENTNETS_CONV_GRAD_MODE", "fp16")
    with pytest.raises(ValueError, match="GARMENTNETS_CONV_GRAD_MODE"):
        AR.Arith.from_env()


# ------------------------------------------------------------------------------------------------ conv_grad_plan
SHAPES = [((32, 32, 32), 128, 0, 32), ((4, 4, 4), 256, 0, 256), ((16, 16, 16), 64, 128, 64), ((2, 6, 4), 64, 32, 64), ((128, 128, 128), 128, 0, 128)]


def test_plan_fp32_mode_always_gives_the_fp32_kernels():
    for arith in (AR.Arith(), AR.Arith().strict_fp32(), AR.Arith(device_packs=True)):
        for dims, c0, c1, cout in SHAPES + [((4, 6, 10), 22, 12, 40)]:
            assert U.conv_grad_plan(arith, dims, c0, c1, cout) == U.ConvGradPlan("fp32", "fp32")


def test_plan_f16x2_and_each_fallback_rule_from_both_sides():
    on = AR.Arith(conv_grad_mode="f16x2")
    for dims, c0, c1, cout in SHAPES:
        assert U.conv_grad_plan(on, dims, c0, c1, cout) == U.ConvGradPlan("f16x2", "f16x2")
    # the data gradient's pack reads the layer's output width 16 channels at a time
    assert not U.grad_data_pack_unsupported(32) and not U.grad_data_pack_unsupported(48) and U.grad_data_pack_unsupported(40)
    assert U.conv_grad_plan(on, (4, 6, 10), 32, 0, 48) == U.ConvGradPlan("f16x2", "f16x2")
    assert U.conv_grad_plan(on, (4, 6, 10), 32, 0, 40) == U.ConvGradPlan("fp32", "f16x2")
    # the weight gradient stages quads of channels that must not straddle the sources
    assert not U.grad_weight_partial_quad(20, 12) and U.grad_weight_partial_quad(22, 12) and U.grad_weight_partial_quad(20, 10)
    assert U.conv_grad_plan(on, (4, 6, 10), 20, 12, 32) == U.ConvGradPlan("f16x2", "f16x2")
    assert U.conv_grad_plan(on, (4, 6, 10), 22, 12, 32) == U.ConvGradPlan("f16x2", "fp32")
    assert U.conv_grad_plan(on, (4, 6, 10), 20, 10, 32) == U.ConvGradPlan("f16x2", "fp32")
    # the forward arithmetic and the pack builders decide nothing here
    assert U.conv_grad_plan(on.strict_fp32().replace(conv_grad_mode="f16x2"), (8, 8, 8), 32, 64, 64) == U.ConvGradPlan("f16x2", "f16x2")
    assert U.conv_grad_plan(on.replace(device_packs=True), (8, 8, 8), 32, 64, 64) == U.ConvGradPlan("f16x2", "f16x2")


def test_plan_is_a_pure_function():
    on = AR.Arith(conv_grad_mode="f16x2")
    a = U.conv_grad_plan(on, (8, 8, 8), 32, 64, 64)
    b = U.conv_grad_plan(AR.Arith(conv_grad_mode="f16x2"), (8, 8, 8), 32, 64, 64)
    assert a == b and isinstance(a, U.ConvGradPlan) and isinstance(a, tuple)
    assert U.conv_grad_plan.__wrapped__(on, (8, 8, 8), 32, 64, 64) == a        # (behind the cache: the same value again)
    with pytest.raises(AttributeError):
        a.data = "fp32"


# ------------------------------------------------------------------------------------------------ the data gradient's pack
@pytest.mark.parametrize("cout,cin", [(32, 16), (48, 20)])
def test_data_gradient_pack_is_the_split_pack_of_the_flipped_transposed_padded_weight(cout, cin):
    """(Cout, Cin) padded as the layer pads them: stored widths round_up(., 32) with zero rows / columns; then flipped over the taps, transposed over
    (ci, co) -- explicitly, index by index -- and packed by pack_conv_weight_split: bit for bit what the backward builds"""
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g)
    cs, ci_s = U.stored_channels(cout), U.stored_channels(cin)
    wp = torch.zeros(cs, ci_s, 3, 3, 3)
    wp[:cout, :cin] = w
    wt = torch.zeros(ci_s, cs, 3, 3, 3)
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                wt[:, :, kd, kh, kw] = wp[:, :, 2 - kd, 2 - kh, 2 - kw].t()
    assert torch.equal(ops.bwd_data_weight(wp), wt)
    want = ops.pack_conv_weight_split(wt, ops.SPLIT_F16X2)
    got = ops.pack_conv_weight_bwd_data_split(wp)
    assert got.mode == ops.SPLIT_F16X2 and got.tensor.dtype == torch.int16
    assert torch.equal(got.tensor, want.tensor) and torch.equal(got.out_scale, want.out_scale)
    # an input width that is no multiple of 32 gets zero output rows, as pack_conv_weight_bwd_data documents
    w16 = torch.randn(32, 16, 3, 3, 3, generator=g)
    assert tuple(ops.bwd_data_weight(w16).shape) == (32, 32, 3, 3, 3) and not bool(ops.bwd_data_weight(w16)[16:].any())
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.bwd_data_weight(torch.zeros(40, 16, 3, 3, 3))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_new_entries():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    declared = set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_workspace_and_refusals_before_any_launch():
    lib = _lib.load()
    # the fp32 entry's chains behind a header of ceil((16 + 4 B) / 256) * 256 bytes
    for args in ((2, 16, 16, 16, 32, 64), (3, 4, 8, 40, 384, 256), (1, 8, 8, 8, 16, 32), (24, 32, 32, 32, 128, 32), (100, 8, 8, 8, 32, 32)):
        header = -(-(16 + 4 * args[0]) // 256) * 256
        assert lib.gn_conv3d_bwd_weight_split_workspace_bytes(*args) == header + lib.gn_conv3d_bwd_weight_workspace_bytes(*args)
    assert lib.gn_conv3d_bwd_weight_split_workspace_bytes(3, 4, 8, 40, 384, 256) == 256 + 8 * 27 * 384 * 256 * 4
    assert lib.gn_conv3d_bwd_weight_split_workspace_bytes(100, 8, 8, 8, 32, 32) % 256 == 0
    assert lib.gn_conv3d_bwd_weight_split_workspace_bytes(1, 8, 8, 8, 16, 48) == 0
    c = _lib.call
    with pytest.raises(ValueError, match="multiple of 32"):
        c("gn_conv3d_bwd_weight_split", None, 16, None, 0, None, None, None, None, None, None, 1, 8, 8, 8, 48, None, 0, None, None)
    with pytest.raises(ValueError, match="multiples of 4"):
        c("gn_conv3d_bwd_weight_split", None, 18, None, 0, None, None, None, None, None, None, 1, 8, 8, 8, 32, None, 0, None, None)
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_conv3d_bwd_weight_split", None, 16, None, 0, None, None, None, None, None, None, 1, 8, 8, 8, 32, None, 16, None, None)
    assert lib.gn_relu_mask_max_workspace_bytes(3) == 3 * 256 * 4 and lib.gn_relu_mask_max_workspace_bytes(0) == 0
    with pytest.raises(ValueError, match="multiple of 4"):
        c("gn_relu_mask_max", None, None, 1, 6, 2, None, None, None, None, None, 0, None)
    with pytest.raises(ValueError, match="come together"):
        c("gn_relu_mask_max", None, None, 1, 8, 2, None, None, 1, None, None, 0, None)
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_relu_mask_max", None, None, 2, 8, 2, None, None, None, None, None, 1024, None)


def test_no_atomics_in_the_source():
    src = open(os.path.join(REPO, "garmentnets_amd", "csrc", "unet_grad_split.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic", code, re.I)


def test_ops_wrapper_checks_its_arguments_before_any_launch():
    x = torch.zeros(1, 8, 8, 8, 16)
    dy = torch.zeros(1, 8, 8, 8, 32)
    a = torch.zeros(1, 16)
    with pytest.raises(ValueError, match="does not match"):
        ops.conv3d_bwd_weight_split(x, None, a, a, None, torch.zeros(1, 4, 8, 8, 32))
    with pytest.raises(ValueError, match=r"must be \[B\]\[C0 \+ C1\]"):
        ops.conv3d_bwd_weight_split(x, None, torch.zeros(1, 8), a, None, dy)
    with pytest.raises(ValueError, match=r"x_inv must be \[B\]"):
        ops.conv3d_bwd_weight_split(x, None, a, a, None, dy, x_inv=torch.zeros(2), gmax=torch.zeros(1))
    with pytest.raises(TypeError):
        ops.conv3d_bwd_weight_split(x.double(), None, a, a, None, dy)
    with pytest.raises(ValueError, match="half-resolution"):
        ops.conv3d_bwd_weight_split(x, torch.zeros(1, 4, 4, 2, 16), torch.zeros(1, 32), torch.zeros(1, 32), None, dy)


# ------------------------------------------------------------------------------------------------ the command line
def test_train_pipeline_knows_split_backward():
    from garmentnets_amd import train_pipeline as TP
    ap = TP.build_parser()
    flag = [act for act in ap._actions if "--split_backward" in act.option_strings]
    assert len(flag) == 1 and flag[0].default is False
    assert ap.get_default("split_backward") is False

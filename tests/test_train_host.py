"""Host side of the training step (no GPU): the new names in the C ABI, the header and autograd.__all__; what FusedAdam refuses and its state layout
against torch.optim.Adam; the command line of garmentnets_amd.train; value_loss's refusal of the row-norm metric."""
import copy
import os
import re

import pytest
import torch

from garmentnets_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gn_nocs_bin_loss_bwd", "gn_value_losses_bwd", "gn_adam_step")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    for struct in ("GnNocsBinGradSet", "GnLossGradSegment", "GnAdamEntry", "GnAdamHyper"):
        assert struct in hdr
    assert f"#define GN_ADAM_CHUNK {_lib.ADAM_CHUNK}" in hdr and f"#define GN_ADAM_MAX_HYPER {_lib.ADAM_MAX_HYPER}" in hdr
    import ctypes
    assert ctypes.sizeof(_lib.NocsBinGradSet) == 48 and ctypes.sizeof(_lib.LossGradSegment) == 48
    assert ctypes.sizeof(_lib.AdamEntry) == 56 and ctypes.sizeof(_lib.AdamHyper) == 56


def test_autograd_exports_the_losses():
    from garmentnets_amd import autograd as A
    for name in ("nocs_bin_loss", "value_loss"):
        assert name in A.__all__ and callable(getattr(A, name))


def test_inference_modules_do_not_import_autograd():
    import subprocess
    import sys
    code = ("import sys; import garmentnets_amd.networks.pointnet2_nocs, garmentnets_amd.networks.conv_implicit_wnf; "
            "bad = [m for m in ('garmentnets_amd.autograd', 'garmentnets_amd.train', 'garmentnets_amd.optim') if m in sys.modules]; "
            "sys.exit(1 if bad else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=REPO).returncode == 0


def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (1, 5, 12)]


def test_fused_adam_refuses_by_name():
    from garmentnets_amd.optim import FusedAdam
    with pytest.raises(NotImplementedError, match="amsgrad"):
        FusedAdam(_params(), amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        FusedAdam(_params(), maximize=True)
    with pytest.raises(TypeError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(TypeError, match="float32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(TypeError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    # a group flag that arrives through a loaded state dict is refused at the step, before any launch
    opt = FusedAdam(_params())
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()


def test_fused_adam_state_layout_is_torch_adams():
    from garmentnets_amd.optim import FusedAdam
    ps = _params()
    ref = torch.optim.Adam(ps, lr=3e-3, betas=(0.8, 0.95), eps=1e-7, weight_decay=1e-2, foreach=False)
    for p in ps:
        p.grad = torch.ones_like(p)
    ref.step()
    ref.step()
    ours = FusedAdam(ps)
    assert set(ours.param_groups[0]) == set(ref.param_groups[0])                  # torch's group keys
    ours.load_state_dict(copy.deepcopy(ref.state_dict()))              # (load_state_dict keeps the tensors it is handed)
    assert ours.param_groups[0]["lr"] == 3e-3 and tuple(ours.param_groups[0]["betas"]) == (0.8, 0.95)
    for p in ps:
        a, b = ours.state[p], ref.state[p]
        assert set(a) == set(b) == {"step", "exp_avg", "exp_avg_sq"}
        assert isinstance(a["step"], torch.Tensor) and a["step"].dtype == b["step"].dtype and float(a["step"]) == 2.0 and not a["step"].is_cuda
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    # and back: our state dict drives torch's Adam to the step torch's own state dict gives
    back = torch.optim.Adam(ps, foreach=False)
    back.load_state_dict(copy.deepcopy(ours.state_dict()))
    before = [p.detach().clone() for p in ps]
    back.step()
    after_ours = [p.detach().clone() for p in ps]
    with torch.no_grad():
        for p, b in zip(ps, before):
            p.copy_(b)
    ref.step()
    assert all(torch.equal(p.detach(), a) for p, a in zip(ps, after_ours))


def test_train_parser():
    from garmentnets_amd import train
    a = train.parse_args(["--model", "pointnet2", "--zarr_in", "x.zarr", "--output_dir", "out", "--epochs", "3", "--num_batches", "2"])
    assert (a.model, a.batch_size, a.epochs, a.num_batches, a.checkpoint_path, a.num_pc_sample) == ("pointnet2", 8, 3, 2, None, 6000)
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--model", "pipeline", "--zarr_in", "x.zarr"])
    assert "not implemented yet: second-stage training step" in str(e.value)


def test_value_loss_refuses_the_row_norm_metric():
    from garmentnets_amd import autograd as A
    x = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(ValueError, match="row_norm"):
        A.value_loss([(x, torch.zeros(4, 3), "row_norm")])
    with pytest.raises(ValueError, match="row_norm"):
        A.value_loss([(x, torch.zeros(4, 3), "l2"), (x, torch.zeros(4, 3), "row_norm", True)], [1.0, 1.0])

"""Host-side checks of the MLP gradients (csrc/linear_grad.hip, autograd.mlp / linear / implicit_decode): no GPU needed -- run with `-m "not gpu"`."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from garmentnets_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gn_linear_act_bwd", "gn_linear_act_bwd_workspace_bytes", "gn_linear_bwd_weight", "gn_linear_bwd_weight_workspace_bytes", "gn_row_affine"]
R = _lib.LINEAR_BWD_CHUNK_ROWS


def test_header_declares_every_mlp_gradient_entry_and_the_chunk_constants():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    declared = set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert int(re.search(r"#define GN_LINEAR_BWD_CHUNK_ROWS (\d+)", hdr).group(1)) == _lib.LINEAR_BWD_CHUNK_ROWS
    assert int(re.search(r"#define GN_LINEAR_ACT_CHUNK_ROWS (\d+)", hdr).group(1)) == _lib.LINEAR_ACT_CHUNK_ROWS


def test_no_float_atomics_in_the_source():
    src = open(os.path.join(REPO, "garmentnets_amd", "csrc", "linear_grad.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"atomic", code, re.I)


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (R, 128, 131), (R + 1, 128, 131), (144000, 256, 256), (0, 128, 131)])
def test_weight_workspace_is_one_partial_per_row_chunk(M, N, K):
    assert _lib.load().gn_linear_bwd_weight_workspace_bytes(M, N, K) == -(-M // R) * N * K * 4


def test_act_workspace_is_three_fp64_rows_per_row_chunk():
    lib, ra = _lib.load(), _lib.LINEAR_ACT_CHUNK_ROWS
    for M, N in ((1, 1), (ra, 65), (ra + 1, 65), (0, 7)):
        assert lib.gn_linear_act_bwd_workspace_bytes(M, N) == -(-M // ra) * 3 * N * 8


def test_c_abi_refuses_bad_arguments_before_any_launch():
    c, big = _lib.call, 1 << 30
    #   g, ldg, x, ldx, M, N, K, ws, ws_bytes, dW, lddw, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 8, None, 8, -1, 8, 8, None, big, None, 8, None)        # M < 0
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 10, 0, 8, None, big, None, 8, None)        # N < 1
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 10, 8, -3, None, big, None, 8, None)       # K < 1
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 7, None, 8, 10, 8, 8, None, big, None, 8, None)        # ldg < N
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 8, None, 7, 10, 8, 8, None, big, None, 8, None)        # ldx < K
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 10, 8, 8, None, big, None, 7, None)        # lddw < K
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 10, 8, 8, None, 8 * 8 * 4 - 1, None, 8, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 10, 8, 8, None, big, None, 8, None)        # g, x, dW
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_linear_bwd_weight", None, 8, None, 8, 0, 8, 8, None, 0, None, 8, None)           # no rows: dW is still written
    #   dy, lddy, r, ldr, sc, M, N, g, ldg, ws, ws_bytes, sums, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_act_bwd", None, 8, None, 8, None, -1, 8, None, 8, None, big, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_linear_act_bwd", None, 7, None, 8, None, 10, 8, None, 8, None, big, None, None)  # lddy < N
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_linear_act_bwd", None, 8, None, 8, None, 10, 8, None, 8, None, 3 * 8 * 8 - 1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_linear_act_bwd", None, 8, None, 8, None, 10, 8, None, 8, None, big, None, None)
    #   r, ldr, sc, sh, M, N, y, ldy, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_row_affine", None, 7, None, None, 10, 8, None, 8, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_row_affine", None, 8, None, None, 10, 8, None, 8, None)


def test_autograd_imports_without_a_gpu_and_refuses_by_name():
    from garmentnets_amd import autograd as A
    from garmentnets_amd.components.mlp import MLP, HipLinear
    for name in ("mlp", "linear", "implicit_decode"):
        assert callable(getattr(A, name)), name
        assert name in A.__all__
    x = torch.zeros(4, 6, requires_grad=True)
    with pytest.raises(TypeError, match="MLPStack"):
        A.mlp(torch.nn.Sequential(torch.nn.Linear(6, 8)), x)
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm"):
        A.mlp(MLP([6, 8, 8]), x)                                  # a fresh module is in training mode
    with pytest.raises(TypeError, match="float32"):
        A.mlp(MLP([6, 8, 8]).eval(), x.double())
    with pytest.raises(TypeError, match="HipLinear"):
        A.linear(torch.nn.Linear(6, 8), x)
    with pytest.raises(TypeError, match="float32"):
        A.linear(HipLinear(6, 8), x.half())
    with pytest.raises(TypeError, match="ImplicitWNFDecoder"):
        A.implicit_decode(MLP([6, 8, 8]).eval(), torch.zeros(1, 6, 4, 4, 4), torch.zeros(1, 5, 3))


def r_block(x, w, b, bn, mask=None):
    """the restatement of one block the GPU tests compare against: F.linear -> relu (or the shared mask) -> eval F.batch_norm.  bn: (running_mean,
    running_var, gamma, beta, eps) or None"""
    h = F.linear(x, w, b)
    r = F.relu(h) if mask is None else h * mask
    return r if bn is None else F.batch_norm(r, bn[0], bn[1], bn[2], bn[3], False, 0.0, bn[4])


@pytest.mark.parametrize("shared_mask", [False, True])
@pytest.mark.parametrize("with_bn", [True, False])
def test_closed_forms_are_the_restatements_gradient(with_bn, shared_mask):
    """the formulas of csrc/linear_grad.hip and autograd._LinearBlock (g, dW, db, dgamma, dbeta, dX) against torch's fp64 autograd of the restatement"""
    gen = torch.Generator().manual_seed(5 + 2 * with_bn + shared_mask)
    M, K, N, eps = 37, 11, 9, 1e-5
    x, w, b = (torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in ((M, K), (N, K), (N,)))
    mean, var = torch.randn(N, generator=gen, dtype=torch.float64), torch.rand(N, generator=gen, dtype=torch.float64) + 0.5
    gamma, beta = (torch.randn(N, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    with torch.no_grad():
        gamma[0], gamma[1] = -0.7, 0.0
    dy = torch.randn(M, N, generator=gen, dtype=torch.float64)
    h = F.linear(x, w, b).detach()
    r = F.relu(h)
    mask = (r > 0).double() if shared_mask else None
    y = r_block(x, w, b, (mean, var, gamma, beta, eps) if with_bn else None, mask)
    params = [x, w, b] + ([gamma, beta] if with_bn else [])
    grads = torch.autograd.grad(y, params, dy)
    inv = 1.0 / torch.sqrt(var + eps)
    sc = (gamma * inv).detach() if with_bn else torch.ones(N, dtype=torch.float64)
    g = torch.where(r > 0, dy * sc, torch.zeros((), dtype=torch.float64))
    closed = [g @ w.detach(), g.t() @ x.detach(), g.sum(0)]
    if with_bn:
        s_dy, s_dy_r = dy.sum(0), (dy * r).sum(0)
        closed += [(s_dy_r - mean * s_dy) * inv, s_dy]
    for name, got, ref in zip(("dX", "dW", "db", "dgamma", "dbeta"), closed, grads):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name

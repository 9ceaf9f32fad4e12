"""Host-side checks of train-mode BatchNorm for the MLP blocks (csrc/linear_grad.hip: gn_col_moments, gn_col_dots, gn_bn_train_bwd; autograd.mlp /
implicit_decode with batch_stats=True): no GPU needed -- run with `-m "not gpu"`.  The three entries reuse gn_linear_act_bwd's row chunk
(GN_LINEAR_ACT_CHUNK_ROWS, _lib.LINEAR_ACT_CHUNK_ROWS); there is no new chunk constant."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from garmentnets_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gn_col_moments", "gn_col_moments_workspace_bytes", "gn_col_dots", "gn_col_dots_workspace_bytes", "gn_bn_train_bwd",
           "gn_bn_train_bwd_workspace_bytes"]
RA = _lib.LINEAR_ACT_CHUNK_ROWS


def test_header_prototypes_and_library_have_the_entries_and_agree_on_the_chunk():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    declared = set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), name
    for name in ENTRIES[1::2]:
        assert _lib._RESTYPES[name] is _lib._sz, name
    # the chunk the header documents for the three entries is the one the library and _lib use (the workspace formulas below are in units of it)
    assert int(re.search(r"#define GN_LINEAR_ACT_CHUNK_ROWS (\d+)", hdr).group(1)) == RA
    section = hdr[hdr.index("Train-mode BatchNorm of an MLP block"):]
    assert section.count("ceil(M / GN_LINEAR_ACT_CHUNK_ROWS)") == 3
    assert lib.gn_col_moments_workspace_bytes(RA + 1, 1) == 2 * 8 and lib.gn_col_moments_workspace_bytes(RA, 1) == 8


@pytest.mark.parametrize("M", [0, 1, RA, RA + 1])
@pytest.mark.parametrize("N", [1, 65])
def test_workspaces_are_fp64_rows_per_row_chunk(M, N):
    lib, chunks = _lib.load(), -(-M // RA)
    assert lib.gn_col_moments_workspace_bytes(M, N) == chunks * N * 8
    assert lib.gn_col_dots_workspace_bytes(M, N) == chunks * 2 * N * 8
    assert lib.gn_bn_train_bwd_workspace_bytes(M, N) == chunks * N * 8


def test_c_abi_refuses_bad_arguments_before_any_launch():
    c, big = _lib.call, 1 << 30
    #   r, ldr, M, N, ws, ws_bytes, moments, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_moments", None, 8, -1, 8, None, big, None, None)                                # M < 0
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_moments", None, 8, 10, 0, None, big, None, None)                                # N < 1
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_moments", None, 7, 10, 8, None, big, None, None)                                # ldr < N
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_col_moments", None, 8, RA + 1, 8, None, 2 * 8 * 8 - 1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_col_moments", None, 8, 10, 8, None, big, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_col_moments", None, 8, 0, 8, None, 0, None, None)                                   # no rows: the zeros are still written
    #   dy, lddy, r, ldr, M, N, ws, ws_bytes, dots, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_dots", None, 8, None, 8, -1, 8, None, big, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_dots", None, 8, None, 8, 10, 0, None, big, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_dots", None, 7, None, 8, 10, 8, None, big, None, None)                          # lddy < N
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_col_dots", None, 8, None, 7, 10, 8, None, big, None, None)                          # ldr < N
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_col_dots", None, 8, None, 8, 10, 8, None, 2 * 8 * 8 - 1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_col_dots", None, 8, None, 8, 10, 8, None, big, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_col_dots", None, 8, None, 8, 0, 8, None, 0, None, None)
    #   dy, lddy, r, ldr, coef, M, N, g, ldg, ws, ws_bytes, sum_g, stream
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, -1, 8, None, 8, None, big, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, 10, 0, None, 8, None, big, None, None)
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_bn_train_bwd", None, 7, None, 8, None, 10, 8, None, 8, None, big, None, None)       # lddy < N
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_bn_train_bwd", None, 8, None, 7, None, 10, 8, None, 8, None, big, None, None)       # ldr < N
    with pytest.raises(ValueError, match="bad sizes"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, 10, 8, None, 7, None, big, None, None)       # ldg < N
    with pytest.raises(ValueError, match="workspace too small"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, 10, 8, None, 8, None, 8 * 8 - 1, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, 10, 8, None, 8, None, big, None, None)
    with pytest.raises(ValueError, match="null pointer"):
        c("gn_bn_train_bwd", None, 8, None, 8, None, 0, 8, None, 8, None, 0, None, None)


def test_mlp_refuses_on_cpu_tensors_before_any_launch():
    from garmentnets_amd import autograd as A
    from garmentnets_amd.components.mlp import MLP
    x = torch.zeros(4, 6, requires_grad=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        A.mlp(MLP([6, 8, 8]), x[:1], batch_stats=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        A.mlp(MLP([6, 8, 8]), x[:1].view(1, 1, 6), batch_stats=True)              # the leading dimensions are flattened: still one row
    stack = MLP([6, 8, 8])
    for block in stack:
        block[2].track_running_stats = False
    with pytest.raises(NotImplementedError, match="track_running_stats=False"):
        A.mlp(stack, x, batch_stats=True)
    stack = MLP([6, 8, 8])
    stack[1][2].running_mean = None                                                # a module built without the buffers
    with pytest.raises(NotImplementedError, match="track_running_stats=False"):
        A.mlp(stack, x, batch_stats=True)
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm"):
        A.mlp(MLP([6, 8, 8]), x)                                                   # without the keyword: the old refusal
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm"):
        A.mlp(MLP([6, 8, 8]), x, batch_stats=False)
    with pytest.raises(TypeError, match="float32"):
        A.mlp(MLP([6, 8, 8]), x.double(), batch_stats=True)                        # the dtype and type errors stay, and come first
    with pytest.raises(TypeError, match="MLPStack"):
        A.mlp(torch.nn.Sequential(torch.nn.Linear(6, 8)), x, batch_stats=True)
    with pytest.raises(TypeError, match="ImplicitWNFDecoder"):
        A.implicit_decode(MLP([6, 8, 8]), torch.zeros(1, 6, 4, 4, 4), torch.zeros(1, 5, 3), batch_stats=True)


def _case():
    """M, K, N = 37, 11, 9 in fp64: a gamma of -0.7 and one of exactly 0, and column 2 dead (a large negative bias: r == 0 in every row)"""
    gen = torch.Generator().manual_seed(17)
    M, K, N = 37, 11, 9
    x, w, b = (torch.randn(s, generator=gen, dtype=torch.float64).requires_grad_(True) for s in ((M, K), (N, K), (N,)))
    gamma, beta = (torch.randn(N, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in range(2))
    with torch.no_grad():
        gamma[0], gamma[1] = -0.7, 0.0
        b[2] = -1e3
    dy = torch.randn(M, N, generator=gen, dtype=torch.float64)
    return M, x, w, b, gamma, beta, dy


def test_closed_forms_are_torchs_gradient_of_training_batch_norm_behind_a_relu():
    """autograd._bn_bwd_coef (what _BatchStatsBlock.backward hands gn_bn_train_bwd) and the formulas around it, in fp64, against torch.autograd.grad of
    F.relu(F.linear) -> F.batch_norm(training=True): dX, dW, db, dgamma, dbeta to 1e-12 relative"""
    from garmentnets_amd import autograd as A
    M, x, w, b, gamma, beta, dy = _case()
    eps = 1e-5
    r = F.relu(F.linear(x, w, b))
    assert not bool(r[:, 2].any()) and bool((r > 0).any(0)[[0, 1, 3]].all())          # the dead column is dead, the others are not
    y = F.batch_norm(r, None, None, gamma, beta, True, 0.0, eps)
    grads = torch.autograd.grad(y, [x, w, b, gamma, beta], dy)
    r = r.detach()
    mean = r.mean(0)
    m2 = ((r - mean) ** 2).sum(0)
    assert float(m2[2]) == 0.0
    inv = 1.0 / torch.sqrt(m2 / M + eps)
    assert float(inv[2]) == float(1.0 / torch.sqrt(torch.tensor(eps, dtype=torch.float64)))         # m2 == 0.0: inv is 1 / sqrt(eps) to the bit
    s_dy, s_dyr = dy.sum(0), (dy * r).sum(0)
    dgamma, (ca, cb, cc) = A._bn_bwd_coef(gamma, mean, inv, s_dy, s_dyr, M)
    g = torch.where(r > 0, ca * dy + cb * r + cc, torch.zeros((), dtype=torch.float64))
    closed = [g @ w.detach(), g.t() @ x.detach(), g.sum(0), dgamma, s_dy]
    for name, got, ref in zip(("dX", "dW", "db", "dgamma", "dbeta"), closed, grads):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), name


@pytest.mark.parametrize("momentum", [0.1, None])
def test_buffer_update_is_batchnorm1ds_over_two_calls(momentum):
    """autograd._bn_update_buffers against nn.BatchNorm1d (fp64) for momentum 0.1 and None (the cumulative average), two consecutive batches"""
    from garmentnets_amd import autograd as A
    gen = torch.Generator().manual_seed(23)
    N = 9
    ours, ref = (torch.nn.BatchNorm1d(N, momentum=momentum).double() for _ in range(2))
    for m in (ours, ref):
        with torch.no_grad():
            m.running_mean.copy_(torch.linspace(-1, 1, N))
            m.running_var.copy_(torch.linspace(0.5, 2, N))
    for call, M in enumerate((37, 5)):
        r = F.relu(torch.randn(M, N, generator=gen, dtype=torch.float64) + 0.3)
        r[:, 2] = 0.0
        ref(r)
        mean = r.mean(0)
        A._bn_update_buffers(ours, mean, ((r - mean) ** 2).sum(0), M)
        assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked) == call + 1
        for name in ("running_mean", "running_var"):
            got, want = getattr(ours, name), getattr(ref, name)
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (name, call)

"""GPU (-m gpu): the training step of the first stage -- the loss gradients of csrc/losses.hip (autograd.nocs_bin_loss / value_loss), gn_adam_step behind
optim.FusedAdam, train.pointnet2_nocs_forward / train_step, and `python -m garmentnets_amd.train` end to end.

The error rule is grad_reference._check: ours against torch-fp64 on the CPU <= 4 x (torch-fp32 on the CPU against the same fp64) + 1 fp32 ulp of the
largest value; every ratio is printed.  The restatements are tests/train_reference.py's.

Measured (MI355X), ours / torch-fp32: nocs_bin_loss 0.06 - 1.00 over 281 checks; value_loss l2 0.25 - 0.50, smooth_l1 0.17, bce_logits 0.08 - 0.45;
gn_adam_step p <= 1.00, exp_avg <= 1.52, exp_avg_sq <= 1.00; the whole model's 74 parameter gradients 0.25 - 2.73 (training mode), 0.29 - 2.61 (eval
mode); sa1's BatchNorm buffers 0 ulp from nn.BatchNorm1d over the 1945 real edge rows; twenty steps take the loss from 4.089 to 2.665.
"""
import copy
import csv
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, autograd as A, ops, train as T  # noqa: E402
from garmentnets_amd.batch import Batch  # noqa: E402
from garmentnets_amd.components.mlp import HipLinear  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from garmentnets_amd.networks.pointnet2_nocs import PointNet2NOCS  # noqa: E402
from garmentnets_amd.optim import FusedAdam  # noqa: E402
from grad_reference import _check, _gen, _randomise_norms  # noqa: E402
import train_reference as R  # noqa: E402

DEV = "cuda:0"


def _metrics_of(bins, axis, wn, wg, logits, gt, glogits, ggt):
    """PointNet2NOCS.validation_metrics on handed-in logits: its methods on a stand-in that carries the four attributes they read"""
    me = types.SimpleNamespace(nocs_bins=bins, symmetry_axis=axis, nocs_loss_weight=wn, grip_point_loss_weight=wg)
    me.metrics_from_sums = types.MethodType(PointNet2NOCS.metrics_from_sums, me)
    return PointNet2NOCS.validation_metrics(me, types.SimpleNamespace(y=gt, nocs_grip_point=ggt), {"per_point_logits": logits, "global_logits": glogits})


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================================================ 1. the binned loss
def _bin_targets(n, bins, g, axis, equal):
    """targets drawn 1e-2 of a bin width away from every bin edge, the margin of 1e-3 asserted on the fp32 values, plain and mirrored; rows 0 / 1 (when
    there) carry the exact 0.0 and 1.0 -- on the mirror axis unless the case wants the two branches equal (then every target there is 0.5)"""
    span = max(bins - 1, 1)
    k = torch.randint(0, span, (n, 3), generator=g).float()
    gt = ((k + 0.01 + 0.98 * torch.rand(n, 3, generator=g)) / span).float()
    exact = torch.zeros(n, 3, dtype=torch.bool)
    col = 0 if axis is None else axis
    if equal:
        gt[:, axis] = 0.5
        col = (axis + 1) % 3
    gt[0, col], exact[0, col] = 1.0, True
    if n > 1:
        gt[1, col], exact[1, col] = 0.0, True
    for t in (gt, R.mirror(gt, axis)):
        f = t * span
        frac = (f - torch.floor(f))[~exact]
        assert frac.numel() == 0 or float(torch.minimum(frac, 1 - frac).min()) >= 1e-3
    return gt


def _bin_case(n, bins, axis, case, seed):
    """three row sets for one launch: n per-point rows (padded: 5 columns more than bins * 3, inside a wider buffer), a global set of 1 row and one of 3"""
    g = _gen(seed)
    sets = []
    for i, rows in enumerate((n, 1, 3)):
        gt = _bin_targets(rows, bins, g, axis, case == "equal")
        lg = torch.randn(rows, bins * 3, generator=g) * 2
        if axis is not None and case in ("plain", "mirrored"):
            # by construction: a large logit at the plain (or the mirrored) target bin of the mirror axis wherever the two bins differ
            t, tm = R.target_bins(gt, bins), R.target_bins(R.mirror(gt, axis), bins)
            win = t if case == "plain" else tm
            l3 = lg.view(rows, bins, 3)
            for r in (t[:, axis] != tm[:, axis]).nonzero().squeeze(1).tolist():
                l3[r, win[r, axis], axis] += 40.0
        if i == 0:
            wide = torch.full((rows, bins * 3 + 9), float("nan"))
            wide[:, :bins * 3 + 5] = torch.cat((lg, torch.randn(rows, 5, generator=g)), 1)
            lg = wide[:, :bins * 3 + 5]
        sets.append((lg, gt))
    return sets


def _bin_reference(sets, bins, axis, weights, dtype, take_mirror, scale):
    leaves = [lg.detach().clone().to(dtype).requires_grad_(True) for lg, _ in sets]
    tg = [R.target_bins(R.mirror(gt, axis) if take_mirror else gt, bins) for _, gt in sets]
    loss = R.r_bin_loss([(l, None) for l in leaves], bins, weights, tg)
    grads = torch.autograd.grad(scale * loss, leaves)
    out = []
    for gr, (lg, _) in zip(grads, sets):
        gr = gr.clone()
        gr[:, bins * 3:] = 0
        out.append(gr)
    return float(loss.detach()), out


BIN_CASES = [(None, "plain"), (0, "plain"), (0, "mirrored"), (0, "equal"), (2, "plain"), (2, "mirrored"), (2, "equal")]


@pytest.mark.parametrize("axis,case", BIN_CASES, ids=[f"axis{a}-{c}" for a, c in BIN_CASES])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("bins", [2, 64])
def test_nocs_bin_loss_gradient(bins, n, axis, case):
    weights = (1.0, 0.7, 1.3)
    sets = _bin_case(n, bins, axis, case, 1000 * bins + 10 * n + (0 if axis is None else axis + 1))
    # the decision, from the fp64 restatement: gap >= 1e-2 in the weighted losses, or exactly equal
    plain64, _ = _bin_reference(sets, bins, axis, weights, torch.float64, False, 1.0)
    mir64, _ = _bin_reference(sets, bins, axis, weights, torch.float64, True, 1.0)
    if axis is None or case == "equal":
        assert plain64 == mir64
        take = False
    else:
        assert (mir64 - plain64 if case == "plain" else plain64 - mir64) >= 1e-2, (plain64, mir64)
        take = case == "mirrored"
    dsets = [(lg.to(DEV), gt.to(DEV)) for lg, gt in sets]
    dsets[0] = (torch.full((n, bins * 3 + 9), float("nan"), device=DEV), dsets[0][1])
    dsets[0][0][:, :bins * 3 + 5] = sets[0][0].to(DEV)
    dsets[0] = (dsets[0][0][:, :bins * 3 + 5], dsets[0][1])                   # ldl > the row's columns > bins * 3

    def run(scale):
        leaves = [lg.detach().requires_grad_(True) for lg, _ in dsets]
        loss, sums = A.nocs_bin_loss([(l, gt) for l, (_, gt) in zip(leaves, dsets)], bins, axis, weights)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and not sums.requires_grad and sums.dtype == torch.float64
        (scale * loss).backward()
        return loss.detach(), [l.grad for l in leaves]

    for scale in (1.0, 2.5):
        loss, grads = run(scale)
        l64, g64 = _bin_reference(sets, bins, axis, weights, torch.float64, take, scale)
        _, g32 = _bin_reference(sets, bins, axis, weights, torch.float32, take, scale)
        assert abs(loss.item() - l64) <= 1e-5 * abs(l64) + 1e-6
        for s, (a, b, c) in enumerate(zip(g64, g32, grads)):
            assert c.is_contiguous() and c.shape == dsets[s][0].shape
            assert not c[:, bins * 3:].cpu().view(torch.int32).any()                        # the pad columns: exactly +0
            _check(f"nocs_bin_loss bins={bins} n={n} axis={axis} {case} x{scale} set {s}", a, b, c)
        _, again = run(scale)
        assert all(_bits(a, b) for a, b in zip(grads, again))                                  # identical calls, identical bits
    # the loss value: validation_metrics' on the same inputs, to the last fp32 bit (two sets: its own call shape)
    wn, wg = 1.0, 0.7
    vm = _metrics_of(bins, axis, wn, wg, dsets[0][0], dsets[0][1], dsets[2][0], dsets[2][1])
    loss2, _ = A.nocs_bin_loss([dsets[0], dsets[2]], bins, axis, (wn, wg))
    assert np.float32(vm["loss"]).view(np.int32) == np.float32(loss2.item()).view(np.int32), (vm["loss"], loss2.item())


# ================================================================================================ 2. the element-wise losses
def _value_case(kind, count, mirror, g):
    """(pred, target) of `count` elements as (count / 3, 3) rows.  mirror: None | "plain" | "mirrored" (which branch wins, by construction).  The
    special elements sit in the y / z columns, which mirroring leaves alone: smooth_l1 at d exactly 0, +1 and -1; bce logits at +30 and -30"""
    tgt = torch.rand(count // 3, 3, generator=g)
    tgt[0, 0] = 0.1                                                              # (a single row still separates the two branches)
    base = R.mirror_x(tgt) if mirror == "mirrored" else tgt
    noise = torch.randn(tgt.shape, generator=g) * torch.tensor([0.05, 1.0, 1.0])   # x: close to the winning branch; y, z: wide
    if kind == "bce_logits":
        pred = 8 * (base - 0.5) + 0.3 * noise
        pred.view(-1)[1], pred.view(-1)[2] = 30.0, -30.0
    else:
        pred = base + (1.5 if kind == "smooth_l1" else 0.3) * noise
        if kind == "smooth_l1":
            tgt.view(-1)[1], tgt.view(-1)[2] = 0.25, 0.5
            pred.view(-1)[1], pred.view(-1)[2] = 1.25, 0.5                        # d = +1 exactly, d = 0
            if count > 4:
                tgt.view(-1)[4], pred.view(-1)[4] = 0.5, -0.5                     # d = -1 exactly
    return pred.float(), tgt.float()


def _value_reference(segs, weights, dtype, takes):
    leaves = [p.detach().clone().to(dtype).requires_grad_(True) for p, *_ in segs]
    loss = 0
    for leaf, (_, t, kind, _), w, take in zip(leaves, segs, weights, takes):
        loss = loss + w * R.VALUE_LOSS[kind](leaf, (R.mirror_x(t) if take else t).to(dtype))
    grads = torch.autograd.grad(loss, leaves)
    return float(loss.detach()), grads


@pytest.mark.parametrize("mirror", [None, "plain", "mirrored"])
@pytest.mark.parametrize("count", [3, 2046, 2049, 6147])
@pytest.mark.parametrize("kind", ["l2", "smooth_l1", "bce_logits"])
def test_value_loss_gradient(kind, count, mirror):
    g = _gen(7 * count + len(kind))
    weights = (1.0, 0.6)
    p0, t0 = _value_case(kind, count, mirror, g)
    p1, t1 = _value_case(kind, 12, None, g)
    segs = [(p0, t0, kind, mirror is not None), (p1, t1, kind, False)]
    takes = [mirror == "mirrored", False]
    if mirror is not None:
        # the gap between the two branches of the mirrored segment, from the fp64 restatement
        a = float(R.VALUE_LOSS[kind](p0.double(), t0.double()))
        b = float(R.VALUE_LOSS[kind](p0.double(), R.mirror_x(t0).double()))
        assert (b - a if mirror == "plain" else a - b) >= 1e-2, (a, b)
    l64, g64 = _value_reference(segs, weights, torch.float64, takes)
    _, g32 = _value_reference(segs, weights, torch.float32, takes)
    leaves = [p.to(DEV).requires_grad_(True) for p, *_ in segs]
    loss, sums = A.value_loss([(leaf, t.to(DEV), k, m) for leaf, (_, t, k, m) in zip(leaves, segs)], weights)
    assert loss.dtype == torch.float32 and not sums.requires_grad and tuple(sums.shape) == (2, 2)
    loss.backward()
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64) + 1e-6
    for s, (a, b, leaf) in enumerate(zip(g64, g32, leaves)):
        _check(f"value_loss {kind} count={count} mirror={mirror} segment {s}", a, b, leaf.grad)
    if kind == "smooth_l1":
        # torch's choice at the joints: the quadratic branch's d at |d| == 1 (= the sign), 0 at d == 0
        flat, one = leaves[0].grad.view(-1).cpu(), float(np.float32(weights[0] / count))
        assert float(flat[2]) == 0.0 and float(flat[1]) == one and (count <= 4 or float(flat[4]) == -one)
        assert float(g32[0].view(-1)[2]) == 0.0 and abs(float(g32[0].view(-1)[1]) - one) <= 1e-6 * one      # torch's own choice at the same joints


def test_value_loss_matches_validation_metrics_to_the_last_bit():
    g = _gen(77)
    lg, gt = torch.rand(257, 3, generator=g).to(DEV), torch.rand(257, 3, generator=g).to(DEV)
    glg, ggt = torch.rand(2, 3, generator=g).to(DEV), torch.rand(2, 3, generator=g).to(DEV)
    for axis in (None, 0):
        vm = _metrics_of(None, axis, 1.0, 0.5, lg, gt, glg, ggt)
        loss, _ = A.value_loss([(lg, gt, "l2", axis is not None), (glg, ggt, "l2", axis is not None)], (1.0, 0.5))
        assert np.float32(vm["loss"]).view(np.int32) == np.float32(loss.item()).view(np.int32)


# ================================================================================================ 3. gn_adam_step
ADAM_SIZES = (1, 3, 5, 1023, 1025, 4099)
ADAM_GROUPS = (dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2))


def _adam_setup():
    """-> (values, layout): group 0 holds the six sizes and a parameter that never gets a gradient; group 1 the SAME 1025 values twice -- once 16-byte
    aligned, once a contiguous view at storage offset 1 of a larger buffer -- and a 5-element tensor"""
    g = _gen(123)
    vals = [torch.randn(n, generator=g) for n in ADAM_SIZES] + [torch.randn(7, generator=g)]
    twin = torch.randn(1025, generator=g)
    vals += [twin, twin.clone(), torch.randn(5, generator=g)]
    return vals, (list(range(0, 7)), [7, 8, 9])


def _adam_grads(vals, step):
    g = _gen(1000 + step)
    grads = [torch.randn(v.shape, generator=g) * (10.0 ** ((i % 3) - 1)) for i, v in enumerate(vals)]
    grads[8] = grads[7].clone()
    if step == 1:
        grads[1] = torch.zeros_like(grads[1])                   # an all-zero gradient at the first step: the update must be exactly 0
    grads[6] = None                                              # never a gradient
    return grads


def _cpu_adam(vals, layout, dtype, snaps):
    ps = [torch.nn.Parameter(v.clone().to(dtype)) for v in vals]
    opt = torch.optim.Adam([dict(params=[ps[i] for i in idx], **kw) for idx, kw in zip(layout, ADAM_GROUPS)], foreach=False)
    out = {}
    for step in range(1, max(snaps) + 1):
        for p, gr in zip(ps, _adam_grads(vals, step)):
            p.grad = None if gr is None else gr.to(dtype)
        opt.step()
        if step in snaps:
            out[step] = [(p.detach().clone(), opt.state[p].get("exp_avg", torch.zeros(0)).clone(), opt.state[p].get("exp_avg_sq", torch.zeros(0)).clone())
                         for p in ps]
    return out


def test_fused_adam_against_torch_adam(monkeypatch):
    vals, layout = _adam_setup()
    snaps = (1, 2, 10)
    r64, r32 = _cpu_adam(vals, layout, torch.float64, snaps), _cpu_adam(vals, layout, torch.float32, snaps)
    ps = []
    for i, v in enumerate(vals):
        if i == 8:
            buf = torch.zeros(v.numel() + 3, device=DEV)
            p = torch.nn.Parameter(buf[1:1 + v.numel()])
            assert p.is_contiguous() and p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(torch.empty_like(v, device=DEV))
            assert p.data_ptr() % 16 == 0
        with torch.no_grad():
            p.copy_(v)
        ps.append(p)
    opt = FusedAdam([dict(params=[ps[i] for i in idx], **kw) for idx, kw in zip(layout, ADAM_GROUPS)])
    launches = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (launches.append(name), call(name, *a))[1])
    for step in range(1, 11):
        for p, gr in zip(ps, _adam_grads(vals, step)):
            p.grad = None if gr is None else gr.to(DEV)
        tracked = [t for p in ps if p.grad is not None for t in (p,) + ((opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) if opt.state[p] else ())]
        versions = [t._version for t in tracked]
        before = ps[1].detach().clone()
        n0 = len(launches)
        opt.step()
        assert launches[n0:].count("gn_adam_step") == 1, launches[n0:]                      # one launch, whatever the number of tensors
        assert all(t._version > v for t, v in zip(tracked, versions))
        if step == 1:
            assert _bits(ps[1].detach(), before)                                               # zero gradient, no weight decay: exactly no update
            assert not opt.state[ps[1]]["exp_avg"].cpu().view(torch.int32).any()
        if step in snaps:
            for i, p in enumerate(ps):
                if i == 6:
                    continue
                for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
                    ours = p.detach() if k == 0 else opt.state[p][name]
                    _check(f"adam step {step} tensor {i} ({vals[i].numel()}) {name}", r64[step][i][k], r32[step][i][k], ours)
            assert float(opt.state[ps[0]]["step"]) == step and not opt.state[ps[0]]["step"].is_cuda
    # the aligned and the unaligned copy of the same data: identical bits (the float4 path against the scalar one)
    assert _bits(ps[7].detach(), ps[8].detach())
    for name in ("exp_avg", "exp_avg_sq"):
        assert _bits(opt.state[ps[7]][name], opt.state[ps[8]][name])
    # the parameter without a gradient: untouched, no state
    assert _bits(ps[6].detach().cpu(), vals[6]) and len(opt.state[ps[6]]) == 0 and ps[6]._version == 1


def test_fused_adam_step_between_forward_and_backward_raises():
    lin = HipLinear(8, 4).to(DEV)
    x = torch.randn(5, 8, device=DEV)
    opt = FusedAdam(lin)
    y = A.linear(lin, x).sum()
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    stale = lin(x).clone()
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward()
    assert not torch.equal(lin(x), stale)                          # FusedAdam(module) invalidated the inference pack
    # ... and so does an optimiser that was never told the module: the pack follows the tensor versions
    opt = FusedAdam(lin.parameters())
    for p in lin.parameters():
        p.grad = torch.ones_like(p)
    stale = lin(x).clone()
    opt.step()
    assert not torch.equal(lin(x), stale)


# ================================================================================================ the model
def _model(dropout=False, bins=8, seed=5, **kw):
    torch.manual_seed(seed)
    hp = dict(feature_dim=16, batch_norm=True, dropout=dropout, sa1_ratio=0.5, sa1_r=0.25, sa2_ratio=0.25, sa2_r=0.5, fp3_k=1, fp2_k=3, fp1_k=3,
              nocs_bins=bins, learning_rate=1e-3)
    hp.update(kw)
    m = PointNet2NOCS(**hp)
    _randomise_norms(m, _gen(seed + 1))
    return m


def _batch(sizes, seed):
    g = _gen(seed)
    n = sum(sizes)
    return Batch(sizes=sizes, x=torch.rand(n, 3, generator=g), pos=torch.rand(n, 3, generator=g), y=torch.rand(n, 3, generator=g),
                 batch=torch.arange(len(sizes)).repeat_interleave(torch.tensor(sizes)), nocs_grip_point=torch.rand(len(sizes), 3, generator=g))


# ------------------------------------------------------------------------------------------------ 4. real-edge statistics
def test_batchnorm_statistics_run_over_real_edges_only():
    model = _model().to(DEV).train()
    sa1 = model.sa1_module
    sa1.max_num_neighbors, sa1.r = 16, 0.24
    batch = _batch([300], 31).to(DEV)
    before = {k: v.detach().cpu().clone() for k, v in sa1.conv.local_nn.state_dict().items()}
    with R.record_forward() as rec:
        T.pointnet2_nocs_forward(model, batch)
    cidx, slot, S, M = rec["sa"][0]
    assert S == 17 and M == 150
    _, cnt = ops.ball_query(batch.pos.contiguous(), Segments([300], DEV).ptr, cidx.to(DEV, torch.int32), Segments([150], DEV).ptr, sa1.r, 16)
    assert int((cnt == 16).sum()) >= 1 and int((cnt < 16).sum()) >= 1 and int((slot < 0).sum()) >= 1     # a full row of the table, and empty slots
    real = int((slot >= 0).sum())
    stack = sa1.conv.local_nn
    tol = {}
    for i, block in enumerate(stack):
        r = rec["r"][i].cpu()
        assert r.shape[0] == real                                                         # local_nn saw the real edges, and only them
        bn = block[2]
        ref = torch.nn.BatchNorm1d(bn.num_features, eps=bn.eps, momentum=bn.momentum).double()
        with torch.no_grad():
            ref.running_mean.copy_(before[f"{i}.2.running_mean"])
            ref.running_var.copy_(before[f"{i}.2.running_var"])
            ref(r.double())
        assert int(bn.num_batches_tracked) == 1
        for k in ("running_mean", "running_var"):
            got, want = getattr(bn, k).cpu().numpy(), getattr(ref, k).float().numpy()
            ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
            print(f"[train] sa1 block {i} {k} over {real} real edge rows: largest difference {float(ulps.max()):.1f} ulp")
            assert (ulps <= 2).all(), (i, k)                                              # test_gpu_bn_train.py::_check_buffers' tolerance
            tol[(i, k)] = (got, 2 * np.spacing(np.abs(want)))
    # not vacuous: the statistics over ALL slot rows (a zero edge row gives relu(bias)) are further away than that tolerance
    r0 = rec["r"][0].cpu().double()
    empty = torch.relu(stack[0][0].bias.detach().cpu().double()).expand(M * S - real, -1)
    ref = torch.nn.BatchNorm1d(stack[0][2].num_features, eps=stack[0][2].eps, momentum=stack[0][2].momentum).double()
    with torch.no_grad():
        ref.running_mean.copy_(before["0.2.running_mean"])
        ref.running_var.copy_(before["0.2.running_var"])
        ref(torch.cat((r0, empty)))
    for k in ("running_mean", "running_var"):
        got, t = tol[(0, k)]
        assert (np.abs(got.astype(np.float64) - getattr(ref, k).numpy()) > t).any(), k


# ------------------------------------------------------------------------------------------------ 5. the whole model's gradient
def _knn_tables(batch, rec, sizes):
    pos0 = batch.pos
    pos1 = pos0[rec["sa"][0][0].to(DEV)].contiguous()
    pos2 = pos1[rec["sa"][1][0].to(DEV)].contiguous()
    pos3 = torch.zeros(len(sizes[0]), 3, device=DEV)
    segs = [Segments(s, DEV) for s in sizes]
    lv = {3: (pos3, segs[3], pos2, segs[2], 1), 2: (pos2, segs[2], pos1, segs[1], 3), 1: (pos1, segs[1], pos0.contiguous(), segs[0], 3)}
    return {k: tuple(t.cpu() for t in ops.knn_neighbours(ps, ss.ptr, pq, sq.ptr, kk)) for k, (ps, ss, pq, sq, kk) in lv.items()}


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_whole_model_gradient(mode):
    sizes0 = [200, 137]
    cpu_model = _model()
    model = copy.deepcopy(cpu_model).to(DEV)
    model.train(mode == "train")
    batch_cpu = _batch(sizes0, 41)
    batch = batch_cpu.to(DEV)
    buffers = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    with R.record_forward() as rec:
        result = T.pointnet2_nocs_forward(model, batch)
        loss, _ = T.loss_and_sums(model, batch, result)
    loss.backward()
    sizes1 = [ops.fps_count(n, 0.5) for n in sizes0]
    sizes2 = [ops.fps_count(n, 0.25) for n in sizes1]
    assert min(sizes2) >= 2
    sizes = [sizes0, sizes1, sizes2, [1] * len(sizes0)]
    knn = _knn_tables(batch, rec, sizes)
    gmask = (result["global_feature"].detach() > 0).cpu()
    tg = [R.target_bins(batch_cpu.y, 8), R.target_bins(batch_cpu.nocs_grip_point, 8)]

    def restated(dtype):
        P = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in model.named_parameters()}
        net = R.Restated(cpu_model, P, buffers, rec, knn, sizes, gmask, dtype, mode == "train")
        lg, glg = net.forward(batch_cpu.x, batch_cpu.pos)
        ls = R.r_bin_loss([(lg, None), (glg, None)], 8, (model.nocs_loss_weight, model.grip_point_loss_weight), tg)
        names = list(P)
        grads = torch.autograd.grad(ls, [P[k] for k in names])
        return float(ls.detach()), dict(zip(names, grads))
    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    print(f"[train] whole model ({mode}): loss fp64 {l64:.9f}  torch-fp32 {l32:.9f}  hip {loss.item():.9f}")
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64)
    failed = []
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        try:
            _check(f"whole model ({mode}) {name}", g64[name], g32[name], p.grad)
        except AssertionError as e:
            failed.append(str(e.args[0])[:200])
    assert not failed, failed
    if mode == "eval":
        with torch.no_grad():
            a, b = T.pointnet2_nocs_forward(model, batch), model(batch)
        assert all(_bits(a[k], b[k]) for k in ("per_point_features", "per_point_logits", "global_logits", "global_feature"))


# ------------------------------------------------------------------------------------------------ 6. one step, end to end
def _same_params(a, b):
    return all(_bits(p.detach(), q.detach()) for p, q in zip(a.parameters(), b.parameters())) and \
        all(_bits(p.float(), q.float()) for p, q in zip(a.buffers(), b.buffers()))


def test_train_step_end_to_end():
    model = _model().to(DEV).train()
    twin = copy.deepcopy(model)
    batch = _batch([200, 137], 41).to(DEV)
    warm = model.eval()(batch)["per_point_logits"].clone()                  # the inference packs exist before the step: they must not survive it
    model.train()
    metrics = T.train_step(model, model.configure_optimizers(), batch)
    assert set(metrics) == set(T.METRIC_KEYS) and all(math.isfinite(v) for v in metrics.values())
    opt2 = FusedAdam(twin.parameters(), lr=twin.learning_rate)
    loss = twin.training_step(batch)
    loss.backward()
    opt2.step()
    assert np.float32(metrics["loss"]) == np.float32(loss.item())
    assert _same_params(model, twin)
    # the very next inference forward reads the new weights: forward's bits are those of a model freshly loaded with the trained state
    fresh = _model().to(DEV)
    fresh.load_state_dict(model.state_dict())
    out = model.eval()(batch)
    with torch.no_grad():
        composed = T.pointnet2_nocs_forward(model, batch)
    ref = fresh.eval()(batch)
    for k in ("per_point_logits", "global_logits", "per_point_features", "global_feature"):
        assert _bits(out[k], composed[k]) and _bits(out[k], ref[k]), k
    assert not torch.equal(out["per_point_logits"], warm)


def test_twenty_steps_reduce_the_loss_and_repeat_bit_for_bit():
    batch = _batch([200, 137], 43).to(DEV)
    start = _model(seed=9).to(DEV).eval()                                    # eval-mode BatchNorm, dropout off: a fixed objective

    def run():
        model = copy.deepcopy(start)
        opt = FusedAdam(model, lr=1e-3)
        losses = [T.train_step(model, opt, batch)["loss"] for _ in range(20)]
        return losses, model
    la, ma = run()
    lb, mb = run()
    print(f"[train] twenty steps: loss {la[0]:.6f} -> {la[-1]:.6f}")
    assert la[-1] < la[0]
    assert la == lb and _same_params(ma, mb)


# ------------------------------------------------------------------------------------------------ 7. dropout
def test_dropout_wiring():
    model = _model(dropout=True).to(DEV)
    batch = _batch([120, 90], 47).to(DEV)

    def run(seed):
        torch.manual_seed(seed)
        with torch.no_grad():
            return T.pointnet2_nocs_forward(model, batch)
    model.train()
    for m in model.modules():                                                # isolate the dropouts: BatchNorm on its running statistics
        if isinstance(m, torch.nn.BatchNorm1d):
            m.eval()
    a, b, c = run(1), run(2), run(1)
    assert _bits(a["per_point_logits"], c["per_point_logits"]) and _bits(a["global_logits"], c["global_logits"])
    assert not torch.equal(a["per_point_logits"], b["per_point_logits"]) and not torch.equal(a["global_logits"], b["global_logits"])
    assert not torch.equal(a["per_point_features"], b["per_point_features"])
    model.eval()
    d, e = run(1), model(batch)
    assert all(_bits(d[k], e[k]) for k in ("per_point_features", "per_point_logits", "global_logits", "global_feature"))


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_train_main_end_to_end(tmp_path):
    from test_validate_host import write_validation_store
    store, out_dir = tmp_path / "ds.zarr", tmp_path / "out"
    write_validation_store(str(store), 20)
    res = T.main(["--model", "pointnet2", "--zarr_in", str(store), "--output_dir", str(out_dir), "--epochs", "1", "--num_batches", "2",
                  "--batch_size", "2", "--num_pc_sample", "400"])
    rows = list(csv.DictReader(open(out_dir / "train_metrics.csv")))
    assert len(rows) == 2 and all(math.isfinite(float(r["train_loss"])) for r in rows)
    assert len(res["val_epochs"]) == 1 and math.isfinite(res["val_epochs"][0]["val_loss"])
    ck = out_dir / "checkpoints" / "last.ckpt"
    loaded = PointNet2NOCS.load_from_checkpoint(str(ck))
    trained = res["model"].state_dict()
    assert set(loaded.state_dict()) == set(trained)
    assert all(torch.equal(v.cpu(), trained[k].cpu()) for k, v in loaded.state_dict().items())
    saved = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert saved["epoch"] == 0 and set(saved) >= {"state_dict", "hyper_parameters", "optimizer_states", "epoch"}
    opt = FusedAdam(loaded.parameters())
    opt.load_state_dict(saved["optimizer_states"][0])
    st = opt.state[next(loaded.parameters())]
    assert float(st["step"]) == 2.0 and st["exp_avg"].shape == next(loaded.parameters()).shape

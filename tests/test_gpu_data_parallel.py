"""GPU (-m gpu): data-parallel training -- gn_grad_pack (csrc/optim.hip) behind ops.grad_pack, parallel.GradientReducer inside the two train_step's, and
both training CLIs under `python -m torch.distributed.run`.

  1. gn_grad_pack against numpy, bit for bit: np.float32(g) / np.float32(world) is IEEE division, which is __fdiv_rn; world == 1 is the copy.
  2. two ranks on the ONE GPU over gloo (GARMENTNETS_DIST_BACKEND=gloo: the ranks share cuda:0; tests/data_parallel_worker.py) against a replay in this
     process: per step and per rank seed, forward, backward; grad = g0 / 2 + g1 / 2; optimizer.step().  torch.equal on every parameter, exp_avg,
     exp_avg_sq and on rank 0's buffers: for two ranks the sum has one order and / 2 is exact.  Nothing of the kind is claimed for more ranks.
  3. BatchNorm in eval mode, two garments per rank: the reduced gradient of every trained tensor against the FULL-batch gradient of
     tests/pipeline_train_reference.py in fp64 on the CPU, by grad_reference._check (ours <= 4 x torch-fp32 + 1 ulp): both ranks hold two garments and the
     same query counts, so the mean of the shard losses IS the full-batch loss.
  4. the CLIs, two ranks on the one GPU: one csv with world = 2, one checkpoint, rows from rank 0 only, the resident shards, and val_epochs.json against
     an in-process validation of last.ckpt over the whole val subset (n x 2^-52 relative, n the number of val batches: the order of an fp64 sum).
  5. the worker over RCCL, one device per rank: needs two GPUs.

The worker is launched once per backend and its records are shared by the tests that read them.

Measured (MI355X, two ranks on the one GPU over gloo): the replays equal bit for bit; the reduced gradient against the full batch in fp64: ours /
torch-fp32 0.01 - 2.24 over 52 tensors (single process, tests/test_gpu_train_pipeline.py (A) eval: 0.29 - 1.34), the mean of the ranks' losses 4.9e-08
relative from the full batch's.  The worker launch takes 8 s and each CLI launch 7 s, the start-up of two interpreters.  The command-line tests add
`--volume_size` and `--num_pc_sample` (the test store holds one volume size and small clouds) to the arguments of the issue.  With `--resident` the
in-process validation assembles its batches on the device too: a resident batch is the host's bit for bit only where no fp32 rotation is involved
(DESIGN.md "Resident dataset"), and the bound is the order of an fp64 sum, not that.  RCCL: not run (one GPU)."""
import csv
import json
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garmentnets_amd import _lib, ops, parallel, train as T, train_pipeline as TP, validate as V  # noqa: E402
from garmentnets_amd.networks.conv_implicit_wnf import ConvImplicitWNFPipeline  # noqa: E402
from garmentnets_amd.networks.pointnet2_nocs import PointNet2NOCS  # noqa: E402
from grad_reference import _check  # noqa: E402
import data_parallel_worker as W  # noqa: E402
import pipeline_train_reference as PR  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMELS = [1, 3, 4, 5, 4095, 4096, 4097, 2 * 4096 + 3]


# ================================================================================================ 1. the kernel
def _specials(n, rng):
    g = rng.standard_normal(n).astype(np.float32)
    sp = np.array([0.0, -0.0, 1e-41, -3e-45, np.inf, -np.inf, np.nan, 3.0000001, 1.1754944e-38], dtype=np.float32)      # +-0, subnormals, inf, nan, FLT_MIN
    k = min(n, sp.size)
    g[:k] = sp[:k] if n >= sp.size else sp[rng.permutation(sp.size)[:k]]
    return g


def _pack_case(numels, null_at=None, odd_at=None, seed=0):
    """-> (sources on the device [None: the null entry], their host values, offsets, total).  odd_at: that tensor is a contiguous view starting one
    element into a 16-byte aligned allocation (its address is 4 mod 16)"""
    rng = np.random.default_rng(seed)
    host = [_specials(n, rng) for n in numels]
    dev = []
    for i, h in enumerate(host):
        if i == null_at:
            dev.append(None)
        elif i == odd_at:
            base = torch.zeros(h.size + 1, dtype=torch.float32, device=DEV)
            base[1:] = torch.from_numpy(h)
            view = base[1:]
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            dev.append(view)
        else:
            dev.append(torch.from_numpy(h).to(DEV))
            assert dev[-1].data_ptr() % 16 == 0
    offsets, total = parallel.plan_flat(numels)
    return dev, host, offsets, total


def _run_pack(dev, numels, offsets, total, world, tail=8):
    """pack into a buffer of total + tail floats preset to a sentinel; the kernel is told `total` -> the whole buffer's bits on the host"""
    rows = [(None if t is None else t.data_ptr(), off, n) for t, off, n in zip(dev, offsets, numels)]
    table, blocks = ops.grad_pack_table(rows, DEV)
    assert blocks == sum(-(-n // _lib.ADAM_CHUNK) for n in numels)
    flat = torch.full((total + tail,), 7.5, dtype=torch.float32, device=DEV)
    ops.grad_pack(table, len(rows), blocks, flat, world, flat_numel=total)
    torch.cuda.synchronize()
    return flat.cpu().numpy().view(np.uint32)


def _expect(host, numels, offsets, total, world, null_at, tail=8):
    want = np.zeros(total + tail, dtype=np.float32)
    want[total:] = 7.5
    with np.errstate(all="ignore"):
        for i, (h, off, n) in enumerate(zip(host, offsets, numels)):
            if i != null_at:
                want[off:off + n] = h if world == 1 else h / np.float32(world)
    return want.view(np.uint32)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_grad_pack_is_numpy_division_bit_for_bit(world):
    numels = NUMELS + [4097, 6]                       # + the misaligned source (two workgroups, a tail) and the null entry
    odd_at, null_at = len(NUMELS), len(NUMELS) + 1
    dev, host, offsets, total = _pack_case(numels, null_at, odd_at, seed=world)
    got = _run_pack(dev, numels, offsets, total, world)
    want = _expect(host, numels, offsets, total, world, null_at)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (world, bad[:8], got[bad[:8]], want[bad[:8]])
    # said again by region: pads and the null entry are exact +0, the sentinel behind flat_numel is untouched
    f = got.view(np.float32)
    for off, n in zip(offsets, numels):
        assert (got[off + n:off + (n + 3) // 4 * 4] == 0).all()
    assert (got[offsets[null_at]:offsets[null_at] + 8] == 0).all() and (f[total:] == 7.5).all()


@pytest.mark.parametrize("n", [1, 5, 4097])
def test_grad_pack_single_entry(n):
    for odd in (None, 0):
        dev, host, offsets, total = _pack_case([n], None, odd, seed=n)
        assert np.array_equal(_run_pack(dev, [n], offsets, total, 2), _expect(host, [n], offsets, total, 2, None))


def test_grad_pack_never_writes_behind_flat_numel():
    """a table that points behind the buffer it is told of (a caller's mistake) leaves everything from flat_numel on untouched"""
    numels = [4096 + 9]
    dev, host, offsets, total = _pack_case(numels, seed=3)
    short = 4096                                      # flat_numel: the second workgroup's slice lies behind it
    rows = [(dev[0].data_ptr(), 0, numels[0])]
    table, blocks = ops.grad_pack_table(rows, DEV)
    flat = torch.full((total + 8,), 7.5, dtype=torch.float32, device=DEV)
    ops.grad_pack(table, 1, blocks, flat, 1, flat_numel=short)
    got = flat.cpu().numpy()
    assert np.array_equal(got[:short].view(np.uint32), host[0][:short].view(np.uint32)) and (got[short:] == 7.5).all()


# ================================================================================================ 2. two ranks against a replay
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _torchrun(backend, args, timeout):
    env = dict(os.environ, GARMENTNETS_DIST_BACKEND=backend, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port())] + args
    out = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-4000:]
    return out


def _launch_worker(backend, out_dir):
    out = _torchrun(backend, [os.path.join(REPO, "tests", "data_parallel_worker.py"), "--out", str(out_dir)], 600)
    assert out.stdout.count("data_parallel_worker: done") == 1, out.stdout[-2000:]
    return {k: torch.load(os.path.join(str(out_dir), k + ".pt"), map_location="cpu", weights_only=False)
            for k in ("first_rank0", "second_rank0", "eval_rank0", "eval_rank1")}


@pytest.fixture(scope="module")
def gloo_records(tmp_path_factory):
    return _launch_worker("gloo", tmp_path_factory.mktemp("dp_gloo"))


def _replay(module, model, batches):
    """the worker's two steps on ONE model: per step, rank 1's and then rank 0's forward and backward from the buffers the step starts with (training
    BatchNorm normalises with the batch's statistics: the buffers do not reach the gradient, and they end as rank 0's own), then the mean, then Adam"""
    optimizer = model.configure_optimizers()
    params = [p for p in model.parameters()]
    for step in range(W.STEPS):
        start = {k: v.detach().clone() for k, v in model.named_buffers()}
        grads = {}
        for rank in (1, 0):
            with torch.no_grad():
                for k, v in model.named_buffers():
                    v.copy_(start[k])
            optimizer.zero_grad(set_to_none=True)
            torch.manual_seed(W.step_seed(rank, step))
            module.training_step(model, batches(rank, step).to(DEV)).backward()
            grads[rank] = [None if p.grad is None else p.grad.detach().clone() for p in params]
        for p, g0, g1 in zip(params, grads[0], grads[1]):
            assert (g0 is None) == (g1 is None)
            p.grad = None if g0 is None else g0 / 2 + g1 / 2
        optimizer.step()
    return optimizer


def _assert_replayed(record, model, optimizer, frozen=""):
    want = record["state_dict"]
    got = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    assert set(got) == set(want)
    diff = [k for k in want if not torch.equal(got[k], want[k])]
    assert not diff, diff[:6]
    names = {id(p): k for k, p in model.named_parameters()}
    trained = {names[id(p)] for p in model.parameters() if optimizer.state.get(p)}
    assert trained == set(record["adam"]) == set(record["with_grad"]) and trained
    assert not frozen or not any(k.startswith(frozen) for k in trained)
    for p in model.parameters():
        st = optimizer.state.get(p)
        if st:
            r = record["adam"][names[id(p)]]
            assert float(st["step"]) == r["step"] == W.STEPS
            assert torch.equal(st["exp_avg"].cpu(), r["exp_avg"]) and torch.equal(st["exp_avg_sq"].cpu(), r["exp_avg_sq"]), names[id(p)]


def test_two_ranks_first_stage_is_the_replay_bit_for_bit(gloo_records):
    model = W.first_model().to(DEV).requires_grad_(True).train()
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    _assert_replayed(gloo_records["first_rank0"], model, _replay(T, model, W.first_batch))
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v.cpu(), before[k])]
    assert len(moved) > len(before) // 2                                   # (the steps did move the model)


def test_two_ranks_second_stage_is_the_replay_bit_for_bit(gloo_records):
    model = W.second_model().to(DEV).requires_grad_(True).train()
    first = {k: v.detach().cpu().clone() for k, v in model.pointnet2_nocs.state_dict().items()}
    record = gloo_records["second_rank0"]
    _assert_replayed(record, model, _replay(TP, model, W.second_batch), frozen=W.FIRST)
    # the frozen first stage inside the worker's pipeline: untouched, and without a gradient
    assert all(torch.equal(record["state_dict"][W.FIRST + k], v) for k, v in first.items())
    assert not any(k.startswith(W.FIRST) for k in record["with_grad"])


# ================================================================================================ 3. the reduced gradient against the full batch in fp64
def _full_batch_check(records, label):
    r0, r1 = records["eval_rank0"], records["eval_rank1"]
    cpu_model = W.second_model()
    b0, b1 = W.eval_batch(0), W.eval_batch(1)
    cells = len(W.SIZES) * int(np.prod(cpu_model.volume_agg.grid_shape))
    rows, flat = torch.cat((r0["rows"], r1["rows"])), torch.cat((r0["flat"].long(), r1["flat"].long() + cells))
    full = types.SimpleNamespace(**{k: torch.cat((getattr(b0, k), getattr(b1, k))) for k in
                                    ("volume_query_points", "surf_query_points", "mc_surf_query_points", "gt_volume_value", "gt_sim_points",
                                     "is_query_point_on_surf")})
    masks = ([torch.cat(pair) for pair in zip(r0["mlp_masks"], r1["mlp_masks"])], [torch.cat(pair) for pair in zip(r0["conv_masks"], r1["conv_masks"])])
    buffers = {k: v.detach().clone() for k, v in cpu_model.named_buffers()}

    def restated(dtype):
        P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in cpu_model.named_parameters() if not k.startswith(W.FIRST)}
        ls = PR.Restated(cpu_model, P, buffers, dtype, False, masks).loss(rows, flat, full)
        return float(ls.detach()), dict(zip(P, torch.autograd.grad(ls, list(P.values()))))
    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    mean_loss = 0.5 * (r0["loss"] + r1["loss"])
    print(f"[data-parallel] {label}: loss fp64 (full batch) {l64:.9f}  torch-fp32 {l32:.9f}  mean of the ranks' {mean_loss:.9f}  "
          f"relative {abs(mean_loss - l64) / abs(l64):.2e}")
    assert abs(mean_loss - l64) <= 1e-5 * abs(l64)
    assert r0["grads_are_views"] and set(r0["grads"]) == set(g64)
    failed, ratios = [], []
    for name in g64:
        try:
            ratios.append(_check(f"{label} {name}", g64[name], g32[name], r0["grads"][name]))
        except AssertionError as e:
            failed.append(str(e.args[0])[:200])
    print(f"[data-parallel] {label}: {len(g64)} tensors, ours / torch-fp32 {min(ratios):.2f} - {max(ratios):.2f}" if ratios else "no ratios")
    assert not failed, failed


def test_mean_of_shard_gradients_is_the_full_batch_gradient(gloo_records):
    _full_batch_check(gloo_records, "two ranks, gloo, eval")


# ================================================================================================ 4. the command lines
def _json_lines(text):
    out = []
    for line in text.splitlines():
        if line.startswith("{"):
            out.append(json.loads(line))
    return out


def _cli_common(store, out_dir):
    from test_validate_host import VOLUME_SIZE
    return ["--zarr_in", str(store), "--output_dir", str(out_dir), "--volume_size", str(VOLUME_SIZE), "--epochs", "1", "--batch_size", "2",
            "--num_pc_sample", "400"]


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    from test_validate_host import write_validation_store
    path = tmp_path_factory.mktemp("dp_store") / "ds.zarr"
    write_validation_store(str(path), 20)
    return path


def _check_cli_outputs(out, out_dir, resident, dataset_args):
    lines = _json_lines(out.stdout)
    train_rows = [l for l in lines if "batch_idx" in l]
    epoch_rows = [l for l in lines if "epoch" in l and "batch_idx" not in l]
    rows = list(csv.DictReader(open(out_dir / "train_metrics.csv")))
    assert len(rows) == len(train_rows) >= 1 and len(epoch_rows) == 1       # rank 0 prints, rank 1 does not
    assert all(r["world"] == "2" for r in rows) and [int(r["batch_idx"]) for r in rows] == list(range(len(rows)))
    assert [f for f in os.listdir(out_dir / "checkpoints")] == ["last.ckpt"]
    reports = [l for l in lines if "resident_subset" in l]
    if resident:
        a = dataset_args("train")
        train = V.make_dataset(a).subset_indices("train")
        for rank in range(2):
            mine = [l for l in reports if l["rank"] == rank and l["resident_subset"] == "train"]
            assert len(mine) == 1 and mine[0]["indices"] == [int(k) for k in parallel.shard_indices(train, rank, 2)]
    else:
        assert not reports
    return json.load(open(out_dir / "val_epochs.json"))


def _in_process_validation(model, a, batch_size, num_batches, task=False, resident=False):
    """validate.py's loop over the WHOLE val subset in this process, batched as the two ranks batch their shares (resident: assembled on the device from
    each share's ResidentDataset, as the ranks assemble them) -> (garment-weighted means, batches)"""
    from garmentnets_amd.io.resident import ResidentDataset
    a.subset, a.static_epoch_seed = "val", True
    dataset = V.make_dataset(a, volume_task_space=task)
    val = dataset.subset_indices("val")
    rows = []
    for rank in range(2):
        share = parallel.shard_indices(val, rank, 2, pad=False)
        batches = ResidentDataset(dataset, share, torch.device(DEV)).batches(share, batch_size) if resident else None
        rows += V.validation_rows(model, dataset, share, batch_size, num_batches, torch.device(DEV), batches=batches)
    return V.epoch_values(rows), len(rows)


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
def test_train_cli_two_ranks(store, tmp_path, resident):
    out_dir = tmp_path / "out"
    args = ["--model", "pointnet2"] + _cli_common(store, out_dir) + ["--num_batches", "2"] + (["--resident"] if resident else [])
    out = _torchrun("gloo", ["-m", "garmentnets_amd.train"] + args, 900)
    got = _check_cli_outputs(out, out_dir, resident, lambda subset: T.parse_args(args))
    assert len(list(csv.DictReader(open(out_dir / "train_metrics.csv")))) == 2
    model = PointNet2NOCS.load_from_checkpoint(str(out_dir / "checkpoints" / "last.ckpt")).to(DEV).eval().requires_grad_(False)
    want, n = _in_process_validation(model, T.parse_args(args), 2, 2, resident=resident)
    assert len(got) == 1 and set(got[0]) == {"epoch"} | set(want) and n >= 2
    for k, v in want.items():
        assert abs(got[0][k] - v) <= n * 2.0 ** -52 * abs(v), (k, got[0][k], v)


def test_train_pipeline_cli_two_ranks(store, tmp_path):
    out_dir = tmp_path / "out"
    args = _cli_common(store, out_dir) + ["--num_volume_sample", "96", "--num_surface_sample", "80", "--grid", "8", "--num_batches", "1"]
    out = _torchrun("gloo", ["-m", "garmentnets_amd.train_pipeline"] + args, 900)
    got = _check_cli_outputs(out, out_dir, False, None)
    model = ConvImplicitWNFPipeline.load_from_checkpoint(str(out_dir / "checkpoints" / "last.ckpt")).to(DEV).eval().requires_grad_(False)
    model.arith = model.arith.replace(device_packs=True)
    want, n = _in_process_validation(model, TP.parse_args(args), 2, 1, task=model.volume_task_space)
    assert len(got) == 1 and set(got[0]) == {"epoch", "device_packs"} | set(want)
    for k, v in want.items():
        assert abs(got[0][k] - v) <= n * 2.0 ** -52 * abs(v), (k, got[0][k], v)


# ================================================================================================ 5. RCCL
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL needs one device per rank")
def test_two_ranks_over_rccl(tmp_path):
    records = _launch_worker("nccl", tmp_path)
    model = W.first_model().to(DEV).requires_grad_(True).train()
    _assert_replayed(records["first_rank0"], model, _replay(T, model, W.first_batch))
    model = W.second_model().to(DEV).requires_grad_(True).train()
    _assert_replayed(records["second_rank0"], model, _replay(TP, model, W.second_batch), frozen=W.FIRST)
    _full_batch_check(records, "two ranks, RCCL, eval")

"""The data-parallel worker of tests/test_gpu_data_parallel.py: one process per rank under `python -m torch.distributed.run`, and the seeded models and
batches it shares with the pytest process that replays it (imported there as a module; it holds no test).

    python -m torch.distributed.run --nproc-per-node 2 tests/data_parallel_worker.py --out DIR

Three records, every GPU call plain (a dead rank ends the launch through torchrun and the process group's timeout):
  first    two train.train_step's with a GradientReducer on the small first-stage model (dropout on, BatchNorm training, bin loss).  Rank 1 spoils its
           parameters and buffers before broadcast_module, so the result proves the broadcast.  Rank 0 saves parameters, buffers and Adam state.
  second   the same on the small second-stage model, configuration (A) of tests/test_gpu_train_pipeline.py.
  eval     BatchNorm in eval mode: forward, backward and reduce() on two garments per rank; every rank saves what the fp64 restatement is handed (the
           rows and cells of ops.grid_features, the ReLU masks of its forward), rank 0 the reduced gradients.
A rank's batch is a function of (rank, step) alone; torch is seeded with step_seed(rank, step) before each step (the dropout masks)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)

import torch  # noqa: E402

STEPS = 2
SIZES = [200, 137]
AABB = torch.tensor([[[-0.4, -0.4, -0.9], [0.4, 0.4, 0.05]]])
FIRST = "pointnet2_nocs."


def step_seed(rank, step):
    return 1000 + 10 * step + rank


def first_model():
    from test_gpu_train import _model
    return _model(dropout=True)


def first_batch(rank, step):
    from test_gpu_train import _batch
    return _batch(SIZES, 200 + 10 * step + rank)


def second_model():
    from test_train_pipeline_host import small_model
    return small_model(1, planted_nocs=True, reduce_method="max")


def pipeline_batch(seed, sizes=SIZES):
    """tests/test_gpu_train_pipeline.py::_setup's batch of configuration (A) under `seed`"""
    from garmentnets_amd.batch import Batch
    from grad_reference import _gen
    from test_train_pipeline_host import targets
    g = _gen(seed)
    n, nb = sum(sizes), len(sizes)
    pos = torch.rand(n, 3, generator=g)
    t = targets(nb, seed + 1)
    return Batch(sizes=sizes, x=torch.rand(n, 3, generator=g), pos=pos, batch=torch.arange(nb).repeat_interleave(torch.tensor(sizes)),
                 cloth_sim_aabb=AABB.repeat(nb, 1, 1), **vars(t))


def second_batch(rank, step):
    return pipeline_batch(300 + 10 * step + rank)


def eval_batch(rank):
    """the batches of tests/test_gpu_train_pipeline.py's own gradient and twenty-step tests (seeds 41 and 43): two garments of 200 and 137 points each"""
    return pipeline_batch((41, 43)[rank])


def state_of(model, optimizer):
    """what rank 0 saves of a record: every parameter and buffer, and exp_avg / exp_avg_sq / step by parameter name"""
    adam = {}
    for name, p in model.named_parameters():
        st = optimizer.state.get(p, {})
        if st:
            adam[name] = {"exp_avg": st["exp_avg"].cpu(), "exp_avg_sq": st["exp_avg_sq"].cpu(), "step": float(st["step"])}
    return {"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "adam": adam,
            "with_grad": [k for k, p in model.named_parameters() if p.grad is not None]}


def grid_rows(model, batch):
    """-> (how many bare-ReLU gn_linear calls the frozen first stage makes, the rows and cells ops.grid_features hands the aggregator)"""
    from garmentnets_amd import ops, train_pipeline as TP
    import pipeline_train_reference as PR
    with PR.record_second_stage() as rec:
        p2 = TP.first_stage(model, batch)
    nd, agg = p2["nocs_data"], model.volume_agg
    rows, flat = ops.grid_features(nd.x, nd.pos.contiguous(), nd.sim_points.float().contiguous(), nd.pred_confidence.contiguous(), nd.batch,
                                   agg.lower_corner, agg.upper_corner, agg.grid_shape, True, True)
    return len(rec["r"]), rows.cpu().contiguous(), flat.cpu()


def _steps(module, model, batches, ranks, out, name):
    from garmentnets_amd import parallel
    if ranks.rank != 0:                                     # rank 0's values must arrive: the replay starts from them
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                t.add_(1)
    parallel.broadcast_module(model)
    optimizer = model.configure_optimizers()
    reducer = parallel.GradientReducer(optimizer, ranks.backend, names=model)
    for step in range(STEPS):
        torch.manual_seed(step_seed(ranks.rank, step))
        module.train_step(model, optimizer, batches(ranks.rank, step).to(ranks.device), reducer=reducer)
    if ranks.rank == 0:
        torch.save(state_of(model, optimizer), os.path.join(out, name + "_rank0.pt"))


def _eval_record(ranks, out):
    from garmentnets_amd import parallel, train_pipeline as TP
    from garmentnets_amd.optim import FusedAdam
    import pipeline_train_reference as PR
    model = second_model().to(ranks.device).requires_grad_(True).eval()
    batch = eval_batch(ranks.rank).to(ranks.device)
    skip, rows, flat = grid_rows(model, batch)
    with PR.record_second_stage() as rec:
        result = TP.pipeline_forward(model, batch)
        loss, _ = TP.loss_and_sums(model, batch, result)
    loss.backward()
    reducer = parallel.GradientReducer(FusedAdam(model, lr=1e-3), ranks.backend, names=model)
    reducer.reduce()
    record = {"rows": rows, "flat": flat, "mlp_masks": [(r > 0).cpu() for r in rec["r"][skip:]], "conv_masks": rec["conv"], "loss": float(loss)}
    if ranks.rank == 0:
        record["grads"] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters() if p.grad is not None}
        record["grads_are_views"] = all(p.grad.untyped_storage().data_ptr() == reducer.flat.untyped_storage().data_ptr()
                                        for p in model.parameters() if p.grad is not None)
    torch.save(record, os.path.join(out, f"eval_rank{ranks.rank}.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from garmentnets_amd import parallel, train as T, train_pipeline as TP
    ranks = parallel.training_ranks(0)
    assert ranks.world > 1, "run under torch.distributed.run"
    _steps(T, first_model().to(ranks.device).requires_grad_(True).train(), first_batch, ranks, a.out, "first")
    _steps(TP, second_model().to(ranks.device).requires_grad_(True).train(), second_batch, ranks, a.out, "second")
    _eval_record(ranks, a.out)
    parallel.finish()
    if ranks.rank == 0:
        print("data_parallel_worker: done", flush=True)


if __name__ == "__main__":
    main()

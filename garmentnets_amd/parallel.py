"""Multi-GPU plumbing: one process per GPU, garments sharded over the ranks.

Inference has NO data-path collective.  The path shards by garment: every op is segmented by example and the 30 MB of weights are
replicated, so garment batches never move between GPUs.  The only collective is an all-gather of a small fixed-size metrics vector per rank (RCCL
over xGMI on GPUs, gloo in the CPU tests) -- latency-bound, bandwidth irrelevant.

Training is data-parallel ("Data-parallel training"): every rank holds the whole model and a fixed share of the train subset
(shard_indices), and a step has ONE collective, the all-reduce of one flat gradient buffer:

  broadcast_module(model)        every parameter and buffer from rank 0, once
  GradientReducer(optimizer)     reduce() between backward() and optimizer.step(): ops.grad_pack (csrc/optim.hip gn_grad_pack: every gradient divided
                                 by the world size into its 16-byte aligned slice of the buffer, one launch) -> all-reduce (sum) -> p.grad becomes a
                                 view of the buffer.  RCCL reduces the device buffer in place; gloo goes through one pinned host buffer.
"""
import datetime
import os

import numpy as np
import torch
import torch.distributed as dist

METRIC_SLOTS = 8   # [garments, seconds, + 6 spare per-stage slots]
INIT_TIMEOUT = 120.0   # seconds: a collective whose peer died raises on the others instead of hanging them


def env_rank_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def init(backend=None, device=None, timeout=INIT_TIMEOUT):
    """Initialise torch.distributed from the torchrun environment (no-op for a single process).  timeout: seconds a collective waits for its peers"""
    rank, local_rank, world = env_rank_world()
    if world > 1 and not dist.is_initialized():
        backend = backend or ("nccl" if torch.cuda.is_available() else "gloo")   # "nccl" IS RCCL on ROCm
        kw = {"device_id": device} if (backend == "nccl" and device is not None) else {}
        dist.init_process_group(backend=backend, timeout=datetime.timedelta(seconds=float(timeout)), **kw)
    return rank, local_rank, world


def dist_backend():
    """the backend the training loop asks for: GARMENTNETS_DIST_BACKEND, "nccl" (RCCL) by default; "gloo" lets ranks share a device (bench.py's rule)"""
    return os.environ.get("GARMENTNETS_DIST_BACKEND", "nccl")


def rank_device(local_rank, backend):
    """the device index of a local rank: its own under RCCL, local_rank % device_count under gloo (bench.py's rule)"""
    return local_rank if backend == "nccl" else local_rank % max(1, torch.cuda.device_count())


def shard_range(total, rank, world):
    """Contiguous slice [lo, hi) of `total` garments owned by `rank`; remainders go to the lowest ranks."""
    base, rem = divmod(int(total), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_batch(global_batch, n_points, seed, rank, world, colour="uniform"):
    """this rank's contiguous shard of the seeded GLOBAL batch of synthetic garments (BASELINE config[3]: 128 garments over 8 GPUs):
    -> (Batch on the host with batch ids restarting at 0, (lo, hi)).  Garment g of the global batch depends on (seed, g) only, so the
    concatenation of the shards over the ranks IS synthetic_cloud(global_batch, n_points, seed) -- tests/test_parallel_cpu.py."""
    from . import synthetic
    from .batch import Batch
    lo, hi = shard_range(global_batch, rank, world)
    x, pos, batch = synthetic.synthetic_cloud(hi - lo, n_points, seed=seed, first=lo, colour=colour)
    return Batch(sizes=[n_points] * (hi - lo), x=x, pos=pos, batch=batch), (lo, hi)


def _parse_cpulist(text):
    cpus = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus.extend(range(int(lo), int(hi or lo) + 1))
    return cpus


def local_cpus_of_device(index):
    """host cores on the NUMA node of HIP device `index` (sysfs local_cpulist of its PCI function) or None when sysfs does not tell"""
    try:
        p = torch.cuda.get_device_properties(index)
        bdf = "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        import glob
        for d in glob.glob(f"/sys/bus/pci/devices/{bdf}.*"):
            cpus = _parse_cpulist(open(os.path.join(d, "local_cpulist")).read())
            if cpus:
                return cpus
    except Exception:
        pass
    return None


def plan_affinity(local_rank, local_world, device_of_rank, cpus_of_device, allowed):
    """pure planning (tested on CPU): the cores rank `local_rank` of `local_world` local ranks should run on.  Every rank takes its
    device's NUMA-local cores (restricted to `allowed`, the process's current mask); ranks whose devices share a core list split it into
    equal contiguous slices in rank order, so that eight host-side tails (mesh slicing, pinned D2H, Python) never pile onto one node's
    cores.  -> sorted list of cores (never empty)"""
    allowed = sorted(allowed)
    lists = []
    for r in range(local_world):
        cpus = cpus_of_device(device_of_rank(r))
        cpus = [c for c in (cpus or allowed) if c in set(allowed)] or allowed
        lists.append(tuple(cpus))
    mine = lists[local_rank]
    peers = [r for r in range(local_world) if lists[r] == mine]
    k, n = peers.index(local_rank), len(peers)
    per = max(1, len(mine) // n)
    sl = list(mine[k * per:(k + 1) * per]) if k * per < len(mine) else [mine[k % len(mine)]]
    return sl or list(mine)


def pin_rank(local_rank, local_world, device_index, max_threads=8):
    """bind this process to its GPU's NUMA-local share of the host cores (plan_affinity) and size torch's CPU thread pool to it.
    -> description dict for the bench line; never raises (a container without sched_setaffinity keeps its mask)"""
    info = {"pinned": False}
    try:
        allowed = os.sched_getaffinity(0)
        ndev = max(1, torch.cuda.device_count())
        cores = plan_affinity(local_rank, local_world, lambda r: r % ndev, local_cpus_of_device, allowed)
        os.sched_setaffinity(0, cores)
        torch.set_num_threads(max(1, min(max_threads, len(cores))))
        info.update(pinned=True, cores=len(cores), first_core=cores[0], last_core=cores[-1], torch_threads=torch.get_num_threads(),
                    numa_local=local_cpus_of_device(device_index) is not None)
    except Exception as e:      # noqa: BLE001
        info["why_not"] = repr(e)
    return info


def barrier():
    if dist.is_initialized():
        dist.barrier()


def finish():
    """leave the process group (the end of a training CLI under torch.distributed.run); nothing for a single process"""
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def gather_metrics(values, device="cpu"):
    """all-gather a short list of floats from every rank -> list (per rank) of lists."""
    v = list(values) + [0.0] * (METRIC_SLOTS - len(values))
    assert len(v) == METRIC_SLOTS
    t = torch.tensor(v, dtype=torch.float64, device=device)
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return [t.tolist()]
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [o.tolist() for o in out]


def gather_vector(values, device="cpu"):
    """all-gather an equal-length list of floats from every rank -> list (per rank) of lists (bench.py: the per-garment result
    checksums of every shard, so that rank 0 can print them in global garment order)"""
    t = torch.tensor(list(values), dtype=torch.float64, device=device)
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return [t.tolist()]
    out = [torch.zeros_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [o.tolist() for o in out]


def aggregate_throughput(per_rank):
    """per_rank: [[garments, seconds, ...], ...] -> (whole-job garments/s with the MAX time over ranks, max seconds)."""
    garments = sum(r[0] for r in per_rank)
    tmax = max(r[1] for r in per_rank)
    return garments / tmax, tmax


# ------------------------------------------------------------------------------------------------ data-parallel training
def plan_flat(numels):
    """pure planning: where each tensor of `numels` elements starts in one flat fp32 buffer.  Every offset is rounded up to 4 floats (16 bytes: the
    pack kernel's stores and the optimiser's loads of the views are 16 bytes wide) -> (offsets, total), total a multiple of 4"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += (int(n) + 3) // 4 * 4
    return offsets, at


def shard_indices(indices, rank, world, pad=True):
    """pure planning: this rank's FIXED share of a subset, indices[rank::world].  pad: the list is first wrapped with its own head to a multiple of
    `world`, so that every rank takes the same number of steps (a rank with fewer would leave the others waiting in the all-reduce); without it the
    shares partition the list exactly (validation: no collective inside the loop).  The share holds for the whole run and an epoch shuffles inside it
    (train_loop.epoch_order over the share), so a rank's resident dataset is 1 / world of the subset -- not DistributedSampler's rule, which deals a
    global permutation out anew every epoch and so needs every rank to reach every sample."""
    if world == 1:
        return indices
    n = len(indices)
    padded = -(-n // world) * world if (pad and n) else n
    picked = [i % n for i in range(padded)][rank::world]
    if isinstance(indices, (list, tuple)):
        return [indices[i] for i in picked]
    return np.asarray(indices)[np.asarray(picked, dtype=np.int64)]


def all_reduce_sum(flat, backend=None, staging=None):
    """sum `flat` over the ranks, in place -> flat.  RCCL ("nccl") and host tensors are reduced where they lie; a device tensor under gloo goes through
    `staging` (a pinned host tensor of flat's size; allocated here when None): D2H, all_reduce, H2D -- gloo's device support is not needed"""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return flat
    backend = backend or dist.get_backend()
    if not flat.is_cuda or backend == "nccl":
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        return flat
    if staging is None:
        staging = torch.empty(flat.shape, dtype=flat.dtype, pin_memory=True)
    staging.copy_(flat)
    dist.all_reduce(staging, op=dist.ReduceOp.SUM)
    flat.copy_(staging)
    return flat


def agree_layout(layout):
    """one all_gather_object of this rank's [(index, numel)] layout; a rank that differs from rank 0 raises the SAME RuntimeError on every rank"""
    layout = [(int(i), int(n)) for i, n in layout]
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return layout
    seen = [None] * dist.get_world_size()
    dist.all_gather_object(seen, layout)
    bad = [r for r, other in enumerate(seen) if other != seen[0]]
    if bad:
        r = bad[0]
        diff = sorted(set(seen[0]) ^ set(seen[r]))[:4]
        raise RuntimeError(f"GradientReducer: the ranks disagree on the gradient layout: rank 0 has {len(seen[0])} tensors, rank {r} has {len(seen[r])}; "
                           f"(index, numel) in one and not in the other: {diff}")
    return layout


def _broadcast_tensors(tensors, src):
    """rank `src`'s values into `tensors` on every rank: one broadcast per dtype (through the host under gloo).  The in-place copies bump the
    version counters, as FusedAdam.step does: the next forward rebuilds its packs from the new values (components.mlp.generation)"""
    gloo = dist.get_backend() != "nccl"
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault(t.dtype, []).append(t)
    for dtype, tensors in by_dtype.items():
        flat = torch.cat([t.detach().reshape(-1) for t in tensors])
        if gloo:
            flat = flat.cpu()
        dist.broadcast(flat, src=src)
        if dist.get_rank() != src:
            at = 0
            for t in tensors:
                t.copy_(flat[at:at + t.numel()].view(t.shape))
                at += t.numel()


@torch.no_grad()
def broadcast_module(model, src=0):
    """every parameter and buffer of `model` becomes rank `src`'s, once, before the first step"""
    if dist.is_initialized() and dist.get_world_size() > 1:
        _broadcast_tensors(list(model.parameters()) + list(model.buffers()), src)
    return model


@torch.no_grad()
def borrow_buffers(model, src=0):
    """validation of a data-parallel run: every rank takes rank `src`'s buffers (the BatchNorm running statistics the checkpoint holds: the epoch's
    values then describe that checkpoint) -> this rank's own, for restore_buffers.  One collective per dtype, before the validation loop, none inside"""
    own = [b.detach().clone() for b in model.buffers()]
    if dist.is_initialized() and dist.get_world_size() > 1:
        _broadcast_tensors(list(model.buffers()), src)
    return own


@torch.no_grad()
def restore_buffers(model, own):
    """the buffers borrow_buffers set aside go back: training goes on with this rank's own running statistics"""
    for b, mine in zip(model.buffers(), own):
        b.copy_(mine)


class GradientReducer:
    """the mean of the ranks' gradients, between backward() and optimizer.step() (the module docstring).

    The layout is fixed by the first reduce(): the optimiser's parameters whose grad is not None, in the optimiser's order (a frozen first stage stays
    out, as it stays out of FusedAdam), agreed between the ranks (agree_layout).  The flat buffer and the device table are allocated once; the table is
    uploaded again only when a gradient's address changed (FusedAdam._launch's rule).  After reduce() every p.grad of the layout is a view of the
    buffer: there is no unpack launch, and FusedAdam reads the views.  names: a module (its named_parameters) or {id(parameter): name}, for the errors"""

    def __init__(self, optimizer, backend=None, names=None):
        self.optimizer = optimizer
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.backend = backend or (dist.get_backend() if dist.is_initialized() else None)
        if isinstance(names, torch.nn.Module):
            names = {id(p): k for k, p in names.named_parameters()}
        self._names = names or {}
        self._layout = None           # [(index in the optimiser's order, numel)]
        self._offsets = self.flat = self._staging = self._table = self._key = None
        self._blocks = 0

    def _params(self):
        return [p for group in self.optimizer.param_groups for p in group["params"]]

    def _name(self, i, p):
        return self._names.get(id(p), f"parameter {i} of the optimiser, shape {tuple(p.shape)}")

    def _first(self, params):
        live = [(i, p) for i, p in enumerate(params) if p.grad is not None]
        self._layout = agree_layout([(i, p.numel()) for i, p in live])
        if not live:
            raise RuntimeError("GradientReducer: no parameter of the optimiser has a gradient")
        self._offsets, total = plan_flat([n for _, n in self._layout])
        dev = live[0][1].grad.device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        if self.backend != "nccl":
            self._staging = torch.empty(total, dtype=torch.float32, pin_memory=True)

    def reduce(self):
        if self.world == 1:
            return
        from . import ops
        params = self._params()
        if self._layout is None:
            self._first(params)
        inside = {i for i, _ in self._layout}
        for i, p in enumerate(params):
            if (p.grad is None) == (i in inside):
                raise RuntimeError(f"GradientReducer: {self._name(i, p)} " + ("has no gradient in this step but had one in the first" if i in inside else
                                                                               "has a gradient in this step but had none in the first") +
                                   ": the layout of the flat buffer is fixed by the first step")
        rows = []
        for (i, n), off in zip(self._layout, self._offsets):
            g = params[i].grad
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != params[i].shape or g.device != self.flat.device:
                raise TypeError(f"GradientReducer: the gradient of {self._name(i, params[i])} must be contiguous torch.float32 of the parameter's shape, "
                                f"on {self.flat.device}")
            rows.append((g.data_ptr(), off, n))
        key = tuple(r[0] for r in rows)
        if key != self._key:
            self._table, self._blocks = ops.grad_pack_table(rows, self.flat.device)
            self._key = key
        ops.grad_pack(self._table, len(rows), self._blocks, self.flat, self.world)
        all_reduce_sum(self.flat, self.backend, self._staging)
        for (i, n), off in zip(self._layout, self._offsets):
            params[i].grad = self.flat[off:off + n].view_as(params[i])


def training_ranks(gpu_id=0):
    """what the training loop needs to know of its place (train_loop.py) -> namespace(rank, local_rank, world, device, backend, metrics_device,
    affinity).  One process (no torchrun): cuda:<gpu_id>, nothing initialised.  WORLD_SIZE > 1: the device is LOCAL_RANK's (rank_device), the process
    group is initialised with the timeout and the process pinned to its device's cores"""
    import types
    rank, local_rank, world = env_rank_world()
    if world == 1:
        return types.SimpleNamespace(rank=0, local_rank=0, world=1, device=torch.device("cuda:{}".format(gpu_id)), backend=None, metrics_device="cpu",
                                     affinity=None)
    backend = dist_backend()
    index = rank_device(local_rank, backend)
    device = torch.device("cuda", index)
    torch.cuda.set_device(device)
    init(backend=backend, device=device)
    affinity = pin_rank(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)), index)
    return types.SimpleNamespace(rank=rank, local_rank=local_rank, world=world, device=device, backend=backend,
                                 metrics_device=device if backend == "nccl" else "cpu", affinity=affinity)


def gather_epoch_values(rows, device="cpu"):
    """validate.epoch_values over the rows of EVERY rank: each rank's (value x garments, garments) sums go through gather_vector and every rank forms
    the garment-weighted mean over the whole subset.  A rank without rows (a subset shorter than the world) adds nothing and returns {}"""
    keys = [k for k in rows[0] if k.startswith("val_")] if rows else []
    width = int(max(r[0] for r in gather_vector([len(keys)], device)))
    w = np.array([r["garments"] for r in rows], dtype=np.float64)
    mine = [float(np.sum(w))] + [float(np.sum(w * np.array([r[k] for r in rows], dtype=np.float64))) for k in keys]
    per_rank = gather_vector(mine + [0.0] * (1 + width - len(mine)), device)
    total = sum(r[0] for r in per_rank)
    return {k: sum(r[1 + j] for r in per_rank) / total for j, k in enumerate(keys)}

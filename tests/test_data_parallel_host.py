"""CPU: the host side of data-parallel training -- parallel.plan_flat / shard_indices (pure), gn_grad_pack's header, prototype, export and its refusals
before any launch, the all-reduce helper and the layout agreement over gloo with two spawned processes, and the training loops' signatures."""
import ctypes
import inspect
import os
import re
import socket

import pytest
import torch
import torch.multiprocessing as mp

from garmentnets_amd import _lib, parallel, train as T, train_pipeline as TP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the pure planners
def test_plan_flat_aligns_every_slice():
    numels = [1, 3, 4, 5, 4095, 4096, 4097]
    offsets, total = parallel.plan_flat(numels)
    assert len(offsets) == len(numels) and offsets[0] == 0 and total % 4 == 0
    assert all(off % 4 == 0 for off in offsets)
    ends = [off + n for off, n in zip(offsets, numels)]
    assert all(end <= nxt for end, nxt in zip(ends, offsets[1:] + [total]))              # no overlap, and the last slice fits
    assert all(nxt - end < 4 for end, nxt in zip(ends, offsets[1:] + [total]))           # the pad is the rounding and no more
    assert parallel.plan_flat([]) == ([], 0) and parallel.plan_flat([8]) == ([0], 8)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9])
def test_shard_indices(n, world):
    indices = [100 + 3 * i for i in range(n)]
    padded = [parallel.shard_indices(indices, r, world, pad=True) for r in range(world)]
    exact = [parallel.shard_indices(indices, r, world, pad=False) for r in range(world)]
    assert len({len(s) for s in padded}) == 1 and len(padded[0]) == -(-n // world)       # equal length: every rank takes the same number of steps
    assert set(k for s in padded for k in s) == set(indices)
    assert sorted(k for s in exact for k in s) == indices                                # an exact partition
    assert all(list(s) == indices[r::world] for r, s in enumerate(exact))
    assert all(list(p[:len(e)]) == list(e) for p, e in zip(padded, exact))               # the pad comes behind a rank's own share, from the list's head
    if world == 1:
        assert padded[0] is indices and exact[0] is indices
    import numpy as np
    arr = parallel.shard_indices(np.asarray(indices, dtype=np.int64), world - 1, world)
    assert [int(k) for k in arr] == list(padded[world - 1])


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_prototype_and_export_agree():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    assert "gn_grad_pack" in set(re.findall(r"\b(gn_[a-z0-9_]+)\s*\(", hdr))
    assert re.search(r"int gn_grad_pack\(const GnPackEntry \*table, int n_entries, int64_t n_blocks,\s*float \*flat, int64_t flat_numel, int world, "
                     r"void \*stream\);", hdr)
    assert _lib.PROTOTYPES["gn_grad_pack"] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    assert hasattr(_lib.load(), "gn_grad_pack")
    # GnPackEntry { const void *src; int64_t dst_off; int64_t numel; int64_t blk0; }
    assert [f[0] for f in _lib.PackEntry._fields_] == ["src", "dst_off", "numel", "blk0"] and ctypes.sizeof(_lib.PackEntry) == 32
    assert re.search(r"const void \*src;[^}]*int64_t dst_off;[^}]*int64_t numel;[^}]*int64_t blk0;[^}]*\} GnPackEntry;", hdr)
    assert _lib.ADAM_CHUNK == int(re.search(r"#define GN_ADAM_CHUNK (\d+)", hdr).group(1))


def test_refusals_before_any_launch():
    c = _lib.call
    table, flat = ctypes.c_void_p(4096), ctypes.c_void_p(8192)       # (never dereferenced: every case is refused before a launch)
    with pytest.raises(ValueError, match="required"):
        c("gn_grad_pack", None, 1, 1, flat, 8, 1, None)
    with pytest.raises(ValueError, match="required"):
        c("gn_grad_pack", table, 1, 1, None, 8, 1, None)
    with pytest.raises(ValueError, match="n_entries"):
        c("gn_grad_pack", table, 0, 1, flat, 8, 1, None)
    with pytest.raises(ValueError, match="world"):
        c("gn_grad_pack", table, 1, 1, flat, 8, 0, None)
    for blocks in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="n_blocks"):
            c("gn_grad_pack", table, 1, blocks, flat, 8, 1, None)
    for numel in (6, 1, -4):
        with pytest.raises(ValueError, match="multiple of 4"):
            c("gn_grad_pack", table, 1, 1, flat, numel, 1, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        c("gn_grad_pack", table, 1, 1, ctypes.c_void_p(8196), 8, 1, None)


# ------------------------------------------------------------------------------------------------ gloo, two processes, host tensors
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    parallel.init(backend="gloo", timeout=60)
    t = torch.arange(10, dtype=torch.float32) * (1 + rank) + 0.25 * rank
    summed = parallel.all_reduce_sum(t.clone())
    same = parallel.agree_layout([(0, 4), (2, 4097)])
    try:
        parallel.agree_layout([(0, 4), (2, 4097)] if rank == 0 else [(0, 4)])
        error = None
    except RuntimeError as e:
        error = str(e)
    q.put((rank, summed.tolist(), same, error))
    parallel.finish()


def test_two_rank_gloo_all_reduce_and_layout_agreement():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = torch.arange(10, dtype=torch.float32), torch.arange(10, dtype=torch.float32) * 2 + 0.25
    assert res[0][1] == res[1][1] == (a + b).tolist()
    assert res[0][2] == res[1][2] == [(0, 4), (2, 4097)]
    assert res[0][3] is not None and res[0][3] == res[1][3] and "disagree" in res[0][3] and "(2, 4097)" in res[0][3]


def test_single_process_reducer_is_a_no_op():
    p = torch.nn.Parameter(torch.ones(5))
    opt = torch.optim.SGD([p], lr=0.1)
    reducer = parallel.GradientReducer(opt)
    p.grad = torch.full((5,), 2.0)
    grad = p.grad
    assert reducer.world == 1 and reducer.reduce() is None
    assert p.grad is grad and reducer.flat is None                   # nothing allocated, nothing launched (this process has no GPU library call to make)
    assert parallel.all_reduce_sum(grad) is grad and parallel.agree_layout([(0, 5)]) == [(0, 5)]
    assert parallel.broadcast_module(torch.nn.Linear(2, 2)) is not None


# ------------------------------------------------------------------------------------------------ signatures
def test_train_steps_take_a_reducer_and_the_parsers_keep_their_defaults():
    for module in (T, TP):
        sig = inspect.signature(module.train_step)
        assert list(sig.parameters)[:4] == ["model", "optimizer", "batch", "monitor"]
        assert sig.parameters["reducer"].default is None and sig.parameters["monitor"].default is None
    assert inspect.signature(parallel.init).parameters["timeout"].default == 120.0
    a = T.build_parser().parse_args(["--zarr_in", "x.zarr"])
    assert (a.batch_size, a.subset, a.epochs, a.learning_rate, a.seed, a.resident, a.resident_gib, a.shuffle, a.gpu_id) == \
        (8, "train", 1, None, 0, False, None, False, 0)
    b = TP.build_parser().parse_args(["--zarr_in", "x.zarr"])
    assert (b.model, b.batch_size, b.subset, b.epochs, b.learning_rate, b.seed, b.resident, b.shuffle, b.host_packs, b.split_backward, b.gpu_id) == \
        ("pipeline", 24, "train", 1, None, 0, False, False, False, False, 0)
    assert not hasattr(a, "world") and not hasattr(b, "world")        # the world comes from torch.distributed.run's environment, not from a flag

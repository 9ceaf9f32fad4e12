"""No wrapper's entry writes past the workspace its size entry asks for.  Every wrapper whose entry carves a workspace of more than one part
(GnCarve, csrc/common.h) runs once with ops._ws handing out the first nbytes bytes of a larger buffer whose last 64 KiB are a guard pattern: the
guard must come back untouched and the outputs must equal those of a plain run, bit for bit.  The shapes are the smallest at which a carve can go
wrong: odd counts, so that every alignment pad is there.  The guard is memory the test allocated: nothing here can fault."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cloth_collision_cases as CC  # noqa: E402
from garmentnets_amd import cloth, ops  # noqa: E402

DEV = "cuda:0"
GUARD, PATTERN = 64 * 1024, 0xA5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _cells(g, n, cells):
    return torch.randint(0, cells, (n,), generator=g).to(torch.int32).to(DEV)


def mc33_batch():
    vols = torch.rand(2, 5, 6, 7, generator=_gen(1)).to(DEV)
    verts, faces, normals, values, counts = ops.mc33_batch(vols, 0.5, 3 * 5 * 6 * 7, 5 * 4 * 5 * 6)
    out = [counts]
    for b, (nv, nf) in enumerate(counts.tolist()):           # rows past a volume's counts are not results
        assert nv > 0 and nf > 0
        out += [verts[b, :nv], faces[b, :nf], normals[b, :nv], values[b, :nv]]
    return out


def mesh_compact():
    g = _gen(2)
    verts, faces = _rand(g, 5, 3), torch.randint(0, 5, (7, 3), generator=g).to(torch.int32).to(DEV)
    return ops.mesh_compact(verts, faces, torch.tensor([1, 1, 0, 1, 1], dtype=torch.bool, device=DEV))


def mesh_largest_component():
    faces = torch.tensor([[0, 2, 4], [1, 3, 1], [4, 2, 0]], dtype=torch.int32, device=DEV)
    return ops.mesh_largest_component(faces, 5, with_labels=True)


def _strip(V, seed):
    """a triangle strip of V vertices, two rows a cell apart, with contacts on"""
    i = np.arange(V)
    X = np.stack([(i // 2) * CC.CELL, (i % 2) * CC.CELL, np.zeros(V)], axis=1) + np.random.default_rng(seed).uniform(-0.1, 0.1, (V, 3)) * CC.CELL
    faces = np.stack([i[:-2], i[1:-1], i[2:]], axis=1).astype(np.int32)
    return cloth.garment(X, faces, 0, CC.params())


def cloth_contact_lists():
    return ops.cloth_contact_lists([_strip(5, 3), _strip(7, 4)], device=DEV)


def cloth_simulate_batch():
    states, stats = ops.cloth_simulate_batch([_strip(5, 3), _strip(7, 4)], 2, device=DEV, stats=True)
    assert any(s["contact_active"] or s["contact_max_list"] for s in stats)
    return states, stats


def _scatter_inputs(seed):
    g = _gen(seed)
    return _rand(g, 7, 4), _cells(g, 7, 27)


def grid_scatter_bwd_max():
    src, flat = _scatter_inputs(5)
    vol = ops.grid_scatter(src, flat, 1, (3, 3, 3), "max")
    return ops.grid_scatter_bwd(_rand(_gen(6), 1, 3, 3, 3, 4), flat, 7, "max", vol=vol, src=src)


def grid_scatter_mul():
    src, flat = _scatter_inputs(7)
    return ops.grid_scatter(src, flat, 1, (3, 3, 3), "mul")


def knn_interpolate_bwd():
    g = _gen(8)
    ps, pq = _rand(g, 7, 3), _rand(g, 5, 3)
    ptr_s, ptr_q = torch.tensor([0, 7], dtype=torch.int32, device=DEV), torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    nbr, d2 = ops.knn_neighbours(ps, ptr_s, pq, ptr_q, 3)
    return ops.knn_interpolate_bwd(_rand(g, 5, 4), nbr, d2, 7)


def trilinear_sample_bwd():
    g = _gen(9)
    vol, query = _rand(g, 1, 3, 4, 5, 4), torch.rand(1, 5, 3, generator=g).to(DEV)
    return ops.trilinear_sample_bwd(_rand(g, 1, 5, 4), vol, query, want_vol=True, want_query=True)


def sa_gather_bwd():
    g = _gen(10)
    slot_src = torch.tensor([0, 4, -1, 2, 2, 0, 3], dtype=torch.int32, device=DEV)
    return ops.sa_gather_bwd(_rand(g, 7, 8), slot_src, 4, 5)


def query_targets_batch():
    g = _gen(11)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1], [0, 3, 4], [1, 4, 2]], dtype=torch.int32, device=DEV)
    meshes = [(_rand(g, 4, 3), faces[:3].contiguous()), (_rand(g, 5, 3), faces)]
    return ops.query_targets_batch(_rand(g, 2, 5, 3), meshes, "nocs_signed_distance_field", return_fp64=True)


def conv3d_bwd_weight_split():
    g = _gen(12)
    src0, dy = _rand(g, 3, 8, 8, 8, 16), _rand(g, 3, 8, 8, 8, 32)
    a, d = (0.5 + torch.rand(3, 16, generator=g)).to(DEV), (0.3 * torch.randn(3, 16, generator=g)).to(DEV)
    return ops.conv3d_bwd_weight_split(src0, None, a, d, _rand(g, 3, 8, 8, 8, 32), dy)


def conv_affine_pack():
    g = _gen(13)
    w = (torch.randn(32, 16, 3, 3, 3, generator=g) / (27 * 16) ** 0.5).to(DEV)
    x = torch.randn(1, 4, 4, 4, 16, generator=g).double()
    a, d = (0.5 + torch.rand(1, 16, generator=g)).to(DEV), (0.3 * torch.randn(1, 16, generator=g)).to(DEV)
    r = ops.conv_affine_pack(w, a, d, (x.sum(dim=(1, 2, 3)).to(DEV), (x ** 2).sum(dim=(1, 2, 3)).to(DEV), 64))
    return r.pack, r.stage_a, r.stage_d, r.out_scale, r.kbias


def conv3d_gcr_split_occupancy():
    from garmentnets_amd.components.unet3d import _class_constants
    g = _gen(14)
    B, C0, Cout, dims = 2, 16, 32, (8, 8, 8)
    x = torch.zeros(B, *dims, C0)
    x[0, 0, 0, 0] = torch.randn(C0, generator=g).abs() * 3.0                # one occupied cell: garment 0's first tile is the only active one
    flat = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = torch.randn(Cout, C0, 3, 3, 3, generator=g) / (27 * C0) ** 0.5
    s = torch.tensor([1.0, 0.5], device=DEV)
    a, d = ((0.5 + torch.rand(B, C0, generator=g)).to(DEV) * s[:, None]).contiguous(), ((0.3 * torch.randn(B, C0, generator=g)).to(DEV) * s[:, None]).contiguous()
    pack = ops.pack_conv_weight_split(w, ops.SPLIT_F16X2).to(DEV)
    launch = lambda v, **kw: ops.conv3d_gcr_split(v, None, a, d, pack, Cout, relu=True, act_inv=(1.0 / s).contiguous(), **kw)   # noqa: E731
    small = launch(torch.zeros((B, 5, 5, 5, C0), dtype=torch.float32, device=DEV))
    flags = ops.grid_tile_flags(flat, B, dims, 1)
    assert flags.sum().item() == 1
    return launch(x.to(DEV), tile_active=flags, kconst=_class_constants(small, 1, Cout), kreach=1)


CASES = [mc33_batch, mesh_compact, mesh_largest_component, cloth_contact_lists, cloth_simulate_batch, grid_scatter_bwd_max, knn_interpolate_bwd,
         trilinear_sample_bwd, sa_gather_bwd, grid_scatter_mul, query_targets_batch, conv3d_bwd_weight_split, conv_affine_pack,
         conv3d_gcr_split_occupancy]


def _flat(out):
    """the tensors and plain values of a wrapper's result, in order"""
    if isinstance(out, dict):
        out = [out[k] for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [x for o in out for x in _flat(o)]
    return [out]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__ for c in CASES])
def test_no_write_past_the_workspace(case, monkeypatch):
    plain = _flat(case())
    handed = []

    def guarded_ws(nbytes, device, zero=False):
        n = max(int(nbytes), 1)
        buf = torch.empty(n + GUARD, dtype=torch.uint8, device=device)       # the window starts where the allocation does: same alignment
        buf[n:] = PATTERN
        if zero:
            buf[:n] = 0
        handed.append((buf, n))
        return buf[:n]

    monkeypatch.setattr(ops, "_ws", guarded_ws)
    got = _flat(case())
    assert handed, "the wrapper allocated no workspace through ops._ws"
    for buf, n in handed:
        assert bool((buf[n:] == PATTERN).all()), f"{case.__name__}: a write past the end of a workspace of {n} bytes"
    assert len(got) == len(plain)
    for k, (x, y) in enumerate(zip(got, plain)):
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and torch.equal(x, y), (case.__name__, k)
        else:
            assert x == y, (case.__name__, k)

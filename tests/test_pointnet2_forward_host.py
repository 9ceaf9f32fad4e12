"""CPU (no launch): what tests/test_gpu_pointnet2_forward_edges.py stands on.  The new entries gn_sa_fused_group / gn_sa_fused_auto_group are
exported and prototyped; the argument checks of gn_sa_fused_group and gn_linear refuse by message before any launch; the fp64 PointConv restatement
(grad_reference.r_point_conv, which forms its slots from the ball-query table alone) equals r_sa_gather -> MLP -> r_segment_max over slots written
out by an explicit loop; the numpy ball-query loop (grad_reference.ball_query_loop) equals the C oracle on every input the GPU file uses.

The C oracle takes any K (its row length is an argument), so the oracle itself is the yardstick of the GPU file at every K, 65, 100 and 130 included;
the loop is held to it here at every one of them and serves the GPU file as a second, independent statement.

The inputs of the ball-query cases live here (the GPU file imports them): `tiny_examples` -- examples of 1, 2, 63, 64, 65 and 129 points in one
ragged batch, every point a centre -- and `lattice_cloud` -- coordinates that are multiples of 0.25, where squared distances of exactly 0.25 = r^2
occur at r = 0.5."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
from garmentnets_amd import _lib
from grad_reference import _gen, ball_query_loop, point_conv_slots, r_point_conv, r_sa_gather, r_segment_max

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BQ_SIZES = [1, 2, 63, 64, 65, 129]
BQ_K = [1, 7, 63, 64, 65, 100, 130]


# ------------------------------------------------------------------------------------------------ inputs shared with the GPU file
def _ptr(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def tiny_examples(seed=11):
    """-> pos (N, 3) float32 in the unit cube, ptr, centre_idx (every point), centre_ptr"""
    n = sum(BQ_SIZES)
    pos = torch.rand(n, 3, generator=_gen(seed)).numpy()
    return pos, _ptr(BQ_SIZES), np.arange(n, dtype=np.int64), _ptr(BQ_SIZES)


def lattice_cloud(seed=12):
    """two examples, the 125 points of {0, .25, .5, .75, 1}^3 and the 64 of {0, .25, .5, .75}^3, each in a shuffled order, every point a centre"""
    g = _gen(seed)
    parts = []
    for n in (5, 4):
        a = torch.arange(n, dtype=torch.float32) * 0.25
        p = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
        parts.append(p[torch.randperm(len(p), generator=g)])
    sizes = [len(p) for p in parts]
    n = sum(sizes)
    return torch.cat(parts).numpy(), _ptr(sizes), np.arange(n, dtype=np.int64), _ptr(sizes)


def on_the_radius(pos, ptr, centre_idx, centre_ptr, r):
    """(centre, point) pairs of one example whose float32 squared distance equals float32(r r)"""
    r2 = np.float32(float(r) * float(r))
    pairs = []
    for b in range(len(ptr) - 1):
        for c in range(int(centre_ptr[b]), int(centre_ptr[b + 1])):
            d = pos[ptr[b]:ptr[b + 1]] - pos[centre_idx[c]][None, :]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            pairs += [(c, int(ptr[b]) + int(j)) for j in np.nonzero(d2 == r2)[0]]
    return pairs


# ------------------------------------------------------------------------------------------------ the entries
def test_group_entries_are_declared_prototyped_and_exported():
    hdr = open(os.path.join(REPO, "include", "garmentnets_hip.h")).read()
    lib = _lib.load()
    for name in ("gn_sa_fused_group", "gn_sa_fused_auto_group"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    # the arguments of gn_sa_fused_scoped, then the group
    assert _lib.PROTOTYPES["gn_sa_fused_group"] == _lib.PROTOTYPES["gn_sa_fused_scoped"] + [ctypes.c_int]
    for c, dims in ((3, (64, 64, 128)), (128, (128, 128, 256))):
        for M in (0, 1, 750, 1920, 3000, 12000, 48000):
            assert lib.gn_sa_fused_auto_group(c, *dims, M) in (2, 4, 8, 16, 32), (c, M)
    assert lib.gn_sa_fused_auto_group(5, 64, 64, 128, 100) == _lib.GN_EINVAL
    assert "not instantiated" in lib.gn_last_error().decode()


def _sa_call(x=0x1000, ldx=128, C=128, M=0, K=64, dims=(128, 128, 256), ldo=256, group=0, entry="gn_sa_fused_group"):
    """argument checks only: the pointers are numbers that are never followed (a refusal, or M == 0, returns before any launch)"""
    vp = ctypes.c_void_p
    args = [vp(x), ldx, C, vp(0x2000), vp(0x3000), vp(0x4000), vp(0x5000), M, K, 1, None, vp(0x6000), vp(0x7000), vp(0x8000), vp(0x9000),
            dims[0], dims[1], dims[2], vp(0xa000), ldo, None]
    return _lib.call(entry, *(args + [group] if entry == "gn_sa_fused_group" else args))


@pytest.mark.parametrize("kwargs,message", [
    (dict(group=3), "group 3 is not one of"), (dict(group=-2), "group -2"), (dict(group=64), "group 64"), (dict(group=1), "group 1 "),
    (dict(K=65), "at most 64 neighbours"), (dict(K=0), "bad sizes"), (dict(ldo=255), "bad sizes"),
    (dict(C=5, ldx=8, dims=(64, 64, 128), ldo=128), "[5+3,64,64,128] is not instantiated"), (dict(dims=(128, 128, 96)), "not instantiated"),
    (dict(ldx=130), "16-byte aligned"), (dict(ldx=127), "16-byte aligned"),
    (dict(x=0x1004), "16-byte aligned base"), (dict(x=0x1008), "16-byte aligned base"), (dict(x=0), "16-byte aligned"),
    (dict(x=0x1004, C=64, ldx=64, dims=(64, 64, 128), ldo=128), "16-byte aligned base"),
])
def test_sa_fused_refusals_by_message(kwargs, message):
    for M in (0, 5):                                   # refused before the M == 0 return and before any launch
        with pytest.raises(ValueError) as e:
            _sa_call(M=M, **kwargs)
        assert message in str(e.value), str(e.value)


def test_sa_fused_accepts_what_it_must_without_a_launch():
    for group in (0, 2, 4, 8, 16, 32):
        assert _sa_call(group=group) == _lib.GN_OK
    assert _sa_call(entry="gn_sa_fused_scoped") == _lib.GN_OK
    # C < 8 is read word by word: neither the base nor the row length is bound to 16 bytes; C == 0 has no feature pointer at all
    assert _sa_call(x=0x1004, C=3, ldx=3, dims=(64, 64, 128), ldo=130) == _lib.GN_OK
    assert _sa_call(x=0, C=0, ldx=0, dims=(64, 64, 128), ldo=128) == _lib.GN_OK
    # the forwarding entries refuse the same way
    with pytest.raises(ValueError) as e:
        _sa_call(x=0x1004, entry="gn_sa_fused_scoped")
    assert "16-byte aligned base" in str(e.value)


def test_linear_refuses_a_scale_without_a_shift():
    vp = ctypes.c_void_p
    for sc, sh in ((vp(0x3000), None), (None, vp(0x3000))):
        with pytest.raises(ValueError) as e:
            _lib.call("gn_linear", vp(0x1000), 8, vp(0x2000), 8, None, sc, sh, 0, 4, 4, 8, vp(0x4000), 4, None)
        assert "must come together" in str(e.value)
    assert _lib.call("gn_linear", vp(0x1000), 8, vp(0x2000), 8, None, vp(0x3000), vp(0x3000), 0, 0, 4, 8, vp(0x4000), 4, None) == _lib.GN_OK   # M == 0


# ------------------------------------------------------------------------------------------------ the PointConv restatement
def _blocks(dims, g, zero_and_negative=True, last_shift=None):
    """three (w, b, sc, sh) blocks for the widths dims = [k, n1, n2, n3]; in every block scale 0 is negative and scale 1 exactly zero"""
    out = []
    for i in range(3):
        k, n = dims[i], dims[i + 1]
        w, b = torch.randn(n, k, generator=g) / k ** 0.5, 0.3 * torch.randn(n, generator=g)
        sc, sh = 0.5 + torch.rand(n, generator=g), 0.3 * torch.randn(n, generator=g)
        if zero_and_negative:
            sc[0::5] *= -1.0
            sc[1] = 0.0
        if last_shift is not None and i == 2:
            sh[:] = last_shift
        out.append((w, b, sc, sh))
    return out


def test_point_conv_restatement_against_gather_mlp_segment_max():
    g = _gen(5)
    sizes, C, K = [25, 15], 5, 8
    n = sum(sizes)
    pos, x = torch.rand(n, 3, generator=g), torch.randn(n, C, generator=g)
    centre_idx = torch.tensor([0, 3, 4, 9, 11, 17, 20, 24, 25, 30, 33, 39], dtype=torch.int32)
    M = len(centre_idx)
    nbr, cnt = ball_query_loop(pos.numpy(), _ptr(sizes), centre_idx.numpy(), np.array([0, 8, 12]), 0.7, K)
    assert cnt.max() == K and cnt.min() < K
    full = [c for c in range(M) if cnt[c] == K]
    nbr[full[0], 0], nbr[full[1], K - 1], nbr[full[2], 3] = full[0], full[1], full[2]       # the centre's own number in its own row
    cnt[5], nbr[5] = 0, -1                                                                    # an empty ball
    self_src = torch.tensor([7, 1, 2, 3, 5, 6, 8, 10, 26, 27, 28, 29], dtype=torch.int32)
    nbr[6, 2], nbr[9, 1] = int(self_src[6]), int(self_src[9])                                  # ... and the scoped node in two rows
    blocks = _blocks([C + 3, 32, 32, 64], g)
    assert all(float(b[2][0]) < 0 and float(b[2][1]) == 0 for b in blocks)
    for self_loops in (True, False):
        for src in (None, self_src):
            for xin in (x, None):
                bl = blocks if xin is not None else [(blocks[0][0][:, C:],) + blocks[0][1:]] + blocks[1:]
                ours = r_point_conv(xin, pos, centre_idx, nbr, cnt, self_loops, None if src is None else src.numpy(), bl, torch.float64)
                # the slots by an explicit loop
                S = K + (1 if self_loops else 0)
                slot_src = torch.full((M, S), -1, dtype=torch.int64)
                removed = 0
                for c in range(M):
                    node = c if src is None else int(src[c])
                    for s in range(int(cnt[c])):
                        if self_loops and int(nbr[c, s]) == node:
                            removed += 1
                        else:
                            slot_src[c, s] = int(nbr[c, s])
                    if self_loops:
                        slot_src[c, K] = node
                assert removed >= (0 if not self_loops else (3 if src is None else 2)), removed   # the planted ones, and what the table held by itself
                assert np.array_equal(point_conv_slots(nbr, cnt, self_loops, None if src is None else src.numpy()), slot_src.numpy())
                h = r_sa_gather(None if xin is None else xin.double(), pos.double(), centre_idx, slot_src.reshape(-1), S)
                for w, b, sc, sh in bl:
                    h = torch.relu(h @ w.double().t() + b.double()) * sc.double() + sh.double()
                ref = r_segment_max(h, slot_src.reshape(-1), M, S)
                assert ours.dtype == torch.float64 and ours.shape == (M, 64)
                assert float((ours - ref).abs().max()) <= 1e-13 * float(ref.abs().max())       # the same fp64 operations, at most another BLAS blocking
                if self_loops:
                    assert bool((ours[5] != 0).any())                                           # the empty ball: the self edge alone
                else:
                    assert bool((ours[5] == 0).all())                                           # ... or nothing: an exact zero row
                has_edge = torch.from_numpy((slot_src.numpy() >= 0).any(1))
                assert bool((ours[has_edge, 1] == blocks[2][3][1].double()).all())              # a zero scale leaves the shift itself


# ------------------------------------------------------------------------------------------------ the ball-query loop against the C oracle
@pytest.mark.parametrize("K", BQ_K)
def test_ball_query_loop_is_the_oracle_on_the_tiny_examples(K):
    pos, ptr, cidx, cptr = tiny_examples()
    for r in (0.0, 0.3, 10.0):
        nbr, cnt = ball_query_loop(pos, ptr, cidx, cptr, r, K)
        onbr, ocnt = O.ball_query(pos, ptr, cidx, cptr, r, K)
        assert np.array_equal(cnt, ocnt) and np.array_equal(nbr, onbr), (K, r)
        if r == 0.0:
            assert not cnt.any() and (nbr == -1).all()
        if r == 10.0:                                     # every row is the first K indices of its example
            for b, n in enumerate(BQ_SIZES):
                want = np.full(K, -1)
                want[:min(n, K)] = ptr[b] + np.arange(min(n, K))
                assert (nbr[cptr[b]:cptr[b + 1]] == want[None, :]).all() and (cnt[cptr[b]:cptr[b + 1]] == min(n, K)).all()
        if r == 0.3:
            assert cnt.min() >= 1 and (K == 1 or (cnt < K).any())


@pytest.mark.parametrize("K", BQ_K)
def test_ball_query_loop_is_the_oracle_on_the_lattice(K):
    pos, ptr, cidx, cptr = lattice_cloud()
    pairs = on_the_radius(pos, ptr, cidx, cptr, 0.5)
    assert len(pairs) >= 100                              # squared distances of exactly r^2 = 0.25 occur ...
    nbr, cnt = ball_query_loop(pos, ptr, cidx, cptr, 0.5, K)
    onbr, ocnt = O.ball_query(pos, ptr, cidx, cptr, 0.5, K)
    assert np.array_equal(cnt, ocnt) and np.array_equal(nbr, onbr)
    assert not any(j in onbr[c] for c, j in pairs)        # ... and the oracle excludes every one of them (strict <)
    if K >= 27:
        assert cnt.max() == 27 and cnt.min() == 8         # the 3 x 3 x 3 block round an inner point, the 2 x 2 x 2 one at a corner
    else:
        assert (cnt == K).all()

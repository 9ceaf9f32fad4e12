"""GPU (-m gpu): the PointNet++ forward kernels -- gn_sa_fused (csrc/sa_fused.hip), gn_linear (csrc/linear.hip), gn_ball_query and gn_nocs_head
(csrc/points.hip) -- on every dispatch branch and at the tails, strides, counts and ties where they could be wrong while tests/test_gpu_parity.py
stays green.  Method and helpers of tests/test_gpu_autograd_edges.py: operands "contiguous" and "wide" (a column slice of a wider NaN buffer), `_bits`,
and the project's rule grad_reference._check (ours against fp64 <= 4 x (the same restatement in torch-fp32 against fp64, measured in the test) + 1 ulp;
it prints the `[grad-error]` line with the ratio before it asserts).  No tolerance here is a constant, except gn_nocs_head's confidence, which keeps
the tolerance of tests/test_gpu_parity.py::test_nocs_head.  tests/test_pointnet2_forward_host.py holds, on the CPU, what this file stands on: the fp64
PointConv restatement against gather -> MLP -> segment max, the numpy ball-query loop against the C oracle (which takes any K), the refusals.

gn_linear's bound is derived, elementwise (test_linear_* below).  With u = 2^-24: the accumulator of an output is a chain of K exact-product
additions in fp32 in some order, the bias one more, K + 1 roundings in all, so |r^ - r| <= ((1 + u)^(K+1) - 1) (|x| . |w| + |b|), which is below
E = (K + 3) u (|x| . |w| + |b|) for every K here (the two spare u also pay for the second-order terms); the ReLU is exact and 1-Lipschitz; the affine
y^ = fl(fl(r^ sc) + sh) adds |sc| E + u |r^ sc| + u (|r^ sc| + |sh|): the issue's bound |sc| E + u (|sc r| + |sh|) holds because the second
u |sc r| is covered by the spare 2 u |sc| (|x| . |w| + |b|) >= 2 u |sc r| inside |sc| E.  Printed per test: max error / bound, and the ratio of our
largest error to torch-fp32's.

The self-loop rule.  With the maximum as the aggregation, REMOVING the table entry that names node c is not observable while self-loops are on: the
removed edge (node c -> centre c) is the very edge add_self_loops puts back, and a maximum does not count.  What IS observable and asserted in
test_sa_fused_self_loop_rule: with self-loops on, the result with node c planted in row c (slots 0, 31, 32, 63; literal and through self_src) has the
bits of the result with that slot emptied, and matches fp64; with self-loops off the planted entry is an ordinary neighbour and MUST contribute -- its
features are scaled so that it wins the maximum, and the row must equal the fp64 row that contains it, far from the one without it.

Measured (MI355X).  gn_sa_fused against fp64, ours / torch-fp32 under the rule, over the 144 checks of this file: 0.58 - 1.71 (the shipped
[3+3, 64, 64, 128] 0.79 - 1.27, [128+3, 128, 128, 256] 0.77 - 1.27; the largest, 1.71, is [128+3, 128, 256, 256] at M = 1); on the same inputs
sa_fused 1.06 / 1.06 and 1.13 / 1.14 (self-loops on / off) beside the unfused chain's 1.00 / 1.00 and 1.00 / 1.00.  gn_linear: largest error at most
0.71 of the derived bound (K = 1; 0.023 at K = 131), 0.98 - 1.31 of torch-fp32's largest error.  The cost rule's group on a 256-CU part with 2
resident workgroups per CU: [3+3, 64, 64, 128] 3000 centres -> 4, 48000 -> 32; [128+3, 128, 128, 256] 750 -> 2, 12000 -> 8.

Mutation record (MI355X; 9 one-line mutants of csrc/sa_fused.hip, csrc/linear.hip and ball_query_kernel, each built as a library of its own apart
from the tree and run once against the tests of this file named below; every mutant stays inside every buffer on those tests -- the K-wide tables
of test_sa_fused_table_widths sit at the head of a taller one for that reason, and the linear operands are slices of wider buffers.  On the
unchanged library all 128 tests of this file pass.)
    1. sa_fused_kernel, an invalid slot contributes 0 instead of -inf to the maximum: fails test_sa_fused_all_negative_outputs (both),
       test_sa_fused_ball_sizes_0_1_31_32_33_64 (both) and test_sa_fused_every_shape_every_group_against_fp64[3-64-64-128-*] (run on these).
    2. sa_fused_kernel, `cnt <= 32 * half` -> `cnt <= 32 * half + 1` (a ball of 1 and the 33rd neighbour are lost): fails
       test_sa_fused_ball_sizes_0_1_31_32_33_64 (both), test_sa_fused_table_widths (all seven K) and
       test_sa_fused_every_shape_every_group_against_fp64[3-64-64-128-*].  The other direction, `cnt < 32 * half`, is HARMLESS BY CONSTRUCTION and was
       not built: it runs the second tile of a ball of exactly 32, whose 32 slots are all -1 and masked.
    3. sa_fused_kernel, the removal applied with self-loops off too (`p.self_loops &&` dropped): fails test_sa_fused_self_loop_rule (all four) and
       test_sa_fused_every_shape_every_group_against_fp64[3-64-64-128-False]; [3-64-64-128-True] passes as it must.  The suggested mutant "the
       comparison removed" is HARMLESS BY CONSTRUCTION with self-loops on (see above: the removed edge is the self edge) and was not built.
    4. sa_fused_kernel, `slot < p.K` removed (a row of K columns read as 64): fails test_sa_fused_table_widths[1, 16, 31, 33, 63]; K = 32 and 64
       pass as they must (slots 32 .. 63 are read only when cnt > 32).
    5. sa_fused_kernel, the self edge taken from the centre's own number although self_src is given: fails test_sa_fused_self_loop_rule[*-self_src];
       [*-literal] and test_sa_fused_ball_sizes_0_1_31_32_33_64 pass as they must (no self_src).
    6. linear.hip, float4 loader without `if (k + 2 >= K) v.z = 0.f`: fails test_linear_tails_and_layouts for every case with K mod 4 in {1, 2}
       (K = 17: all M and N tails; K = 1, 2, 5, 33) and test_linear_epilogue (all eight, K = 17); K = 3, 4, 15, 16, 31, 131 pass as they must.
    7. linear.hip, scalar loader reading p[1] without `k + 1 < K`: fails the same cases but K = 2, which passes as it must with K = 3, 4, 15, 16, 31, 131
       (only K mod 4 == 1 ends a group after its first element).
    8. ball_query_kernel, `d < r2` -> `d <= r2`: fails test_ball_query_excludes_points_exactly_on_the_radius (all seven K) and
       test_ball_query_tiny_examples_every_radius (all seven K: at r = 0 the centre itself has d == r2).
    9. ball_query_kernel, the -1 fill started one slot late: fails test_ball_query_tiny_examples_every_radius (all seven K) and
       test_ball_query_excludes_points_exactly_on_the_radius[63, 64, 65, 100, 130]; [1] and [7] pass as they must (every lattice ball holds at least 8
       points: the row is full).
   Not built: a moved dispatch threshold of gn_linear or another choice of sa_fused's cost rule.  Both are HARMLESS BY CONSTRUCTION for the values:
   test_linear_bits_do_not_depend_on_variant_or_loader and the six-group comparison of every sa_fused test assert that every variant gives the same
   bits, so the thresholds decide speed alone (test_linear_every_tile_variant restates the dispatch and runs both sides of each threshold).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
from garmentnets_amd import _lib, ops  # noqa: E402
from garmentnets_amd.components.pointnet2 import Segments  # noqa: E402
from oracle import pipeline as P  # noqa: E402
from grad_reference import _check, _gen, ball_query_loop, r_point_conv  # noqa: E402
from test_gpu_autograd import DEV  # noqa: E402
from test_gpu_autograd_edges import _bits, _no_nan, _operand  # noqa: E402
from test_pointnet2_forward_host import BQ_K, BQ_SIZES, _blocks, lattice_cloud, on_the_radius, tiny_examples  # noqa: E402

U = 2.0 ** -24
GROUPS = (0, 2, 4, 8, 16, 32)
SA_SHAPES = [(3, 64, 64, 128), (128, 128, 128, 256), (3, 32, 32, 64), (3, 32, 64, 128), (3, 64, 64, 64), (3, 64, 128, 128), (64, 64, 64, 128),
             (64, 64, 128, 256), (128, 128, 128, 128), (128, 128, 256, 256), (0, 64, 64, 128)]          # SA_SHAPES of csrc/sa_fused.hip
SHIPPED = SA_SHAPES[:2]
_id = lambda s: "-".join(str(v) for v in s)


def _wide(t, off, width, tall=2):
    """t (rows, C) -> the same values on the GPU as columns off..off+C of a (rows + tall, width) NaN buffer (`_operand`'s "wide" at a chosen offset)"""
    t = t.detach().cpu().float()
    rows, C = t.shape
    assert off + C <= width
    buf = torch.full((rows + tall, width), float("nan"), dtype=torch.float32)
    buf[:rows, off:off + C] = t
    return buf.to(DEV)[:rows, off:off + C]


def _nan_out(rows, C, off=4, extra=8):
    """-> (buffer, view): a (rows + 2, C + extra) NaN buffer on the GPU and its [rows, off:off+C] window"""
    buf = torch.full((rows + 2, C + extra), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:rows, off:off + C]


def _outside_is_nan(buf, rows, C, off=4):
    mask = torch.ones(buf.shape, dtype=torch.bool)
    mask[:rows, off:off + C] = False
    return bool(torch.isnan(buf.cpu()[mask]).all())


# ================================================================================================ gn_sa_fused
SA_SIZES, SA_RATIO, SA_RADIUS = [300, 37, 1, 130], 0.5, 0.15


@functools.lru_cache(maxsize=None)
def _sa_case():
    """the ragged cloud [300, 37, 1, 130] (each example a blob whose points are spread over 0.01 .. 0.4 of its size: dense and sparse regions), the
    GPU's fps centres and its K = 64 ball-query table at a radius that gives capped balls, balls of 1 and everything between"""
    g = _gen(21)
    ps = []
    for n in SA_SIZES:
        sig = torch.exp(torch.rand(n, 1, generator=g) * np.log(40.0)) * 0.01
        ps.append(0.5 + sig * torch.randn(n, 3, generator=g))
    pos = torch.cat(ps)
    seg = Segments(SA_SIZES, DEV)
    counts = [ops.fps_count(n, SA_RATIO) for n in SA_SIZES]
    cseg = Segments(counts, DEV)
    pos_d = pos.to(DEV)
    cidx = ops.fps(pos_d, seg.ptr, cseg.ptr, max(SA_SIZES), sum(counts))
    nbr, cnt = ops.ball_query(pos_d, seg.ptr, cidx, cseg.ptr, SA_RADIUS, 64)
    c = cnt.cpu().numpy()
    M = len(c)
    assert M == 235 and M % 32 != 0
    assert c.max() == 64 and (c == 64).sum() >= 24 and (c == 1).sum() >= 10 and ((c > 1) & (c < 32)).any() and ((c > 32) & (c < 64)).any()
    return dict(pos=pos, pos_d=pos_d, seg=seg, cseg=cseg, cidx=cidx, cidx_c=cidx.cpu(), nbr=nbr, cnt=cnt, nbr_c=nbr.cpu().numpy(), cnt_c=c, M=M,
                N=pos.shape[0], capped=[int(i) for i in np.nonzero(c == 64)[0]])


def _features(cin, seed):
    """point features (N, cin) on the CPU (None for cin == 0)"""
    return torch.randn(sum(SA_SIZES), cin, generator=_gen(seed)) if cin else None


def _x_dev(x, layout="contiguous"):
    """the features on the GPU: rows of pad4(C) floats from a 16-byte aligned base ("contiguous") or a slice at column 4 of a wider NaN buffer whose
    row length is a multiple of 4 ("wide": the 16-byte contract holds, NaN on both sides of every row)"""
    if x is None:
        return None
    C = x.shape[1]
    if layout == "wide":
        xd = _wide(x, 4, ops.pad4(C) + 8)
    else:
        xd = ops.new_rows(x.shape[0], C, DEV)
        xd.copy_(x.to(DEV))
    assert C < 8 or (xd.data_ptr() % 16 == 0 and xd.stride(0) % 4 == 0)
    return xd


def _sa(T, xd, pack, self_loops, nbr=None, cnt=None, M=None, **kw):
    nbr, cnt = T["nbr"] if nbr is None else nbr, T["cnt"] if cnt is None else cnt
    M = T["M"] if M is None else M
    if "self_src" in kw and kw["self_src"] is not None:
        kw["self_src"] = kw["self_src"][:M].contiguous()
    return ops.sa_fused(xd, T["pos_d"], T["cidx"][:M].contiguous(), nbr[:M].contiguous(), cnt[:M].contiguous(), pack, self_loops=self_loops, **kw)


def _ref(T, x, blocks, self_loops, nbr=None, cnt=None, self_src=None):
    """(fp64, torch-fp32) restatements on the CPU"""
    nbr, cnt = T["nbr_c"] if nbr is None else nbr, T["cnt_c"] if cnt is None else cnt
    return tuple(r_point_conv(x, T["pos"], T["cidx_c"], nbr, cnt, self_loops, self_src, blocks, dt) for dt in (torch.float64, torch.float32))


def _dev_table(nbr, cnt):
    return torch.from_numpy(np.ascontiguousarray(nbr, np.int32)).to(DEV), torch.from_numpy(np.ascontiguousarray(cnt, np.int32)).to(DEV)


@pytest.mark.parametrize("self_loops", [True, False])
@pytest.mark.parametrize("shape", SA_SHAPES, ids=_id)
def test_sa_fused_every_shape_every_group_against_fp64(shape, self_loops):
    """every instantiated edge MLP, M = 1, 32, 33 and the natural 235 (7 groups of 32 and 11 centres), each under every forced group and the cost
    rule: six results with the same bits, held to fp64; every BatchNorm has negative scales and one exactly 0"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    assert ops.sa_fused_supported(cin, dims)
    x = _features(cin, 30 + cin)
    blocks = _blocks([cin + 3] + dims, _gen(sum(shape)))
    pack = ops.pack_sa_fused(blocks).to(DEV)
    xd = _x_dev(x)
    r64, r32 = _ref(T, x, blocks, self_loops)
    nat = None
    for M in (T["M"], 1, 32, 33):
        outs = [_sa(T, xd, pack, self_loops, M=M, group=G) for G in GROUPS]
        for G, o in zip(GROUPS[1:], outs[1:]):
            assert _bits(outs[0], o), f"group {G} differs from the cost rule's at M = {M}"
        nat = outs[0] if nat is None else nat
        assert _bits(outs[0], nat[:M]), M                                      # a centre's row does not depend on how many centres follow
        _check(f"sa_fused {_id(shape)} self_loops={self_loops} M={M}", r64[:M], r32[:M], outs[0])
    zero_scale = blocks[2][3][1]
    assert bool((nat[:, 1].cpu() == zero_scale).all())                         # a zero scale in the last block leaves the shift itself


def test_sa_fused_auto_group_record():
    """the group the cost rule takes for the two shipped edge MLPs at the centre counts of batch 1 and batch 16 (a record, printed)"""
    for (cin, *dims), per_garment in zip(SHIPPED, (3000, 750)):
        for batch in (1, 16):
            g = ops.sa_fused_auto_group(cin, dims, per_garment * batch)
            print(f"[sa-group] edge MLP {cin}+3-{_id(dims)}: {per_garment * batch} centres (batch {batch}) -> G = {g}")
            assert g in GROUPS[1:]
    with pytest.raises(ValueError):
        ops.sa_fused_auto_group(5, [64, 64, 128], 100)


@pytest.mark.parametrize("shape", SHIPPED, ids=_id)
def test_sa_fused_all_negative_outputs(shape):
    """last block: scales negative or 0, shifts -10 -> every output is at most -10: none may meet the `-inf -> 0` rule or be moved behind the max"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    x = _features(cin, 31)
    blocks = _blocks([cin + 3] + dims, _gen(77), last_shift=-10.0)
    w, b, sc, sh = blocks[2]
    blocks[2] = (w, b, -sc.abs(), sh)
    pack = ops.pack_sa_fused(blocks).to(DEV)
    for self_loops in (True, False):
        r64, r32 = _ref(T, x, blocks, self_loops)
        assert float(r64.max()) <= -10.0
        out = _sa(T, _x_dev(x), pack, self_loops)
        assert not bool((out == 0).any()) and not bool(torch.isinf(out).any())
        _check(f"sa_fused {_id(shape)} all-negative self_loops={self_loops}", r64, r32, out)


@pytest.mark.parametrize("K", [1, 16, 31, 32, 33, 63, 64])
def test_sa_fused_table_widths(K):
    """tables of K columns from ops.ball_query(K = ...) (bit-equal to the oracle's), both shipped edge MLPs, self-loops on and off"""
    T = _sa_case()
    nbr, cnt = ops.ball_query(T["pos_d"], T["seg"].ptr, T["cidx"], T["cseg"].ptr, SA_RADIUS, K)
    ptr, cptr = np.concatenate(([0], np.cumsum(SA_SIZES))), np.concatenate(([0], np.cumsum(T["cseg"].sizes)))
    onbr, ocnt = O.ball_query(T["pos"].numpy(), ptr, T["cidx_c"].numpy(), cptr, SA_RADIUS, K)
    assert np.array_equal(nbr.cpu().numpy(), onbr) and np.array_equal(cnt.cpu().numpy(), ocnt) and ocnt.max() == K
    tall = torch.zeros((T["M"] + 64 // K + 1, K), dtype=torch.int32, device=DEV)       # the table at the head of a taller one (valid indices behind it): a
    tall[:T["M"]] = nbr                                                                  # kernel that reads 64 slots of a K-wide row stays inside the buffer
    nbr = tall[:T["M"]]
    for shape in SHIPPED:
        cin, dims = shape[0], list(shape[1:])
        x = _features(cin, 32)
        blocks = _blocks([cin + 3] + dims, _gen(K))
        pack = ops.pack_sa_fused(blocks).to(DEV)
        for self_loops in (True, False):
            r64, r32 = _ref(T, x, blocks, self_loops, onbr, ocnt)
            _check(f"sa_fused {_id(shape)} K={K} self_loops={self_loops}", r64, r32, _sa(T, _x_dev(x), pack, self_loops, nbr, cnt))


@pytest.mark.parametrize("shape", SHIPPED, ids=_id)
def test_sa_fused_ball_sizes_0_1_31_32_33_64(shape):
    """the capped balls of the real K = 64 table truncated to cnt = 0, 1, 31, 32, 33 and 64 in rotation (valid entries first, the rest -1): the
    second 32-row tile exists from 33 on; an empty ball is an exact zero row without self-loops and the self edge alone with them"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    nbr, cnt = T["nbr_c"].copy(), T["cnt_c"].copy()
    sizes = [0, 1, 31, 32, 33, 64]
    for i, c in enumerate(T["capped"]):
        cnt[c] = sizes[i % 6]
        nbr[c, cnt[c]:] = -1
    empty = T["capped"][0::6]
    assert all((cnt[T["capped"]] == s).sum() >= 4 for s in sizes)
    x = _features(cin, 33)
    blocks = _blocks([cin + 3] + dims, _gen(9))
    pack = ops.pack_sa_fused(blocks).to(DEV)
    nd, cd = _dev_table(nbr, cnt)
    for self_loops in (True, False):
        r64, r32 = _ref(T, x, blocks, self_loops, nbr, cnt)
        outs = [_sa(T, _x_dev(x), pack, self_loops, nd, cd, group=G) for G in GROUPS]
        assert all(_bits(outs[0], o) for o in outs[1:])
        _check(f"sa_fused {_id(shape)} truncated balls self_loops={self_loops}", r64, r32, outs[0])
        rows = outs[0].cpu()[empty]
        if self_loops:
            only_self = r_point_conv(x, T["pos"], T["cidx_c"], np.full_like(nbr, -1), np.zeros_like(cnt), True, None, blocks, torch.float64)[empty]
            assert float((r64[empty] - only_self).abs().max()) <= 1e-12 * float(only_self.abs().max()) and bool((rows != 0).any())
        else:
            assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())


@pytest.mark.parametrize("scoped", [False, True], ids=["literal", "self_src"])
@pytest.mark.parametrize("shape", SHIPPED, ids=_id)
def test_sa_fused_self_loop_rule(shape, scoped):
    """node c (the centre's own number, or self_src[c]) planted in row c of the table at slots 0, 31, 32 and 63 -- see the module docstring"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    M, slots = T["M"], [0, 31, 32, 63]
    node = np.arange(M)
    if scoped:
        node = (node * 7 + 3) % T["N"]                      # any point may play "node c"
    rows = [c for c in T["capped"] if node[c] not in T["nbr_c"][c]][:4]          # full balls that do not hold their node by themselves
    assert len(rows) == 4
    nbr, x = T["nbr_c"].copy(), _features(cin, 34)
    for c, s in zip(rows, slots):
        nbr[c, s] = node[c]
        x[node[c]] *= 40.0                                  # the planted source would win the maximum
    emptied = nbr.copy()
    for c, s in zip(rows, slots):
        emptied[c, s] = -1
    self_src = node.astype(np.int32) if scoped else None
    src_d = torch.from_numpy(self_src).to(DEV) if scoped else None
    blocks = _blocks([cin + 3] + dims, _gen(10), zero_and_negative=False)
    pack = ops.pack_sa_fused(blocks).to(DEV)
    xd = _x_dev(x)
    planted_d, emptied_d = _dev_table(nbr, T["cnt_c"])[0], _dev_table(emptied, T["cnt_c"])[0]
    # self-loops on: the planted entry is removed and comes back as the self edge
    r64, r32 = _ref(T, x, blocks, True, nbr, self_src=self_src)
    on = _sa(T, xd, pack, True, planted_d, self_src=src_d)
    _check(f"sa_fused {_id(shape)} self-loop rule on ({'self_src' if scoped else 'literal'})", r64, r32, on)
    assert _bits(on, _sa(T, xd, pack, True, emptied_d, self_src=src_d))
    # self-loops off: an ordinary neighbour, which must contribute
    w64, w32 = _ref(T, x, blocks, False, nbr, self_src=self_src)
    without = _ref(T, x, blocks, False, emptied)[0]
    off = _sa(T, xd, pack, False, planted_d, self_src=src_d)
    _check(f"sa_fused {_id(shape)} self-loop rule off ({'self_src' if scoped else 'literal'})", w64, w32, off)
    for c in rows:
        gap = (w64[c] - without[c])
        ch = int(gap.argmax())
        assert float(gap[ch]) > 1.0, (c, float(gap[ch]))                           # the planted source wins that channel by a wide margin ...
        assert abs(float(off[c, ch]) - float(w64[c, ch])) < 1e-3 * float(gap[ch])   # ... and the kernel's row holds it


@pytest.mark.parametrize("shape", [SA_SHAPES[0], SA_SHAPES[1], SA_SHAPES[6], SA_SHAPES[10]], ids=_id)
def test_sa_fused_layouts(shape):
    """x contiguous and as a slice at column 4 of a wider NaN buffer (16-byte contract kept), out with ldo > N3 inside a NaN buffer: the same bits,
    no NaN in the result, every cell outside [M, N3] still NaN"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    x = _features(cin, 35)
    blocks = _blocks([cin + 3] + dims, _gen(11))
    pack = ops.pack_sa_fused(blocks).to(DEV)
    M, N3 = T["M"], dims[2]
    for self_loops in (True, False):
        base = _sa(T, _x_dev(x), pack, self_loops)
        r64, r32 = _ref(T, x, blocks, self_loops)
        _check(f"sa_fused {_id(shape)} layouts self_loops={self_loops}", r64, r32, base)
        for layout in ("contiguous", "wide"):
            for G in (0, 32, 2):
                buf, view = _nan_out(M, N3)
                out = _sa(T, _x_dev(x, layout), pack, self_loops, out=view, group=G)
                assert out.data_ptr() == view.data_ptr() and out.stride(0) == N3 + 8
                assert _bits(out, base) and _no_nan(out) and _outside_is_nan(buf, M, N3), (layout, G)


@pytest.mark.parametrize("shape", SHIPPED, ids=_id)
def test_sa_fused_and_the_unfused_chain_under_the_same_rule(shape):
    """the same inputs through gn_sa_gather -> gn_linear x 3 -> gn_segment_max: both ratios side by side"""
    T = _sa_case()
    cin, dims = shape[0], list(shape[1:])
    x = _features(cin, 36)
    blocks = _blocks([cin + 3] + dims, _gen(12))
    pack = ops.pack_sa_fused(blocks).to(DEV)
    xd = _x_dev(x)
    for self_loops in (True, False):
        r64, r32 = _ref(T, x, blocks, self_loops)
        h, slot_src, S = ops.sa_gather(xd, T["pos_d"], T["cidx"], T["nbr"], self_loops=self_loops)
        for w, b, sc, sh in blocks:
            k = w.shape[1]
            wp = torch.zeros(w.shape[0], ops.pad4(k), device=DEV)
            wp[:, :k] = w.to(DEV)
            h = ops.linear(h, wp, b.to(DEV), sc.to(DEV), sh.to(DEV), relu=True, K=k)
        chain = ops.segment_max(h, slot_src, T["M"], S)
        a = _check(f"sa_fused {_id(shape)} self_loops={self_loops}", r64, r32, _sa(T, xd, pack, self_loops))
        b_ = _check(f"unfused chain {_id(shape)} self_loops={self_loops}", r64, r32, chain)
        print(f"[sa-ratios] {_id(shape)} self_loops={self_loops}: sa_fused {a:.2f}  unfused chain {b_:.2f}  (x torch-fp32's error)")


# ================================================================================================ gn_linear
def _variant(M, N):
    """the dispatch of gn_linear (csrc/linear.hip), restated"""
    cdiv = lambda a, b: -(-a // b)
    full = cdiv(M, 128) * cdiv(N, 128)
    return "N<=32" if N <= 32 else "N<=64" if N <= 64 else "128x128" if full >= 384 else "64x128" if 2 * full >= 256 else "64x64"


def _lin_inputs(M, N, K, seed, bias=True, affine=True):
    g = _gen(seed)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    sc = sh = None
    if affine:
        sc, sh = 0.5 + torch.rand(N, generator=g), torch.randn(N, generator=g)
        sc[0::3] *= -1.0
        sc[N // 2] = 0.0
    return x, w, b, sc, sh


def _lin_ref(x, w, b, sc, sh, relu):
    """-> (fp64 result, the derived elementwise bound, the same in torch-fp32)"""
    K = x.shape[1]
    res = []
    for dt in (torch.float64, torch.float32):
        r = x.to(dt) @ w.to(dt).t()
        if b is not None:
            r = r + b.to(dt)
        r = torch.relu(r) if relu else r
        res.append((r, r * sc.to(dt) + sh.to(dt) if sc is not None else r))
    (r64, y64), (_, y32) = res
    E = (K + 3) * U * (x.double().abs() @ w.double().abs().t() + (b.double().abs() if b is not None else 0.0))
    bound = E if sc is None else sc.double().abs() * E + U * ((sc.double() * r64).abs() + sh.double().abs())
    return y64, bound, y32


def _lin_check(name, out, y64, bound, y32):
    o = out.detach().cpu().double()
    assert o.shape == y64.shape and bool(torch.isfinite(o).all()), name
    err = (o - y64).abs()
    rel = float((err / bound.clamp(min=1e-300)).max())
    e32 = float((y32.double() - y64).abs().max())
    print(f"[linear-error] {name}: max error / derived bound {rel:.3e}   hip {float(err.max()):.3e}  torch-fp32 {e32:.3e}  ratio {float(err.max()) / max(e32, 1e-300):.2f}")
    assert bool((err <= bound).all()), (name, rel)
    return rel


def _lin_call(x, w, b, sc, sh, relu, loader, nan_out=True):
    """loader "aligned": x and w at column 4 of NaN buffers whose rows are a multiple of 4 floats (NaN right behind column K - 1: the float4 loader's
    k + 1 .. k + 3 masks alone keep it out); "scalar": at column 1 (`_operand`'s wide layout).  Output into a NaN buffer with ldy > N.
    -> (result view, its buffer or None)"""
    M, K = x.shape
    N = w.shape[0]
    if loader == "aligned":
        xd, wd = _wide(x, 4, ops.pad4(K) + 8), _wide(w, 4, ops.pad4(K) + 12)
        assert xd.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0 and xd.stride(0) % 4 == 0 and wd.stride(0) % 4 == 0
    else:
        xd, wd = _operand(x, "wide", 0), _operand(w, "wide", 1)
        assert xd.data_ptr() % 16 != 0 or xd.stride(0) % 4 != 0
    d = lambda t: None if t is None else t.to(DEV)
    buf, view = _nan_out(M, N, off=3, extra=7) if nan_out else (None, None)
    out = ops.linear(xd, wd, d(b), d(sc), d(sh), relu=relu, out=view)
    return out, buf


VARIANT_SHAPES = [(300, 32, "N<=32"), (300, 33, "N<=64"), (300, 64, "N<=64"), (24449, 129, "128x128"), (24448, 129, "64x128"), (8065, 129, "64x128"),
                  (8064, 129, "64x64"), (1000, 65, "64x64")]


@pytest.mark.parametrize("loader", ["aligned", "scalar"])
@pytest.mark.parametrize("M,N,variant", VARIANT_SHAPES)
def test_linear_every_tile_variant(M, N, variant, loader):
    """one shape (and the neighbour across each threshold) per tile variant, by the dispatch's own arithmetic, under both loaders"""
    assert _variant(M, N) == variant
    K = 19
    x, w, b, sc, sh = _lin_inputs(M, N, K, M + N)
    y64, bound, y32 = _lin_ref(x, w, b, sc, sh, True)
    out, buf = _lin_call(x, w, b, sc, sh, True, loader)
    _lin_check(f"linear {variant} {M}x{N}x{K} {loader}", out, y64, bound, y32)
    assert _outside_is_nan(buf, M, N, off=3)


def test_linear_bits_do_not_depend_on_variant_or_loader():
    """49153 rows (K = 19, N = 129) whole (128 x 128 tiles), their first 20000 (64 x 128) and first 1000 (64 x 64), each under the float4 loader and the
    scalar loader (ld no multiple of 4): shared rows have the same bits"""
    M, K, N = 49153, 19, 129
    assert [_variant(m, N) for m in (M, 20000, 1000)] == ["128x128", "64x128", "64x64"]
    x, w, b, sc, sh = _lin_inputs(M, N, K, 5)
    xa = ops.new_rows(M, K, DEV)
    xa.copy_(x.to(DEV))
    wa = ops.new_rows(N, K, DEV)
    wa.copy_(w.to(DEV))
    xs, ws = x.to(DEV), w.to(DEV)
    assert xa.stride(0) % 4 == 0 and xa.data_ptr() % 16 == 0 and wa.data_ptr() % 16 == 0 and xs.stride(0) % 4 != 0
    bd, scd, shd = b.to(DEV), sc.to(DEV), sh.to(DEV)
    whole = ops.linear(xa, wa, bd, scd, shd, relu=True)
    y64, bound, y32 = _lin_ref(x, w, b, sc, sh, True)
    _lin_check(f"linear {M}x{N}x{K} whole", whole, y64, bound, y32)
    for m in (M, 20000, 1000):
        for xin, win, name in ((xa, wa, "aligned"), (xs, ws, "scalar")):
            out = ops.linear(xin[:m], win, bd, scd, shd, relu=True)
            assert _bits(out, whole[:m]), (m, name)


TAILS = [(m, 65, 17) for m in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 257)] + \
        [(129, n, 17) for n in (1, 3, 31, 32, 33, 63, 64, 127, 128, 129, 257)] + [(129, 65, k) for k in (1, 2, 3, 4, 5, 15, 16, 31, 33, 131)]


@pytest.mark.parametrize("M,N,K", TAILS)
def test_linear_tails_and_layouts(M, N, K):
    """around M = 129, N = 65, K = 17, one size at a time; x and w behind NaN under both loaders, the output inside a NaN buffer"""
    x, w, b, sc, sh = _lin_inputs(M, N, K, 1000 * M + 10 * N + K)
    y64, bound, y32 = _lin_ref(x, w, b, sc, sh, True)
    outs = []
    for loader in ("aligned", "scalar"):
        out, buf = _lin_call(x, w, b, sc, sh, True, loader)
        _lin_check(f"linear tail {M}x{N}x{K} {loader}", out, y64, bound, y32)
        assert _no_nan(out) and _outside_is_nan(buf, M, N, off=3), loader
        outs.append(out)
    assert _bits(outs[0], outs[1])
    plain = _lin_call(x, w, b, sc, sh, True, "aligned", nan_out=False)[0]          # the wrapper's own output rows
    assert _bits(plain, outs[0])


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_linear_epilogue(bias, relu, affine):
    """no bias / bias, ReLU off / on, affine off / on (negative scales, one exactly 0); a single NaN in x makes exactly its own row NaN"""
    M, N, K = 129, 65, 17
    x, w, b, sc, sh = _lin_inputs(M, N, K, 4 * bias + 2 * relu + affine, bias=bias, affine=affine)
    y64, bound, y32 = _lin_ref(x, w, b, sc, sh, relu)
    for loader in ("aligned", "scalar"):
        out, _ = _lin_call(x, w, b, sc, sh, relu, loader)
        _lin_check(f"linear epilogue bias={bias} relu={relu} affine={affine} {loader}", out, y64, bound, y32)
        if affine:
            assert torch.equal(out[:, N // 2].cpu(), sh[N // 2].expand(M))             # the zero scale leaves the shift itself
        xn = x.clone()
        xn[57, 5] = float("nan")
        bad, _ = _lin_call(xn, w, b, sc, sh, relu, loader)
        nan = torch.isnan(bad).cpu()
        assert bool(nan[57].all()) and int(nan.sum()) == N
        keep = torch.arange(M) != 57
        assert _bits(bad[keep], out[keep])


# ================================================================================================ gn_ball_query
def _ball_query(pos, ptr, cidx, cptr, r, K):
    """ops.ball_query into buffers this test filled first (nbr with 12345, cnt with -7): what the kernel leaves alone shows"""
    pos_d = torch.from_numpy(pos).to(DEV)
    t32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).to(DEV)
    ptr_d, cidx_d, cptr_d = t32(ptr), t32(cidx), t32(cptr)
    M = len(cidx)
    nbr = torch.full((M, K), 12345, dtype=torch.int32, device=DEV)
    cnt = torch.full((M,), -7, dtype=torch.int32, device=DEV)
    r2 = float(np.float32(float(r) * float(r)))
    _lib.call("gn_ball_query", ops._p(pos_d), ops._p(ptr_d), ops._p(cidx_d), ops._p(cptr_d), len(ptr) - 1, M, r2, K, ops._p(nbr), ops._p(cnt), ops._stream())
    wn, wc = ops.ball_query(pos_d, ptr_d, cidx_d, cptr_d, r, K)
    nbr, cnt = nbr.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(wn.cpu().numpy(), nbr) and np.array_equal(wc.cpu().numpy(), cnt)     # the wrapper hands over the same call
    return nbr, cnt


def _bq_check(nbr, cnt, pos, ptr, cidx, cptr, r, K):
    onbr, ocnt = O.ball_query(pos, ptr, cidx, cptr, r, K)
    lnbr, lcnt = ball_query_loop(pos, ptr, cidx, cptr, r, K)
    assert np.array_equal(ocnt, lcnt) and np.array_equal(onbr, lnbr)
    assert np.array_equal(cnt, ocnt), (K, r)                                       # every centre
    assert np.array_equal(nbr, onbr), (K, r)
    assert ((np.arange(K)[None, :] >= cnt[:, None]) == (nbr == -1)).all()          # -1 from cnt on, and nowhere before
    return onbr, ocnt


@pytest.mark.parametrize("K", BQ_K)
def test_ball_query_tiny_examples_every_radius(K):
    """examples of 1, 2, 63, 64, 65 and 129 points in one batch, every point a centre; r = 0 (nothing), 0.3 and one that holds everything"""
    pos, ptr, cidx, cptr = tiny_examples()
    for r in (0.0, 0.3, 10.0):
        nbr, cnt = _ball_query(pos, ptr, cidx, cptr, r, K)
        _bq_check(nbr, cnt, pos, ptr, cidx, cptr, r, K)
        if r == 0.0:
            assert not cnt.any() and (nbr == -1).all()
        if r == 10.0:
            for b, n in enumerate(BQ_SIZES):                                       # the first K indices of the example
                want = np.full(K, -1)
                want[:min(n, K)] = ptr[b] + np.arange(min(n, K))
                assert (nbr[cptr[b]:cptr[b + 1]] == want[None, :]).all() and (cnt[cptr[b]:cptr[b + 1]] == min(n, K)).all()


@pytest.mark.parametrize("K", BQ_K)
def test_ball_query_excludes_points_exactly_on_the_radius(K):
    pos, ptr, cidx, cptr = lattice_cloud()
    pairs = on_the_radius(pos, ptr, cidx, cptr, 0.5)
    onbr, _ = O.ball_query(pos, ptr, cidx, cptr, 0.5, K)
    assert len(pairs) >= 100 and not any(j in onbr[c] for c, j in pairs)           # d2 == r2 occurs in fp32 and the oracle excludes it (CPU, before the call)
    nbr, cnt = _ball_query(pos, ptr, cidx, cptr, 0.5, K)
    _bq_check(nbr, cnt, pos, ptr, cidx, cptr, 0.5, K)
    assert not any(j in nbr[c] for c, j in pairs)


# ================================================================================================ gn_nocs_head
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("bins", [2, 7, 64, 100])
def test_nocs_head_bins_rows_and_ties(bins, N):
    """rows of pad4(3 bins) floats (ldl != 3 bins for 2 and 7 bins) with NaN in the pad; a tie of the maximum planted in every axis of two rows"""
    g = _gen(bins * 1000 + N)
    logits = torch.randn(N, 3 * bins, generator=g) * 3
    first = {}
    for row in {0, N // 2}:
        for a in range(3):
            k1 = int(torch.randint(0, bins - 1, (1,), generator=g))
            k2 = int(torch.randint(k1 + 1, bins, (1,), generator=g))
            logits[row, 3 * k1 + a] = logits[row, 3 * k2 + a] = 50.0
            first[(row, a)] = k1
    ld = ops.pad4(3 * bins)
    buf = torch.full((N + 1, ld), float("nan"), dtype=torch.float32)
    buf[:N, :3 * bins] = logits
    view = buf.to(DEV)[:N, :3 * bins]
    assert ops.rows_view(view)[1] == ld and (ld != 3 * bins) == (bins in (2, 7))
    idx, conf, nocs = ops.nocs_head(view, bins)
    ridx, rconf, rnocs = P.nocs_postprocess(logits, bins)
    assert np.array_equal(idx.cpu().numpy(), ridx.reshape(N, 3).numpy())
    assert all(int(idx[row, a]) == k for (row, a), k in first.items())
    assert _bits(nocs, rnocs.reshape(N, 3).float())
    np.testing.assert_allclose(conf.cpu().numpy(), rconf.reshape(N, 3).numpy(), rtol=1e-5, atol=1e-6)

"""Plain restatements of the implicit decoder's forward operations (csrc/decode.hip) and the inputs its edge suite shares
(tests/test_decoder_reference_host.py on the CPU, tests/test_gpu_decoder_edges.py on the GPU).  Nothing here is a copy of a kernel: the sampler is
numpy float32 with one rounding per operation, the MLP is torch float64, the bound is a textbook running error analysis.

Sampler.  F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True) on a 5-D input as ATen's grid_sampler_3d evaluates it on the CPU:
    x   = fl(fl(fl(fl(fl(2 q) - 1) + 1) / 2) * (size - 1))                     un-normalise
    x   = fmin(size - 1, fmax(x, 0))                                            border clamp
    x0  = floor(x);  w0 = fl(fl(x0 + 1) - x);  w1 = fl(x - x0)                  the cell and its weights
    out = sum over the corners c = dx + 2 dy + 4 dz in ascending c (ATen's tnw, tne, tsw, tse, bnw, bne, bsw, bse) of
          fl(v[z0 + dz][y0 + dy][x0 + dx] * fl(fl(wx[dx] * wy[dy]) * wz[dz])), a corner past the upper face skipped (never multiplied by zero)
Query component 0 indexes the LAST volume axis.  tests/test_decoder_reference_host.py proves the restatement equal to torch on the CPU bit for bit.

The project's rule for a NaN query component is fmax's: NaN -> source index 0 (weights 1, 0).  ATen's std::max / std::min chain gives size - 1
there, an artefact of the argument order; the restatement and every kernel follow fmax and no test compares a NaN query with torch.
"""
import numpy as np
import torch

# ------------------------------------------------------------------------------------------------ the suite's geometries and queries
BASE_DIMS = (3, 4, 5)
GEOMETRIES = [(1, 4, 6), (5, 1, 3), (4, 7, 1), (1, 1, 5), (1, 1, 1), (2, 2, 2), (2, 5, 3)]
GEOMETRY_CHANNELS = [3, 24, 32]
N_QUERIES = 1500


def spread(shape, seed):
    """float32 normal values scaled over 13 binades: a sum of them in another order rounds differently with near certainty"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())).numpy()


def axis_table(n):
    """the per-axis query table: every exact voxel coordinate k / (n - 1) of an axis of n voxels, both fp32 neighbours of each, and the fixed values.
    0.3, 0.5 and 0.7 are there so that every geometry has queries well inside a cell: with lattice values alone one corner carries all the weight
    on a 2-voxel axis and the accumulation order does not show in the bits (tests/test_decoder_reference_host.py)"""
    vals = []
    for k in range(n if n > 1 else 0):
        v = np.float32(k) / np.float32(n - 1)
        vals += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
    vals += [0.0, 1.0, -0.0, -0.05, 1.05, 1e30, -1e30, np.inf, -np.inf, 0.3, 0.5, 0.7]
    return np.array(vals, np.float32)


def query_table(dims, n=N_QUERIES, seed=0):
    """[n][3] float32: the axis tables of (W, H, D) (component 0 indexes the last axis), each repeated to n entries and shuffled with a fixed seed"""
    D, H, W = dims
    rng = np.random.default_rng(1000 + seed)
    q = np.empty((n, 3), np.float32)
    for a, size in enumerate((W, H, D)):
        t = axis_table(size)
        q[:, a] = rng.permutation(np.resize(t, n))
    return q


# ------------------------------------------------------------------------------------------------ sampler
def tri_axis(q, size):
    """one axis in float32 -> (x0 int64, weight of x0, weight of x0 + 1); NaN -> index 0 (fmax / fmin return the number)"""
    q = np.asarray(q, np.float32)
    s1 = np.float32(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (((np.float32(2) * q - np.float32(1)) + np.float32(1)) / np.float32(2)) * s1
        x = np.fmin(s1, np.fmax(x, np.float32(0)))
        x0 = np.floor(x)
        w0, w1 = (x0 + np.float32(1)) - x, x - x0
    assert x.dtype == np.float32 and w0.dtype == np.float32 and w1.dtype == np.float32
    return x0.astype(np.int64), w0, w1


def tri_rows(vol, query, reverse=False):
    """vol [D][H][W][C] float32, query [M][3] float32 -> [M][C] float32 (the module docstring's arithmetic); reverse: corners 7 .. 0 instead"""
    vol, query = np.ascontiguousarray(vol, np.float32), np.ascontiguousarray(query, np.float32)
    D, H, W, C = vol.shape
    (x0, wx0, wx1), (y0, wy0, wy1), (z0, wz0, wz1) = tri_axis(query[:, 0], W), tri_axis(query[:, 1], H), tri_axis(query[:, 2], D)
    acc = np.zeros((len(query), C), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in (range(7, -1, -1) if reverse else range(8)):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            xx, yy, zz = x0 + dx, y0 + dy, z0 + dz
            ok = (xx < W) & (yy < H) & (zz < D)
            w = ((wx1 if dx else wx0) * (wy1 if dy else wy0)) * (wz1 if dz else wz0)
            v = vol[np.minimum(zz, D - 1), np.minimum(yy, H - 1), np.minimum(xx, W - 1)]
            acc = np.where(ok[:, None], acc + v * w[:, None], acc)
    assert acc.dtype == np.float32
    return acc


def lattice_queries(Q, m0, M):
    """rows m0 .. m0 + M - 1 of the flattened (Q, Q, Q) lattice: row g = (i Q + j) Q + k holds fl(fl((i, j, k) * fl(1 / fl(Q - 1))) + (-0.0))"""
    g = m0 + np.arange(M, dtype=np.int64)
    ijk = np.stack([g // (Q * Q), (g // Q) % Q, g % Q], axis=1).astype(np.float32)
    sc = np.float32(1) / (np.float32(Q) - np.float32(1))
    out = ijk * sc + np.float32(-0.0)
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    """float32 arrays equal bit for bit, a NaN equal to any NaN (payloads are not compared)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def brick_extent(Q, size, i0, points=4):
    """voxels along one axis of `size` that the lattice points i0 .. min(i0 + points, Q) - 1 of a Q-lattice touch, formed as trilinear_brick_kernel
    forms its box from fp32 coordinates: floor(src(first)) .. min(floor(src(last)) + 1, size - 1).  Q, size, i0 broadcast."""
    Q, size, i0 = np.broadcast_arrays(np.asarray(Q, np.int64), np.asarray(size, np.int64), np.asarray(i0, np.int64))
    i1 = np.minimum(i0 + points, Q) - 1
    sc = np.float32(1) / (Q.astype(np.float32) - np.float32(1))
    s1 = (size - 1).astype(np.float32)

    def src(i):
        q = i.astype(np.float32) * sc + np.float32(-0.0)
        x = (((np.float32(2) * q - np.float32(1)) + np.float32(1)) / np.float32(2)) * s1
        return np.floor(np.fmin(s1, np.fmax(x, np.float32(0)))).astype(np.int64)

    return np.minimum(src(i1) + 1, size - 1) - src(i0) + 1


# ------------------------------------------------------------------------------------------------ decoder MLP
WIDTH_SETS = [(32, 256, 256, 1), (128, 256, 256, 3), (64, 512, 256, 2), (32, 256, 512, 4), (160, 512, 512, 1)]
BN_MODES = {"all": (True, True, True), "none": (False, False, False), "middle": (False, True, False)}
ROW_COUNTS = [1, 31, 32, 33, 65]
U = 2.0 ** -24
SPARSE_UNITS = [7, 70, 133, 200]


def make_layers(widths, bn="all", seed=0):
    """raw layers [(w [N][K], b [N], s [N] or None, t [N] or None)] x 3, float32, Kaiming-scaled normal weights, with three planted features:
    column 0 of the first weight is positive and at least 0.05, so that a row with a large negative component 0 has every first-layer
    pre-activation negative; input channel 1 is read by the four units SPARSE_UNITS only (weight 0.5), so that the one-hot row of decoder_rows
    exercises a handful of paths; and row 0 of the last weight is positive, so that output 0 is not clipped to an uninformative 0 by the last ReLU"""
    g = torch.Generator().manual_seed(7919 * seed + sum(widths))
    raw = []
    for i in range(3):
        k, n = widths[i], widths[i + 1]
        w = torch.randn(n, k, generator=g) * (2.0 / k) ** 0.5
        if i == 0:
            w[:, 0] = w[:, 0].abs() + 0.05
            w[:, 1] = 0.0
            w[SPARSE_UNITS, 1] = 0.5
        if i == 2:
            w[0] = w[0].abs()
        b = torch.randn(n, generator=g) * 0.1
        s = (torch.rand(n, generator=g) + 0.5) if BN_MODES[bn][i] else None
        t = torch.randn(n, generator=g) * 0.1 if BN_MODES[bn][i] else None
        raw.append((w, b, s, t))
    return raw


def decoder_rows(c0, M, seed=0):
    """[M][c0] float32 N(0, 1) rows; from M >= 5 on: row 1 all zero, row 2 with every first-layer pre-activation of make_layers negative (component 0 =
    -100, the rest 0.01 N(0, 1)), row 3 scaled by 1e4, row 4 by 1e-4; from M >= 6 on row 5 is one-hot: 1e3 in component 1, the channel four units read.
    Magnitudes from 1e-4 to 1e4 against weights of O(0.1): no product underflows."""
    g = torch.Generator().manual_seed(104729 * seed + c0 + M)
    x = torch.randn(M, c0, generator=g)
    if M >= 5:
        x[1] = 0.0
        x[2] *= 0.01
        x[2, 0] = -100.0
        x[3] *= 1e4
        x[4] *= 1e-4
    if M >= 6:
        x[5] = 0.0
        x[5, 1] = 1e3
    return x


def decoder_fp64(rows, raw_layers, upto=3):
    """three relu(x W^T + b)[* s + t] layers in float64 (upto: only the first layers)"""
    h = rows.double()
    for w, b, s, t in raw_layers[:upto]:
        h = torch.relu(h @ w.double().t() + b.double())
        if s is not None:
            h = h * s.double() + t.double()
    return h


def gamma(n):
    return n * U / (1.0 - n * U)


def decoder_fp32_bound(rows, raw_layers):
    """A bound, per output element, on |y32 - decoder_fp64| for ANY float32 evaluation of the three layers that rounds every operation to nearest
    (unit roundoff u = 2^-24), in any summation order, with or without fused multiply-adds.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Let x be the exact (float64) input of a layer, xh the computed
    one and e >= |xh - x| elementwise; rows and weights are float32 values, so e = 0 at the input.  A computed dot product of K terms plus a bias is
    an exact sum of the K + 1 terms each multiplied by at most K + 1 factors (1 + d), |d| <= u: one rounding for the product (none under an fma) and
    at most K for the additions it passes through, whatever the order or the tree -- the MFMA's k groups, the fmaf partial sums per lane, the 16-lane
    row sum and the 8-way fold of the last layer alike.  Hence
        |fl(W xh + b) - (W x + b)| <= |W| e + gamma_{K+1} (|W| |xh| + |b|),      gamma_n = n u / (1 - n u).
    The bound uses gamma_{K+2} and the exact |x| in place of |xh| <= |x| + e.  What that omits, gamma_{K+1} |W| e, is of second order in u (e is itself
    O(K u) relative to |x|: below 1e-4 of it for K <= 512); the spare rounding adds u (|W| |x| + |b|), a (K + 1)-th of the first-order term, which
    is larger.  ReLU is 1-Lipschitz: e passes unchanged.  BatchNorm folded to r s + t (one product, one sum, two roundings):
        e_bn = |s| e + gamma_2 (|r s| + |t|).
    The analysis assumes that no product underflows; decoder_rows and make_layers keep every magnitude between 1e-4 and 1e4 (exact zeros are exact).
    Nothing in it is fitted to a measurement."""
    x = rows.double()
    e = torch.zeros_like(x)
    for w, b, s, t in raw_layers:
        wa, K = w.double().abs(), w.shape[1]
        pre = x @ w.double().t() + b.double()
        e = e @ wa.t() + gamma(K + 2) * (x.abs() @ wa.t() + b.double().abs())
        x = torch.relu(pre)
        if s is not None:
            e = s.double().abs() * e + gamma(2) * ((x * s.double()).abs() + t.double().abs())
            x = x * s.double() + t.double()
    return e


def decoder_fp32_cpu(rows, raw_layers):
    """the same layers in torch float32 on the CPU"""
    h = rows.float()
    for w, b, s, t in raw_layers:
        h = torch.relu(h @ w.t() + b)
        if s is not None:
            h = h * s + t
    return h

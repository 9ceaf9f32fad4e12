"""Thin torch-tensor wrappers over the C ABI (include/garmentnets_hip.h).

torch is used for device memory and streams only; every function below launches hand-written HIP kernels on the
current torch stream.  Tensors must live on a ROCm device -- there is no CPU path.
"""
import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib

_i32 = torch.int32


class _CallState(threading.local):
    """per HOST THREAD: the device of the tensors of the C-ABI call being assembled (arguments are evaluated left to right, _stream()
    last).  Thread-local, so two threads driving two models / devices never see each other's half-assembled call"""
    dev = None


_CALL = _CallState()


def _stream():
    """torch's current stream ON THE DEVICE OF THE CALL'S TENSORS (not of torch's current device: a model on cuda:1 with the
    process default device 0 must launch on cuda:1's stream; the C ABI binds the HIP device to the stream's, csrc/common.h gn_stream)"""
    dev, _CALL.dev = _CALL.dev, None
    if dev is not None and dev.index is not None and dev.index != torch.cuda.current_device():
        torch.cuda.set_device(dev)            # the null stream means "current device" to HIP: make the two agree
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.GarmentNetsHipError("garmentnets_amd ops need tensors on the GPU (no CPU fallback)")
    if _CALL.dev is None:
        _CALL.dev = t.device
    elif _CALL.dev != t.device:
        dev, _CALL.dev = _CALL.dev, None
        raise _lib.GarmentNetsHipError(f"garmentnets_amd ops: tensors on different devices ({dev} vs {t.device})")
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype, name):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def pad4(c):
    return (c + 3) // 4 * 4


def rows_view(t):
    """(rows, ld) of a 2-D tensor whose rows are contiguous (stride(1)==1); ld = stride(0)."""
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), "need row-major rows"
    return t.shape[0], (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def new_rows(n, c, device):
    """[n][c] fp32 buffer whose leading dimension is padded to a multiple of 4 (16-byte rows for the GEMM loader)."""
    buf = torch.empty((n, pad4(c)), dtype=torch.float32, device=device)
    return buf[:, :c]


# ------------------------------------------------------------------------------------------------ points
def fps_count(n, ratio):
    """torch_cluster: ceil(n * ratio) evaluated in float32."""
    return int(math.ceil(float(np.float32(n) * np.float32(ratio))))


def segment_ptr(batch, B):
    _chk(batch, torch.int64, "batch")
    ptr = torch.empty(B + 1, dtype=_i32, device=batch.device)
    _lib.call("gn_segment_ptr", _p(batch), batch.numel(), B, _p(ptr), _stream())
    return ptr


def fps(pos, ptr, out_ptr, max_points, m_total, start_idx=None, gap_out=None, nested_gap=None):
    """start_idx: optional int32 [B] local start point per example (None = first point).
    gap_out / nested_gap: float32 [B] (include/garmentnets_hip.h gn_fps_nested): a cascade's second level hands in the first level's gap_out and
    gets the prefix 0..m-1 of every example whose first-level running maximum stayed positive -- the same indices without the serial steps."""
    _chk(pos, torch.float32, "pos")
    idx = torch.empty(m_total, dtype=_i32, device=pos.device)
    B = ptr.numel() - 1
    for t, name in ((gap_out, "gap_out"), (nested_gap, "nested_gap")):
        if t is not None:
            _chk(t, torch.float32, name)
    # more points per example than the LDS-resident kernels hold: running distances in a device workspace
    nbytes = _lib.load().gn_fps_workspace_bytes(B, int(max_points))
    ws = _ws(nbytes, pos.device) if nbytes else None
    _lib.call("gn_fps_nested_ws", _p(pos), _p(ptr), _p(out_ptr), _p(start_idx), B, int(max_points), _p(idx), _p(gap_out), _p(nested_gap),
              _p(ws), nbytes, _stream())
    return idx


def ball_query(pos, ptr, centre_idx, centre_ptr, r, K=64):
    M = centre_idx.numel()
    nbr = torch.empty((M, K), dtype=_i32, device=pos.device)
    cnt = torch.empty(M, dtype=_i32, device=pos.device)
    r2 = float(np.float32(float(r) * float(r)))
    _lib.call("gn_ball_query", _p(pos), _p(ptr), _p(centre_idx), _p(centre_ptr), ptr.numel() - 1, M, r2, K, _p(nbr), _p(cnt), _stream())
    return nbr, cnt


def sa_gather(x, pos, centre_idx, nbr, self_loops=True, self_src=None):
    """self_src: int32 [M] scope of the self-loop rule (include/garmentnets_hip.h: gn_sa_gather_scoped) or None = PyG's literal rule"""
    M, K = nbr.shape
    C = 0 if x is None else x.shape[1]
    S = K + (1 if self_loops else 0)
    out = new_rows(M * S, C + 3, pos.device)
    slot_src = torch.empty(M * S, dtype=_i32, device=pos.device)
    ldx = 0 if x is None else rows_view(x)[1]
    _lib.call("gn_sa_gather_scoped", _p(x), ldx, C, _p(pos), _p(centre_idx), _p(nbr), M, K, 1 if self_loops else 0,
              _p(_chk(self_src, _i32, "self_src") if self_src is not None else None), _p(out), out.stride(0), _p(slot_src), _stream())
    return out, slot_src, S


def segment_max(h, slot_src, M, S):
    C = h.shape[1]
    out = new_rows(M, C, h.device)
    _lib.call("gn_segment_max", _p(h), rows_view(h)[1], _p(slot_src), M, S, C, _p(out), out.stride(0), _stream())
    return out


class SaFusedPack:
    """weights / epilogue tables of gn_sa_fused for one edge MLP [cin+3, n1, n2, n3]"""

    def __init__(self, w1p, w2p, w3p, tab, cin, dims):
        self.w1p, self.w2p, self.w3p, self.tab, self.cin, self.dims = w1p, w2p, w3p, tab, int(cin), tuple(int(v) for v in dims)
        self.cout = self.dims[2]
        self.macs_per_edge = (self.cin + 3) * self.dims[0] + self.dims[0] * self.dims[1] + self.dims[1] * self.dims[2]

    def to(self, device):
        return SaFusedPack(self.w1p.to(device), self.w2p.to(device), self.w3p.to(device), self.tab.to(device), self.cin, self.dims)


def sa_fused_supported(cin, dims):
    return len(dims) == 3 and bool(_lib.load().gn_sa_fused_supported(int(cin), int(dims[0]), int(dims[1]), int(dims[2])))


def pack_sa_fused(layers):
    """layers = ((w1,b1,s1,t1), (w2,b2,s2,t2), (w3,b3,s3,t3)): Linear weight (n, k) / bias and the folded eval-BatchNorm scale / shift (or
    None) of the three blocks of a PointConv local_nn; w1 is (n1, cin + 3) -> SaFusedPack.  A-fragment order of csrc/sa_fused.hip:
    Wp[nb][kb][qq][lane = 32 h + r][i] = W[32 nb + r][32 kb + 8 qq + 4 h + i] (zero beyond k); tables in accumulator-register order:
    register q of lane half h of block nb is unit 32 nb + 8 (q >> 2) + (q & 3) + 4 h."""
    ar = torch.arange
    packs, tabs, dims = [], [], []
    for w, b, sc, sh in layers:
        w = w.detach().float().cpu()
        n, k = w.shape
        assert n % 32 == 0
        kb_n = (((k + 7) // 8 * 8) + 31) // 32
        wz = torch.zeros((n, kb_n * 32), dtype=torch.float32)
        wz[:, :k] = w
        nb, kb, qq, h, r, i = torch.meshgrid(ar(n // 32), ar(kb_n), ar(4), ar(2), ar(32), ar(4), indexing="ij")
        packs.append(wz[32 * nb + r, 32 * kb + 8 * qq + 4 * h + i].contiguous())                 # [nb][kb][qq][h][r][4]
        nbt, ht, q = torch.meshgrid(ar(n // 32), ar(2), ar(16), indexing="ij")
        u = 32 * nbt + 8 * (q >> 2) + (q & 3) + 4 * ht                                            # [nb][2][16]
        one = lambda v, fill: (torch.full((n,), fill) if v is None else v.detach().float().cpu())
        tabs.append(torch.stack((one(b, 0.0)[u], one(sc, 1.0)[u], one(sh, 0.0)[u]), dim=2).reshape(-1))   # [nb][2][3][16]
        dims.append(n)
    cin = layers[0][0].shape[1] - 3
    return SaFusedPack(packs[0], packs[1], packs[2], torch.cat(tabs).contiguous(), cin, dims)


def sa_fused(x, pos, centre_idx, nbr, cnt, pack, self_loops=True, self_src=None, group=0, out=None):
    """fps centres + ball-query table -> [M][n3] set-abstraction features (PointConv(local_nn, max) in one kernel, csrc/sa_fused.hip).
    group: centres per workgroup, 2 / 4 / 8 / 16 / 32, or 0 = the library's cost rule (every group gives the same bits); out: [M][n3] rows to write"""
    M, K = nbr.shape
    if out is None:
        out = new_rows(M, pack.cout, pos.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (M, pack.cout):
        raise ValueError(f"sa_fused: out must be float32 [{M}][{pack.cout}]")
    ldx = 0 if x is None else rows_view(x)[1]
    _lib.call("gn_sa_fused_group", _p(x), ldx, pack.cin, _p(_chk(pos, torch.float32, "pos")), _p(centre_idx), _p(nbr), _p(cnt), M, K, 1 if self_loops else 0,
              _p(_chk(self_src, _i32, "self_src") if self_src is not None else None), _p(pack.w1p), _p(pack.w2p), _p(pack.w3p), _p(pack.tab), pack.dims[0], pack.dims[1], pack.dims[2], _p(out), rows_view(out)[1], _stream(),
              int(group))
    return out


def sa_fused_auto_group(cin, dims, M):
    """the group gn_sa_fused's cost rule takes for M centres of the edge MLP [cin + 3, *dims] on the current device"""
    g = _lib.load().gn_sa_fused_auto_group(int(cin), int(dims[0]), int(dims[1]), int(dims[2]), int(M))
    if g <= 0:
        raise ValueError(f"sa_fused_auto_group: {_lib.load().gn_last_error().decode(errors='replace')}")
    return g


def global_max_pool(h, ptr, B):
    C = h.shape[1]
    out = new_rows(B, C, h.device)
    _lib.call("gn_global_max_pool", _p(h), rows_view(h)[1], _p(ptr), B, C, _p(out), out.stride(0), _stream())
    return out


KNN_MAXK = 8          # gn_knn_interpolate's largest k


def knn_interpolate(xs, ps, ptr_s, pq, ptr_q, k, out=None):
    Nq, C = pq.shape[0], xs.shape[1]
    if out is None:
        out = new_rows(Nq, C, xs.device)
    # k <= 8: the register-list kernel; larger k: one pass per neighbour (gn_knn_interpolate_any)
    _lib.call("gn_knn_interpolate" if int(k) <= KNN_MAXK else "gn_knn_interpolate_any", _p(xs), rows_view(xs)[1], _p(ps), _p(ptr_s), _p(pq), _p(ptr_q),
              ptr_s.numel() - 1, Nq, C, int(k), _p(out), rows_view(out)[1], _stream())
    return out


def linear(x, w, bias=None, bn_scale=None, bn_shift=None, relu=False, out=None, K=None):
    """x [M][K] rows, w [N][ldw] (packed, possibly K-padded) -> [M][N]."""
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    N = w.shape[0]
    if out is None:
        out = new_rows(M, N, x.device)
    _lib.call("gn_linear", _p(x), rows_view(x)[1], _p(w), rows_view(w)[1], _p(bias), _p(bn_scale), _p(bn_shift), 1 if relu else 0,
              M, N, K, _p(out), rows_view(out)[1], _stream())
    return out


def nocs_head(logits, bins):
    N = logits.shape[0]
    dev = logits.device
    idx = torch.empty((N, 3), dtype=torch.int64, device=dev)
    conf = torch.empty((N, 3), dtype=torch.float32, device=dev)
    nocs = torch.empty((N, 3), dtype=torch.float32, device=dev)
    _lib.call("gn_nocs_head", _p(logits), rows_view(logits)[1], N, bins, _p(idx), _p(conf), _p(nocs), _stream())
    return idx, conf, nocs


# ------------------------------------------------------------------------------------------------ gridding
def _f3(v):
    return (ctypes.c_float * 3)(*[float(a) for a in v])


def _i3(v):
    return (ctypes.c_int * 3)(*[int(a) for a in v])


def grid_features(feat, nocs, sim_pos, conf, batch, lower, upper, grid_shape, include_point=True, include_conf=True):
    N, Cf = feat.shape
    C = Cf + (6 if include_point else 0) + (3 if include_conf else 0)
    out = new_rows(N, C, feat.device)
    flat = torch.empty(N, dtype=_i32, device=feat.device)
    _lib.call("gn_grid_features", _p(feat), rows_view(feat)[1], Cf, _p(_chk(nocs, torch.float32, "nocs")),
              _p(_chk(sim_pos, torch.float32, "sim_pos")), _p(_chk(conf, torch.float32, "conf")), _p(_chk(batch, torch.int64, "batch")),
              N, _f3(lower), _f3(upper), _i3(grid_shape), 1 if include_point else 0, 1 if include_conf else 0, _p(out),
              out.stride(0), _p(flat), _stream())
    return out, flat


def zeroed_volume(B, grid_shape, C, device):
    """(vol, count workspace) of grid_scatter, zero-filled on torch's CURRENT stream (callers put it on a side stream)"""
    vol = torch.zeros((B,) + tuple(grid_shape) + (C,), dtype=torch.float32, device=device)
    cnt = torch.zeros(B * int(np.prod(grid_shape)), dtype=_i32, device=device)
    return vol, cnt


# torch_scatter.scatter's reductions (networks/conv_implicit_wnf.py:92-94) -> gn_grid_scatter's reduce codes
REDUCE_CODES = {"max": 0, "mean": 1, "sum": 2, "add": 2, "min": 3, "mul": 4}


def grid_scatter(src, flat_idx, B, grid_shape, reduce, with_stats=False, prezeroed=None, c_real=None):
    """-> channel-last volume [B][G0][G1][G2][C] (and its per-channel statistics, from the occupied cells only).
    prezeroed: (vol, cnt) from zeroed_volume that the caller has already ordered before this call.
    c_real: channels [c_real, C) of src are pads (zeros): they stay 0 in every cell, also under 'mul', whose empty cells are 1 elsewhere"""
    N, C = src.shape
    if reduce not in REDUCE_CODES:
        raise ValueError(f"grid_scatter: reduce={reduce!r} is not one of {sorted(REDUCE_CODES)}")
    if with_stats and reduce == "mul":
        raise ValueError("grid_scatter: the occupied-cell statistics assume empty cells are 0, which 'mul' leaves at 1")
    cps = int(np.prod(grid_shape))
    cells = B * cps
    if prezeroed is not None:
        vol, cnt = prezeroed
        assert vol.shape == (B,) + tuple(grid_shape) + (C,) and cnt.numel() == cells
    else:
        vol = torch.empty((B,) + tuple(grid_shape) + (C,), dtype=torch.float32, device=src.device)
        cnt = torch.empty(cells, dtype=_i32, device=src.device)
    code = REDUCE_CODES[reduce]
    nbytes = _lib.load().gn_grid_scatter_workspace_bytes(N, C, code)
    ws = _ws(nbytes, src.device) if nbytes else None
    _lib.call("gn_grid_scatter_ex", _p(src), rows_view(src)[1], _p(flat_idx), N, C, C if c_real is None else int(c_real), cells, code, _p(vol), _p(cnt),
              _p(ws), nbytes, 0 if prezeroed is None else 1, _stream())
    if not with_stats:
        return vol
    s, q = _stats_buffers(B, C, src.device, True)
    _lib.call("gn_grid_stats", _p(vol), _p(flat_idx), N, C, cps, B, _p(cnt), _p(s), _p(q), _stream())
    return vol, (s, q, cps)


# ------------------------------------------------------------------------------------------------ UNet
def channel_stats(x):
    """x channel-last [B][D][H][W][C] -> (sum, sumsq) fp64 [B][C]"""
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // (B * C)
    s, q = _stats_buffers(B, C, x.device, True)
    # (gn_channel_stats_any: the channel counts gn_channel_stats does not take -- the UNet's channel-padded widths 96, 160, 384 ...)
    narrow = (C <= 256 and 256 % C == 0) or C % 256 == 0
    _lib.call("gn_channel_stats" if narrow else "gn_channel_stats_any", _p(x), B, V, C, _p(s), _p(q), _stream())
    return s, q, V


def groupnorm_affine(st0, st1, groups, eps, gamma, beta, with_act_scale=False, real=None):
    """-> (a, d) [B][C0+C1]; with_act_scale: -> (a, d, act_inv_scale [B]) with the sample's power-of-two range normalisation folded
    into a and d (split-operand convs: conv3d_gcr_split undoes it in the epilogue).
    real: the real channel count of each source when the statistics cover channel-padded storage (C0, C1 stored): the groups are formed over
    the real channels (gamma / beta hold those), a = d = 0 on the pads (gn_groupnorm_affine_map, which also takes more than 1024 channels)"""
    s0, q0, V0 = st0
    B, C0 = s0.shape
    if st1 is not None:
        s1, q1, V1 = st1
        C1 = s1.shape[1]
        rep = V0 // V1
    else:
        s1 = q1 = None
        C1, V1, rep = 0, 0, 1
    a = torch.empty((B, C0 + C1), dtype=torch.float32, device=s0.device)
    d = torch.empty_like(a)
    inv = torch.empty(B, dtype=torch.float32, device=s0.device) if with_act_scale else None
    r0, r1 = (C0, C1) if real is None else (int(real[0]), int(real[1]) if len(real) > 1 else 0)
    if (r0, r1) == (C0, C1) and C0 + C1 <= GNA_MAXC:
        _lib.call("gn_groupnorm_affine", _p(s0), _p(q0), C0, V0, _p(s1), _p(q1), C1, V1, rep, B, groups, float(eps), _p(gamma), _p(beta),
                  _p(a), _p(d), _p(inv), _stream())
    else:
        _lib.call("gn_groupnorm_affine_map", _p(s0), _p(q0), r0, C0, V0, _p(s1), _p(q1), r1, C1, V1, rep, B, groups, float(eps), _p(gamma),
                  _p(beta), _p(a), _p(d), _p(inv), _stream())
    return (a, d, inv) if with_act_scale else (a, d)


GNA_MAXC = 1024        # gn_groupnorm_affine's channel limit; gn_groupnorm_affine_map takes what fits 160 KB of LDS


def pack_conv_weight(w):
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) -> [27 taps][Cin/16][Cout][16] (the B-operand pack of gn_conv3d_gcr)."""
    cout, cin = w.shape[:2]
    assert cin % 16 == 0
    return w.detach().float().permute(2, 3, 4, 1, 0).reshape(27, cin // 16, 16, cout).permute(0, 1, 3, 2).contiguous()


from .arith import CONV_FP32, CONV_MODE_NAMES, SPLIT_BF16X2, SPLIT_BF16X3, SPLIT_F16X2  # noqa: E402,F401  (which arithmetic runs is an arith.Arith carried by the call)


class SplitPack:
    """weight planes of the split-precision conv: .tensor (int16 bit patterns, MFMA-fragment order), .mode, .out_scale (fp32 [Cout]:
    the exact powers of two that undo the per-output-channel weight scales)"""

    def __init__(self, tensor, mode, out_scale):
        self.tensor, self.mode, self.out_scale = tensor, int(mode), out_scale

    def to(self, device):
        return SplitPack(self.tensor.to(device), self.mode, self.out_scale.to(device))


def pack_conv_weight_split(w, mode):
    """(Cout, Cin, 3,3,3) fp32 -> exact plane decomposition (w = w1 + w2 [+ w3], residual chain) in MFMA-fragment order
    [Cin/16][27][Cout/32][planes][h 2][r 32][8] (lane 32h+r holds channels 8h..8h+7 of cout 32*blk+r), followed by eight zero
    (slice, tap) steps: the kernels' fragment DMA runs up to two groups of three steps ahead of the last one.  mode SPLIT_BF16X2/3: bf16 planes;
    SPLIT_F16X2: two fp16 planes of w * 2^k(cout), k chosen PER OUTPUT CHANNEL so that the row maximum max|w[cout]| * 2^k is in [1, 2)
    (out_scale[cout] = 2^-k undoes it exactly): every weight within 2^3 of its row's largest keeps a normal second plane (residual
    <= 2^-22 |w|), smaller ones are carried to 2^-25 of the row maximum -- always far below the row's own dot-product magnitude,
    also for a heavy-tailed trained tensor (a per-TENSOR scale would push whole rows into the subnormal second plane)."""
    if mode not in (SPLIT_BF16X2, SPLIT_BF16X3, SPLIT_F16X2):
        raise ValueError(f"unknown split mode {mode}")
    cout, cin = w.shape[:2]
    w = w.detach().float()
    planes, dt = (2, torch.float16) if mode == SPLIT_F16X2 else (int(mode), torch.bfloat16)
    scale = torch.ones(cout, dtype=torch.float32)
    if mode == SPLIT_F16X2:
        m = w.reshape(cout, -1).abs().amax(dim=1).cpu()
        ok = torch.isfinite(m) & (m > 0)
        scale = torch.where(ok, torch.exp2(-torch.floor(torch.log2(torch.where(ok, m, torch.ones_like(m))))), scale).float()
    base = (w * scale.to(w.device).view(cout, 1, 1, 1, 1)).permute(2, 3, 4, 1, 0).reshape(27, cin // 16, 2, 8, cout // 32, 32)                # [tap][S][h][8][blk][r]
    base = base.permute(1, 0, 4, 2, 5, 3)                                                                # [S][tap][blk][h][r][8]
    out, r = [], base
    for _ in range(planes):
        p = r.to(dt)
        out.append(p)
        r = r - p.float()
    pk = torch.stack(out, dim=3).contiguous()                                                            # [S][tap][blk][planes][h][r][8]
    pk = pk.reshape(cin // 16 * 27, -1)
    pk = torch.cat([pk, torch.zeros_like(pk[:1]).repeat(8, 1)], dim=0)
    return SplitPack(pk.contiguous().view(torch.int16), mode, (1.0 / scale).contiguous().to(w.device))


def wino_supported(cin, cout, dims):
    """shapes gn_conv3d_gcr_split_wino takes: one source, 32-bit byte offsets inside a sample, and whole 4 x 8 x 8 tiles with Cin <= 256 for the 128-wide
    kernel (Cout % 128 == 0, csrc/unet_wino.hip) / whole 8 x 8 x 8 tiles with Cin <= 128 for the 32-wide column-block kernel (csrc/unet_wino32.hip)"""
    D, H, W = [int(v) for v in dims]
    if not (cin % 16 == 0 and cout % 32 == 0 and H % 8 == 0 and W % 8 == 0 and D * H * W <= (1 << 27) and D * H * W * cin * 4 < (1 << 32)):
        return False
    return (cin <= 256 and D % 4 == 0) if cout % 128 == 0 else (cin <= 128 and D % 8 == 0)


def pack_conv_weight_split_wino(w):
    """(Cout, Cin, 3,3,3) fp32 -> the Winograd F(2,3)-along-x pack of gn_conv3d_gcr_split_wino (csrc/unet_wino.hip): per (kd, kh, channel) the three
    kw taps g0 g1 g2 become the four transform positions (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2), in fp64; per-output-channel power-of-two
    scale over the TRANSFORMED row (row maximum in [1, 2)), two fp16 planes, fragment order [Cin/16][36 steps = (j * 3 + kd) * 3 + kh][Cout/32][plane]
    [h 2][r 32][8] + six zero steps (the kernel's fragment DMA runs two groups of three steps ahead)."""
    cout, cin = w.shape[:2]
    w = w.detach().double().cpu()
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    u = torch.einsum("jk,nczyk->nczyj", G, w)                                                           # (Cout, Cin, kd, kh, j)
    m = u.reshape(cout, -1).abs().amax(dim=1)
    scale = _pow2_floor_inv(m)
    base = (u * scale.view(cout, 1, 1, 1, 1)).float().permute(4, 2, 3, 1, 0).reshape(36, cin // 16, 2, 8, cout // 32, 32)   # [step][S][h][8][blk][r]
    base = base.permute(1, 0, 4, 2, 5, 3)                                                               # [S][step][blk][h][r][8]
    p1 = base.to(torch.float16)
    p2 = (base - p1.float()).to(torch.float16)
    pk = torch.stack((p1, p2), dim=3).contiguous().reshape(cin // 16 * 36, -1)                          # [S * step][blk][plane][h][r][8]
    pk = torch.cat([pk, torch.zeros_like(pk[:6])], dim=0)
    return SplitPack(pk.contiguous().view(torch.int16), SPLIT_F16X2, (1.0 / scale).float().contiguous())


def conv3d_gcr_split_wino(src, a, d, pack, cout, relu=True, with_stats=False, act_inv=None, tile_active=None, kconst=None, kreach=1, partial=None):
    """the literal form through the Winograd kernels (pack = pack_conv_weight_split_wino); partial: the polyphase partial of a decoder's first
    convolution (upconv_partial), 32- / 64-wide layers only"""
    return _conv3d_wino("conv3d_gcr_split_wino", src, a, d, pack.tensor, pack.out_scale, act_inv, None, cout, relu, with_stats, tile_active, kconst, kreach,
                        partial)


def _conv3d_wino(who, src, a, d, pack, out_scale, act_inv, kbias, cout, relu, with_stats, tile_active, kconst, kreach, partial):
    """both operand forms through the Winograd kernels (kbias None: literal, else affine-in-weights): gn_conv3d_gcr_split_wino, or its _partial entry
    when a polyphase partial is added (never occupancy-aware)"""
    B, D, H, W, C0 = src.shape
    if partial is not None and tile_active is not None:
        raise ValueError(f"{who}: the occupancy-aware launch cannot take a polyphase partial")
    out, s, q, ows, ows_bytes = _conv_outputs(src, cout, with_stats, tile_active)
    if partial is not None:
        _lib.call("gn_conv3d_gcr_split_wino_partial", _p(src), C0, _p(a), _p(d), _p(pack), _p(out_scale), _p(act_inv), _p(kbias), B, D, H, W, cout,
                  1 if relu else 0, _p(out), _p(s), _p(q), _p(_chk(partial, torch.float32, "partial")), _stream())
    else:
        _lib.call("gn_conv3d_gcr_split_wino", _p(src), C0, _p(a), _p(d), _p(pack), _p(out_scale), _p(act_inv), _p(kbias), B, D, H, W, cout,
                  1 if relu else 0, _p(out), _p(s), _p(q), _p(tile_active), _p(kconst), int(kreach), _p(ows), ows_bytes, _stream())
    return (out, (s, q, D * H * W)) if with_stats else out


def grid_tile_flags(flat_idx, B, grid_shape, reach=1):
    """uint8 [B][tiles]: the 4 x 8 x 8 output tiles of a 3x3x3 conv over the scattered volume that can see an occupied cell (reach 1),
    or of the conv behind it (reach 2)"""
    g0, g1, g2 = [int(v) for v in grid_shape]
    tiles = -(-g0 // 4) * -(-g1 // 8) * -(-g2 // 8)
    flags = torch.empty((B, tiles), dtype=torch.uint8, device=flat_idx.device)
    _lib.call("gn_grid_tile_flags", _p(_chk(flat_idx, _i32, "flat_idx")), flat_idx.numel(), B, g0, g1, g2, int(reach), _p(flags), _stream())
    return flags


def polyphase_weights(w, c0):
    """nn.Conv3d weight (Cout, C0 + C1, 3,3,3) of a layer that reads cat((skip [C0 ch], upsample_nearest_x2(x) [C1 ch])) ->
    (w0 (Cout, C0, 3,3,3): the full-resolution part unchanged;
     wm (8 * Cout, C1, 3,3,3): the upsampled part as a convolution over the COARSE volume, output channel (class, n), class = 4 pz + 2 py + px
         the parity of the fine output voxel: a fine tap d in {-1, 0, +1} of an even voxel lands on coarse offset {-1, 0, 0}, of an odd voxel
         on {0, 0, +1}, so the 27 fine taps merge (sums of weights, fp64) into 2 x 2 x 2 coarse taps per class -- exact algebra;
     tapmask int32 [27]: bit i = 32-wide output block i of wm has a non-zero weight at tap (kd * 3 + kh) * 3 + kw -- diagnostic: every
         class uses exactly 2 x 2 x 2 of the 27 coarse taps)."""
    w = w.detach().double().cpu()
    cout = w.shape[0]
    w0, w1 = w[:, :c0].float(), w[:, c0:]
    M = torch.zeros(2, 3, 3, dtype=torch.float64)            # [parity][coarse tap][fine tap]
    M[0, 0, 0] = M[0, 1, 1] = M[0, 1, 2] = 1.0
    M[1, 1, 0] = M[1, 1, 1] = M[1, 2, 2] = 1.0
    blocks = [torch.einsum("az,by,cx,nkzyx->nkabc", M[pz], M[py], M[px], w1) for pz in (0, 1) for py in (0, 1) for px in (0, 1)]
    wm = torch.cat(blocks, dim=0).float()                    # (8 * Cout, C1, 3, 3, 3)
    nz = (wm.reshape(8 * cout // 32, 32, -1, 27) != 0).any(dim=2).any(dim=1)       # [block][tap]
    mask = torch.zeros(27, dtype=torch.int64)
    for blk in range(nz.shape[0]):
        mask |= nz[blk].to(torch.int64) << blk
    return w0.contiguous(), wm.contiguous(), mask.to(torch.int32)


def pack_upconv_weight(wm, cout, mode):
    """merged polyphase weights wm (8 * cout, C1, 3,3,3) of polyphase_weights -> SplitPack for gn_upconv_partial: the 8 taps class
    (pz, py, px) uses are wm[..., pz + iz, py + iy, px + ix], i in {0,1}; fragment order [C1/16][tap = 4 iz + 2 iy + ix][class][cout/32]
    [plane][h][r][8] (lane 32 h + r holds channels 8h..8h+7 of output r of the block), per-row power-of-two scale for fp16 planes."""
    if mode not in (SPLIT_BF16X2, SPLIT_F16X2):
        raise ValueError("gn_upconv_partial runs the two-plane modes only")
    wm = wm.detach().float().cpu()
    c1 = wm.shape[1]
    assert wm.shape[0] == 8 * cout and c1 % 16 == 0 and cout % 32 == 0
    taps = torch.empty((8, 8, cout, c1), dtype=torch.float32)                                     # [class][tap][n][k]
    for c in range(8):
        pz, py, px = c >> 2, (c >> 1) & 1, c & 1
        for t in range(8):
            iz, iy, ix = t >> 2, (t >> 1) & 1, t & 1
            taps[c, t] = wm[c * cout:(c + 1) * cout, :, pz + iz, py + iy, px + ix]
    scale = torch.ones(8, cout)
    if mode == SPLIT_F16X2:
        m = taps.abs().amax(dim=(1, 3))
        ok = torch.isfinite(m) & (m > 0)
        scale = torch.where(ok, torch.exp2(-torch.floor(torch.log2(torch.where(ok, m, torch.ones_like(m))))), scale)
    dt = torch.float16 if mode == SPLIT_F16X2 else torch.bfloat16
    t_ = (taps * scale[:, None, :, None]).reshape(8, 8, cout // 32, 32, c1 // 16, 2, 8)            # [class][tap][blk][r][S][h][i]
    t_ = t_.permute(4, 1, 0, 2, 5, 3, 6)                                                          # [S][tap][class][blk][h][r][i]
    p1 = t_.to(dt)
    p2 = (t_ - p1.float()).to(dt)
    pk = torch.stack((p1, p2), dim=4).contiguous()                                                # [S][tap][class][blk][plane][h][r][i]
    return SplitPack(pk.view(torch.int16).reshape(-1), mode, (1.0 / scale).reshape(-1).contiguous())


def _device_pack_args(who, w, c_lo, c_n):
    """the checks the device builders share, before any launch: a raw fp32 contiguous Conv3d weight on the GPU and widths the kernels take
    -> (w detached, cout, cin, c_lo, c_n)"""
    if not isinstance(w, torch.Tensor) or w.dim() != 5 or tuple(w.shape[2:]) != (3, 3, 3):
        raise ValueError(f"{who}: expected a Conv3d weight (Cout, Cin, 3, 3, 3)")
    if w.dtype != torch.float32:
        raise ValueError(f"{who}: expected torch.float32, got {w.dtype}")
    if not w.is_contiguous():
        raise ValueError(f"{who}: the weight must be contiguous")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    c_lo = int(c_lo)
    c_n = cin - c_lo if c_n is None else int(c_n)
    if c_lo < 0 or c_n <= 0 or c_lo + c_n > cin:
        raise ValueError(f"{who}: input channels [{c_lo}, {c_lo + c_n}) outside the weight's {cin}")
    if c_n % 16 != 0 or cout % 32 != 0:
        raise ValueError(f"{who}: channels must be multiples of 16 (in) / 32 (out), got {c_n} / {cout}")
    if not w.is_cuda:
        raise ValueError(f"{who}: the weight must be on the GPU (the host builder takes a CPU tensor)")
    return w.detach(), cout, cin, c_lo, c_n


def pack_conv_weight_split_device(w, mode, c_lo=0, c_n=None):
    """pack_conv_weight_split(w[:, c_lo:c_lo + c_n], mode) built on the device (csrc/weight_pack.hip): same layout, same bits, no host round trip and
    no synchronising call.  w: the raw fp32 contiguous weight on the GPU; the channel range packs a polyphase layer's full-resolution part without a copy.
    Row scale from the exponent field of the row maximum: the rule pack_conv_weight_split documents (the host's log2 leaves a maximum a few ulps below
    a power of two in [0.5, 1); include/garmentnets_hip.h).  ValueError, before any launch: a CPU / non-contiguous / non-fp32 weight, refused widths"""
    if mode not in (SPLIT_BF16X2, SPLIT_BF16X3, SPLIT_F16X2):
        raise ValueError(f"unknown split mode {mode}")
    w, cout, cin, c_lo, c_n = _device_pack_args("pack_conv_weight_split_device", w, c_lo, c_n)
    planes = 2 if mode == SPLIT_F16X2 else int(mode)
    nbytes = _lib.load().gn_weight_pack_split_bytes(c_n, cout, int(mode))
    pk = torch.empty((nbytes // 2,), dtype=torch.int16, device=w.device).view(-1, cout // 32 * planes * 512)      # one row per (slice, tap) step
    scale = torch.empty((cout,), dtype=torch.float32, device=w.device)
    _lib.call("gn_weight_pack_split", _p(w), cout, cin, c_lo, c_n, int(mode), _p(pk), pk.numel() * 2, _p(scale), _stream())
    return SplitPack(pk, mode, scale)


def pack_conv_weight_split_wino_device(w, c_lo=0, c_n=None):
    """pack_conv_weight_split_wino(w[:, c_lo:c_lo + c_n]) built on the device (csrc/weight_pack.hip); as pack_conv_weight_split_device"""
    w, cout, cin, c_lo, c_n = _device_pack_args("pack_conv_weight_split_wino_device", w, c_lo, c_n)
    nbytes = _lib.load().gn_weight_pack_split_wino_bytes(c_n, cout)
    pk = torch.empty((nbytes // 2,), dtype=torch.int16, device=w.device).view(-1, cout // 32 * 2 * 512)
    scale = torch.empty((cout,), dtype=torch.float32, device=w.device)
    _lib.call("gn_weight_pack_split_wino", _p(w), cout, cin, c_lo, c_n, _p(pk), pk.numel() * 2, _p(scale), _stream())
    return SplitPack(pk, SPLIT_F16X2, scale)


def pack_upconv_weight_device(w, c0, mode):
    """pack_upconv_weight(polyphase_weights(w, c0)[1], Cout, mode) built on the device from the RAW weight (Cout, C0 + C1, 3,3,3): the merged weights are
    never materialised (csrc/weight_pack.hip); as pack_conv_weight_split_device"""
    if mode not in (SPLIT_BF16X2, SPLIT_F16X2):
        raise ValueError("gn_upconv_partial runs the two-plane modes only")
    w, cout, cin, c0, c1 = _device_pack_args("pack_upconv_weight_device", w, c0, None)
    pk = torch.empty((_lib.load().gn_weight_pack_upconv_bytes(c1, cout) // 2,), dtype=torch.int16, device=w.device)
    scale = torch.empty((8 * cout,), dtype=torch.float32, device=w.device)
    _lib.call("gn_weight_pack_upconv", _p(w), cout, cin, c0, int(mode), _p(pk), pk.numel() * 2, _p(scale), _stream())
    return SplitPack(pk, mode, scale)


def upconv_partial(src1, a1, d1, pack, cout, act_inv=None):
    """coarse source [B][Dc][Hc][Wc][C1] -> polyphase partial sums [B][Dc][Hc][Wc][8 * cout] (csrc/upconv.hip).  a1, d1 [B][C1]: the GroupNorm affine of
    THESE channels (the layer's a[:, c0:], not its full-width rows); act_inv [B] or None; pack: pack_upconv_weight[_device] of the same C1 and cout.
    TypeError / ValueError, before any launch: the kernel reads every one of them by the strides these shapes imply"""
    _chk(src1, torch.float32, "src1")
    if src1.dim() != 5:
        raise ValueError(f"src1: expected [B][Dc][Hc][Wc][C1], got {tuple(src1.shape)}")
    B, Dc, Hc, Wc, C1 = src1.shape
    cout = int(cout)
    for t, name in ((a1, "a"), (d1, "d")):
        if tuple(_chk(t, torch.float32, name).shape) != (B, C1):
            raise ValueError(f"{name}: expected [B][C1] = {(B, C1)} (the affine of the upsampled channels alone), got {tuple(t.shape)}")
    if act_inv is not None and tuple(_chk(act_inv, torch.float32, "act_inv").shape) != (B,):
        raise ValueError(f"act_inv: expected [B] = {(B,)}, got {tuple(act_inv.shape)}")
    if pack.mode not in (SPLIT_BF16X2, SPLIT_F16X2):
        raise ValueError("gn_upconv_partial runs the two-plane modes only")
    # (widths the entry refuses have no pack size: the entry names them)
    need = _lib.load().gn_weight_pack_upconv_bytes(C1, cout)
    have = _chk(pack.tensor, pack.tensor.dtype, "pack").numel() * pack.tensor.element_size()
    if need and have != need:
        raise ValueError(f"pack: {have} bytes, the polyphase pack of C1 = {C1}, cout = {cout} has {need} (pack_upconv_weight)")
    if tuple(_chk(pack.out_scale, torch.float32, "pack.out_scale").shape) != (8 * cout,):
        raise ValueError(f"pack.out_scale: expected [8 * cout] = {(8 * cout,)}, got {tuple(pack.out_scale.shape)}")
    part = torch.empty((B, Dc, Hc, Wc, 8 * cout), dtype=torch.float32, device=src1.device)
    _lib.call("gn_upconv_partial", _p(src1), C1, _p(a1), _p(d1), _p(pack.tensor), pack.mode, _p(pack.out_scale), _p(act_inv), B, Dc, Hc, Wc, cout,
              _p(part), _stream())
    return part


def conv3d_gcr_split(src0, src1, a, d, pack, cout, relu=True, with_stats=False, act_inv=None, tile_active=None, kconst=None, kreach=1,
                     partial=None):
    B, D, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[-1]
    out, s, q, ows, ows_bytes = _conv_outputs(src0, cout, with_stats, tile_active)
    _lib.call("gn_conv3d_gcr_split", _p(src0), C0, _p(src1), C1, _p(a), _p(d), _p(pack.tensor), pack.mode, _p(pack.out_scale), _p(act_inv), B, D, H, W, cout,
              1 if relu else 0, _p(out), _p(s), _p(q), _p(tile_active), _p(kconst), int(kreach), _p(partial), _p(ows), ows_bytes, _stream())
    return (out, (s, q, D * H * W)) if with_stats else out


class AffinePack:
    """what gn_conv_affine_pack prepared for ONE batch of one 'gcr' layer: per-sample fp16x2 weight sets with the GroupNorm affine folded
    in, the staging affine (s, -c s), the output scales and the border-class bias table"""
    __slots__ = ("pack", "stage_a", "stage_d", "out_scale", "kbias", "cin", "cout", "wino")


def conv_affine_pack(weight, a, d, stats, rest=None, wino=False):
    """weight: the raw Conv3d weight [Cout][Cin][3][3][3] (fp32, device); a, d [B][Cin]: the GroupNorm affine (groupnorm_affine without the
    sample scale); stats = (sum, sumsq, V) of the layer's input; rest [B][Cin] or None (zeros): the value the input holds away from its
    support -> AffinePack (csrc/conv_prep.hip).  wino: the pack holds the Winograd F(2,3)-along-x transformed weights (csrc/unet_wino.hip)"""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    B, dev = a.shape[0], a.device
    w = weight.detach()
    _chk(w, torch.float32, "weight")
    _chk(a, torch.float32, "a"); _chk(d, torch.float32, "d")
    if rest is not None:
        _chk(rest, torch.float32, "rest")
        assert tuple(rest.shape) == (B, cin)
    sfx = "_wino" if wino else ""
    nbytes = getattr(_lib.load(), "gn_conv_affine_pack" + sfx + "_bytes")(B, cin, cout)
    if nbytes == 0 and B > 0:
        raise ValueError("conv_affine_pack: channel counts must be multiples of 16 (in) / 32 (out)")
    r = AffinePack()
    r.cin, r.cout, r.wino = cin, cout, bool(wino)
    r.pack = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    r.stage_a = torch.empty((B, cin), dtype=torch.float32, device=dev)
    r.stage_d = torch.empty((B, cin), dtype=torch.float32, device=dev)
    r.out_scale = torch.empty((B, cout), dtype=torch.float32, device=dev)
    r.kbias = torch.empty((B, 64, cout), dtype=torch.float32, device=dev)
    # (16 bytes more than the entry asks for, as this wrapper has always passed: the recorded launch traces of the UNet hold that scalar)
    ws_bytes = _lib.load().gn_conv_affine_pack_workspace_bytes(B, cin, cout) + 16
    ws = _ws(ws_bytes, dev)
    _lib.call("gn_conv_affine_pack" + sfx, _p(w), cin, cout, _p(a), _p(d), _p(stats[0]), _p(stats[1]), int(stats[2]), _p(rest), B, _p(r.pack), nbytes,
              _p(r.stage_a), _p(r.stage_d), _p(r.out_scale), _p(r.kbias), _p(ws), ws_bytes, _stream())
    return r


def conv3d_gcr_split_persample(src, prep, relu=True, with_stats=False, tile_active=None, kconst=None, kreach=1, partial=None):
    """the 'gcr' layer from an AffinePack (GN_SPLIT_F16X2 arithmetic; the operand is exactly zero wherever the input is at rest)"""
    B, D, H, W, C = src.shape
    assert C == prep.cin and B == prep.stage_a.shape[0]
    if prep.wino:
        return _conv3d_wino("conv3d_gcr_split_persample", src, prep.stage_a, prep.stage_d, prep.pack, prep.out_scale, None, prep.kbias, prep.cout, relu,
                            with_stats, tile_active, kconst, kreach, partial)
    out, s, q, ows, ows_bytes = _conv_outputs(src, prep.cout, with_stats, tile_active)
    _lib.call("gn_conv3d_gcr_split_persample", _p(src), C, _p(prep.stage_a), _p(prep.stage_d), _p(prep.pack), _p(prep.out_scale), _p(prep.kbias),
              B, D, H, W, prep.cout, 1 if relu else 0, _p(out), _p(s), _p(q), _p(tile_active), _p(kconst), int(kreach), _p(partial), _p(ows), ows_bytes,
              _stream())
    return (out, (s, q, D * H * W)) if with_stats else out


def _occupancy_ws(tile_active, B, D, H, W, device):
    """workspace of an occupancy-aware conv launch (the compact list of active tiles): (tensor | None, bytes)"""
    if tile_active is None:
        return None, 0
    n = _lib.load().gn_conv3d_occupancy_workspace_bytes(B, D, H, W)
    return _ws(n, device), n


def _conv_outputs(src, cout, with_stats, tile_active):
    """what a split-operand conv launch over src [B][D][H][W][C] writes: (the output [B][D][H][W][cout], the sum and sumsq buffers of its statistics
    or None twice, the occupancy workspace or None, its bytes)"""
    B, D, H, W = src.shape[:4]
    out = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=src.device)
    return (out,) + _stats_buffers(B, cout, src.device, with_stats) + _occupancy_ws(tile_active, B, D, H, W, src.device)


def _stats_buffers(B, C, device, want):
    if not want:
        return None, None
    sq = torch.empty((2, B, C), dtype=torch.float64, device=device)      # back to back: the library zeroes the pair with one fill (gn_zero_stats)
    return sq[0], sq[1]


def conv3d_gcr(src0, src1, a, d, wp, cout, relu=True, with_stats=False):
    """-> out, or (out, (sum, sumsq, V)) with the statistics of the output when with_stats"""
    B, D, H, W, C0 = src0.shape
    C1 = 0 if src1 is None else src1.shape[-1]
    out = torch.empty((B, D, H, W, cout), dtype=torch.float32, device=src0.device)
    s, q = _stats_buffers(B, cout, src0.device, with_stats)
    _lib.call("gn_conv3d_gcr", _p(src0), C0, _p(src1), C1, _p(a), _p(d), _p(wp), B, D, H, W, cout, 1 if relu else 0, _p(out),
              _p(s), _p(q), _stream())
    return (out, (s, q, D * H * W)) if with_stats else out


ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_ELU = 0, 1, 2, 3


def affine_act(x, a=None, d=None, bias=None, act=ACT_NONE, out=None):
    """y = act(x * a[b][c] + d[b][c] + bias[c]) over a channel-last volume [B][...][C] (gn_affine_act: the non-'gcr' layer orders' odds and ends);
    in place when out is x"""
    B, C = x.shape[0], x.shape[-1]
    V = x.numel() // max(B * C, 1)
    if out is None:
        out = torch.empty_like(x)
    _lib.call("gn_affine_act", _p(x), B, V, C, _p(a), _p(d), _p(bias), int(act), _p(out), _stream())
    return out


def maxpool3d_2(x, with_stats=False):
    B, D, H, W, C = x.shape
    out = torch.empty((B, D // 2, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    # the kernel's statistics epilogue takes C / 4 | 256; other widths get their statistics from one gn_channel_stats(_any) pass
    epilogue = with_stats and 0 < C <= 256 and C % 4 == 0 and 256 % (C // 4) == 0
    s, q = _stats_buffers(B, C, x.device, epilogue)
    _lib.call("gn_maxpool3d_2", _p(x), B, D, H, W, C, _p(out), _p(s), _p(q), _stream())
    if with_stats and not epilogue:
        return out, channel_stats(out)
    return (out, (s, q, (D // 2) * (H // 2) * (W // 2))) if with_stats else out


# ------------------------------------------------------------------------------------------------ decoder
def trilinear_sample(vol_b, query=None, Q=0, m0=0, M=None, out=None):
    """vol_b: one sample, channel-last [D][H][W][C], packed fp32.  query [M][3] or lattice rows m0..m0+M of (Q,Q,Q)."""
    D, H, W, C = _chk(vol_b, torch.float32, "vol_b").shape
    if query is not None:
        M = query.shape[0]
        _chk(query, torch.float32, "query")
    if out is None:
        out = new_rows(M, C, vol_b.device)
    elif out.dtype != torch.float32:
        raise TypeError(f"out: expected {torch.float32}, got {out.dtype}")
    _lib.call("gn_trilinear_sample", _p(vol_b), D, H, W, C, _p(query), int(Q), int(m0), int(M), _p(out), rows_view(out)[1], _stream())
    return out


def pack_kpair(w):
    """Linear weight W[n][k] -> Wp[k/16][n][2][8] with Wp[g][n][h][j] = W[n][16g + 8h + j]: the B-operand pack of
    gn_implicit_decode (32 contiguous bytes per lane, 2 KB per wave per 16-deep k-group)."""
    n, k = w.shape
    assert k % 16 == 0
    return w.detach().float().reshape(n, k // 16, 2, 8).permute(1, 0, 2, 3).contiguous()


def implicit_decode(vol_b, layers, query=None, Q=0, m0=0, M=None, out=None, xin=None, run_if=None):
    """vol_b [D][H][W][C0]; layers = ((w1p,b1,s1,t1,N1), (w2p,b2,s2,t2,N2), (w3,b3,s3,t3,OUT)) -> out [M][OUT].
    xin: optional pre-sampled rows [M][C0] (then only the MLP runs).  run_if: optional device float; the launch is a no-op unless it
    is non-zero (the fp32 twin of a gated implicit_decode_split call)."""
    (w1p, b1, s1, t1, N1), (w2p, b2, s2, t2, N2), (w3, b3, s3, t3, OUT) = layers
    if xin is not None:
        if xin.dtype != torch.float32:
            raise TypeError(f"xin: expected {torch.float32}, got {xin.dtype}")
        D = H = W = 0
        M, C0 = xin.shape
        ldxin = rows_view(xin)[1]
        vol_b = None                                    # (unused by the kernel)
    else:
        D, H, W, C0 = _chk(vol_b, torch.float32, "vol_b").shape
        ldxin = 0
    if query is not None:
        M = query.shape[0]
        _chk(query, torch.float32, "query")
    if out is None:
        out = torch.empty((M, OUT), dtype=torch.float32, device=(xin if xin is not None else vol_b).device)
    elif out.dtype != torch.float32:
        raise TypeError(f"out: expected {torch.float32}, got {out.dtype}")
    _lib.call("gn_implicit_decode", _p(vol_b), D, H, W, C0, _p(xin), ldxin, _p(query), int(Q), int(m0), int(M), _p(w1p), _p(b1), _p(s1), _p(t1), N1,
              _p(w2p), _p(b2), _p(s2), _p(t2), N2, _p(w3), _p(b3), _p(s3), _p(t3), OUT, _p(out), rows_view(out)[1], _p(run_if), _stream())
    return out


def _chk_row_sets(t, name):
    """t (B, M, C) fp32 as the batch kernels address it: rows of unit stride, leading dimension stride(1), row sets packed back to back"""
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected {torch.float32}, got {t.dtype}")
    if t.dim() == 3 and t.numel() == 0:              # (nothing is addressed: the kernels return before any launch)
        return t
    if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1) or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
        raise ValueError(f"{name}: need (B, M, C) rows of unit stride, the row sets packed back to back")
    return t


def trilinear_sample_batch(vol, query, out=None):
    """vol (B, D, H, W, C) channel-last, query (B, M, 3) -> rows (B, M, C) [leading dimension padded to 4]: every volume's queries in one launch"""
    B, D, H, W, C = vol.shape
    M = query.shape[1]
    _chk(vol, torch.float32, "vol")
    _chk(query, torch.float32, "query")
    if out is None:
        out = torch.empty((B, M, pad4(C)), dtype=torch.float32, device=vol.device)[:, :, :C]
    _chk_row_sets(out, "out")
    _lib.call("gn_trilinear_sample_batch", _p(vol), B, vol.stride(0), D, H, W, C, _p(query), int(M), _p(out), out.stride(1), _stream())
    return out


def implicit_decode_batch(xin, layers, out, run_if=None, run_if_stride=0):
    """implicit_decode(xin=...) for B row sets in one launch: xin (B, M, C0) [row stride = leading dimension], out (B, M, OUT); run_if: one device flag per
    row set at run_if[b * run_if_stride] (the gated fp32 twin of implicit_decode_split_batch)"""
    (w1p, b1, s1, t1, N1), (w2p, b2, s2, t2, N2), (w3, b3, s3, t3, OUT) = layers
    B, M, C0 = _chk_row_sets(xin, "xin").shape
    _chk_row_sets(out, "out")
    _lib.call("gn_implicit_decode_batch", _p(xin), xin.stride(1), int(M), B, C0, _p(w1p), _p(b1), _p(s1), _p(t1), N1, _p(w2p), _p(b2), _p(s2), _p(t2), N2,
              _p(w3), _p(b3), _p(s3), _p(t3), OUT, _p(out), out.stride(1), _p(run_if), int(run_if_stride), _stream())
    return out


def implicit_decode_split_batch(xin, pack, out, xscale=None):
    """implicit_decode_split for B row sets in ONE launch: xin (B, M, C0), out (B, M, OUT), xscale None or (B, 4) -- row set b with its own input scale
    record; row for row the results of the single call (the persistent workgroups are shared between the sets through blockIdx.y)"""
    B, M, C0 = xin.shape
    assert xin.stride(0) == M * xin.stride(1) and out.stride(0) == M * out.stride(1), "row sets must be packed back to back"
    _lib.call("gn_implicit_decode_split_batch", _p(xin), xin.stride(1), int(M), B, _p(pack.wpack), _p(pack.tab), _p(xscale),
              C0, pack.hidden, pack.hidden, pack.out_channels, _p(out), out.stride(1), _stream())
    return out


class DecodeSplitPack:
    """weights / epilogue tables of gn_implicit_decode_split for one [128 | 32, 256, 256, OUT] decoder; smax: upper bound for the run-time
    input scale (keeps the scaled biases small, see pack_decode_split)"""

    def __init__(self, wpack, tab, smax, out_channels, hidden=256):
        self.wpack, self.tab, self.smax, self.out_channels, self.hidden = wpack, tab, float(smax), int(out_channels), int(hidden)

    def to(self, device):
        return DecodeSplitPack(self.wpack.to(device), self.tab.to(device), self.smax, self.out_channels, self.hidden)


def _pow2_floor_inv(m):
    """per-row power of two r with r * m in [1, 2) (1 where m is 0 / non-finite); m: fp64 tensor"""
    ok = torch.isfinite(m) & (m > 0)
    return torch.where(ok, torch.exp2(-torch.floor(torch.log2(torch.where(ok, m, torch.ones_like(m))))), torch.ones_like(m))


def _d_unit(q, h):
    """hidden unit (within a 32-unit block) held by accumulator register q of lane half h (32x32 MFMA D layout)"""
    return (q & 3) + 8 * (q >> 2) + 4 * h


def pack_decode_split(layers):
    """layers = ((w1,b1,s1,t1), (w2,b2,s2,t2), (w3,b3,s3,t3)) with w1 (N,128) or (N,32), w2 (N,N), w3 (OUT,N) fp32, N = 256 (the shipped decoders) or 512
    (the class default, networks/conv_implicit_wnf.py:122; 32-channel folded input only), s/t = folded BatchNorm scale/shift or None -> DecodeSplitPack.
    The BatchNorm affine of hidden layer i is folded into layer i+1 (W' = W diag(s), b' = b + W t, in fp64).  Every hidden unit j carries a static
    power-of-two scale r_j (its weight row's maximum scaled into [1, 2)): the kernel keeps hidden activations in those units (r_j * s_x * h_j, s_x =
    the garment's run-time input scale) and 1 / r_j is folded into the next layer's column j -- all exact.  Weight stages of 16 KB:
    [4 k-groups][2 blocks][2 planes][64 lanes][8 fp16], steps in (block pair, k-group) order, layer 1 then layer 2; layer 2's k order follows the
    register layout the layer-1 accumulators already have (see csrc/decode_split.hip).  w1 (N, 32): the first layer with the UNet's final 1x1x1
    convolution folded in (ImplicitWNFDecoder.folded_pack)."""
    (w1, b1, s1, t1), (w2, b2, s2, t2), (w3, b3, s3, t3) = layers
    dd = lambda v, n, fill: (torch.full((n,), fill, dtype=torch.float64) if v is None else v.detach().double().cpu())
    w1, w2, w3 = w1.detach().double().cpu(), w2.detach().double().cpu(), w3.detach().double().cpu()
    out_c, N = w3.shape[0], w2.shape[0]
    assert N in (256, 512) and w1.shape[0] == N and w2.shape == (N, N) and w3.shape[1] == N and 1 <= out_c <= 4
    assert w1.shape[1] in ((128, 32) if N == 256 else (32,)), "the 512-wide pack takes the folded 32-channel first layer"
    k0g, npair, nb_, kg2 = w1.shape[1] // 16, N // 64, N // 32, N // 16                           # 16-deep k-groups of layer 1; block pairs, blocks, k-groups of layer 2
    b2f = dd(b2, N, 0.0) + w2 @ dd(t1, N, 0.0)
    w2 = w2 * dd(s1, N, 1.0)[None, :]
    b3f = (dd(b3, out_c, 0.0) + w3 @ dd(t2, N, 0.0)).float()
    w3 = w3 * dd(s2, N, 1.0)[None, :]
    b1f = dd(b1, N, 0.0)
    # per-unit scales (exact powers of two); a weight or bias that leaves fp32's range through them would be a broken checkpoint anyway
    r1 = _pow2_floor_inv(w1.abs().amax(dim=1))
    w1s, b1s = (w1 * r1[:, None]).float(), (b1f * r1).float()
    w2 = w2 / r1[None, :]
    r2 = _pow2_floor_inv(w2.abs().amax(dim=1))
    w2s, b2s = (w2 * r2[:, None]).float(), (b2f * r2).float()
    w3s = (w3 / r2[None, :]).float()
    # run-time input scale s_x <= smax keeps every scaled bias below 2^13 (hidden values = accumulator + bias stay inside fp16)
    bmax = max(float(b1s.abs().max()), float(b2s.abs().max()))
    smax = 2.0 ** 60 if not (bmax > 0 and math.isfinite(bmax)) else min(2.0 ** 60, 2.0 ** math.floor(math.log2(8192.0 / bmax)))
    ar = torch.arange
    bp, g1, blk, h, r, i = torch.meshgrid(ar(npair), ar(k0g), ar(2), ar(2), ar(32), ar(8), indexing="ij")
    a1 = w1s[32 * (2 * bp + blk) + r, 16 * g1 + 8 * h + i]                                       # [pair][k-group][blk][h][r][i]
    bp, g2, blk, h, r, i = torch.meshgrid(ar(npair), ar(kg2), ar(2), ar(2), ar(32), ar(8), indexing="ij")
    q = 8 * (g2 & 1) + i
    a2 = w2s[32 * (2 * bp + blk) + r, 32 * (g2 >> 1) + (q & 3) + 8 * (q >> 2) + 4 * h]          # [pair][k-group][blk][h][r][i]

    def planes(a):                                   # [..steps..][blk][h][r][i] -> [stage][4 steps][blk][plane][h][r][i]
        p1 = a.to(torch.float16)
        p2 = (a - p1.float()).to(torch.float16)
        st = torch.stack((p1, p2), dim=-4)                                                        # [...][blk][plane][h][r][i]
        return st.reshape(-1, 4, 2, 2, 2, 32, 8)                                                  # steps in (pair, k-group) order, 4 per stage

    wpack = torch.cat((planes(a1), planes(a2)), dim=0).contiguous().view(torch.int16)             # [(npair * (k0g + kg2)) / 4 stages][...]
    assert wpack.numel() * 2 == npair * (k0g + kg2) // 4 * 16384
    nb, hh, qq = torch.meshgrid(ar(nb_), ar(2), ar(16), indexing="ij")
    u = 32 * nb + (qq & 3) + 8 * (qq >> 2) + 4 * hh                                               # [blocks][2][16]
    tab1 = b1s[u]
    tab2 = torch.stack([b2s[u]] + [w3s[o][u] for o in range(out_c)], dim=2)                       # [blocks][2][1+OUT][16]
    tail = torch.stack((b3f, dd(s3, out_c, 1.0).float(), dd(t3, out_c, 0.0).float()))
    tab = torch.cat((tab1.reshape(-1), tab2.reshape(-1), tail.reshape(-1))).float().contiguous()
    return DecodeSplitPack(wpack, tab, smax, out_c, hidden=N)


def decoder_input_scale(sumsq, V, smax):
    """per-garment input scale of gn_implicit_decode_split from the per-(sample, channel) sums of squares of the sampled volume
    -> float32 [B][4] = (s, 1/s, unsafe, 0); unsafe = 1: the garment goes to the gated fp32 kernel (decided on the device)"""
    B, C = sumsq.shape
    out = torch.empty((B, 4), dtype=torch.float32, device=sumsq.device)
    _lib.call("gn_decoder_input_scale", _p(_chk(sumsq, torch.float64, "sumsq")), int(V), B, C, float(smax), _p(out), _stream())
    return out


def implicit_decode_split(xin, pack, out=None, xscale=None):
    """pre-sampled rows xin [M][128 | 32] -> out [M][OUT] through the [128 | 32, 256, 256, OUT] decoder on the 16-bit matrix cores.
    xscale: the garment's (s, 1/s, unsafe, 0) row of decoder_input_scale (None: unscaled rows -- fine for O(1) inputs only); with
    unsafe != 0 the launch is a no-op and the caller's implicit_decode(..., run_if=xscale[2:3]) fills `out`"""
    M, C0 = xin.shape
    if out is None:
        out = torch.empty((M, pack.out_channels), dtype=torch.float32, device=xin.device)
    _lib.call("gn_implicit_decode_split", _p(xin), rows_view(xin)[1], int(M), _p(pack.wpack), _p(pack.tab), _p(xscale),
              C0, pack.hidden, pack.hidden, pack.out_channels, _p(out), rows_view(out)[1], _stream())
    return out


def implicit_decode_lattice_split(vol_b, Q, pack, out, xscale=None, m0=0, M=None):
    """rows m0 .. m0+M-1 of the (Q,Q,Q) lattice through the folded scalar decoder, sampled INSIDE the decoder kernel from the channel-last
    volume vol_b [D][H][W][32] (bricks of 4 x 8 x 8 lattice points out of LDS, no sampled-row buffer); bit-identical to trilinear_sample +
    implicit_decode_split.  Needs Q >= D, H, W (lattice_split_supported(vol_b, pack, Q))"""
    D, H, W, C0 = vol_b.shape
    M = Q * Q * Q - m0 if M is None else M
    _lib.call("gn_implicit_decode_lattice_split", _p(_chk(vol_b, torch.float32, "vol")), D, H, W, C0, int(Q), int(m0), int(M), _p(pack.wpack), _p(pack.tab),
              _p(xscale), pack.hidden, pack.hidden, pack.out_channels, _p(out), rows_view(out)[1], _stream())
    return out


def lattice_split_shapes(dims, c0, hidden, out_channels, Q=None):
    """the shapes implicit_decode_lattice_split takes: a (D, H, W) volume of c0 channels, the decoder's widths -- and, with Q, the lattice: a brick's
    voxel box is bounded only when the lattice is at least as fine as the volume (Q >= D, H, W), a coarser lattice keeps the sampler + decoder pair"""
    D, H, W = dims
    if Q is not None and not max(2, D, H, W) <= Q <= 1024:
        return False
    return c0 == 32 and out_channels == 1 and hidden == 256 and D * H * W * 128 < 2 ** 32


def lattice_split_supported(vol_b, pack, Q=None):
    """whether implicit_decode_lattice_split takes this (contiguous) volume and decoder pack -- and, with Q, this lattice (lattice_split_shapes)"""
    return lattice_split_shapes(tuple(vol_b.shape[:3]), vol_b.shape[3], pack.hidden, pack.out_channels, Q) and vol_b.is_contiguous()


# ------------------------------------------------------------------------------------------------ isosurface
def _ggm_tmp(shape, sigma, device):
    """the 8-pass form's workspace; None for the fused launch (kernel radius <= 2: csrc/iso.hip GGM_R)"""
    return None if int(4.0 * float(sigma) + 0.5) <= 2 else torch.empty((2,) + tuple(shape), dtype=torch.float32, device=device)


def ggm3d(vol, sigma):
    _chk(vol, torch.float32, "vol")
    n0, n1, n2 = vol.shape
    tmp = _ggm_tmp(vol.shape, sigma, vol.device)
    out = torch.empty_like(vol)
    _lib.call("gn_ggm3d", _p(vol), n0, n1, n2, float(sigma), _p(tmp), _p(out), _stream())
    return out


def minmax(x):
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _lib.call("gn_minmax", _p(_chk(x, torch.float32, "x")), x.numel(), _p(out), _stream())
    return out


def ggm3d_batch(vols, sigma):
    """ggm3d of every (n0,n1,n2) volume of a (B,n0,n1,n2) batch in one set of launches"""
    _chk(vols, torch.float32, "vols")
    B, n0, n1, n2 = vols.shape
    tmp = _ggm_tmp(vols.shape, sigma, vols.device)
    out = torch.empty_like(vols)
    _lib.call("gn_ggm3d_batch", _p(vols), B, n0, n1, n2, float(sigma), _p(tmp), _p(out), _stream())
    return out


def ggm3d_batch_range(vols, sigma, accum_bits=64):
    """ggm3d_batch + the (B,2) float32 (min, max) record of every volume from the same launch (NaN-propagating like numpy's; no pass of its own
    over the volumes: gn_ggm3d_batch_ex).  accum_bits=32: the taps accumulate in fp32 (no scipy bit-parity; Arith.ggm_fp32)"""
    _chk(vols, torch.float32, "vols")
    B, n0, n1, n2 = vols.shape
    tmp = _ggm_tmp(vols.shape, sigma, vols.device)
    out = torch.empty_like(vols)
    rng = torch.empty((B, 2), dtype=torch.float32, device=vols.device)
    nws = _lib.load().gn_ggm3d_range_workspace_bytes(B, n0, n1, n2)             # a (min, max) pair per wave of the fused launch; scratch
    ws = _ws(nws, vols.device)
    _lib.call("gn_ggm3d_batch_ex", _p(vols), B, n0, n1, n2, float(sigma), _p(tmp), _p(out), int(accum_bits), _p(rng), _p(ws), nws, _stream())
    return out, rng


def minmax_batch(vols):
    """-> (B,2) float32: (min, max) of every volume of a (B,...) batch (NaN-propagating: a NaN anywhere gives NaN, as numpy.min / numpy.max)"""
    _chk(vols, torch.float32, "vols")
    B = vols.shape[0]
    out = torch.empty((B, 2), dtype=torch.float32, device=vols.device)
    if B:
        _lib.call("gn_minmax_batch", _p(vols), B, vols.numel() // B, _p(out), _stream())
    return out


def mc33_batch(vols, level, cap_v, cap_f):
    """mc33 of every volume of a (B,n0,n1,n2) batch at one level in one set of launches
    -> verts_vox [B][cap_v][3], faces [B][cap_f][3], normals, values [B][cap_v], counts (device int64 [B][2] = V, F)"""
    _chk(vols, torch.float32, "vols")
    B, n0, n1, n2 = vols.shape
    dev = vols.device
    nbytes = _lib.load().gn_mc33_batch_workspace_bytes(B, n0, n1, n2)
    ws = _ws(nbytes, dev)
    verts = torch.zeros((B, cap_v, 3), dtype=torch.float32, device=dev)      # rows past a volume's vertex count stay finite (padded consumers)
    faces = torch.empty((B, cap_f, 3), dtype=_i32, device=dev)
    normals = torch.empty((B, cap_v, 3), dtype=torch.float32, device=dev)
    values = torch.empty((B, cap_v), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    _lib.call("gn_mc33_batch", _p(vols), B, n0, n1, n2, float(level), _p(ws), nbytes, _p(verts), _p(faces), _p(normals), _p(values), cap_v, cap_f,
              _p(counts), _stream())
    return verts, faces, normals, values, counts


def mc33_batch_profiled(vols, level, cap_v=None):
    """bench.py's hbm_members: one gn_mc33_batch of the (B,Q,Q,Q) batch with its stages timed inside the call (it synchronises) ->
    {stage: (ms, algorithmic bytes)}; bytes: classify = the volume once + one count byte per cell; scan = the block sums; vertices =
    (12 + 12 + 4) B per vertex + the count bytes; faces = 12 B per face + the count bytes"""
    _chk(vols, torch.float32, "vols")
    B, n0, n1, n2 = vols.shape
    dev = vols.device
    cap_v = int(cap_v or max(4096, 6 * n0 * n0))
    cap_f = 2 * cap_v + 64
    while True:
        nbytes = _lib.load().gn_mc33_batch_workspace_bytes(B, n0, n1, n2)
        ws = _ws(nbytes, dev)
        verts = torch.empty((B, cap_v, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((B, cap_f, 3), dtype=_i32, device=dev)
        normals = torch.empty((B, cap_v, 3), dtype=torch.float32, device=dev)
        values = torch.empty((B, cap_v), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
        ms = (ctypes.c_float * 4)()
        _lib.call("gn_mc33_batch_profiled", _p(vols), B, n0, n1, n2, float(level), _p(ws), nbytes, _p(verts), _p(faces), _p(normals), _p(values), cap_v, cap_f,
                  _p(counts), _stream(), ms)
        c = counts.cpu()
        nv, nf = int(c[:, 0].max()), int(c[:, 1].max())
        if nv <= cap_v and nf <= cap_f:
            break
        cap_v = max(nv, (nf + 1) // 2) + 64
        cap_f = 2 * cap_v + 64
    V, F = int(c[:, 0].sum()), int(c[:, 1].sum())
    cells = float(B) * (n0 - 1) * (n1 - 1) * (n2 - 1)
    return {"mc_classify": (ms[0], vols.numel() * 4.0 + cells), "mc_scan": (ms[1], cells / 1024 * 16.0), "mc_vertices_attrs": (ms[2], V * 28.0 + cells),
            "mc_faces": (ms[3], F * 12.0 + cells), "_mesh": (0.0, float(V))}


def mc33(vol, level, cap_v, cap_f):
    """-> verts_vox [cap_v][3], faces [cap_f][3], normals, values, counts (device int64 [2] = V, F)"""
    _chk(vol, torch.float32, "vol")
    n0, n1, n2 = vol.shape
    dev = vol.device
    nbytes = _lib.load().gn_mc33_workspace_bytes(n0, n1, n2)
    ws = _ws(nbytes, dev)
    verts = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((cap_f, 3), dtype=_i32, device=dev)
    normals = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
    values = torch.empty(cap_v, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.call("gn_mc33", _p(vol), n0, n1, n2, float(level), _p(ws), nbytes, _p(verts), _p(faces), _p(normals), _p(values), cap_v, cap_f,
              _p(counts), _stream())
    return verts, faces, normals, values, counts


def gather_nn(vol, verts_vox, spacing):
    nv = verts_vox.shape[0]
    out = torch.empty(nv, dtype=torch.float32, device=vol.device)
    _lib.call("gn_gather_nn", _p(vol), *vol.shape, _p(verts_vox), nv, float(spacing), _p(out), _stream())
    return out


def gather_nn_batch(vols, verts_vox, spacing):
    """vols (B,n0,n1,n2), verts_vox (B,M,3) padded rows -> (B,M): the nearest-voxel value of every row in its own volume"""
    B, M = verts_vox.shape[:2]
    out = torch.empty((B, M), dtype=torch.float32, device=vols.device)
    _lib.call("gn_gather_nn_batch", _p(_chk(vols, torch.float32, "vols")), B, *vols.shape[1:], _p(_chk(verts_vox, torch.float32, "verts_vox")), M, float(spacing),
              _p(out), _stream())
    return out


def scale_verts(verts_vox, spacing):
    out = torch.empty_like(verts_vox)
    _lib.call("gn_scale_verts", _p(verts_vox), verts_vox.shape[0], float(spacing), _p(out), _stream())
    return out


def mesh_compact(verts, faces, on_surface):
    """delete_invalid_verts on the GPU -> (verts' (V',3) same dtype, faces' (F',3) int32); one host synchronisation for the two sizes.
    A face index outside [0, V) raises IndexError, as the reference's numpy indexing does (common/marching_cubes_util.py:41)."""
    assert verts.dim() == 2 and verts.shape[1] == 3 and verts.dtype in (torch.float32, torch.float64)
    verts = verts.contiguous()
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"faces: expected an integer tensor, got {faces.dtype}")
    if verts.shape[0] >= 2 ** 31:
        raise ValueError("mesh_compact: more than 2^31 vertices")
    if faces.dtype == torch.int64:          # int32 on the device; an index that does not fit is out of range for any V < 2^31: keep it so
        faces = faces.clamp(min=-1, max=2 ** 31 - 1)
    faces = _chk(faces.to(torch.int32).contiguous(), torch.int32, "faces")
    flag = on_surface.to(torch.uint8).contiguous()
    V, F = verts.shape[0], faces.shape[0]
    if flag.numel() != V:
        raise ValueError("is_vert_on_surface must have one entry per vertex")
    nbytes = _lib.load().gn_mesh_compact_workspace_bytes(V, F)
    ws = _ws(nbytes, verts.device)
    out_v, out_f = torch.empty_like(verts), torch.empty_like(faces)
    counts = torch.empty(3, dtype=torch.int64, device=verts.device)
    _lib.call("gn_mesh_compact", _p(verts), verts.element_size() * 3, _p(faces), _p(flag), V, F, _p(ws), nbytes, _p(out_v), _p(out_f), _p(counts), _stream())
    nv, nf, bad = [int(c) for c in counts.cpu()]
    if bad:
        raise IndexError(f"delete_invalid_verts: a face index is out of bounds for {V} vertices")
    return out_v[:nv], out_f[:nf]


def mesh_largest_component(faces, num_verts, with_labels=False):
    """eval.py:497-503: -> (is_cc_vert bool [V], info dict) -- the vertices of the largest connected component of the mesh (ties: the
    component holding the lowest vertex index, as np.argmax over libigl's numbering); info: num_components, size, label [, labels]."""
    if faces.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"faces: expected an integer tensor, got {faces.dtype}")
    V, F = int(num_verts), faces.shape[0]
    if V >= 2 ** 31:
        raise ValueError("mesh_largest_component: more than 2^31 vertices")
    if F == 0:
        raise ValueError("attempt to get argmax of an empty sequence")          # what np.argmax(cc_sizes) says for a mesh without faces
    if faces.dtype == torch.int64:
        faces = faces.clamp(min=-1, max=2 ** 31 - 1)
    faces = _chk(faces.to(torch.int32).contiguous(), torch.int32, "faces")
    dev = faces.device
    nbytes = _lib.load().gn_mesh_largest_component_workspace_bytes(V)
    ws = _ws(nbytes, dev)
    mask = torch.empty(V, dtype=torch.uint8, device=dev)
    label = torch.empty(V, dtype=_i32, device=dev) if with_labels else None
    info = torch.empty(4, dtype=torch.int64, device=dev)
    _lib.call("gn_mesh_largest_component", _p(faces), F, V, _p(ws), nbytes, _p(mask), _p(label), _p(info), _stream())
    ncomp, size, lab, bad = [int(c) for c in info.cpu()]
    if bad:
        raise IndexError(f"connected components: a face index is out of bounds for {V} vertices")
    out = dict(num_components=ncomp, size=size, label=lab)
    if with_labels:
        out["labels"] = label
    return mask.bool(), out


# ------------------------------------------------------------------------------------------------ evaluation helpers
def nearest_neighbor(query, ref):
    """-> (idx int32 [Nq], d2 float32 [Nq]) exact 1-NN of every query point in `ref`"""
    query = _chk(query.float().contiguous(), torch.float32, "query")
    ref = _chk(ref.float().contiguous(), torch.float32, "ref")
    nq = query.shape[0]
    idx = torch.empty(nq, dtype=_i32, device=query.device)
    d2 = torch.empty(nq, dtype=torch.float32, device=query.device)
    _lib.call("gn_nearest_neighbor", _p(query), nq, _p(ref), ref.shape[0], _p(idx), _p(d2), _stream())
    return idx, d2


def _rows3_f64(t, name):
    t = t.to(torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected an (N, 3) tensor, got {tuple(t.shape)}")
    return t


def _rows3_f32(t, name):
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: expected an (N, 3) tensor, got {tuple(t.shape)}")
    return _chk(t.contiguous(), torch.float32, name)


def _cat_sets(tensors, name, dtype=torch.float64, width=3, dedup=True):
    """concatenate point / face sets -> (joint tensor, row offset of each entry); dedup: a tensor passed more than once is stored once (for
    the READ-ONLY sets: query rows are also output rows and must not share them)"""
    uniq, offs, seen, n = [], [], {}, 0
    for k, t in enumerate(tensors):
        key = id(t) if dedup else k
        if key not in seen:
            seen[key] = n
            uniq.append(t)
            n += t.shape[0]
        offs.append(seen[key])
    if not uniq:
        return None, offs
    joint = torch.cat([u.reshape(-1, width) for u in uniq]) if len(uniq) > 1 else uniq[0]
    return _chk(joint.to(dtype).contiguous(), dtype, name), offs


def _pairs_table(rows, device):
    if len(rows) > 65535:
        raise ValueError(f"at most 65535 pairs per launch, got {len(rows)}")
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), -1).to(device, non_blocking=False)


def nearest_neighbor_f64_batch(queries, refs):
    """fp64 exact 1-NN for every (queries[k], refs[k]) pair in ONE launch (gn_nearest_neighbor_f64_batch) -> list of (idx int32 [nq_k],
    d2 float64 [nq_k]).  d2 in cKDTree's summation order; ties -> lowest index; an empty reference set gives (+inf, -1)."""
    if len(queries) != len(refs):
        raise ValueError("nearest_neighbor_f64_batch: one reference set per query set")
    if not queries:
        return []
    queries = [_rows3_f64(q, "query") for q in queries]
    refs = [_rows3_f64(r, "ref") for r in refs]
    dev = queries[0].device
    q, qo = _cat_sets(queries, "query", dedup=False)
    r, ro = _cat_sets(refs, "ref")
    if r.shape[0] >= 2 ** 31:
        raise ValueError("nearest_neighbor_f64_batch: more than 2^31 reference points")
    rows = [(qo[k], queries[k].shape[0], ro[k], refs[k].shape[0]) for k in range(len(queries))]
    pairs = _pairs_table(rows, dev)
    max_nq = max(n for _, n, _, _ in rows)
    idx = torch.empty(q.shape[0], dtype=_i32, device=dev)
    d2 = torch.empty(q.shape[0], dtype=torch.float64, device=dev)
    _lib.call("gn_nearest_neighbor_f64_batch", _p(q), _p(r), _p(pairs), len(rows), max_nq, _p(idx), _p(d2), _stream())
    return [(idx[o:o + n], d2[o:o + n]) for o, n, _, _ in rows]


def nearest_neighbor_f64(query, ref):
    """-> (idx int32 [Nq], d2 float64 [Nq]): exact fp64 1-NN of every query point in `ref` (cKDTree.query(k=1) before its sqrt)"""
    return nearest_neighbor_f64_batch([query], [ref])[0]


def _faces_i32(f):
    if f.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"faces: expected an integer tensor, got {f.dtype}")
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces: expected an (F, 3) tensor, got {tuple(f.shape)}")
    if f.dtype == torch.int64:              # int32 on the device; an index that does not fit is out of range: keep it so
        f = f.clamp(min=-1, max=2 ** 31 - 1)
    return f


def _mesh_sets(who, meshes, queries=None, rows3=_rows3_f64, dedup=False):
    """the list-of-meshes work of the mesh-pair wrappers: every mesh's (verts, faces) checked (rows3: _rows3_f64, or _rows3_f32 for the entry that
    takes fp32 and does not cast), the joint vertices and int32 faces (dedup: a mesh tensor passed more than once is stored once), the 2^31 refusal
    under the caller's name, and the int64 device table: with `queries` (a list of row sets, one per mesh; output rows, so never shared) a pair row
    (q0, nq, v0, nv, f0, nf) per mesh, without them the CSR rows (v0, f0) closed by the totals.  -> (joint queries or None, v, f, table, rows)"""
    queries = None if queries is None else [_rows3_f64(q, "query") for q in queries]
    verts = [rows3(v, "verts") for v, _ in meshes]
    faces = [_faces_i32(f) for _, f in meshes]
    q, qo = (None, None) if queries is None else _cat_sets(queries, "query", dedup=False)
    v, vo = _cat_sets(verts, "verts", dtype=verts[0].dtype, dedup=dedup)
    f, fo = _cat_sets(faces, "faces", dtype=_i32, dedup=dedup)
    if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: more than 2^31 vertices or faces")
    if queries is None:
        rows = [(vo[k], fo[k]) for k in range(len(meshes))] + [(v.shape[0], f.shape[0])]
    else:
        rows = [(qo[k], queries[k].shape[0], vo[k], verts[k].shape[0], fo[k], faces[k].shape[0]) for k in range(len(meshes))]
    return q, v, f, _pairs_table(rows, v.device), rows


def _raise_bad_face(flag, who):
    if flag:
        raise IndexError(f"{who}: a face index is out of bounds for its mesh's vertices")


def point_mesh_sqdist_batch(queries, meshes):
    """fp64 unsigned squared distance of every query to the nearest triangle of its mesh, every (queries[k], meshes[k] = (verts, faces))
    pair in ONE launch (gn_point_mesh_sqdist_batch) -> list of (face_idx int32 [nq_k], d2 float64 [nq_k]).  libigl's
    point_mesh_squared_distance; ties -> lowest face index; an empty mesh gives (+inf, -1).  A face index outside [0, V) raises IndexError
    (after the launch: one host synchronisation)."""
    if len(queries) != len(meshes):
        raise ValueError("point_mesh_sqdist_batch: one mesh per query set")
    if not queries:
        return []
    q, v, f, pairs, rows = _mesh_sets("point_mesh_sqdist_batch", meshes, queries, dedup=True)
    face_idx = torch.empty(q.shape[0], dtype=_i32, device=q.device)
    d2 = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    bad = torch.zeros(1, dtype=torch.int64, device=q.device)
    _lib.call("gn_point_mesh_sqdist_batch", _p(q), _p(v), _p(f), _p(pairs), len(rows), max(r[1] for r in rows), _p(face_idx), _p(d2), _p(bad),
              _stream())
    _raise_bad_face(bad.item(), "point_mesh_sqdist")
    return [(face_idx[r[0]:r[0] + r[1]], d2[r[0]:r[0] + r[1]]) for r in rows]


def point_mesh_sqdist(query, verts, faces):
    """-> (face_idx int32 [Nq], d2 float64 [Nq]): squared distance of every query to the nearest triangle of (verts, faces)"""
    return point_mesh_sqdist_batch([query], [(verts, faces)])[0]


def winding_number_batch(queries, meshes):
    """fp64 generalised winding number of every query about its mesh, every (queries[k], meshes[k] = (verts, faces)) pair in ONE launch
    (gn_winding_number_batch) -> list of float64 [nq_k].  The exact all-pairs sum of Van Oosterom-Strackee solid angles in face-index order,
    divided by 4 pi (garmentnets_amd/winding.py has the definition): a pure function of (query, mesh), whatever else the launch carries.
    An empty mesh gives 0.  A face index outside [0, V) raises IndexError (after the launch: one host synchronisation)."""
    if len(queries) != len(meshes):
        raise ValueError("winding_number_batch: one mesh per query set")
    if not queries:
        return []
    q, v, f, pairs, rows = _mesh_sets("winding_number_batch", meshes, queries, dedup=True)
    out = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    bad = torch.zeros(1, dtype=torch.int64, device=q.device)
    _lib.call("gn_winding_number_batch", _p(q), _p(v), _p(f), _p(pairs), len(rows), max(r[1] for r in rows), _p(out), _p(bad), _stream())
    _raise_bad_face(bad.item(), "winding_number")
    return [out[r[0]:r[0] + r[1]] for r in rows]


def winding_number(query, verts, faces):
    """-> float64 [Nq]: the generalised winding number of every query about the mesh (verts, faces)"""
    return winding_number_batch([query], [(verts, faces)])[0]


def winding_field_batch(meshes, shape):
    """the winding number of every mesh of `meshes` = [(verts, faces)] at every node of a `shape` = (D, H, W) lattice over the unit cube, all
    meshes in ONE launch (gn_winding_field_batch) -> (B, D, H, W) float32.  Node (i, j, k) is the point (i/(D-1), j/(H-1), k/(W-1)) (what
    io.dataset.nocs_grid_sample reads); the kernel forms the points itself and writes float(w), rounded once: bit for bit
    winding_number_batch at the lattice points, .float().  A face index outside [0, V) raises IndexError (after the launch)."""
    D, H, W = (int(n) for n in shape)
    if not meshes:
        raise ValueError("winding_field_batch: no meshes")
    _, v, f, csr, _ = _mesh_sets("winding_field_batch", meshes)
    out = torch.empty((len(meshes), D, H, W), dtype=torch.float32, device=v.device)
    bad = torch.zeros(1, dtype=torch.int64, device=v.device)
    _lib.call("gn_winding_field_batch", _p(v), _p(f), _p(csr), len(meshes), D, H, W, _p(out), _p(bad), _stream())
    _raise_bad_face(bad.item(), "winding_field")
    return out


def distance_field_batch(meshes, shape):
    """the squared distance from every node of a `shape` = (D, H, W) lattice over the unit cube (the lattice of winding_field_batch) to every mesh
    of `meshes` = [(verts, faces)], all meshes in ONE launch (gn_distance_field_batch) -> (d2 float64 (B, D, H, W), face_idx int32 (B, D, H, W)).
    Bit for bit point_mesh_sqdist_batch at the lattice points: ties -> lowest face index, an empty mesh gives (+inf, -1).  A face index outside
    [0, V) raises IndexError (after the launch: one host synchronisation)."""
    D, H, W = (int(n) for n in shape)
    if not meshes:
        raise ValueError("distance_field_batch: no meshes")
    if min(D, H, W) < 2 or D * H * W >= 2 ** 31 - 1:        # the limits of the entry, refused here before the outputs are allocated
        raise ValueError(f"gn_distance_field_batch: lattice {(D, H, W)}: every axis needs >= 2 nodes and D*H*W < 2^31")
    _, v, f, csr, _ = _mesh_sets("distance_field_batch", meshes)
    face_idx = torch.empty((len(meshes), D, H, W), dtype=_i32, device=v.device)
    d2 = torch.empty((len(meshes), D, H, W), dtype=torch.float64, device=v.device)
    bad = torch.zeros(1, dtype=torch.int64, device=v.device)
    _lib.call("gn_distance_field_batch", _p(v), _p(f), _p(csr), len(meshes), D, H, W, _p(face_idx), _p(d2), _p(bad), _stream())
    _raise_bad_face(bad.item(), "distance_field")
    return d2, face_idx


def _qt_kind(kind, who):
    if kind not in _lib.QT_KINDS:
        raise ValueError(f"{who}: unknown kind {kind!r}; expected one of {sorted(_lib.QT_KINDS)}")
    return _lib.QT_KINDS[kind]


def _qt_bad(bad, who):
    index, short = (int(v) for v in bad.tolist())                    # one host synchronisation
    if short:
        raise _lib.GarmentNetsHipError(f"{who}: a mesh has more faces than the max_nf the workspace was sized for")
    _raise_bad_face(index, who)


def query_targets_batch(queries, meshes, kind, tsdf_clip_value=None, absolute=False, return_fp64=False):
    """the float32 training target of volume_group `kind` at queries (B, M, 3) fp32, garment b against meshes[b] = (verts fp32 (V, 3), faces (F, 3)), from
    the meshes alone: two launches of gn_query_targets_batch -> target (B, M) float32; return_fp64: (target, w, d2, face_idx) with w, d2 float64 (B, M) and
    face_idx int32 (B, M), None for what `kind` does not compute.  garmentnets_amd/targets.py has the definition: w is winding_number_batch's sum cut into
    chunks of QT_FACE_CHUNK faces (its bits when F <= QT_FACE_CHUNK), (d2, face_idx) are point_mesh_sqdist_batch's bits; then tsdf_clip_value and
    absolute as the dataset's data_io applies them.  A face index outside [0, V) raises IndexError (after the launch: one host synchronisation)."""
    code = _qt_kind(kind, "query_targets_batch")
    queries = _chk(queries, torch.float32, "queries")
    if queries.dim() != 3 or queries.shape[2] != 3:
        raise ValueError(f"queries: expected a (B, M, 3) tensor, got {tuple(queries.shape)}")
    B, M = int(queries.shape[0]), int(queries.shape[1])
    if len(meshes) != B:
        raise ValueError("query_targets_batch: one mesh per query set")
    dev = queries.device
    need_w, need_d = kind != "nocs_distance_field", code in (1, 2)
    target = torch.empty((B, M), dtype=torch.float32, device=dev)
    w = torch.empty((B, M), dtype=torch.float64, device=dev) if return_fp64 and need_w else None
    d2 = torch.empty((B, M), dtype=torch.float64, device=dev) if return_fp64 and need_d else None
    face_idx = torch.empty((B, M), dtype=_i32, device=dev) if return_fp64 and need_d else None
    if B:
        _, v, f, csr, _ = _mesh_sets("query_targets_batch", meshes, rows3=_rows3_f32)
        max_nf = max(int(x.shape[0]) for _, x in meshes)
        nbytes = _lib.load().gn_query_targets_workspace_bytes(B, M, max_nf, code)
        ws = _ws(nbytes, dev)
        bad = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.call("gn_query_targets_batch", _p(queries), _p(v), _p(f), _p(csr), B, M, max_nf, code, int(tsdf_clip_value is not None),
                  float(tsdf_clip_value) if tsdf_clip_value is not None else 0.0, int(bool(absolute)), _p(ws), nbytes, _p(target), _p(w), _p(d2),
                  _p(face_idx), _p(bad), _stream())
        _qt_bad(bad, "query_targets")
    return (target, w, d2, face_idx) if return_fp64 else target


# ------------------------------------------------------------------------------------------------ validation losses
def _check_sets(n):
    if not 1 <= n <= _lib.LOSS_MAX_SETS:
        raise ValueError(f"1..{_lib.LOSS_MAX_SETS} sets per launch, got {n}")


def _table(cls, rows):
    return (cls * len(rows))(*[cls(*r) for r in rows])


def _table_dev(tab, device):
    """a host ctypes table -> its bytes as a uint8 tensor on the device (a copy: the host table may be reused or freed)"""
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)


def nocs_bin_metrics(sets, bins, mirror_axis=None):
    """binned NOCS head metrics of 1..8 row sets in ONE launch (gn_nocs_bin_metrics).  sets: [(logits (N, >= bins*3) fp32 rows laid out
    (bins, 3), gt (N, 3))], N >= 1.  -> (nsets, 4) fp64 on the device: the sums over the set of CE at the target bin, CE at the mirrored
    target bin, |arg-max coordinate - gt| and |arg-max coordinate - mirrored gt| (mirror_axis None: the mirrored columns repeat the plain ones)"""
    _check_sets(len(sets))
    keep = []
    for logits, gt in sets:
        if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] < bins * 3:
            raise ValueError(f"logits: expected (N, >= {bins * 3}) float32 rows, got {tuple(logits.shape)} {logits.dtype}")
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        n, ldl = rows_view(logits)
        gt = gt.float().contiguous()
        if n < 1 or gt.shape != (n, 3):
            raise ValueError(f"gt: expected ({n}, 3) with at least one row, got {tuple(gt.shape)}")
        keep.append((logits, gt, n, ldl))
    rows = [(_p(lg).value, _p(gt).value, n, ldl, 0) for lg, gt, n, ldl in keep]
    tab = _table(_lib.NocsBinSet, rows)
    dev = keep[0][1].device
    nws = _lib.load().gn_nocs_bin_metrics_workspace_bytes(tab, len(rows))
    ws = _ws(max(nws, 8), dev)
    out = torch.empty((len(rows), 4), dtype=torch.float64, device=dev)
    _lib.call("gn_nocs_bin_metrics", tab, len(rows), int(bins), -1 if mirror_axis is None else int(mirror_axis), _p(ws), nws, _p(out), _stream())
    return out


def value_losses(segments):
    """element-wise loss sums of 1..8 segments in ONE launch (gn_value_losses).  segments: [(pred, target, kind[, mirror])], kind one of
    "l2" | "smooth_l1" | "bce_logits" (per element) | "row_norm" (|pred - target| per (M, 3) row); pred and target of the same number of
    elements (any shape, read flat); mirror: also the sum against the x-mirrored target of (M, 3) rows.  -> (nsegs, 2) fp64 on the device:
    (sum, mirrored sum; 0 without mirror)"""
    _check_sets(len(segments))
    keep = []
    for seg in segments:
        pred, target, kind = seg[:3]
        mirror = bool(seg[3]) if len(seg) > 3 else False
        if kind not in _lib.LOSS_KINDS:
            raise ValueError(f"loss kind {kind!r}: expected one of {sorted(_lib.LOSS_KINDS)}")
        pred, target = pred.float().contiguous(), target.float().contiguous()
        if pred.numel() != target.numel():
            raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()}) differ in size")
        count = pred.numel()
        if kind == "row_norm" or mirror:
            if count % 3:
                raise ValueError(f"{kind} {'(mirrored) ' if mirror else ''}needs (M, 3) rows, got {count} elements")
            count = count // 3 if kind == "row_norm" else count
        keep.append((pred, target, count, _lib.LOSS_KINDS[kind], int(mirror)))
    rows = [(_p(pr).value, _p(tg).value, n, k, m) for pr, tg, n, k, m in keep]
    tab = _table(_lib.LossSegment, rows)
    dev = keep[0][0].device
    nws = _lib.load().gn_value_losses_workspace_bytes(tab, len(rows))
    ws = _ws(max(nws, 8), dev)
    out = torch.empty((len(rows), 2), dtype=torch.float64, device=dev)
    _lib.call("gn_value_losses", tab, len(rows), _p(ws), nws, _p(out), _stream())
    return out


def nocs_bin_loss_bwd(sets, bins, mirror_axis, sums, weights, upstream):
    """gradient of the weighted binned NOCS loss sum_s weights[s] * CE_s / (3 n_s) to the logits of 1..8 row sets in ONE launch
    (gn_nocs_bin_loss_bwd).  sets: [(logits (N, >= bins*3) fp32, gt (N, 3))] as nocs_bin_metrics takes them; sums: ITS (nsets, 4) fp64 result, on
    the device -- with a mirror_axis the kernel decides from them whether the whole batch takes the mirrored targets; upstream: fp32 device
    scalar, the gradient of the loss.  -> one contiguous fp32 gradient per set, shaped like its logits (pad columns exactly 0)."""
    _check_sets(len(sets))
    if len(weights) != len(sets):
        raise ValueError(f"{len(sets)} sets but {len(weights)} weights")
    keep = []
    for logits, gt in sets:
        if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape[1] < bins * 3:
            raise ValueError(f"logits: expected (N, >= {bins * 3}) float32 rows, got {tuple(logits.shape)} {logits.dtype}")
        if logits.shape[1] > 1 and logits.stride(1) != 1:
            logits = logits.contiguous()
        n, ldl = rows_view(logits)
        gt = gt.float().contiguous()
        if n < 1 or gt.shape != (n, 3):
            raise ValueError(f"gt: expected ({n}, 3) with at least one row, got {tuple(gt.shape)}")
        keep.append((logits, gt, torch.empty(tuple(logits.shape), dtype=torch.float32, device=logits.device), n, ldl))
    sums = _chk(sums, torch.float64, "sums")
    if tuple(sums.shape) != (len(sets), 4):
        raise ValueError(f"sums: expected ({len(sets)}, 4), got {tuple(sums.shape)}")
    upstream = _chk(upstream.reshape(1), torch.float32, "upstream")
    rows = [(_p(lg).value, _p(gt).value, _p(g).value, n, ldl, g.shape[1], g.shape[1], 0) for lg, gt, g, n, ldl in keep]
    tab = _table(_lib.NocsBinGradSet, rows)
    w = (ctypes.c_double * len(rows))(*[float(x) for x in weights])
    _lib.call("gn_nocs_bin_loss_bwd", tab, len(rows), int(bins), -1 if mirror_axis is None else int(mirror_axis), _p(sums), w, _p(upstream), _stream())
    return [k[2] for k in keep]


def value_losses_bwd(segments, sums, weights, upstream):
    """gradient of sum_s weights[s] * (segment s's sum, the mirrored one where that is strictly smaller) / count_s to pred, for 1..8 segments in ONE
    launch (gn_value_losses_bwd).  segments: [(pred, target, kind[, mirror])] as value_losses takes them, kind "l2" | "smooth_l1" | "bce_logits"
    ("row_norm" is a metric: ValueError); sums: value_losses' (nsegs, 2) fp64 result, on the device; upstream: fp32 device scalar.
    -> one contiguous fp32 gradient per segment, shaped like its pred"""
    _check_sets(len(segments))
    if len(weights) != len(segments):
        raise ValueError(f"{len(segments)} segments but {len(weights)} weights")
    keep = []
    for seg, wt in zip(segments, weights):
        pred, target, kind = seg[:3]
        mirror = bool(seg[3]) if len(seg) > 3 else False
        if kind == "row_norm":
            raise ValueError("row_norm is a metric, not a loss: it has no gradient")
        if kind not in _lib.LOSS_KINDS:
            raise ValueError(f"loss kind {kind!r}: expected one of {sorted(_lib.LOSS_KINDS)}")
        shape = tuple(pred.shape)
        pred, target = pred.float().contiguous(), target.float().contiguous()
        if pred.numel() != target.numel():
            raise ValueError(f"pred ({pred.numel()} elements) and target ({target.numel()}) differ in size")
        count = pred.numel()
        if mirror and count % 3:
            raise ValueError(f"{kind} (mirrored) needs (M, 3) rows, got {count} elements")
        keep.append((pred, target, torch.empty(shape, dtype=torch.float32, device=pred.device), count, float(wt) / max(count, 1), _lib.LOSS_KINDS[kind],
                     int(mirror)))
    sums = _chk(sums, torch.float64, "sums")
    if tuple(sums.shape) != (len(segments), 2):
        raise ValueError(f"sums: expected ({len(segments)}, 2), got {tuple(sums.shape)}")
    upstream = _chk(upstream.reshape(1), torch.float32, "upstream")
    rows = [(_p(pr).value, _p(tg).value, _p(g).value, n, c, k, m) for pr, tg, g, n, c, k, m in keep]
    tab = _table(_lib.LossGradSegment, rows)
    _lib.call("gn_value_losses_bwd", tab, len(rows), _p(sums), _p(upstream), _stream())
    return [k[2] for k in keep]


# ------------------------------------------------------------------------------------------------ operator gradients (csrc/grad.hip)
def _ws(nbytes, device, zero=False):
    """THE workspace allocation of every wrapper: nbytes bytes as a size entry of the library gave them (at least one, so that the pointer is
    never null), zero-filled on request"""
    return (torch.zeros if zero else torch.empty)(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def fp32_rows(t, name, rows=None, cols=None):
    """t as fp32 2-D rows the C ABI reads in place (unit column stride, row stride >= columns), else a contiguous copy: autograd may hand over an
    expanded or otherwise strided tensor.  rows / cols: the counts t is held to.  TypeError for the dtype, ValueError for the shape."""
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected torch.float32, got {t.dtype}")
    if t.dim() != 2 or (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name}: expected rows ({'M' if rows is None else rows}, {'N' if cols is None else cols}), got shape {tuple(t.shape)}")
    return t if (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= t.shape[1] else t.contiguous()


def grid_scatter_bwd(grad_vol, flat_idx, N, reduce, vol=None, src=None, c_real=None):
    """grad_vol: channel-last [B][G0][G1][G2][C] -> grad_src [N][C].  max / min need the forward's output `vol` and input `src` (the winner of a
    cell is the lowest point index whose value is bit-equal to the stored one).  'mul' is refused by name."""
    if reduce not in REDUCE_CODES:
        raise ValueError(f"grid_scatter_bwd: reduce={reduce!r} is not one of {sorted(REDUCE_CODES)}")
    if reduce == "mul":
        raise ValueError("grid_scatter_bwd: reduce='mul' has no gradient here (nobody trains with it; it divides by zero at a zero factor)")
    _chk(grad_vol, torch.float32, "grad_vol")
    _chk(flat_idx, _i32, "flat_idx")
    C = grad_vol.shape[-1]
    cells = grad_vol.numel() // C
    N = int(N)
    if flat_idx.numel() != N:
        raise ValueError(f"grid_scatter_bwd: flat_idx has {flat_idx.numel()} entries for {N} points")
    sel = reduce in ("max", "min")
    if sel:
        if vol is None or src is None:
            raise ValueError(f"grid_scatter_bwd: reduce={reduce!r} needs the forward's output and input")
        _chk(vol, torch.float32, "vol")
        if vol.shape != grad_vol.shape or src.dtype != torch.float32 or tuple(src.shape) != (N, C):
            raise ValueError("grid_scatter_bwd: vol / src do not match grad_vol")
    code = REDUCE_CODES[reduce]
    out = new_rows(N, C, grad_vol.device)
    if N == 0:
        return out
    nbytes = _lib.load().gn_grid_scatter_bwd_workspace_bytes(N, C, cells, code)
    ws = _ws(nbytes, grad_vol.device) if nbytes else None
    _lib.call("gn_grid_scatter_bwd", _p(grad_vol), _p(vol if sel else None), _p(src if sel else None), rows_view(src)[1] if sel else 0, _p(flat_idx), N, C,
              C if c_real is None else int(c_real), cells, code, _p(ws), nbytes, _p(out), out.stride(0), _stream())
    return out


def segment_max_bwd(grad_out, out, h, slot_src, M, S):
    """gradient of segment_max with respect to h [M * S][C]"""
    C = h.shape[1]
    grad_out = fp32_rows(grad_out, "grad_out", cols=C)
    if tuple(out.shape) != (M, C) or h.shape[0] != M * S or grad_out.shape[0] != M or slot_src.numel() != M * S:
        raise ValueError("segment_max_bwd: shapes do not match (M, S, C)")
    _chk(slot_src, _i32, "slot_src")
    g = new_rows(M * S, C, h.device)
    _lib.call("gn_segment_max_bwd", _p(grad_out), rows_view(grad_out)[1], _p(out), rows_view(out)[1], _p(h), rows_view(h)[1], _p(slot_src), M, S, C,
              _p(g), g.stride(0), _stream())
    return g


def global_max_pool_bwd(grad_out, out, h, ptr, B):
    C = h.shape[1]
    grad_out = fp32_rows(grad_out, "grad_out", cols=C)
    if tuple(out.shape) != (B, C) or grad_out.shape[0] != B or ptr.numel() != B + 1:
        raise ValueError("global_max_pool_bwd: shapes do not match (B, C)")
    _chk(ptr, _i32, "ptr")
    g = new_rows(h.shape[0], C, h.device)
    _lib.call("gn_global_max_pool_bwd", _p(grad_out), rows_view(grad_out)[1], _p(out), rows_view(out)[1], _p(h), rows_view(h)[1], _p(ptr), B, C,
              _p(g), g.stride(0), _stream())
    return g


def sa_gather_bwd(grad_edge, slot_src, C, n_points):
    """gradient of sa_gather with respect to x [n_points][C]: the feature part (columns :C) of the edge rows, summed per source in ascending row"""
    grad_edge = fp32_rows(grad_edge, "grad_edge")
    _chk(slot_src, _i32, "slot_src")
    rows = slot_src.numel()
    if grad_edge.shape[0] != rows or grad_edge.shape[1] < C or C < 1:
        raise ValueError("sa_gather_bwd: grad_edge does not match slot_src / C")
    g = new_rows(n_points, C, grad_edge.device)
    if n_points == 0:
        return g
    nbytes = _lib.load().gn_sa_gather_bwd_workspace_bytes(rows, n_points)
    ws = _ws(nbytes, grad_edge.device)
    _lib.call("gn_sa_gather_bwd", _p(grad_edge), rows_view(grad_edge)[1], _p(slot_src), rows, C, n_points, _p(ws), nbytes, _p(g), g.stride(0), _stream())
    return g


def knn_neighbours(ps, ptr_s, pq, ptr_q, k):
    """-> (nbr int32 [Nq][k], d2 fp32 [Nq][k]): the neighbours knn_interpolate uses, ascending (d2, index); -1 / 0 past an example's sources"""
    _chk(ps, torch.float32, "ps")
    _chk(pq, torch.float32, "pq")
    Nq, k = pq.shape[0], int(k)
    if k < 1:
        raise ValueError("knn_neighbours: k must be >= 1")
    nbr = torch.empty((Nq, k), dtype=_i32, device=pq.device)
    d2 = torch.empty((Nq, k), dtype=torch.float32, device=pq.device)
    if Nq:
        _lib.call("gn_knn_neighbours", _p(ps), _p(ptr_s), _p(pq), _p(ptr_q), ptr_s.numel() - 1, Nq, k, _p(nbr), _p(d2), _stream())
    return nbr, d2


def knn_interpolate_bwd(grad_y, nbr, d2, n_sources):
    """gradient of knn_interpolate with respect to the source features [n_sources][C] (nbr, d2: knn_neighbours)"""
    grad_y = fp32_rows(grad_y, "grad_y")
    _chk(nbr, _i32, "nbr")
    _chk(d2, torch.float32, "d2")
    Nq, k = nbr.shape
    C = grad_y.shape[1]
    if grad_y.shape[0] != Nq or d2.shape != nbr.shape:
        raise ValueError("knn_interpolate_bwd: grad_y / d2 do not match nbr")
    if Nq == 0 or n_sources == 0:
        return torch.zeros((n_sources, pad4(C)), dtype=torch.float32, device=grad_y.device)[:, :C]
    g = new_rows(n_sources, C, grad_y.device)
    nbytes = _lib.load().gn_knn_interpolate_bwd_workspace_bytes(Nq, k, n_sources)
    ws = _ws(nbytes, grad_y.device)
    _lib.call("gn_knn_interpolate_bwd", _p(nbr), _p(d2), Nq, k, _p(grad_y), rows_view(grad_y)[1], n_sources, C, _p(ws), nbytes, _p(g), g.stride(0), _stream())
    return g


def trilinear_sample_bwd(grad_rows, vol, query, want_vol=True, want_query=False):
    """gradient of trilinear_sample_batch: grad_rows (B, M, C), vol (B, D, H, W, C) channel-last, query (B, M, 3)
    -> (grad_vol like vol or None, grad_query (B, M, 3) or None).  grad_vol is an ordered sum per voxel (no float atomics): bit-identical repeats."""
    _chk(vol, torch.float32, "vol")
    _chk(query, torch.float32, "query")
    if vol.dim() != 5 or query.dim() != 3 or query.shape[0] != vol.shape[0] or query.shape[2] != 3:
        raise ValueError("trilinear_sample_bwd: vol must be (B, D, H, W, C) and query (B, M, 3)")
    B, D, H, W, C = vol.shape
    M = query.shape[1]
    if grad_rows.dtype != torch.float32:
        raise TypeError(f"grad_rows: expected torch.float32, got {grad_rows.dtype}")
    if tuple(grad_rows.shape) != (B, M, C):
        raise ValueError(f"trilinear_sample_bwd: grad_rows must be {(B, M, C)}, got {tuple(grad_rows.shape)}")
    if M and B and not (grad_rows.stride(2) == 1 and grad_rows.stride(1) >= C and grad_rows.stride(0) == M * grad_rows.stride(1)):
        grad_rows = grad_rows.contiguous()
    gv = gq = None
    if B == 0 or M == 0:           # nothing was sampled: empty / zero gradients without a launch
        return (torch.zeros_like(vol) if want_vol else None), (torch.zeros_like(query) if want_query else None)
    nbytes = 0
    ws = None
    if want_vol:
        gv = torch.empty_like(vol)
        nbytes = _lib.load().gn_trilinear_sample_bwd_workspace_bytes(B, M, D, H, W)
        ws = _ws(nbytes, vol.device)
    if want_query:
        gq = torch.empty_like(query)
    if want_vol or want_query:
        _lib.call("gn_trilinear_sample_bwd", _p(grad_rows), grad_rows.stride(1), _p(vol), B, D, H, W, C, _p(query), M, _p(ws), nbytes, _p(gv), _p(gq), _stream())
    return gv, gq


# ------------------------------------------------------------------------------------------------ UNet gradients (csrc/unet_grad.hip)
def _vol5(t, name, like=None):
    _chk(t, torch.float32, name)
    if t.dim() != 5 or (like is not None and tuple(t.shape) != tuple(like.shape)):
        raise ValueError(f"{name}: expected a channel-last volume [B][D][H][W][C]" + (f" of shape {tuple(like.shape)}" if like is not None else "")
                         + f", got {tuple(t.shape)}")
    return t


def pack_conv_weight_bwd_data(w):
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) -> the gn_conv3d_gcr pack of the layer's DATA gradient: the transposed convolution as a forward one, the
    weight flipped over the taps and transposed over (ci, co), wt[ci][co][kd][kh][kw] = w[co][ci][2-kd][2-kh][2-kw], its output width Cin padded with
    zero rows to a multiple of 32 (the forward kernel's rule, roles swapped): [27][Cout/16][round_up(Cin, 32)][16].  Cout % 16 == 0.  Runs on any device."""
    cout, cin = w.shape[:2]
    if cout % 16 != 0:
        raise ValueError(f"pack_conv_weight_bwd_data: Cout={cout} must be a multiple of 16 (it is the input width of the transposed convolution)")
    return pack_conv_weight(bwd_data_weight(w))


def _bwd_weight_args(who, src0, src1, a, d, y, dy):
    """the checks the two weight-gradient entries share, before any launch -> (B, D, H, W, C0, C1, Cout)"""
    _vol5(src0, "src0")
    B, D, H, W, C0 = src0.shape
    C1 = 0
    if src1 is not None:
        _vol5(src1, "src1")
        C1 = src1.shape[-1]
        if tuple(src1.shape[:4]) != (B, D // 2, H // 2, W // 2) or D % 2 or H % 2 or W % 2:
            raise ValueError(f"{who}: src1 {tuple(src1.shape)} is not the half-resolution companion of src0 {tuple(src0.shape)}")
    _vol5(dy, "dy")
    cout = dy.shape[-1]
    if tuple(dy.shape[:4]) != (B, D, H, W):
        raise ValueError(f"{who}: dy {tuple(dy.shape)} does not match src0 {tuple(src0.shape)}")
    if y is not None:
        _vol5(y, "y", dy)
    for t, name in ((a, "a"), (d, "d")):
        _chk(t, torch.float32, name)
        if tuple(t.shape) != (B, C0 + C1):
            raise ValueError(f"{who}: {name} must be [B][C0 + C1] = {(B, C0 + C1)}, got {tuple(t.shape)}")
    return B, D, H, W, C0, C1, cout


def conv3d_bwd_weight(src0, src1, a, d, y, dy):
    """-> dw (Cout, C0 + C1, 3, 3, 3) over the stored widths: the weight gradient of one 'gcr' layer (gn_conv3d_bwd_weight).  a, d: the forward's
    GroupNorm affine [B][C0 + C1]; y: the layer's stored output (ReLU mask), None for a layer without ReLU; dy: the gradient at that output."""
    B, D, H, W, C0, C1, cout = _bwd_weight_args("conv3d_bwd_weight", src0, src1, a, d, y, dy)
    dw = torch.empty((cout, C0 + C1, 3, 3, 3), dtype=torch.float32, device=src0.device)
    nbytes = _lib.load().gn_conv3d_bwd_weight_workspace_bytes(B, D, H, W, C0 + C1, cout)
    ws = _ws(nbytes, src0.device)
    _lib.call("gn_conv3d_bwd_weight", _p(src0), C0, _p(src1), C1, _p(a), _p(d), _p(y), _p(dy), B, D, H, W, cout, _p(ws), nbytes, _p(dw), _stream())
    return dw


def relu_mask(y, dy, out=None):
    """g = y > 0 ? dy : 0 (gn_relu_mask); in place when out is dy"""
    _chk(y, torch.float32, "y")
    _chk(dy, torch.float32, "dy")
    if y.shape != dy.shape or y.numel() % 4 != 0:
        raise ValueError(f"relu_mask: y {tuple(y.shape)} and dy {tuple(dy.shape)} must match, a multiple of 4 values")
    if out is None:
        out = torch.empty_like(dy)
    _lib.call("gn_relu_mask", _p(y), _p(dy), y.numel(), _p(out), _stream())
    return out


def conv3d_bwd_data(g, wp_t, cin_p):
    """the data gradient at a 'gcr' layer's conv operand: gn_conv3d_gcr over the (ReLU-masked) output gradient g with the pack of
    pack_conv_weight_bwd_data, identity affine, no ReLU -> [B][D][H][W][cin_p]"""
    _vol5(g, "g")
    B, cout = g.shape[0], g.shape[-1]
    one = torch.ones((B, cout), dtype=torch.float32, device=g.device)
    return conv3d_gcr(g, None, one, torch.zeros_like(one), wp_t, cin_p, relu=False)


# ---- the f16x2 form (csrc/unet_grad_split.hip; DESIGN.md "f16x2 backward of the UNet convolutions")
def bwd_data_weight(w):
    """nn.Conv3d weight (Cout, Cin, 3, 3, 3) -> the weight of the layer's data gradient as a forward convolution, (round_up(Cin, 32), Cout, 3, 3, 3)
    contiguous: flipped over the taps, transposed over (ci, co), zero rows beyond Cin -- what pack_conv_weight_bwd_data packs.  Device-side copies only."""
    cout, cin = w.shape[:2]
    if cout % 16 != 0:
        raise ValueError(f"bwd_data_weight: Cout={cout} must be a multiple of 16 (it is the input width of the transposed convolution)")
    cin_p = -(-cin // 32) * 32
    wt = w.detach().float().flip(2, 3, 4).transpose(0, 1)
    if cin_p != cin:
        wt = torch.cat((wt, wt.new_zeros((cin_p - cin,) + tuple(wt.shape[1:]))), 0)
    return wt.contiguous()


def pack_conv_weight_bwd_data_split(w, device_packs=False):
    """the GN_SPLIT_F16X2 pack of the layer's DATA gradient: pack_conv_weight_split of bwd_data_weight(w) (on the weight's device), or, device_packs and a
    weight on the GPU, pack_conv_weight_split_device of it (no host round trip)"""
    wt = bwd_data_weight(w)
    if device_packs and wt.is_cuda:
        return pack_conv_weight_split_device(wt, SPLIT_F16X2)
    return pack_conv_weight_split(wt, SPLIT_F16X2).to(w.device)


def relu_mask_max(y, dy, with_scale=True):
    """gn_relu_mask_max over a channel-last volume [B][...][C]: g = y > 0 ? dy : 0 (y None: g = dy) -> (g, gmax [B], scale [B][C], inv [B]): the largest
    finite |g| per sample and the power-of-two range scale from it, all on the device (scale / inv None without with_scale)"""
    _chk(dy, torch.float32, "dy")
    if dy.dim() < 2:
        raise ValueError(f"relu_mask_max: dy {tuple(dy.shape)} must be [B][...][C]")
    if y is not None:
        _chk(y, torch.float32, "y")
        if y.shape != dy.shape:
            raise ValueError(f"relu_mask_max: y {tuple(y.shape)} and dy {tuple(dy.shape)} must match")
    B, C = dy.shape[0], dy.shape[-1]
    n = dy.numel() // B if B else 0
    if n % 4 != 0:
        raise ValueError(f"relu_mask_max: {n} values per sample are not a multiple of 4")
    g = torch.empty_like(dy)
    gmax = torch.empty((B,), dtype=torch.float32, device=dy.device)
    scale = torch.empty((B, C), dtype=torch.float32, device=dy.device) if with_scale else None
    inv = torch.empty((B,), dtype=torch.float32, device=dy.device) if with_scale else None
    nbytes = _lib.load().gn_relu_mask_max_workspace_bytes(B)
    ws = _ws(nbytes, dy.device)
    _lib.call("gn_relu_mask_max", _p(y), _p(dy), B, n, C, _p(g), _p(gmax), _p(scale), _p(inv), _p(ws), nbytes, _stream())
    return g, gmax, scale, inv


def conv3d_bwd_data_split(g, scale, inv, pack, cin_p):
    """the data gradient at a 'gcr' layer's conv operand on the 16-bit matrix cores: gn_conv3d_gcr_split (direct form, no ReLU, no statistics) over the
    masked output gradient g with the pack of pack_conv_weight_bwd_data_split; scale [B][Cout] / inv [B]: relu_mask_max's -> [B][D][H][W][cin_p]"""
    _vol5(g, "g")
    return conv3d_gcr_split(g, None, scale, torch.zeros_like(scale), pack, cin_p, relu=False, act_inv=inv)


def conv3d_bwd_weight_split(src0, src1, a, d, y, dy, x_inv=None, gmax=None):
    """-> dw (Cout, C0 + C1, 3, 3, 3) over the stored widths as conv3d_bwd_weight, on fp16 planes (gn_conv3d_bwd_weight_split).  a, d [B][C0 + C1]: the
    forward's GroupNorm affine; with x_inv [B] they carry each sample's power-of-two activation scale and x_inv is its inverse
    (groupnorm_affine(with_act_scale=True)), without it the operand x * a + d must lie inside fp16's range as it is.  gmax [B]: relu_mask_max's
    per-sample maximum of the masked gradient; None: one masking pass finds it here."""
    B, D, H, W, C0, C1, cout = _bwd_weight_args("conv3d_bwd_weight_split", src0, src1, a, d, y, dy)
    for t, name in ((x_inv, "x_inv"), (gmax, "gmax")):
        if t is not None:
            _chk(t, torch.float32, name)
            if tuple(t.shape) != (B,):
                raise ValueError(f"conv3d_bwd_weight_split: {name} must be [B] = {(B,)}, got {tuple(t.shape)}")
    if gmax is None:
        gmax = relu_mask_max(y, dy, with_scale=False)[1]
    dw = torch.empty((cout, C0 + C1, 3, 3, 3), dtype=torch.float32, device=src0.device)
    nbytes = _lib.load().gn_conv3d_bwd_weight_split_workspace_bytes(B, D, H, W, C0 + C1, cout)
    ws = _ws(nbytes, src0.device)
    _lib.call("gn_conv3d_bwd_weight_split", _p(src0), C0, _p(src1), C1, _p(a), _p(d), _p(x_inv), _p(y), _p(dy), _p(gmax), B, D, H, W, cout, _p(ws), nbytes,
              _p(dw), _stream())
    return dw


def _gn_bwd_dims(dxn, goff, x, half, who):
    _vol5(dxn, "dxn")
    _vol5(x, "x")
    B, D, H, W, C = x.shape
    k = 2 if half else 1
    if tuple(dxn.shape[:4]) != (B, k * D, k * H, k * W) or goff < 0 or goff + C > dxn.shape[-1]:
        raise ValueError(f"{who}: dxn {tuple(dxn.shape)} (columns {goff}..{goff + C}) does not cover x {tuple(x.shape)}" + (" at twice its resolution" if half else ""))
    return B, D, H, W, C


def groupnorm_bwd_stats(dxn, goff, x, half=False):
    """-> (sum dxn, sum dxn * x) fp64 [B][C] of one source of a 'gcr' layer (gn_groupnorm_bwd_stats)"""
    B, D, H, W, C = _gn_bwd_dims(dxn, goff, x, half, "groupnorm_bwd_stats")
    s = torch.empty((2, B, C), dtype=torch.float64, device=x.device)
    nbytes = _lib.load().gn_groupnorm_bwd_stats_workspace_bytes(B, D * H * W, C)
    ws = _ws(nbytes, x.device)
    _lib.call("gn_groupnorm_bwd_stats", _p(dxn), dxn.shape[-1], int(goff), _p(x), B, D, H, W, C, 1 if half else 0, _p(ws), nbytes, _p(s[0]), _p(s[1]), _stream())
    return s[0], s[1]


def groupnorm_bwd_coef(t0, t1, st0, st1, groups, eps, gamma, real=None):
    """t0 / t1: groupnorm_bwd_stats of source 0 / 1 (t1, st1 None: one source); st0 / st1: the forward's (sum, sumsq, V); real: as groupnorm_affine.
    -> (p, q, r [B][C0 + C1 stored], dgamma, dbeta [real channels])  (gn_groupnorm_bwd_coef)"""
    s0, q0, V0 = st0
    B, C0 = s0.shape
    if st1 is not None:
        s1, q1, V1 = st1
        C1, rep = s1.shape[1], V0 // V1
        a1, b1 = t1
    else:
        s1 = q1 = a1 = b1 = None
        C1, V1, rep = 0, 0, 1
    r0, r1 = (C0, C1) if real is None else (int(real[0]), int(real[1]) if len(real) > 1 else 0)
    _chk(gamma, torch.float32, "gamma")
    if gamma.numel() != r0 + r1:
        raise ValueError(f"groupnorm_bwd_coef: gamma has {gamma.numel()} entries for {r0 + r1} real channels")
    for t in (t0[0], t0[1]) + ((a1, b1) if st1 is not None else ()):
        _chk(t, torch.float64, "groupnorm_bwd_coef: sums")
    dev = s0.device
    pqr = torch.empty((3, B, C0 + C1), dtype=torch.float32, device=dev)
    dgb = torch.empty((2, r0 + r1), dtype=torch.float32, device=dev)
    _lib.call("gn_groupnorm_bwd_coef", _p(t0[0]), _p(t0[1]), _p(s0), _p(q0), r0, C0, V0, _p(a1), _p(b1), _p(s1), _p(q1), r1, C1, V1, rep, B, int(groups),
              float(eps), _p(gamma), _p(pqr[0]), _p(pqr[1]), _p(pqr[2]), _p(dgb[0]), _p(dgb[1]), _stream())
    return pqr[0], pqr[1], pqr[2], dgb[0], dgb[1]


def groupnorm_bwd_apply(dxn, goff, x, p, q, r, coff, half=False, out=None):
    """dx = dxn * p + x * q + r for one source (half: the x2 nearest upsampling's backward folded in); out given: the result is ADDED to it
    (gn_groupnorm_bwd_apply)"""
    B, D, H, W, C = _gn_bwd_dims(dxn, goff, x, half, "groupnorm_bwd_apply")
    cs = p.shape[-1]
    for t in (p, q, r):
        _chk(t, torch.float32, "groupnorm_bwd_apply: coefficients")
        if tuple(t.shape) != (B, cs) or coff < 0 or coff + C > cs:
            raise ValueError(f"groupnorm_bwd_apply: coefficients must be [B][>= {coff + C}], got {tuple(t.shape)}")
    acc = out is not None
    if acc:
        _vol5(out, "out", x)
    else:
        out = torch.empty_like(x)
    _lib.call("gn_groupnorm_bwd_apply", _p(dxn), dxn.shape[-1], int(goff), _p(x), B, D, H, W, C, 1 if half else 0, _p(p), _p(q), _p(r), cs, int(coff),
              1 if acc else 0, _p(out), _stream())
    return out


def maxpool3d_2_bwd(grad_out, x):
    """gradient of maxpool3d_2 with respect to its stored input x [B][D][H][W][C] (even D, H, W): gn_maxpool3d_2_bwd"""
    _vol5(x, "x")
    _vol5(grad_out, "grad_out")
    B, D, H, W, C = x.shape
    if tuple(grad_out.shape) != (B, D // 2, H // 2, W // 2, C):
        raise ValueError(f"maxpool3d_2_bwd: grad_out {tuple(grad_out.shape)} does not match the pooled shape of x {tuple(x.shape)}")
    g = torch.empty_like(x)
    _lib.call("gn_maxpool3d_2_bwd", _p(grad_out), _p(x), B, D, H, W, C, _p(g), _stream())
    return g


# ------------------------------------------------------------------------------------------------ MLP gradients (csrc/linear_grad.hip)
def linear_act_bwd(dy, r=None, sc=None, out=None):
    """the backward of a block's epilogue y = r * sc + sh, r = relu(.): rows dy [M][N], the saved r [M][N] (None: no ReLU) and the folded scale sc [N]
    (None: 1) -> (g [M][N] = r > 0 ? dy * sc : 0, sums fp64 [3][N] = sum g, sum dy, sum dy * r)  (gn_linear_act_bwd).  With neither r nor sc, g IS dy
    (nothing is written).  out: the buffer of g (may be dy)."""
    dy = fp32_rows(dy, "linear_act_bwd: dy")
    M, N = dy.shape
    if r is not None:
        r = fp32_rows(r, "linear_act_bwd: r", M, N)
    if sc is not None:
        _chk(sc, torch.float32, "linear_act_bwd: sc")
        if sc.numel() != N:
            raise ValueError(f"linear_act_bwd: sc has {sc.numel()} entries for {N} columns")
    if r is None and sc is None:
        g = None
    else:
        g = new_rows(M, N, dy.device) if out is None else fp32_rows(out, "linear_act_bwd: out", M, N)
        if out is not None and g is not out:
            raise ValueError("linear_act_bwd: out must have unit column stride")
    sums = torch.empty((3, N), dtype=torch.float64, device=dy.device)
    nbytes = _lib.load().gn_linear_act_bwd_workspace_bytes(M, N)
    ws = _ws(nbytes, dy.device)
    _lib.call("gn_linear_act_bwd", _p(dy), rows_view(dy)[1], _p(r), 0 if r is None else rows_view(r)[1], _p(sc), M, N, _p(g),
              0 if g is None else rows_view(g)[1], _p(ws), nbytes, _p(sums), _stream())
    return (dy if g is None else g), sums


def linear_bwd_weight(g, x, K=None, out=None):
    """rows g [M][N], x [M][>= K] -> dW [N][K] = g^T x on the fp32 matrix cores (gn_linear_bwd_weight); out: rows [N][K] with any row stride"""
    g = fp32_rows(g, "linear_bwd_weight: g")
    M, N = g.shape
    x = fp32_rows(x, "linear_bwd_weight: x", M)
    K = x.shape[1] if K is None else int(K)
    if not 1 <= K <= x.shape[1]:
        raise ValueError(f"linear_bwd_weight: K={K} outside x {tuple(x.shape)}")
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=x.device)
    elif fp32_rows(out, "linear_bwd_weight: out", N, K) is not out:
        raise ValueError("linear_bwd_weight: out must have unit column stride")
    nbytes = _lib.load().gn_linear_bwd_weight_workspace_bytes(M, N, K)
    ws = _ws(nbytes, x.device)
    _lib.call("gn_linear_bwd_weight", _p(g), rows_view(g)[1], _p(x), rows_view(x)[1], M, N, K, _p(ws), nbytes, _p(out), rows_view(out)[1], _stream())
    return out


def row_affine(r, sc, sh, out=None):
    """y = fadd(fmul(r, sc[n]), sh[n]) over rows r [M][N]: gn_linear's BatchNorm epilogue as its own pass, the same bits (gn_row_affine)"""
    r = fp32_rows(r, "row_affine: r")
    M, N = r.shape
    for t in (sc, sh):
        _chk(t, torch.float32, "row_affine: sc / sh")
        if t.numel() != N:
            raise ValueError(f"row_affine: sc / sh have {t.numel()} entries for {N} columns")
    if out is None:
        out = new_rows(M, N, r.device)
    _lib.call("gn_row_affine", _p(r), rows_view(r)[1], _p(sc), _p(sh), M, N, _p(out), rows_view(out)[1], _stream())
    return out


# ------------------------------------------------------------------------------------------------ train-mode BatchNorm (csrc/linear_grad.hip)
def col_moments(r):
    """rows r [M][N] -> fp64 [2][N]: the column mean and m2 = sum_m (r - mean)^2, two passes (gn_col_moments); a constant column has m2 == 0.0"""
    r = fp32_rows(r, "col_moments: r")
    M, N = r.shape
    out = torch.empty((2, N), dtype=torch.float64, device=r.device)
    nbytes = _lib.load().gn_col_moments_workspace_bytes(M, N)
    ws = _ws(nbytes, r.device)
    _lib.call("gn_col_moments", _p(r), rows_view(r)[1], M, N, _p(ws), nbytes, _p(out), _stream())
    return out


def col_dots(dy, r):
    """rows dy, r [M][N] -> fp64 [2][N] = sum_m dy, sum_m dy * r (gn_col_dots)"""
    dy = fp32_rows(dy, "col_dots: dy")
    M, N = dy.shape
    r = fp32_rows(r, "col_dots: r", M, N)
    out = torch.empty((2, N), dtype=torch.float64, device=dy.device)
    nbytes = _lib.load().gn_col_dots_workspace_bytes(M, N)
    ws = _ws(nbytes, dy.device)
    _lib.call("gn_col_dots", _p(dy), rows_view(dy)[1], _p(r), rows_view(r)[1], M, N, _p(ws), nbytes, _p(out), _stream())
    return out


def bn_train_bwd(dy, r, coef, out=None):
    """rows dy, r [M][N], coef fp64 [3][N] = (a, b, c) -> (g [M][N] = r > 0 ? a * dy + b * r + c : 0, evaluated in fp64 and rounded once; sum_g fp64 [N])
    (gn_bn_train_bwd).  out: the buffer of g (may be dy)."""
    dy = fp32_rows(dy, "bn_train_bwd: dy")
    M, N = dy.shape
    r = fp32_rows(r, "bn_train_bwd: r", M, N)
    _chk(coef, torch.float64, "bn_train_bwd: coef")
    if tuple(coef.shape) != (3, N):
        raise ValueError(f"bn_train_bwd: coef must be (3, {N}), got {tuple(coef.shape)}")
    g = new_rows(M, N, dy.device) if out is None else fp32_rows(out, "bn_train_bwd: out", M, N)
    if out is not None and g is not out:
        raise ValueError("bn_train_bwd: out must have unit column stride")
    sum_g = torch.empty(N, dtype=torch.float64, device=dy.device)
    nbytes = _lib.load().gn_bn_train_bwd_workspace_bytes(M, N)
    ws = _ws(nbytes, dy.device)
    _lib.call("gn_bn_train_bwd", _p(dy), rows_view(dy)[1], _p(r), rows_view(r)[1], _p(coef), M, N, _p(g), rows_view(g)[1], _p(ws), nbytes, _p(sum_g),
              _stream())
    return g, sum_g


# ------------------------------------------------------------------------------------------------ resident dataset (csrc/resident.hip)
def resident_store(arrays, volume_shape=(0, 0, 0)):
    """the GnResidentStore of a dict of device tensors keyed by _lib.RESIDENT_ARRAYS (a missing / None entry: NULL); the caller keeps the tensors alive"""
    n = arrays["meta"].shape[0]
    if tuple(arrays["meta"].shape) != (n, len(_lib.RESIDENT_META)) or arrays["meta"].dtype != torch.int64:
        raise ValueError(f"resident_store: meta must be int64 (n, {len(_lib.RESIDENT_META)})")
    dtypes = {"pc_rgb": torch.uint8, "faces": torch.int32, "mc_faces": torch.int32, "cdf_nocs": torch.float64, "cdf_task": torch.float64,
              "cdf_mc": torch.float64, "meta": torch.int64}
    ptrs = []
    for k in _lib.RESIDENT_ARRAYS:
        t = arrays.get(k)
        ptrs.append(None if t is None else _p(_chk(t, dtypes.get(k, torch.float32), "resident_store: " + k)).value)
    _CALL.dev = None
    return _lib.ResidentStore(*ptrs, n, *[int(v) for v in volume_shape])


def _res(store):
    return ctypes.byref(store)


def resident_points(store, slots, sel, noise, rot, x, y, pos, batch):
    """gn_resident_points: sel int32 (B, P) -> x, y, pos (B*P, 3) fp32 and batch (B*P,) int64, written in place"""
    B, P = sel.shape
    _lib.call("gn_resident_points", _res(store), _p(_chk(slots, torch.int32, "slots")), B, P, _p(_chk(sel, torch.int32, "sel")),
              _p(None if noise is None else _chk(noise, torch.float64, "noise")), _p(None if rot is None else _chk(rot, torch.float32, "rot")),
              _p(x), _p(y), _p(pos), _p(_chk(batch, torch.int64, "batch")), _stream())


def resident_garment(store, slots, sel, rot, grip_pc_idx, sim_grip, nocs_grip, scale_bits, dataset_idx, aabb, rot_out):
    """gn_resident_garment: the per-garment fields of a batch, written in place"""
    B, P = sel.shape
    _lib.call("gn_resident_garment", _res(store), _p(slots), B, P, _p(sel), _p(rot), _p(_chk(grip_pc_idx, torch.int64, "grip_pc_idx")), _p(sim_grip),
              _p(nocs_grip), _p(_chk(scale_bits, torch.int64, "scale_bits")), _p(_chk(dataset_idx, torch.int64, "dataset_idx")), _p(aabb), _p(rot_out),
              _stream())


def resident_volume(store, slots, uniform, face_u, uv, noise, rot, occupancy, query, value):
    """gn_resident_volume: query (B, M, 3), value (B, M) fp32 written in place; uniform (B, n_uniform, 3) fp32; face_u / uv / noise fp64 or None"""
    B, M = value.shape
    _lib.call("gn_resident_volume", _res(store), _p(slots), B, M, uniform.shape[1], _p(_chk(uniform, torch.float32, "uniform")),
              _p(None if face_u is None else _chk(face_u, torch.float64, "face_u")), _p(None if uv is None else _chk(uv, torch.float64, "uv")),
              _p(None if noise is None else _chk(noise, torch.float64, "noise")), _p(rot), int(bool(occupancy)), _p(query), _p(value), _stream())


def resident_volume_queries(store, slots, uniform, face_u, uv, noise, rot, plain, query):
    """gn_resident_volume_queries: the queries of resident_volume alone, query (B, M, 3) written in place; plain (B, M, 3) or None: the queries before `rot`"""
    B, M = query.shape[0], query.shape[1]
    _lib.call("gn_resident_volume_queries", _res(store), _p(slots), B, M, uniform.shape[1], _p(_chk(uniform, torch.float32, "uniform")),
              _p(None if face_u is None else _chk(face_u, torch.float64, "face_u")), _p(None if uv is None else _chk(uv, torch.float64, "uv")),
              _p(None if noise is None else _chk(noise, torch.float64, "noise")), _p(rot), _p(None if plain is None else _chk(plain, torch.float32, "plain")),
              _p(_chk(query, torch.float32, "query")), _stream())


def resident_query_targets(store, slots, query, task_space, total_verts, max_nf, kind, tsdf_clip_value, absolute, value, bad):
    """gn_resident_query_targets: value (B, M) fp32 written in place = the target of volume_group `kind` at query (B, M, 3), garment b against the resident
    mesh of slots[b] (task_space: its task-space vertices); bad int64 (2,), zeroed by the caller, stays on the device: nothing is read back here"""
    B, M = value.shape
    code = _qt_kind(kind, "resident_query_targets")
    nbytes = _lib.load().gn_query_targets_workspace_bytes(B, M, int(max_nf), code)
    ws = _ws(nbytes, value.device)
    _lib.call("gn_resident_query_targets", _res(store), _p(slots), B, M, int(bool(task_space)), int(total_verts), int(max_nf), code,
              int(tsdf_clip_value is not None), float(tsdf_clip_value) if tsdf_clip_value is not None else 0.0, int(bool(absolute)),
              _p(_chk(query, torch.float32, "query")), _p(ws), nbytes, _p(_chk(value, torch.float32, "value")), _p(_chk(bad, torch.int64, "bad")), _stream())


def resident_surface(store, slots, face_u, uv, task_space, rot, query, target):
    """gn_resident_surface: query, target (B, M, 3) fp32 written in place; face_u (B, M), uv (B, M, 2) fp64"""
    B, M = face_u.shape
    _lib.call("gn_resident_surface", _res(store), _p(slots), B, M, _p(_chk(face_u, torch.float64, "face_u")), _p(_chk(uv, torch.float64, "uv")),
              int(bool(task_space)), _p(rot), _p(query), _p(target), _stream())


def resident_mc_surface(store, slots, face_u, uv, query, on_surf):
    """gn_resident_mc_surface: query (B, M, 3), on_surf (B, M, 1) fp32 written in place"""
    B, M = face_u.shape
    _lib.call("gn_resident_mc_surface", _res(store), _p(slots), B, M, _p(_chk(face_u, torch.float64, "face_u")), _p(_chk(uv, torch.float64, "uv")),
              _p(query), _p(on_surf), _stream())


# ------------------------------------------------------------------------------------------------ training monitors
def _render_dims(who, n_images, img_size):
    """the limits of the two render entries that size an output: refused here, before it is allocated, in the entry's words"""
    S = int(img_size)
    if not 1 <= S <= _lib.RENDER_MAX_SIZE:
        raise ValueError(f"{who}: image size S={S} outside [1, {_lib.RENDER_MAX_SIZE}]")
    if n_images > 65535:
        raise ValueError(f"{who}: I={n_images} images outside [0, 65535]")
    return S


def _side(s):
    return _lib.RENDER_SIDES.get(s, s) if isinstance(s, str) else int(s)


def render_points_batch(points, seg, sides, kernel_sizes, img_size):
    """the reference's render_points_idx behind its camera, I images in ONE launch (gn_render_points_batch) -> (I, S, S) int32 holding the uint32 index
    images (0xFFFFFFFF, i.e. -1, where no point covers the pixel).  points: (N, 3) fp32 on the device; image i draws points seg[i] .. seg[i+1] (seg: I + 1
    host integers, non-decreasing) from sides[i] ('front' / 'top' / 'left' or 0 / 1 / 2) with a kernel_sizes[i]-wide footprint.  A pixel holds the index,
    counted from seg[i], of the covering point nearest to the camera (fp64 depth; equal depths: the lowest index)."""
    points = _chk(points, torch.float32, "points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: expected an (N, 3) tensor, got {tuple(points.shape)}")
    seg = np.ascontiguousarray(np.asarray(seg, dtype=np.int64).reshape(-1))
    n = seg.shape[0] - 1
    side = np.ascontiguousarray(np.array([_side(s) for s in sides], dtype=np.int32).reshape(-1))
    ks = np.ascontiguousarray(np.asarray(kernel_sizes, dtype=np.int32).reshape(-1))
    if n < 0 or side.shape[0] != n or ks.shape[0] != n:
        raise ValueError(f"render_points_batch: seg holds I + 1 entries for I sides and kernel sizes (got {seg.shape[0]}, {side.shape[0]}, {ks.shape[0]})")
    S = _render_dims("gn_render_points_batch", n, img_size)
    if n and (seg[0] < 0 or np.any(np.diff(seg) < 0) or seg[-1] > points.shape[0]):
        raise ValueError("render_points_batch: seg must be non-decreasing within [0, N]")
    out = torch.empty((n, S, S), dtype=_i32, device=points.device)
    if n == 0:
        return out
    tab = torch.from_numpy(np.stack([seg[:-1], seg[1:], side.astype(np.int64), ks.astype(np.int64)], axis=1)).to(points.device)
    _lib.call("gn_render_points_batch", _p(points), seg.ctypes.data_as(ctypes.c_void_p), side.ctypes.data_as(ctypes.c_void_p),
              ks.ctypes.data_as(ctypes.c_void_p), _p(tab), n, S, _p(out), _stream())
    return out


def color_idx_batch(idx_img, images, colors=None, values=None):
    """the reference's color_idx_img for I index images in ONE launch (gn_color_idx_batch) -> (I, S, S, 4) fp32 RGBA.  idx_img: (I, S, S) int32 as
    render_points_batch returns it.  images: one dict per image --
        offset, count     the image's rows of `colors` ((M, 4) fp32) or entries of `values` ((M,) fp32); index j reads row offset + j
        mode              "table" (colors) or "viridis" (values through matplotlib's viridis over (vmin, vmax))
        side, default_color (4 floats; default (1, 1, 1, 0)), vmin, vmax
        overlays          up to 3 of (xyz, rgba, kernel_size): overlay_grip's one-point images, applied in order"""
    idx_img = _chk(idx_img, _i32, "idx_img")
    if idx_img.dim() != 3 or idx_img.shape[1] != idx_img.shape[2]:
        raise ValueError(f"idx_img: expected an (I, S, S) tensor, got {tuple(idx_img.shape)}")
    n = idx_img.shape[0]
    if len(images) != n:
        raise ValueError(f"color_idx_batch: {len(images)} image entries for {n} index images")
    S = _render_dims("gn_color_idx_batch", n, idx_img.shape[1])
    dev = idx_img.device
    for name, t, width in (("colors", colors, 4), ("values", values, None)):
        if t is None:
            continue
        _chk(t, torch.float32, name)
        if t.device != dev or (t.dim() != 2 or t.shape[1] != 4 if width else t.dim() != 1):
            raise ValueError(f"{name}: expected {'an (M, 4)' if width else 'an (M,)'} tensor on {dev}, got {tuple(t.shape)} on {t.device}")
    if colors is not None and colors.data_ptr() % 16:
        colors = colors.clone()                              # (the kernel reads a row as one float4)
    out = torch.empty((n, S, S, 4), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    tab = (_lib.ColorImage * n)()
    for e, im in zip(tab, images):
        mode = im.get("mode", "table")
        if mode not in ("table", "viridis"):
            raise ValueError(f"color_idx_batch: unknown mode {mode!r}")
        src = colors if mode == "table" else values
        e.offset, e.count = int(im.get("offset", 0)), int(im["count"])
        if e.offset < 0 or e.count < 0 or e.offset + e.count > (0 if src is None else src.shape[0]):
            raise ValueError(f"color_idx_batch: rows {e.offset} .. {e.offset + e.count} are outside the image's colour source")
        e.mode, e.side = (_lib.COLOR_TABLE if mode == "table" else _lib.COLOR_VIRIDIS), _side(im.get("side", "front"))
        e.vmin, e.vmax = float(im.get("vmin", 0.0)), float(im.get("vmax", 1.0))
        e.default_color[:] = [float(v) for v in im.get("default_color", (1, 1, 1, 0))]
        overlays = im.get("overlays", ())
        if len(overlays) > _lib.RENDER_MAX_OVERLAYS:
            raise ValueError(f"color_idx_batch: {len(overlays)} overlays (at most {_lib.RENDER_MAX_OVERLAYS})")
        e.num_overlays = len(overlays)
        for o, (xyz, rgba, k) in zip(e.overlay, overlays):
            o.xyz[:], o.rgba[:], o.kernel_size = [float(v) for v in xyz], [float(v) for v in rgba], int(k)
    tab_dev = _table_dev(tab, dev)
    _lib.call("gn_color_idx_batch", _p(idx_img), ctypes.cast(tab, ctypes.c_void_p), _p(tab_dev), _p(colors), _p(values), n, S, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------ lists of meshes -> the device
def meshes_f64(meshes, device=None):
    """[(verts, faces)] numpy arrays -> [(fp64 (V, 3), int64 (F, 3))] on the device (default: the current one): what the field entries take"""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    return [(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev),
             torch.from_numpy(np.ascontiguousarray(np.asarray(f).reshape(-1, 3), dtype=np.int64)).to(dev)) for v, f in meshes]


def pack_meshes(meshes, extra_widths=(), device=None):
    """[(verts, faces, *per-vertex extras)], numpy arrays or torch tensors on the host or the device -> (verts (V, 3) fp32, faces (F, 3) int32,
    *extras (V, width) fp32, vseg, fseg): the meshes back to back on the device (arrays go to `device`, default the current one; tensors stay where
    they are) with their host CSRs, as the segmented-mesh entries take them"""
    def dev(a, dtype, width):
        if not torch.is_tensor(a):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32 if dtype == _i32 else np.float32)).to(device or "cuda")
        return a.detach().to(dtype).reshape(-1, width)

    columns = [[dev(m[k], _i32 if k == 1 else torch.float32, w) for m in meshes] for k, w in enumerate((3, 3) + tuple(extra_widths))]
    vseg, fseg = (np.concatenate([[0], np.cumsum([t.shape[0] for t in col])]).astype(np.int64) for col in columns[:2])
    return tuple(torch.cat(col).contiguous() for col in columns) + (vseg, fseg)


# ------------------------------------------------------------------------------------------------ mesh images
def _segmented_meshes(who, verts, faces, vseg, fseg, entries):
    """the shared head of _mesh_args / _depth_args: the checked tensors and the two host CSRs.  entries(M by vseg, M by fseg) refuses the caller's own
    per-image lists in between; then what only sizes an access is refused (a segment beyond its tensor).  The CSRs' order is the entry's to refuse"""
    verts, faces = _chk(verts, torch.float32, "verts"), _chk(faces, _i32, "faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.device != verts.device:
        raise ValueError(f"{who}: expected (V, 3) fp32 verts and (F, 3) int32 faces on one device, got {tuple(verts.shape)}, {tuple(faces.shape)}")
    vseg = np.ascontiguousarray(np.asarray(vseg, dtype=np.int64).reshape(-1))
    fseg = np.ascontiguousarray(np.asarray(fseg, dtype=np.int64).reshape(-1))
    entries(vseg.shape[0] - 1, fseg.shape[0] - 1)
    if vseg.shape[0] > 1 and (vseg.max() > verts.shape[0] or fseg.max() > faces.shape[0]):
        raise ValueError(f"{who}: a segment ends beyond its tensor ({verts.shape[0]} verts, {faces.shape[0]} faces)")
    return verts, faces, vseg, fseg


def _mesh_args(who, verts, faces, vseg, fseg, sides, ambients, default_colors):
    """_segmented_meshes and the GnMeshImage table (host, device) of the mesh entries; sides and ambients are the entry's to refuse, in its words"""
    def entries(n, nf):
        nonlocal side, ambients, default_colors
        side = [_side(s) for s in sides]
        ambients = [0.35] * n if ambients is None else list(ambients)
        default_colors = [(1.0, 1.0, 1.0, 0.0)] * n if default_colors is None else list(default_colors)
        if n < 0 or nf != n or len(side) != n or len(ambients) != n or len(default_colors) != n:
            raise ValueError(f"{who}: vseg and fseg hold I + 1 entries for I sides, ambients and default colours")

    side = None
    verts, faces, vseg, fseg = _segmented_meshes(who, verts, faces, vseg, fseg, entries)
    n = len(side)
    tab = (_lib.MeshImage * max(n, 1))()
    for i in range(n):
        e = tab[i]
        e.vert_begin, e.vert_end, e.face_begin, e.face_end = int(vseg[i]), int(vseg[i + 1]), int(fseg[i]), int(fseg[i + 1])
        e.side, e.ambient = side[i], float(ambients[i])
        e.default_color[:] = [float(v) for v in default_colors[i]]
    return verts, faces, vseg, fseg, tab, _table_dev(tab, verts.device), n


def render_mesh_batch(verts, faces, vseg, fseg, sides, img_size):
    """the triangle rasteriser, I images in ONE launch (gn_render_mesh_batch) -> (I, S, S) int32 holding the uint32 index images (0xFFFFFFFF, i.e. -1,
    where no face covers the pixel's sample).  verts: (V, 3) fp32 and faces: (F, 3) int32 on the device; image i draws the faces fseg[i] .. fseg[i+1],
    which index into the vertices vseg[i] .. vseg[i+1] from 0, seen from sides[i].  A pixel holds the index, counted from fseg[i], of the covering face
    with the smallest interpolated fp64 depth (equal depths: the lowest index).  DESIGN.md "Mesh images" has the rules."""
    verts, faces, vseg, fseg, tab, tab_dev, n = _mesh_args("render_mesh_batch", verts, faces, vseg, fseg, sides, None, None)
    S = _render_dims("gn_render_mesh_batch", n, img_size)
    out = torch.empty((n, S, S), dtype=_i32, device=verts.device)
    if n == 0:
        return out
    _lib.call("gn_render_mesh_batch", _p(verts), _p(faces), vseg.ctypes.data_as(ctypes.c_void_p), fseg.ctypes.data_as(ctypes.c_void_p),
              ctypes.cast(tab, ctypes.c_void_p), _p(tab_dev), n, S, _p(out), _stream())
    return out


def color_mesh_batch(idx_img, verts, faces, colors, vseg, fseg, sides, ambients=None, default_colors=None):
    """render_mesh_batch's index images -> (I, S, S, 4) fp32 RGBA in ONE launch (gn_color_mesh_batch): shade * the barycentric mix of the winning
    face's vertex colours with alpha 1, default_colors[i] where nobody covers.  colors: (V, 4) fp32, one row per row of verts; ambients[i] in [0, 1]
    (default 0.35: a look, not a measurement): shade = ambient + (1 - ambient) * |n_z| / |n| of the face's camera-space normal."""
    idx_img = _chk(idx_img, _i32, "idx_img")
    if idx_img.dim() != 3 or idx_img.shape[1] != idx_img.shape[2]:
        raise ValueError(f"idx_img: expected an (I, S, S) tensor, got {tuple(idx_img.shape)}")
    verts, faces, vseg, fseg, tab, tab_dev, n = _mesh_args("color_mesh_batch", verts, faces, vseg, fseg, sides, ambients, default_colors)
    colors = _chk(colors, torch.float32, "colors")
    if colors.dim() != 2 or colors.shape[1] != 4 or colors.shape[0] != verts.shape[0] or colors.device != verts.device or idx_img.device != verts.device:
        raise ValueError(f"color_mesh_batch: expected ({verts.shape[0]}, 4) colors on {verts.device}, got {tuple(colors.shape)} on {colors.device}")
    if idx_img.shape[0] != n:
        raise ValueError(f"color_mesh_batch: {n} image entries for {idx_img.shape[0]} index images")
    S = _render_dims("gn_color_mesh_batch", n, idx_img.shape[1])
    if colors.data_ptr() % 16:
        colors = colors.clone()                              # (the kernel reads a row as one float4)
    out = torch.empty((n, S, S, 4), dtype=torch.float32, device=verts.device)
    if n == 0:
        return out
    _lib.call("gn_color_mesh_batch", _p(idx_img), _p(verts), _p(faces), _p(colors), vseg.ctypes.data_as(ctypes.c_void_p),
              fseg.ctypes.data_as(ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p), _p(tab_dev), n, S, _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------ point clouds from meshes
def _depth_args(who, verts, faces, vseg, fseg, mesh_of, cameras, ambients, base_colors):
    """_segmented_meshes, the images' mesh numbers and the GnDepthImage table (host, device).  cameras: one record per image ({"R" (3, 3), "t" (3,),
    "f", "c", "near"}; point_cloud.camera_ring builds them).  A mesh number outside the CSRs would size an access too and is refused here; cameras
    and ambients are the entry's to refuse, in its words"""
    def entries(m, mf):
        nonlocal mesh_of, cameras, ambients, base_colors
        mesh_of = np.ascontiguousarray(np.asarray(mesh_of, dtype=np.int32).reshape(-1))
        n, cameras = mesh_of.shape[0], list(cameras)
        ambients = [0.35] * n if ambients is None else list(ambients)
        base_colors = [(0.5, 0.5, 0.5)] * n if base_colors is None else list(base_colors)
        if m < 0 or mf != m or len(cameras) != n or len(ambients) != n or len(base_colors) != n:
            raise ValueError(f"{who}: vseg and fseg hold M + 1 entries for M meshes; mesh_of, cameras, ambients and base colours one entry per image")
        if n and (m == 0 or mesh_of.min() < 0 or mesh_of.max() >= m):
            raise ValueError(f"{who}: an image's mesh number is outside [0, M={m})")

    verts, faces, vseg, fseg = _segmented_meshes(who, verts, faces, vseg, fseg, entries)
    m, n = vseg.shape[0] - 1, mesh_of.shape[0]
    tab = (_lib.DepthImage * max(n, 1))()
    for i in range(n):
        e, cam, g = tab[i], cameras[i], int(mesh_of[i])
        e.vert_begin, e.vert_end, e.face_begin, e.face_end = int(vseg[g]), int(vseg[g + 1]), int(fseg[g]), int(fseg[g + 1])
        e.R[:] = [float(v) for v in np.asarray(cam["R"], dtype=np.float64).reshape(9)]
        e.t[:] = [float(v) for v in np.asarray(cam["t"], dtype=np.float64).reshape(3)]
        e.f, e.c, e.znear, e.ambient = float(cam["f"]), float(cam["c"]), float(cam["near"]), float(ambients[i])
        e.base_color[:] = [float(v) for v in base_colors[i]]
    return verts, faces, vseg, fseg, mesh_of, tab, _table_dev(tab, verts.device), m, n


def depth_render_batch(verts, faces, vseg, fseg, mesh_of, cameras, img_size):
    """the triangle rasteriser behind perspective cameras, I images in ONE launch (gn_depth_render_batch) -> (I, S, S) int32 holding the uint32 index
    images (0xFFFFFFFF, i.e. -1, where no face covers the pixel's sample).  verts: (V, 3) fp32 and faces: (F, 3) int32 on the device, M meshes behind the
    CSRs vseg / fseg; image i draws mesh mesh_of[i] through cameras[i].  A pixel holds the index, counted from the mesh's first face, of the covering
    face with the largest perspective-correct inverse depth (equal ones: the lowest index).  DESIGN.md "Point clouds from meshes" has the rules."""
    verts, faces, vseg, fseg, mesh_of, tab, tab_dev, m, n = _depth_args("depth_render_batch", verts, faces, vseg, fseg, mesh_of, cameras, None, None)
    S = _render_dims("gn_depth_render_batch", n, img_size)
    out = torch.empty((n, S, S), dtype=_i32, device=verts.device)
    if n == 0:
        return out
    _lib.call("gn_depth_render_batch", _p(verts), _p(faces), vseg.ctypes.data_as(ctypes.c_void_p), fseg.ctypes.data_as(ctypes.c_void_p), m,
              mesh_of.ctypes.data_as(ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p), _p(tab_dev), n, S, _p(out), _stream())
    return out


def depth_cloud(idx_img, verts, nocs, faces, vseg, fseg, mesh_of, cameras, ambients=None, base_colors=None):
    """depth_render_batch's index images -> (point (N, 3) fp32, nocs (N, 3) fp32, rgb (N, 3) uint8, sizes (I,) int64 on the HOST): the covered pixels as
    point rows, image after image, within an image in raster order.  Two entries: gn_depth_cloud_offsets (a count per image row and one scan; the
    per-image sizes come back to the host to size the outputs) and gn_depth_cloud_write.  nocs: (V, 3) fp32, one row per row of verts."""
    idx_img = _chk(idx_img, _i32, "idx_img")
    if idx_img.dim() != 3 or idx_img.shape[1] != idx_img.shape[2]:
        raise ValueError(f"idx_img: expected an (I, S, S) tensor, got {tuple(idx_img.shape)}")
    verts, faces, vseg, fseg, mesh_of, tab, tab_dev, m, n = _depth_args("depth_cloud", verts, faces, vseg, fseg, mesh_of, cameras, ambients, base_colors)
    nocs = _chk(nocs, torch.float32, "nocs")
    if nocs.shape != verts.shape or nocs.device != verts.device or idx_img.device != verts.device:
        raise ValueError(f"depth_cloud: expected {tuple(verts.shape)} nocs on {verts.device}, got {tuple(nocs.shape)} on {nocs.device}")
    if idx_img.shape[0] != n:
        raise ValueError(f"depth_cloud: {n} image entries for {idx_img.shape[0]} index images")
    S = _render_dims("gn_depth_cloud_offsets", n, idx_img.shape[1])
    dev = verts.device
    if n == 0:
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.float32, device=dev),
                torch.empty((0, 3), dtype=torch.uint8, device=dev), np.zeros(0, dtype=np.int64))
    row_off = torch.empty(n * S + 1, dtype=torch.int64, device=dev)
    sizes = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.call("gn_depth_cloud_offsets", _p(idx_img), n, S, _p(row_off), _p(sizes), _stream())
    sizes = sizes.cpu().numpy()
    total = int(sizes.sum())
    point = torch.empty((total, 3), dtype=torch.float32, device=dev)
    label = torch.empty((total, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((total, 3), dtype=torch.uint8, device=dev)
    _lib.call("gn_depth_cloud_write", _p(idx_img), _p(verts), _p(nocs), _p(faces), vseg.ctypes.data_as(ctypes.c_void_p),
              fseg.ctypes.data_as(ctypes.c_void_p), m, mesh_of.ctypes.data_as(ctypes.c_void_p), ctypes.cast(tab, ctypes.c_void_p), _p(tab_dev),
              _p(row_off), n, S, total, _p(point), _p(label), _p(rgb), _stream())
    return point, label, rgb, sizes


# ------------------------------------------------------------------------------------------------ the hanging garment (cloth.py)
CLOTH_SUBSTEPS_PER_LAUNCH = 256        # a launch of the solver stays in the milliseconds on a shared machine


def cloth_device_tables(garments, states, dev):
    """the device arguments of gn_cloth_simulate_batch for `garments` and their (x, v) `states` (numpy) -> dict: x, v (fresh copies: the entry
    writes them), w, pairs, l0, alpha_t, colour_off, csr tensors, consts (ctypes double[6]), v_off (numpy), totals"""
    v_off = np.concatenate([[0], np.cumsum([len(g.w) for g in garments])])
    c_off = np.concatenate([[0], np.cumsum([len(g.l0) for g in garments])])
    k_off = np.concatenate([[0], np.cumsum([len(g.colour_off) for g in garments])])
    if v_off[-1] >= 2 ** 31 - 1 or c_off[-1] >= 2 ** 31 - 1:
        raise ValueError("cloth_simulate_batch: more than 2^31 vertices or constraints")

    def up(parts, dtype, width=None):
        a = np.concatenate([np.asarray(p).reshape((-1,) if width is None else (-1, width)) for p in parts]).astype(dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {"x": up([s[0] for s in states], np.float64, 3), "v": up([s[1] for s in states], np.float64, 3), "w": up([g.w for g in garments], np.float64),
         # an index that does not fit int32 is out of range: keep it so
         "pairs": up([np.clip(g.pairs, -1, 2 ** 31 - 1) for g in garments], np.int32, 2),
         "l0": up([g.l0 for g in garments], np.float64), "alpha_t": up([g.alpha_t for g in garments], np.float64),
         "colour_off": up([g.colour_off for g in garments], np.int64),
         "csr": torch.from_numpy(np.stack([v_off, c_off, k_off], axis=1).astype(np.int64)).to(dev), "v_off": v_off,
         "total_verts": int(v_off[-1]), "total_constraints": int(c_off[-1])}
    if not (torch.isfinite(t["w"]).all() and torch.isfinite(t["l0"]).all() and torch.isfinite(t["alpha_t"]).all()):
        raise ValueError("cloth_simulate_batch: an inverse mass, rest length or compliance is not finite")
    c = garments[0].consts
    t["consts"] = (ctypes.c_double * 6)(c["h"], c["inv_h"], c["hg"][0], c["hg"][1], c["hg"][2], c["damp"])
    return t


CLOTH_CELL_SLACK = 2.0 ** -10          # the grid's cell edge is r * (1 + CLOTH_CELL_SLACK): DESIGN.md "Hanging garments" argues why that admits every pair


def cloth_collision_constants(garments, who):
    """the collision record the garments of one call share (cloth.collision_constants) -> None with contacts off, else the record with "cell" (the grid's
    cell edge) and "host" (ctypes double[4] = t2, r2, cell, relax) added.  Refused by name: records that differ, a constant that is not finite or not
    positive, K outside [1, 64], R < 1, relax outside (0, 1]."""
    col = garments[0].collision
    if any(g.collision != col for g in garments):
        raise ValueError(f"{who}: the garments of one call must share their collision constants (thickness, margin, rebuild, max_list, relax)")
    if col is None:
        return None
    for k in ("t2", "r", "r2", "half_margin", "relax"):
        if not (np.isfinite(col[k]) and col[k] > 0):
            raise ValueError(f"{who}: collision constant {k}={col[k]} is not finite and positive")
    if int(col["K"]) != col["K"] or not 1 <= col["K"] <= _lib.CLOTH_MAX_LIST:
        raise ValueError(f"{who}: collision_max_list K={col['K']} outside [1, {_lib.CLOTH_MAX_LIST}]")
    if int(col["R"]) != col["R"] or col["R"] < 1:
        raise ValueError(f"{who}: collision_rebuild R={col['R']} < 1")
    if not col["relax"] <= 1:
        raise ValueError(f"{who}: collision_relax={col['relax']} outside (0, 1]")
    cell = float(np.float64(col["r"]) * (np.float64(1.0) + np.float64(CLOTH_CELL_SLACK)))
    return dict(col, cell=cell, host=(ctypes.c_double * 4)(col["t2"], col["r2"], cell, col["relax"]))


def cloth_contact_buffers(garments, t, col, dev):
    """what the two contact entries need beside cloth_device_tables' `t`: x0, the lists (rows of stride K), corr, diag and the grid's workspace"""
    n, B, K = t["total_verts"], len(garments), col["K"]
    max_verts = max(len(g.w) for g in garments)
    buckets = int(_lib.load().gn_cloth_contact_buckets(max_verts))
    if n >= (2 ** 31 - 1) // _lib.CLOTH_MAX_LIST or buckets <= 0:
        raise ValueError("cloth contacts: the lists must stay below 2^31 entries")
    ws_bytes = int(_lib.load().gn_cloth_contact_workspace_bytes(n, B, buckets))
    return {"x0": torch.from_numpy(np.ascontiguousarray(np.concatenate([g.x0 for g in garments]).reshape(-1, 3))).to(dev),
            "list_j": torch.full((n, K), -1, dtype=torch.int32, device=dev), "list_tm2": torch.zeros((n, K), dtype=torch.float64, device=dev),
            "list_n": torch.zeros(n, dtype=torch.int32, device=dev), "list_total": torch.zeros(n, dtype=torch.int32, device=dev),
            "corr": torch.zeros((n, 3), dtype=torch.float64, device=dev), "diag": torch.zeros((B, 4), dtype=torch.int64, device=dev),
            "workspace": _ws(ws_bytes, dev, zero=True), "workspace_bytes": ws_bytes, "max_verts": max_verts,
            "buckets": buckets}


def _cloth_lists_call(t, c, col, B, flags):
    _lib.call("gn_cloth_contact_lists", _p(t["x"]), _p(c["x0"]), _p(t["csr"]), B, t["total_verts"], c["max_verts"], c["buckets"],
              ctypes.cast(col["host"], ctypes.c_void_p), col["K"], flags, _p(c["workspace"]), c["workspace_bytes"], _p(c["list_j"]), _p(c["list_tm2"]),
              _p(c["list_n"]), _p(c["list_total"]), _p(c["diag"]), _stream())


def cloth_contact_stats(diag, col):
    """the rows of the device's diag table -> one dict of the definition's four diagnostics per garment"""
    d = diag.cpu().numpy()
    travel = np.sqrt(np.ascontiguousarray(d[:, 3]).view(np.float64)) / np.float64(col["half_margin"])
    return [{"contact_overflow": int(r[0]), "contact_max_list": int(r[1]), "contact_travel": float(tr), "contact_active": int(r[2])}
            for r, tr in zip(d, travel)]


def cloth_face_collision_constants(garments, who):
    """the face-contact record the garments of one call share (cloth.face_collision_constants) -> None with face contacts off, else the record with
    "host" (ctypes double[2] = tf2, rf2) added.  Refused by name: records that differ, a record with the vertex contacts off, a constant that is not
    finite or not positive, Kf outside [1, 32]."""
    fcol = garments[0].face_collision
    if any(g.face_collision != fcol for g in garments):
        raise ValueError(f"{who}: the garments of one call must share their face-contact constants (face_thickness, margin, face_max_list)")
    if fcol is None:
        return None
    if any(g.collision is None for g in garments):
        raise ValueError(f"{who}: face-contact constants are set but the vertex contacts are off (collision_thickness = 0)")
    for k in ("tf2", "rf", "rf2"):
        if not (np.isfinite(fcol[k]) and fcol[k] > 0):
            raise ValueError(f"{who}: face-contact constant {k}={fcol[k]} is not finite and positive")
    if int(fcol["Kf"]) != fcol["Kf"] or not 1 <= fcol["Kf"] <= _lib.CLOTH_FACE_MAX_LIST:
        raise ValueError(f"{who}: face_max_list Kf={fcol['Kf']} outside [1, {_lib.CLOTH_FACE_MAX_LIST}]")
    return dict(fcol, host=(ctypes.c_double * 2)(fcol["tf2"], fcol["rf2"]))


CLOTH_FACE_HIT_BYTES = 256 << 20       # the most the per-chunk hit buffers of a face-list build may take: fewer chunks beyond it


def cloth_face_chunks(n_garments, max_verts, max_faces, total_verts, Kf):
    """the face chunks of a face-list build: enough workgroups (vertex blocks x chunks x garments) for about two per compute unit, no chunk below one
    tile of 128 faces, the hit buffers within CLOTH_FACE_HIT_BYTES.  The lists do not depend on it."""
    blocks = max(1, n_garments * -(-max_verts // _lib.CLOTH_FACE_BLOCK))
    chunks = max(1, min(-(-512 // blocks), -(-max_faces // 128), 64))
    while chunks > 1 and total_verts * chunks * Kf * 12 > CLOTH_FACE_HIT_BYTES:
        chunks //= 2
    return chunks


def cloth_face_buffers(garments, t, fcol, dev, chunks=None, x0=None):
    """what the two face-contact entries need beside cloth_device_tables' `t`: x0 (or the tensor cloth_contact_buffers made), faces and their CSR, the
    per-chunk hit buffers, the lists (rows of stride Kf) and fdiag, each a tensor of its own"""
    n, B, Kf = t["total_verts"], len(garments), fcol["Kf"]
    faces = [np.clip(np.asarray(g.faces, dtype=np.int64).reshape(-1, 3), -1, 2 ** 31 - 1) for g in garments]      # an index beyond int32 stays out of range
    f_off = np.concatenate([[0], np.cumsum([len(f) for f in faces])])
    max_verts, max_faces = max(len(g.w) for g in garments), max(len(f) for f in faces)
    if f_off[-1] >= (2 ** 31 - 1) // 3 or n >= (2 ** 31 - 1) // _lib.CLOTH_MAX_LIST:
        raise ValueError("cloth face contacts: the tables must stay below 2^31 entries")
    chunks = cloth_face_chunks(B, max_verts, max_faces, n, Kf) if chunks is None else int(chunks)
    if not 1 <= chunks <= _lib.CLOTH_FACE_MAX_CHUNKS:
        raise ValueError(f"cloth face contacts: chunks={chunks} outside [1, {_lib.CLOTH_FACE_MAX_CHUNKS}]")
    if x0 is None:
        x0 = torch.from_numpy(np.ascontiguousarray(np.concatenate([g.x0 for g in garments]).reshape(-1, 3))).to(dev)
    return {"x0": x0,
            "faces": torch.from_numpy(np.ascontiguousarray(np.concatenate(faces).astype(np.int32))).to(dev),
            "fcsr": torch.from_numpy(f_off.astype(np.int64)).to(dev), "total_faces": int(f_off[-1]), "max_verts": max_verts, "chunks": chunks,
            "hit_f": torch.empty((n, chunks, Kf), dtype=torch.int32, device=dev), "hit_tm2": torch.empty((n, chunks, Kf), dtype=torch.float64, device=dev),
            "hit_n": torch.zeros((n, chunks), dtype=torch.int32, device=dev),
            "list_f": torch.full((n, Kf), -1, dtype=torch.int32, device=dev), "list_tm2": torch.zeros((n, Kf), dtype=torch.float64, device=dev),
            "list_n": torch.zeros(n, dtype=torch.int32, device=dev), "list_total": torch.zeros(n, dtype=torch.int32, device=dev),
            "fdiag": torch.zeros((B, 3), dtype=torch.int64, device=dev)}


def _cloth_face_lists_call(t, fc, col, fcol, B, bad):
    _lib.call("gn_cloth_face_contact_lists", _p(t["x"]), _p(fc["x0"]), _p(t["csr"]), _p(fc["faces"]), _p(fc["fcsr"]), B, t["total_verts"],
              fc["total_faces"], fc["max_verts"], ctypes.cast(fcol["host"], ctypes.c_void_p), ctypes.cast(col["host"], ctypes.c_void_p), fcol["Kf"],
              fc["chunks"], _p(fc["hit_f"]), _p(fc["hit_tm2"]), fc["hit_f"].numel(), _p(fc["hit_n"]), fc["hit_n"].numel(), _p(fc["list_f"]),
              _p(fc["list_tm2"]), fc["list_f"].numel(), _p(fc["list_n"]), _p(fc["list_total"]), fc["list_n"].numel(), _p(fc["fdiag"]),
              fc["fdiag"].shape[0], _p(bad), _stream())


def cloth_face_contact_stats(fdiag):
    """the rows of the device's fdiag table -> one dict of the definition's three face diagnostics per garment"""
    return [{"face_contact_overflow": int(r[0]), "face_contact_max_list": int(r[1]), "face_contact_active": int(r[2])} for r in fdiag.cpu().numpy()]


def cloth_face_contact_lists(garments, states=None, backend="hip", device=None, chunks=None):
    """the face-contact lists of cloth.py's definition for every garment at the positions of `states` (None: the start pose), all garments in the same
    launches (gn_cloth_face_contact_lists: all (vertex, face) pairs, the faces of a garment spread over `chunks` workgroups per block of vertices; None:
    cloth_face_chunks) -> [((idx (V, Kf) int32, tm2 (V, Kf) float64), counts (V,) int64, overflow (V,) int64)] tensors: bit for bit
    cloth.face_contact_lists_reference (backend "numpy"), whatever `chunks`.  The garments must have face contacts on and share their constants.  A face
    index outside [0, V) raises IndexError (after the launch; nothing is read or written through it)."""
    from . import cloth
    if backend not in ("hip", "numpy"):
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'numpy'")
    states = [None] * len(garments) if states is None else list(states)
    if len(states) != len(garments):
        raise ValueError("cloth_face_contact_lists: one state per garment")
    states = [cloth.state_arrays(g, *(s if s is not None else (None, None)), who="cloth_face_contact_lists") for g, s in zip(garments, states)]
    if not garments:
        return []
    col = cloth_collision_constants(garments, "cloth_face_contact_lists")
    fcol = cloth_face_collision_constants(garments, "cloth_face_contact_lists")
    if fcol is None:
        raise ValueError("cloth_face_contact_lists: the garments have face contacts off (face_thickness = 0)")
    if backend == "numpy":
        out = []
        for g, (x, _) in zip(garments, states):
            (idx, tm2), counts, overflow = cloth.face_contact_lists_reference(g, x)
            out.append(((torch.from_numpy(idx), torch.from_numpy(tm2)), torch.from_numpy(counts), torch.from_numpy(overflow)))
        return out
    if len(garments) > 65535:
        raise ValueError(f"cloth_face_contact_lists: at most 65535 garments per call, got {len(garments)}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    t = cloth_device_tables(garments, states, dev)
    fc = cloth_face_buffers(garments, t, fcol, dev, chunks)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    _cloth_face_lists_call(t, fc, col, fcol, len(garments), bad)
    _raise_bad_face(bad.item(), "cloth_face_contact_lists")
    counts, total = fc["list_n"].to(torch.int64), fc["list_total"].to(torch.int64)
    return [((fc["list_f"][a:b], fc["list_tm2"][a:b]), counts[a:b], total[a:b] - counts[a:b]) for a, b in zip(t["v_off"][:-1], t["v_off"][1:])]


def cloth_contact_lists(garments, states=None, backend="hip", device=None):
    """the contact lists of cloth.py's definition for every garment at the positions of `states` (None: the start pose), all garments in the same
    launches (gn_cloth_contact_lists: a hashed uniform grid, many workgroups per garment) -> [((idx (V, K) int32, tm2 (V, K) float64), counts (V,)
    int64, overflow (V,) int64)] tensors: bit for bit cloth.contact_lists_reference (backend "numpy").  The garments must have contacts on and share
    their collision constants."""
    from . import cloth
    if backend not in ("hip", "numpy"):
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'numpy'")
    states = [None] * len(garments) if states is None else list(states)
    if len(states) != len(garments):
        raise ValueError("cloth_contact_lists: one state per garment")
    states = [cloth.state_arrays(g, *(s if s is not None else (None, None)), who="cloth_contact_lists") for g, s in zip(garments, states)]
    if not garments:
        return []
    col = cloth_collision_constants(garments, "cloth_contact_lists")
    if col is None:
        raise ValueError("cloth_contact_lists: the garments have contacts off (collision_thickness = 0)")
    if backend == "numpy":
        out = []
        for g, (x, _) in zip(garments, states):
            (idx, tm2), counts, overflow = cloth.contact_lists_reference(g, x)
            out.append(((torch.from_numpy(idx), torch.from_numpy(tm2)), torch.from_numpy(counts), torch.from_numpy(overflow)))
        return out
    if len(garments) > 65535:
        raise ValueError(f"cloth_contact_lists: at most 65535 garments per call, got {len(garments)}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    t = cloth_device_tables(garments, states, dev)
    c = cloth_contact_buffers(garments, t, col, dev)
    _cloth_lists_call(t, c, col, len(garments), _lib.CLOTH_LISTS_BUILD)
    counts, total = c["list_n"].to(torch.int64), c["list_total"].to(torch.int64)
    return [((c["list_j"][a:b], c["list_tm2"][a:b]), counts[a:b], total[a:b] - counts[a:b]) for a, b in zip(t["v_off"][:-1], t["v_off"][1:])]


def cloth_simulate_batch(garments, substeps, states=None, backend="hip", lds_budget=None, max_substeps_per_launch=CLOTH_SUBSTEPS_PER_LAUNCH,
                         block=None, device=None, stats=False):
    """`substeps` substeps of cloth.py's definition on every cloth.Garment of `garments`, all of them in the same launches (gn_cloth_simulate_batch: one
    workgroup per garment) -> [(x, v)] float64 (V, 3) tensors, on the device (backend "hip") or on the host (backend "numpy": cloth.simulate_reference).
    states: None or one (x, v) / None per garment (None: the start pose at rest); the inputs are not written.  The device gives the restatement's bits
    whatever the batch, `block` (threads per workgroup, a multiple of 64 up to 1024), lds_budget (bytes: a garment whose positions, 24 bytes per vertex,
    fit it keeps them in LDS, any other in global memory; default all 160 KiB) and max_substeps_per_launch (a longer run is several launches).  The
    garments must share their step constants.  A face index outside [0, V) raises IndexError (after the launch, nothing is read or written through
    it); a state that is not finite, a bad budget / block / substep count raise ValueError before it.

    Garments with contacts on (ClothParams.collision_thickness > 0; the garments of one call share their collision constants) run the contact pass of
    the definition: the wrapper alternates gn_cloth_contact_lists (every collision_rebuild substeps, counted from the call's first) and
    gn_cloth_simulate_contacts_batch on one stream, without a host synchronisation between them.  stats=True returns (states, [the four contact
    diagnostics of the definition per garment]) (all 0 with contacts off); without it the return value is what it always was.

    Garments with face contacts on as well (ClothParams.face_thickness > 0, Garment.face_collision; shared by the garments of one call) run the
    face entries of the definition: gn_cloth_face_contact_lists follows every gn_cloth_contact_lists build on the same stream and the solver is
    gn_cloth_simulate_face_contacts_batch; stats=True then carries the three face diagnostics too.  With face contacts off nothing changes."""
    from . import cloth
    if backend not in ("hip", "numpy"):
        raise ValueError(f"backend {backend!r}: expected 'hip' or 'numpy'")
    substeps = int(substeps)
    if substeps < 0 or int(max_substeps_per_launch) < 1:
        raise ValueError(f"cloth_simulate_batch: substeps={substeps}, max_substeps_per_launch={max_substeps_per_launch}")
    states = [None] * len(garments) if states is None else list(states)
    if len(states) != len(garments):
        raise ValueError("cloth_simulate_batch: one state per garment")
    states = [cloth.state_arrays(g, *(s if s is not None else (None, None)), who="cloth_simulate_batch") for g, s in zip(garments, states)]
    if not garments:
        return []
    if any(g.consts != garments[0].consts for g in garments):
        raise ValueError("cloth_simulate_batch: the garments of one call must share their step constants (h, gravity, damping, compliances)")
    col = cloth_collision_constants(garments, "cloth_simulate_batch")
    fcol = cloth_face_collision_constants(garments, "cloth_simulate_batch")
    if backend == "numpy":
        ref = [cloth.simulate_reference(g, substeps, x, v, stats=True) for g, (x, v) in zip(garments, states)]
        out = [tuple(torch.from_numpy(a) for a in r[:2]) for r in ref]
        return (out, [r[2] for r in ref]) if stats else out
    budget = _lib.CLOTH_MAX_LDS if lds_budget is None else int(lds_budget)
    if not 0 <= budget <= _lib.CLOTH_MAX_LDS:
        raise ValueError(f"cloth_simulate_batch: lds_budget={budget} outside [0, {_lib.CLOTH_MAX_LDS}]")
    nv = [len(g.w) for g in garments]
    if block is None:
        block = 256 if max(len(g.l0) for g in garments) <= 4096 else _lib.CLOTH_MAX_BLOCK
    block = int(block)
    if block % 64 or not 64 <= block <= _lib.CLOTH_MAX_BLOCK:
        raise ValueError(f"cloth_simulate_batch: block={block}: a multiple of 64 in [64, {_lib.CLOTH_MAX_BLOCK}]")
    if len(garments) > 65535:
        raise ValueError(f"cloth_simulate_batch: at most 65535 garments per call, got {len(garments)}")
    lds = max([24 * n for n in nv if 24 * n <= budget], default=0)            # the LDS the launch asks for: its largest garment that fits the budget
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    t = cloth_device_tables(garments, states, dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    solver = (_p(t["x"]), _p(t["v"]), _p(t["w"]), _p(t["pairs"]), _p(t["l0"]), _p(t["alpha_t"]), _p(t["csr"]), _p(t["colour_off"]), len(garments),
              t["total_verts"], t["total_constraints"])
    tail = (int(max_substeps_per_launch), ctypes.cast(t["consts"], ctypes.c_void_p), lds, block, _p(bad))
    if col is None:
        _lib.call("gn_cloth_simulate_batch", *solver, substeps, *tail, _stream())
        contact_stats = [{"contact_overflow": 0, "contact_max_list": 0, "contact_travel": 0.0, "contact_active": 0} for _ in garments]
    else:
        c = cloth_contact_buffers(garments, t, col, dev)
        lists = (_p(c["list_j"]), _p(c["list_tm2"]), _p(c["list_n"]), col["K"], ctypes.cast(col["host"], ctypes.c_void_p), _p(c["corr"]),
                 _p(c["diag"]))
        entry = "gn_cloth_simulate_contacts_batch"
        if fcol is not None:
            fc = cloth_face_buffers(garments, t, fcol, dev, x0=c["x0"])
            entry = "gn_cloth_simulate_face_contacts_batch"
            lists += (_p(fc["faces"]), _p(fc["fcsr"]), fc["total_faces"], _p(fc["list_f"]), _p(fc["list_tm2"]), fc["list_f"].numel(), _p(fc["list_n"]),
                      fc["list_n"].numel(), fcol["Kf"], ctypes.cast(fcol["host"], ctypes.c_void_p), _p(fc["fdiag"]), fc["fdiag"].shape[0])
        done = 0
        while True:                                                           # one pass with substeps == 0: the table is still checked
            n = min(col["R"], substeps - done)
            if n > 0:
                _cloth_lists_call(t, c, col, len(garments), _lib.CLOTH_LISTS_BUILD | (_lib.CLOTH_LISTS_TRAVEL if done else 0))
                if fcol is not None:
                    _cloth_face_lists_call(t, fc, col, fcol, len(garments), bad)
            _lib.call(entry, *solver, n, *tail, *lists, _stream())
            done += n
            if done >= substeps:
                break
        if substeps > 0:
            _cloth_lists_call(t, c, col, len(garments), _lib.CLOTH_LISTS_TRAVEL)
        contact_stats = cloth_contact_stats(c["diag"], col) if stats else None
        if stats and fcol is not None:
            contact_stats = [dict(a, **b) for a, b in zip(contact_stats, cloth_face_contact_stats(fc["fdiag"]))]
    _raise_bad_face(bad.item(), "cloth_simulate")
    out = [(t["x"][a:b], t["v"][a:b]) for a, b in zip(t["v_off"][:-1], t["v_off"][1:])]
    return (out, contact_stats) if stats else out


def cloth_storage_path(garment, lds_budget=None):
    """"lds" or "global": where cloth_simulate_batch keeps the working positions of `garment` under `lds_budget`"""
    budget = _lib.CLOTH_MAX_LDS if lds_budget is None else int(lds_budget)
    return "lds" if 24 * len(garment.w) <= budget else "global"


# ------------------------------------------------------------------------------------------------ gradient pack (data-parallel training)
def grad_pack_table(rows, device):
    """the device table of gn_grad_pack.  rows: [(source pointer or None, dst_off, numel)] in the order of their workgroups; dst_off a multiple of 4
    (parallel.plan_flat).  -> (uint8 device tensor, number of workgroups)"""
    entries, blk = [], 0
    for ptr, off, numel in rows:
        if off % 4 or off < 0 or numel < 0:
            raise ValueError(f"grad_pack_table: dst_off must be a non-negative multiple of 4 and numel non-negative, got ({off}, {numel})")
        entries.append((ptr or None, int(off), int(numel), blk))
        blk += -(-int(numel) // _lib.ADAM_CHUNK)
    host = _table(_lib.PackEntry, entries)
    return _table_dev(host, device), blk


def grad_pack(table, n_entries, n_blocks, flat, world=1, flat_numel=None):
    """gn_grad_pack: every source of the device `table` (grad_pack_table) into its slice of the fp32 buffer `flat`, divided by `world` (bit copies for
    world == 1), pads and null sources as zeros, in ONE launch.  flat_numel: the floats of flat the kernel may write (default: all of it).  -> flat"""
    flat = _chk(flat, torch.float32, "flat")
    if table.dtype != torch.uint8 or not table.is_contiguous() or table.numel() < int(n_entries) * ctypes.sizeof(_lib.PackEntry):
        raise ValueError("grad_pack: table must be the contiguous uint8 tensor of grad_pack_table, n_entries entries long")
    numel = flat.numel() if flat_numel is None else int(flat_numel)
    if numel > flat.numel():
        raise ValueError(f"grad_pack: flat_numel {numel} exceeds the buffer's {flat.numel()} elements")
    _lib.call("gn_grad_pack", _p(table), int(n_entries), int(n_blocks), _p(flat), numel, int(world), _stream())
    return flat

"""What the polyphase up-conv tests share (test_upconv_reference_host.py, test_gpu_upconv_partial.py): the DEFINITION of the partial that
gn_upconv_partial (csrc/upconv.hip) computes, in fp64 on the CPU; a restatement that is wrong on purpose (the padding before the affine); the inputs
and the case table; the launch rule and the XCD remap of the entry, restated.  A plain module, imported by its siblings; it holds no test.

Nothing here goes through ops.polyphase_weights or through a pack: the definition is the literal one -- affine, nearest upsampling, a 3x3x3 convolution
with zero padding at the FINE border, then a de-interleave of the fine voxels into their eight parity classes."""
import torch
import torch.nn.functional as F

GROUPS, EPS = 8, 1e-5            # the GroupNorm of the inputs below
C0 = 16                          # full-resolution columns in front of the upsampled ones in the raw layer weight (the device pack starts at w[:, C0:])
BIG = 1                          # the sample of a batched case that is 2^10 larger than the others

# (coarse dims, C1, Cout, B): what each exercises is told in test_gpu_upconv_partial.py's docstring
CASES = (
    ((1, 1, 1), 16, 32, 1),
    ((1, 1, 1), 16, 64, 1),
    ((2, 8, 8), 32, 32, 1),
    ((1, 8, 8), 32, 64, 1),
    ((3, 9, 5), 48, 32, 3),
    ((3, 9, 5), 48, 96, 1),
    ((3, 9, 5), 16, 64, 3),
    ((3, 9, 5), 32, 192, 1),
    ((2, 3, 5), 384, 128, 1),
    ((5, 10, 17), 32, 64, 2),
    ((4, 8, 16), 16, 64, 1),
    ((16, 8, 8), 16, 32, 1),
)


def case_id(case):
    (Dc, Hc, Wc), C1, Cout, B = case
    return f"{Dc}x{Hc}x{Wc}-{C1}to{Cout}-B{B}"


# ---------------------------------------------------------------------------------------------------- the definition
def deinterleave(fine):
    """fine [B][2Dc][2Hc][2Wc][C] -> [B][Dc][Hc][Wc][8 * C], entry (4 pz + 2 py + px) * C + n of coarse voxel (i, j, k) = fine voxel
    (2i + pz, 2j + py, 2k + px): the layout of the partial buffer"""
    B, D, H, W, C = fine.shape
    return fine.reshape(B, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(B, D // 2, H // 2, W // 2, 8 * C)


def _affine_upsampled(x1, a1, d1):
    """g = a1 * x1 + d1 per sample and channel in fp64, nearest-upsampled by 2 per axis, channel-first (B, C1, 2Dc, 2Hc, 2Wc)"""
    g = x1.double() * a1.double()[:, None, None, None, :] + d1.double()[:, None, None, None, :]
    return F.interpolate(g.permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest")


def partial_reference(x1, a1, d1, w1):
    """x1 [B][Dc][Hc][Wc][C1], a1 / d1 [B][C1], w1 (Cout, C1, 3, 3, 3): the layer weight's upsampled columns -> [B][Dc][Hc][Wc][8 * Cout] in fp64.
    The zero padding comes AFTER the affine, at the fine border"""
    y = F.conv3d(_affine_upsampled(x1, a1, d1), w1.double(), None, padding=1)
    return deinterleave(y.permute(0, 2, 3, 4, 1))


def padding_before_affine(x1, a1, d1, w1):
    """WRONG on purpose: the source is padded with zeros first and the affine applied to the pad as well (the border sees d1, not 0).  Used only to prove
    that the cases can tell the two apart"""
    up = F.pad(F.interpolate(x1.double().permute(0, 4, 1, 2, 3), scale_factor=2, mode="nearest"), (1, 1, 1, 1, 1, 1))
    g = up * a1.double()[:, :, None, None, None] + d1.double()[:, :, None, None, None]
    y = F.conv3d(g, w1.double(), None, padding=0)
    return deinterleave(y.permute(0, 2, 3, 4, 1))


def class_errors(got, ref, cout):
    """largest |got - ref| of each of the 8 parity classes -> list of 8 floats"""
    diff = (got.double() - ref).abs().reshape(-1, 8, cout)
    return [float(v) for v in diff.amax(dim=(0, 2))]


# ---------------------------------------------------------------------------------------------------- inputs
def make_inputs(case, seed=0):
    """-> dict(x1 [B][Dc][Hc][Wc][C1], w (Cout, C0 + C1, 3, 3, 3) the raw layer weight, w1 = w[:, C0:], gamma, beta [C1]) on the CPU, fp32, from a seeded
    generator: the partial is O(1); exact zeros and -0.0 in x1; sample BIG of a batched case 2^10 above the others; d far from zero"""
    (Dc, Hc, Wc), C1, Cout, B = case
    g = torch.Generator().manual_seed(7919 * seed + 1000 * C1 + Cout + 100 * Dc + 10 * Hc + Wc + B)
    x1 = torch.randn(B, Dc, Hc, Wc, C1, generator=g) * 1.5 + 0.2
    x1[:, 0, 0, 0, ::4] = 0.0                      # a corner voxel (of the (1, 1, 1) volume: the only one)
    x1[:, -1, -1, -1, 1::4] = -0.0
    x1[:, Dc // 2, Hc // 2, :, 2::8] = 0.0         # a row inside
    if B > 1:
        x1[BIG] *= 1024.0                          # (a power of two: the zeros stay zeros, every other value exact)
    w = torch.randn(Cout, C0 + C1, 3, 3, 3, generator=g) / (27 * C1) ** 0.5
    gamma = torch.rand(C1, generator=g) + 0.5
    beta = torch.randn(C1, generator=g) + 1.0
    return dict(x1=x1, w=w, w1=w[:, C0:].contiguous(), gamma=gamma, beta=beta)


def affine_reference(x1, gamma, beta, groups=GROUPS, eps=EPS):
    """the GroupNorm affine of x1 [B][...][C1] from its real statistics, fp64 -> (a, d) [B][C1]: GroupNorm(x) = a x + d"""
    B, C1 = x1.shape[0], x1.shape[-1]
    xg = x1.double().reshape(B, -1, groups, C1 // groups)
    mean = xg.mean(dim=(1, 3))
    var = (xg * xg).mean(dim=(1, 3)) - mean * mean
    rstd = (var.clamp_min(0.0) + eps).rsqrt()
    a = gamma.double()[None, :] * rstd.repeat_interleave(C1 // groups, dim=1)
    d = beta.double()[None, :] - mean.repeat_interleave(C1 // groups, dim=1) * a
    return a, d


# ---------------------------------------------------------------------------------------------------- the launch rule of gn_upconv_partial, restated
def _cdiv(a, b):
    return -(-a // b)


def launch_rule(case):
    """-> (NT, TZC, ncb, nblk): the template upconv_partial_kernel<NT, *> (NT = 2 iff Cout % 64 == 0; TZC coarse z-slices per workgroup, 2 iff NT == 1),
    its column blocks per tile and gridDim.x"""
    (Dc, Hc, Wc), _, Cout, _ = case
    NT = 2 if Cout % 64 == 0 else 1
    TZC = 2 if NT == 1 else 1
    ncb = Cout // (32 * NT)
    return NT, TZC, ncb, _cdiv(Dc, TZC) * _cdiv(Hc, 8) * _cdiv(Wc, 8) * ncb


def nblk_class(nblk):
    """the four kinds of grid the XCD remap tells apart"""
    if nblk == 1:
        return "one"
    if nblk < 8:
        return "below 8"
    return "multiple of 8" if nblk % 8 == 0 else "above 8, ragged"


NBLK_CLASSES = ("one", "below 8", "multiple of 8", "above 8, ragged")


def xcd_logical(block, nblk):
    """blockIdx.x -> the (tile, column block) index the workgroup works on: every XCD (blockIdx.x % 8) walks a contiguous range"""
    xcd, jx, qx, rx = block & 7, block >> 3, nblk >> 3, nblk & 7
    return (xcd * (qx + 1) if xcd < rx else rx * (qx + 1) + (xcd - rx) * qx) + jx

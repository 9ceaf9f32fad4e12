// losses.hip -- validation losses of the two Lightning modules (networks/pointnet2_nocs.py:257-440, networks/conv_implicit_wnf.py:405-452)
//   gn_nocs_bin_metrics   binned NOCS head: cross entropy against the target bin and the mirrored target bin, arg-max coordinate error
//   gn_value_losses       decoders and the regression head: l2 / smooth_l1 / bce_logits / row-norm sums, optionally also against the x-mirrored
//                         target
//
// Per-element terms are fp32 in torch's formulas; sums are fp64.  Reduction is deterministic: every workgroup reduces its threads in a
// fixed shuffle / LDS tree and stores ONE partial with a plain store; a second launch folds each set's partials in a fixed order.  No
// atomics, so two identical calls give identical bits.
#include "common.h"

// the binning / mirroring maths below decides integers from floats: never let the compiler fuse a multiply into an add
#pragma clang fp contract(off)

#define LOSS_WG 256
#define VL_ITEMS 8   // elements per thread of gn_value_losses (a workgroup covers LOSS_WG * VL_ITEMS elements of one segment)

struct NocsSetsArg {
    const float *logits[GN_LOSS_MAX_SETS];
    const float *gt[GN_LOSS_MAX_SETS];
    int64_t n[GN_LOSS_MAX_SETS];
    int ldl[GN_LOSS_MAX_SETS];
    int blk0[GN_LOSS_MAX_SETS + 1];   // first workgroup of every set; blk0[nsets] = total
    int nsets;
};

struct SegsArg {
    const float *pred[GN_LOSS_MAX_SETS];
    const float *target[GN_LOSS_MAX_SETS];
    int64_t count[GN_LOSS_MAX_SETS];
    int kind[GN_LOSS_MAX_SETS];
    int mirror[GN_LOSS_MAX_SETS];
    int blk0[GN_LOSS_MAX_SETS + 1];
    int nsets;
};

__device__ __forceinline__ int loss_set_of(const int *blk0, int nsets, int b) {
    int s = 0;
    while (s + 1 < nsets && b >= blk0[s + 1]) ++s;
    return s;
}

// fixed-order sum of NV doubles over the workgroup (LOSS_WG threads); the result is valid in thread 0
template <int NV>
__device__ __forceinline__ void loss_block_sum(double (&v)[NV]) {
    __shared__ double part[LOSS_WG / GN_WAVE][NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
        for (int off = GN_WAVE / 2; off >= 1; off >>= 1) v[j] += __shfl_down(v[j], off);
    const int lane = threadIdx.x & (GN_WAVE - 1), w = threadIdx.x / GN_WAVE;
    if (lane == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) part[w][j] = v[j];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            double s = part[0][j];
            for (int k = 1; k < LOSS_WG / GN_WAVE; ++k) s += part[k][j];
            v[j] = s;
        }
}

// VirtualGrid.get_points_grid_idxs over the unit cube (components/gridding.py:54-61): fp32 (p + (-0)) * (bins - 1), truncation toward zero,
// clamp to [0, bins - 1].  The comparisons stand in for the clamp of the truncated integer and agree with it for every finite p.
__device__ __forceinline__ int nocs_bin_of(float p, int bins) {
    const float f = __fmul_rn(__fadd_rn(p, -0.0f), (float)(bins - 1));
    if (!(f >= 1.0f)) return 0;                    // (-1, 1) truncates to 0; below -1 clamps to 0
    if (f >= (float)(bins - 1)) return bins - 1;
    return (int)f;
}

// correctly rounded fp32 square root: the fp64 root of an fp32 value rounded once is exact (53 >= 2 * 24 + 2 bits), where the fp32 root
// on gfx950 lowers to v_sqrt_f32 (1 ulp)
__device__ __forceinline__ float loss_sqrt_rn(float x) { return (float)__dsqrt_rn((double)x); }

// components/symmetry.py: (p - 0.5) * -1 + 0.5, fp32, each step rounded
__device__ __forceinline__ float nocs_mirror(float p) { return __fadd_rn(__fmul_rn(__fsub_rn(p, 0.5f), -1.0f), 0.5f); }

// one thread per row: for each axis one pass for the first maximum and the two target logits, one pass for the sum of exp(x - max)
__global__ __launch_bounds__(LOSS_WG) void nocs_bin_metrics_kernel(NocsSetsArg a, int bins, int mirror_axis, double *__restrict__ part) {
    const int s = loss_set_of(a.blk0, a.nsets, blockIdx.x);
    const int64_t r = (int64_t)(blockIdx.x - a.blk0[s]) * LOSS_WG + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < a.n[s]) {
        const float *row = a.logits[s] + r * a.ldl[s];
        const float *g = a.gt[s] + r * 3;
        const float scale = __fdiv_rn(1.0f, __fsub_rn((float)bins, 1.0f));    // gn_nocs_head's bin -> coordinate
        float d2 = 0.f, d2m = 0.f;
        for (int ax = 0; ax < 3; ++ax) {
            const float gt = g[ax];
            const float gtm = ax == mirror_axis ? nocs_mirror(gt) : gt;
            const int t = nocs_bin_of(gt, bins);
            const int tm = ax == mirror_axis ? nocs_bin_of(gtm, bins) : t;
            float mx = row[ax];
            int arg = 0;
            for (int k = 1; k < bins; ++k) {
                const float x = row[k * 3 + ax];
                if (x > mx) { mx = x; arg = k; }
            }
            float sum = 0.f;
            for (int k = 0; k < bins; ++k) sum = __fadd_rn(sum, expf(__fsub_rn(row[k * 3 + ax], mx)));
            const float lse = logf(sum);
            // torch: -log_softmax[t] = -((x_t - max) - log(sum))
            const float ce = __fsub_rn(lse, __fsub_rn(row[t * 3 + ax], mx));
            const float cem = tm == t ? ce : __fsub_rn(lse, __fsub_rn(row[tm * 3 + ax], mx));
            v[0] += (double)ce;
            v[1] += (double)cem;
            const float pred = __fadd_rn(__fmul_rn((float)arg, scale), 0.0f);
            const float d = __fsub_rn(pred, gt), dm = __fsub_rn(pred, gtm);
            d2 = __fadd_rn(d2, __fmul_rn(d, d));
            d2m = __fadd_rn(d2m, __fmul_rn(dm, dm));
        }
        v[2] = (double)loss_sqrt_rn(d2);
        v[3] = (double)loss_sqrt_rn(d2m);
    }
    loss_block_sum<4>(v);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[(int64_t)blockIdx.x * 4 + j] = v[j];
}

struct FoldArg {
    int blk0[GN_LOSS_MAX_SETS + 1];
};

// all sets in one fold launch: workgroup s folds set s
template <int NV>
__global__ __launch_bounds__(LOSS_WG) void loss_fold_sets_kernel(const double *__restrict__ part, FoldArg f, double *__restrict__ out) {
    const int s = blockIdx.x;
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    for (int b = f.blk0[s] + (int)threadIdx.x; b < f.blk0[s + 1]; b += LOSS_WG)
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += part[(int64_t)b * NV + j];
    loss_block_sum<NV>(v);
    if (threadIdx.x == 0)
#pragma unroll
        for (int j = 0; j < NV; ++j) out[(int64_t)s * NV + j] = v[j];
}

__device__ __forceinline__ float value_loss_term(float p, float t, int kind) {
    if (kind == GN_LOSS_BCE_LOGITS) {
        // max(x, 0) - x * y + log1p(exp(-|x|))
        return __fadd_rn(__fsub_rn(fmaxf(p, 0.0f), __fmul_rn(p, t)), log1pf(expf(-fabsf(p))));
    }
    const float d = __fsub_rn(p, t);
    if (kind == GN_LOSS_SMOOTH_L1) {
        const float z = fabsf(d);                  // beta = 1: z < 1 ? 0.5 * z * z : z - 0.5
        return z < 1.0f ? __fmul_rn(__fmul_rn(0.5f, z), z) : __fsub_rn(z, 0.5f);
    }
    return __fmul_rn(d, d);
}

__global__ __launch_bounds__(LOSS_WG) void value_losses_kernel(SegsArg a, double *__restrict__ part) {
    const int s = loss_set_of(a.blk0, a.nsets, blockIdx.x);
    const int64_t e0 = (int64_t)(blockIdx.x - a.blk0[s]) * (LOSS_WG * VL_ITEMS) + threadIdx.x;
    const int64_t n = a.count[s];
    const float *pred = a.pred[s], *tgt = a.target[s];
    const int kind = a.kind[s], mirror = a.mirror[s];
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < VL_ITEMS; ++i) {
        const int64_t e = e0 + (int64_t)i * LOSS_WG;
        if (e < n && kind == GN_LOSS_ROW_NORM) {
            // element e is the row pred[3e .. 3e+2]: fp32 sqrt((dx*dx + dy*dy) + dz*dz), the x target mirrored for the second sum
            float d2 = 0.f, d2m = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float p = pred[e * 3 + c], t = tgt[e * 3 + c];
                const float d = __fsub_rn(p, t), dm = __fsub_rn(p, c == 0 ? nocs_mirror(t) : t);
                d2 = __fadd_rn(d2, __fmul_rn(d, d));
                d2m = __fadd_rn(d2m, __fmul_rn(dm, dm));
            }
            v[0] += (double)loss_sqrt_rn(d2);
            if (mirror) v[1] += (double)loss_sqrt_rn(d2m);
        } else if (e < n) {
            const float p = pred[e], t = tgt[e];
            v[0] += (double)value_loss_term(p, t, kind);
            if (mirror) {
                // components/loss.py MirrorMSELoss: (t - [0.5, 0, 0]) * [-1, 1, 1] + [0.5, 0, 0] on (M, 3) rows
                const float tm = (e % 3) == 0 ? nocs_mirror(t) : t;
                v[1] += (double)value_loss_term(p, tm, kind);
            }
        }
    }
    loss_block_sum<2>(v);
    if (threadIdx.x == 0) {
        part[(int64_t)blockIdx.x * 2] = v[0];
        part[(int64_t)blockIdx.x * 2 + 1] = v[1];
    }
}

// ------------------------------------------------------------------------------------------------ entry points
static int nocs_blocks(const GnNocsBinSet *sets, int nsets, int *blk0) {
    int64_t tot = 0;
    for (int s = 0; s < nsets; ++s) {
        blk0[s] = (int)tot;
        tot += gn_cdiv(sets[s].n, LOSS_WG);
    }
    blk0[nsets] = (int)tot;
    return (int)tot;
}

static int seg_blocks(const GnLossSegment *segs, int nsegs, int *blk0) {
    int64_t tot = 0;
    for (int s = 0; s < nsegs; ++s) {
        blk0[s] = (int)tot;
        tot += gn_cdiv(segs[s].count, LOSS_WG * VL_ITEMS);
    }
    blk0[nsegs] = (int)tot;
    return (int)tot;
}

extern "C" size_t gn_nocs_bin_metrics_workspace_bytes(const GnNocsBinSet *sets_host, int nsets) {
    if (sets_host == nullptr || nsets < 1 || nsets > GN_LOSS_MAX_SETS) return 0;
    int64_t tot = 0;
    for (int s = 0; s < nsets; ++s) tot += sets_host[s].n > 0 ? gn_cdiv(sets_host[s].n, LOSS_WG) : 0;
    return (size_t)tot * 4 * sizeof(double);
}

extern "C" int gn_nocs_bin_metrics(const GnNocsBinSet *sets_host, int nsets, int bins, int mirror_axis, void *ws, size_t ws_bytes, double *out,
                                   void *stream) {
    GN_REQUIRE(sets_host != nullptr && nsets >= 1 && nsets <= GN_LOSS_MAX_SETS, "gn_nocs_bin_metrics: 1..%d row sets", GN_LOSS_MAX_SETS);
    GN_REQUIRE(bins >= 1, "gn_nocs_bin_metrics: bins must be >= 1");
    GN_REQUIRE(mirror_axis >= -1 && mirror_axis <= 2, "gn_nocs_bin_metrics: mirror_axis must be -1 (none), 0, 1 or 2");
    GN_REQUIRE(out != nullptr, "gn_nocs_bin_metrics: out is required");
    int64_t tot = 0;
    for (int s = 0; s < nsets; ++s) {
        const GnNocsBinSet &t = sets_host[s];
        GN_REQUIRE(t.n >= 1 && t.logits != nullptr && t.gt != nullptr, "gn_nocs_bin_metrics: set %d: N >= 1 rows and both pointers", s);
        GN_REQUIRE(t.ldl >= bins * 3, "gn_nocs_bin_metrics: set %d: ldl (%d) < bins * 3 (%d)", s, t.ldl, bins * 3);
        GN_REQUIRE(t.n <= ((int64_t)1 << 40) / t.ldl, "gn_nocs_bin_metrics: set %d: too many rows", s);
        tot += gn_cdiv(t.n, LOSS_WG);
    }
    GN_REQUIRE(tot <= 0x7fffffff, "gn_nocs_bin_metrics: too many rows");
    GN_REQUIRE(ws != nullptr && ws_bytes >= gn_nocs_bin_metrics_workspace_bytes(sets_host, nsets),
               "gn_nocs_bin_metrics: ws needs gn_nocs_bin_metrics_workspace_bytes() bytes");
    NocsSetsArg a = {};
    a.nsets = nsets;
    for (int s = 0; s < nsets; ++s) {
        a.logits[s] = sets_host[s].logits;
        a.gt[s] = sets_host[s].gt;
        a.n[s] = sets_host[s].n;
        a.ldl[s] = sets_host[s].ldl;
    }
    const int nblk = nocs_blocks(sets_host, nsets, a.blk0);
    FoldArg f = {};
    for (int s = 0; s <= nsets; ++s) f.blk0[s] = a.blk0[s];
    hipStream_t st = gn_stream(stream);
    double *part = reinterpret_cast<double *>(ws);
    hipLaunchKernelGGL(nocs_bin_metrics_kernel, dim3((unsigned)nblk), dim3(LOSS_WG), 0, st, a, bins, mirror_axis, part);
    hipLaunchKernelGGL((loss_fold_sets_kernel<4>), dim3((unsigned)nsets), dim3(LOSS_WG), 0, st, (const double *)part, f, out);
    GN_LAUNCH_CHECK("gn_nocs_bin_metrics");
    return GN_OK;
}

extern "C" size_t gn_value_losses_workspace_bytes(const GnLossSegment *segs_host, int nsegs) {
    if (segs_host == nullptr || nsegs < 1 || nsegs > GN_LOSS_MAX_SETS) return 0;
    int64_t tot = 0;
    for (int s = 0; s < nsegs; ++s) tot += segs_host[s].count > 0 ? gn_cdiv(segs_host[s].count, LOSS_WG * VL_ITEMS) : 0;
    return (size_t)tot * 2 * sizeof(double);
}

extern "C" int gn_value_losses(const GnLossSegment *segs_host, int nsegs, void *ws, size_t ws_bytes, double *out, void *stream) {
    GN_REQUIRE(segs_host != nullptr && nsegs >= 1 && nsegs <= GN_LOSS_MAX_SETS, "gn_value_losses: 1..%d segments", GN_LOSS_MAX_SETS);
    GN_REQUIRE(out != nullptr, "gn_value_losses: out is required");
    int64_t tot = 0;
    for (int s = 0; s < nsegs; ++s) {
        const GnLossSegment &g = segs_host[s];
        GN_REQUIRE(g.count >= 0 && (g.count == 0 || (g.pred != nullptr && g.target != nullptr)), "gn_value_losses: segment %d: bad count / pointers", s);
        GN_REQUIRE(g.kind == GN_LOSS_L2 || g.kind == GN_LOSS_SMOOTH_L1 || g.kind == GN_LOSS_BCE_LOGITS || g.kind == GN_LOSS_ROW_NORM,
                   "gn_value_losses: segment %d: unknown kind %d", s, g.kind);
        GN_REQUIRE(!g.mirror || g.kind == GN_LOSS_ROW_NORM || g.count % 3 == 0, "gn_value_losses: segment %d: a mirrored segment holds (M, 3) rows", s);
        tot += gn_cdiv(g.count, LOSS_WG * VL_ITEMS);
    }
    GN_REQUIRE(tot <= 0x7fffffff, "gn_value_losses: too many elements");
    GN_REQUIRE(tot == 0 || (ws != nullptr && ws_bytes >= gn_value_losses_workspace_bytes(segs_host, nsegs)),
               "gn_value_losses: ws needs gn_value_losses_workspace_bytes() bytes");
    SegsArg a = {};
    a.nsets = nsegs;
    for (int s = 0; s < nsegs; ++s) {
        a.pred[s] = segs_host[s].pred;
        a.target[s] = segs_host[s].target;
        a.count[s] = segs_host[s].count;
        a.kind[s] = segs_host[s].kind;
        a.mirror[s] = segs_host[s].mirror;
    }
    const int nblk = seg_blocks(segs_host, nsegs, a.blk0);
    FoldArg f = {};
    for (int s = 0; s <= nsegs; ++s) f.blk0[s] = a.blk0[s];
    hipStream_t st = gn_stream(stream);
    double *part = reinterpret_cast<double *>(ws);
    if (nblk > 0) hipLaunchKernelGGL(value_losses_kernel, dim3((unsigned)nblk), dim3(LOSS_WG), 0, st, a, part);
    hipLaunchKernelGGL((loss_fold_sets_kernel<2>), dim3((unsigned)nsegs), dim3(LOSS_WG), 0, st, (const double *)part, f, out);
    GN_LAUNCH_CHECK("gn_value_losses");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ loss gradients
// The backward of the two launches above, for a training step (garmentnets_amd/autograd.py nocs_bin_loss / value_loss).  Each reads the fp64 sums the
// forward left on the device and takes the mirror decision there: every thread evaluates the same fp64 comparison, so no host branch sits between the
// forward and the backward.  Every output element is written exactly once with a plain store: identical calls give identical bits.
struct NocsGradArg {
    const float *logits[GN_LOSS_MAX_SETS];
    const float *gt[GN_LOSS_MAX_SETS];
    float *grad[GN_LOSS_MAX_SETS];
    int64_t n[GN_LOSS_MAX_SETS];
    double coef[GN_LOSS_MAX_SETS];     // weight_s / (3 n_s)
    double weight[GN_LOSS_MAX_SETS];
    int ldl[GN_LOSS_MAX_SETS];
    int ldg[GN_LOSS_MAX_SETS];
    int ncols[GN_LOSS_MAX_SETS];
    int blk0[GN_LOSS_MAX_SETS + 1];
    int nsets;
};

// validation_metrics' rule: loss_c = w_0 * (sum_0c / (3 n_0)) + w_1 * (sum_1c / (3 n_1)) + ... in fp64, left to right; the WHOLE batch takes the mirrored
// targets iff the mirrored loss is strictly smaller (plain when equal)
__device__ __forceinline__ bool nocs_take_mirror(const NocsGradArg &a, const double *__restrict__ sums) {
    double plain = 0.0, mirrored = 0.0;
    for (int s = 0; s < a.nsets; ++s) {
        const double d = (double)(a.n[s] * 3);
        const double tp = a.weight[s] * (sums[s * 4] / d), tm = a.weight[s] * (sums[s * 4 + 1] / d);
        plain = s == 0 ? tp : plain + tp;
        mirrored = s == 0 ? tm : mirrored + tm;
    }
    return mirrored < plain;
}

// one thread per (row, axis): the forward's max-subtracted softmax (the sum of the fp32 exponentials kept in fp64), minus the one-hot of the target bin
__global__ __launch_bounds__(LOSS_WG) void nocs_bin_loss_bwd_kernel(NocsGradArg a, int bins, int mirror_axis, const double *__restrict__ sums,
                                                                    const float *__restrict__ upstream) {
    const int s = loss_set_of(a.blk0, a.nsets, blockIdx.x);
    const int64_t i = (int64_t)(blockIdx.x - a.blk0[s]) * LOSS_WG + threadIdx.x;
    if (i >= a.n[s] * 3) return;
    const int64_t r = i / 3;
    const int ax = (int)(i - r * 3);
    const float *row = a.logits[s] + r * a.ldl[s];
    float *g = a.grad[s] + r * a.ldg[s];
    const bool mir = mirror_axis >= 0 && nocs_take_mirror(a, sums);
    float gt = a.gt[s][r * 3 + ax];
    if (mir && ax == mirror_axis) gt = nocs_mirror(gt);
    const int t = nocs_bin_of(gt, bins);
    float mx = row[ax];
    for (int k = 1; k < bins; ++k) {
        const float x = row[k * 3 + ax];
        if (x > mx) mx = x;
    }
    double sum = 0.0;
    for (int k = 0; k < bins; ++k) sum += (double)expf(__fsub_rn(row[k * 3 + ax], mx));
    const double scale = a.coef[s] * (double)upstream[0];
    for (int k = 0; k < bins; ++k) {
        const double p = (double)expf(__fsub_rn(row[k * 3 + ax], mx)) / sum;
        g[k * 3 + ax] = (float)((p - (k == t ? 1.0 : 0.0)) * scale);
    }
    if (ax == 0)
        for (int c = bins * 3; c < a.ncols[s]; ++c) g[c] = 0.0f;      // the pad columns of a padded row
}

struct SegsGradArg {
    const float *pred[GN_LOSS_MAX_SETS];
    const float *target[GN_LOSS_MAX_SETS];
    float *grad[GN_LOSS_MAX_SETS];
    int64_t count[GN_LOSS_MAX_SETS];
    double coef[GN_LOSS_MAX_SETS];
    int kind[GN_LOSS_MAX_SETS];
    int mirror[GN_LOSS_MAX_SETS];
    int blk0[GN_LOSS_MAX_SETS + 1];
    int nsets;
};

// d value_loss_term / d p in fp64 of the fp32 operands.  smooth_l1 (beta 1) takes torch's choice: the quadratic branch's d for -1 <= d <= 1 -- so
// exactly -1 / +1 at |d| == 1, where the two branches agree, and 0 at d == 0 -- and the sign beyond.  bce_logits: sigmoid(p) - t.
__device__ __forceinline__ double value_loss_dterm(float p, float t, int kind) {
    if (kind == GN_LOSS_BCE_LOGITS) {
        const double x = (double)p;
        const double sg = x >= 0.0 ? 1.0 / (1.0 + exp(-x)) : exp(x) / (1.0 + exp(x));
        return sg - (double)t;
    }
    const double d = (double)p - (double)t;
    if (kind == GN_LOSS_SMOOTH_L1) return d < -1.0 ? -1.0 : d > 1.0 ? 1.0 : d;
    return 2.0 * d;
}

__global__ __launch_bounds__(LOSS_WG) void value_losses_bwd_kernel(SegsGradArg a, const double *__restrict__ sums, const float *__restrict__ upstream) {
    const int s = loss_set_of(a.blk0, a.nsets, blockIdx.x);
    const int64_t e0 = (int64_t)(blockIdx.x - a.blk0[s]) * (LOSS_WG * VL_ITEMS) + threadIdx.x;
    const int64_t n = a.count[s];
    const float *pred = a.pred[s], *tgt = a.target[s];
    float *g = a.grad[s];
    const int kind = a.kind[s];
    // MirrorMSELoss, per segment: the mirrored target iff its sum is strictly smaller
    const bool mir = a.mirror[s] && sums[s * 2 + 1] < sums[s * 2];
    const double scale = a.coef[s] * (double)upstream[0];
#pragma unroll
    for (int i = 0; i < VL_ITEMS; ++i) {
        const int64_t e = e0 + (int64_t)i * LOSS_WG;
        if (e < n) {
            float t = tgt[e];
            if (mir && (e % 3) == 0) t = nocs_mirror(t);
            g[e] = (float)(value_loss_dterm(pred[e], t, kind) * scale);
        }
    }
}

extern "C" int gn_nocs_bin_loss_bwd(const GnNocsBinGradSet *sets_host, int nsets, int bins, int mirror_axis, const double *sums,
                                    const double *weights_host, const float *upstream, void *stream) {
    GN_REQUIRE(sets_host != nullptr && nsets >= 1 && nsets <= GN_LOSS_MAX_SETS, "gn_nocs_bin_loss_bwd: 1..%d row sets", GN_LOSS_MAX_SETS);
    GN_REQUIRE(bins >= 1, "gn_nocs_bin_loss_bwd: bins must be >= 1");
    GN_REQUIRE(mirror_axis >= -1 && mirror_axis <= 2, "gn_nocs_bin_loss_bwd: mirror_axis must be -1 (none), 0, 1 or 2");
    GN_REQUIRE(sums != nullptr && weights_host != nullptr && upstream != nullptr, "gn_nocs_bin_loss_bwd: sums, weights and upstream are required");
    NocsGradArg a = {};
    a.nsets = nsets;
    int64_t tot = 0;
    for (int s = 0; s < nsets; ++s) {
        const GnNocsBinGradSet &t = sets_host[s];
        GN_REQUIRE(t.n >= 1 && t.logits != nullptr && t.gt != nullptr && t.grad != nullptr, "gn_nocs_bin_loss_bwd: set %d: N >= 1 rows and three pointers", s);
        GN_REQUIRE(t.ncols >= bins * 3 && t.ldl >= t.ncols && t.ldg >= t.ncols,
                   "gn_nocs_bin_loss_bwd: set %d: need bins * 3 (%d) <= ncols (%d) <= ldl (%d), ldg (%d)", s, bins * 3, t.ncols, t.ldl, t.ldg);
        GN_REQUIRE(t.n <= ((int64_t)1 << 40) / t.ldl && t.n <= ((int64_t)1 << 40) / t.ldg, "gn_nocs_bin_loss_bwd: set %d: too many rows", s);
        a.logits[s] = t.logits;
        a.gt[s] = t.gt;
        a.grad[s] = t.grad;
        a.n[s] = t.n;
        a.ldl[s] = t.ldl;
        a.ldg[s] = t.ldg;
        a.ncols[s] = t.ncols;
        a.weight[s] = weights_host[s];
        a.coef[s] = weights_host[s] / (double)(t.n * 3);
        a.blk0[s] = (int)tot;
        tot += gn_cdiv(t.n * 3, LOSS_WG);
        GN_REQUIRE(tot <= 0x7fffffff, "gn_nocs_bin_loss_bwd: too many rows");
    }
    a.blk0[nsets] = (int)tot;
    hipLaunchKernelGGL(nocs_bin_loss_bwd_kernel, dim3((unsigned)tot), dim3(LOSS_WG), 0, gn_stream(stream), a, bins, mirror_axis, sums, upstream);
    GN_LAUNCH_CHECK("gn_nocs_bin_loss_bwd");
    return GN_OK;
}

extern "C" int gn_value_losses_bwd(const GnLossGradSegment *segs_host, int nsegs, const double *sums, const float *upstream, void *stream) {
    GN_REQUIRE(segs_host != nullptr && nsegs >= 1 && nsegs <= GN_LOSS_MAX_SETS, "gn_value_losses_bwd: 1..%d segments", GN_LOSS_MAX_SETS);
    GN_REQUIRE(sums != nullptr && upstream != nullptr, "gn_value_losses_bwd: sums and upstream are required");
    SegsGradArg a = {};
    a.nsets = nsegs;
    int64_t tot = 0;
    for (int s = 0; s < nsegs; ++s) {
        const GnLossGradSegment &g = segs_host[s];
        GN_REQUIRE(g.count >= 0 && (g.count == 0 || (g.pred != nullptr && g.target != nullptr && g.grad != nullptr)),
                   "gn_value_losses_bwd: segment %d: bad count / pointers", s);
        GN_REQUIRE(g.kind != GN_LOSS_ROW_NORM, "gn_value_losses_bwd: segment %d: row_norm is a metric, not a loss: it has no gradient", s);
        GN_REQUIRE(g.kind == GN_LOSS_L2 || g.kind == GN_LOSS_SMOOTH_L1 || g.kind == GN_LOSS_BCE_LOGITS, "gn_value_losses_bwd: segment %d: unknown kind %d", s,
                   g.kind);
        GN_REQUIRE(!g.mirror || g.count % 3 == 0, "gn_value_losses_bwd: segment %d: a mirrored segment holds (M, 3) rows", s);
        a.pred[s] = g.pred;
        a.target[s] = g.target;
        a.grad[s] = g.grad;
        a.count[s] = g.count;
        a.coef[s] = g.coef;
        a.kind[s] = g.kind;
        a.mirror[s] = g.mirror;
        a.blk0[s] = (int)tot;
        tot += gn_cdiv(g.count, LOSS_WG * VL_ITEMS);
        GN_REQUIRE(tot <= 0x7fffffff, "gn_value_losses_bwd: too many elements");
    }
    a.blk0[nsegs] = (int)tot;
    if (tot > 0) hipLaunchKernelGGL(value_losses_bwd_kernel, dim3((unsigned)tot), dim3(LOSS_WG), 0, gn_stream(stream), a, sums, upstream);
    GN_LAUNCH_CHECK("gn_value_losses_bwd");
    return GN_OK;
}

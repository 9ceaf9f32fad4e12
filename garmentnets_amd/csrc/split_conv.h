// split_conv.h -- definitions shared by the split-operand conv kernels (unet_split.hip: direct 27-tap forms; unet_wino.hip: the
// Winograd F(2,3)-along-x form of the 128-wide kernel): launch arguments, work-item order, border classes, halo layout (plane split and MFMA wrapper: device_prims.h).
#pragma once
#include "common.h"

#define SP_KS 16

// border class of coordinate z on an axis of length D for reach r (see SplitArgs::kreach)
__device__ __forceinline__ int sp_axis_class(int z, int D, int r) { return z < r ? z : (z >= D - r ? 2 * r - (D - 1 - z) : r); }
// border mask of coordinate g on an axis of length n for the 3x3x3 taps (see SplitArgs::kbias)
__device__ __forceinline__ int sp_axis_mask(int g, int n) { return (g > 0 ? 1 : 0) | (g < n - 1 ? 2 : 0); }

struct SplitArgs {
    const float *src0;
    const float *src1;
    const float *a;
    const float *d;
    const uint4 *wp;   // [slice][tap][Cout/32][P][lane 64] x 16 B (8 bf16: channels 8h..8h+7 of cout 32*blk + r, lane = 32h + r), + eight zero pad steps
    float *out;
    double *osum;
    double *osq;
    int C0, C1, B, D, H, W, Cout, relu;
    int tiles_y, tiles_x;
    const float *out_scale;   // [Cout] exact powers of two undoing the pack's per-output-channel weight scales (1 for the bf16 modes)
    const float *act_inv;     // NULL or [B]: exact power of two undoing the sample's activation scale (gn_groupnorm_affine)
    // occupancy-aware launch (the layers behind a scattered volume): only the tiles listed in active_list -- entries b * tiles_per_sample + tile at
    // the kernel's tile granularity, ascending, *active_count of them (device values: occ_compact_kernel) -- are visited by this kernel; the grid is the
    // dense launch's, workgroups past the list's end return at once.  Every other tile holds nothing but border-class constants and is written by
    // conv_fill_inactive_kernel (kconst[b][class][Cout], class = (cz * n + cy) * n + cx with n = 2 kreach + 1, c = z < r ? z : (z >= D - r ? 2r - (D-1-z) : r)).
    const int *active_list;
    const int *active_count;
    const float *kconst;
    // polyphase form of a layer whose second source is nearest-upsampled (the decoders' first convolutions): the upsampled part is a
    // 2x2x2-tap convolution per output parity class on the COARSE volume (8/27 of the MACs), computed by gn_upconv_partial (upconv.hip);
    // the launch over the full-resolution source then adds partial[b][z>>1][y>>1][x>>1][((z&1)*4 + (y&1)*2 + (x&1)) * Cout + n] before
    // the ReLU.
    const float *partial;
    // affine-in-weights form (gn_conv_affine_pack, conv_prep.hip): the pack holds one weight set PER SAMPLE (wp_bstride bytes apart; 0 = one
    // set for the batch), out_scale is [B][Cout] (osc_bstride = Cout; 0 = [Cout]) and the GroupNorm shift arrives as the per-(sample, border
    // class, output channel) constant kbias[B][64][Cout] added before the ReLU (class = (mz * 4 + my) * 4 + mx, m = (has a previous voxel
    // on the axis) | (has a next one) << 1; 63 = interior).  The operand is then (x - c) s: exactly zero wherever the layer's input is at rest.
    const float *kbias;
    int64_t wp_bstride;
    int osc_bstride;
    int kreach;               // 1: the layer fed by the scattered volume (27 classes); 2: the layer behind it (125 classes: distance 0 / 1 from
                              // a face or further, per axis); class index per axis c = z < r ? z : (z >= D - r ? 2r - (D-1-z) : r), kconst
                              // [B][(2r+1)^3][Cout] ordered (cz * n + cy) * n + cx
    int chain;                // conv3d_split_wino_kernel: tiles per workgroup (set by gn_launch_conv3d_wino)
};

// Work item of this workgroup: sample b, tile (index inside the sample at the kernel's tile granularity), column block cb.
// XCD-aware order (workgroup i runs on XCD i % 8, each XCD has its own L2): every XCD walks a CONTIGUOUS range of (tile, column block) pairs,
// column blocks of one tile adjacent, tiles in z-fastest order -> the halo overlap of neighbouring tiles and the other column blocks' re-read of
// the same input hit that XCD's L2.  Bijective for any size.  Dense launch: per sample (blockIdx.y) over gridDim.x items.  Compacted launch
// (active_list): over the *active_count * ncb items of the whole batch, linear workgroup id across the grid; -> false: nothing to do.
__device__ __forceinline__ bool sp_work_item(const SplitArgs &p, int ncb, int tiles_per_sample, int &b, int &tile, int &cb) {
    unsigned nblk = gridDim.x, lin = blockIdx.x;
    if (p.active_list) {
        nblk = (unsigned)(*p.active_count) * (unsigned)ncb;
        lin = blockIdx.y * gridDim.x + blockIdx.x;
        if (lin >= nblk) return false;
    }
    const unsigned xcd = lin & 7u, jx = lin >> 3, qx = nblk >> 3, rx = nblk & 7u;
    const unsigned logical = (xcd < rx ? xcd * (qx + 1) : rx * (qx + 1) + (xcd - rx) * qx) + jx;
    const unsigned t = logical / (unsigned)ncb;
    cb = (int)(logical % (unsigned)ncb);
    if (p.active_list) {
        const int item = p.active_list[t];
        b = item / tiles_per_sample;
        tile = item - b * tiles_per_sample;
    } else {
        b = blockIdx.y;
        tile = (int)t;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ tile decode
// Tile index inside the sample -> origin of the tile, TZ x 8 x 8 voxels.  z-fastest order: the z halo is the fattest (2 of TZ + 2 slices), so tiles
// adjacent in z run back to back.  tiles_z: the caller's (the Winograd kernels take whole tiles only: D / TZ).
__device__ __forceinline__ void sp_tile_origin(const SplitArgs &p, int tile, int tiles_z, int TZ, int &z0, int &y0, int &x0) {
    const int tz = tile % tiles_z; tile /= tiles_z;
    const int tx = tile % p.tiles_x; tile /= p.tiles_x;
    const int ty = tile;
    z0 = tz * TZ; y0 = ty * GN_CONV_TY; x0 = tx * GN_CONV_TX;
}
// the tile lies inside the volume / no voxel of it lies on a face of the volume (both workgroup-uniform)
__device__ __forceinline__ bool sp_tile_full(const SplitArgs &p, int z0, int y0, int x0, int TZ, int TY, int TX) {
    return z0 + TZ <= p.D && y0 + TY <= p.H && x0 + TX <= p.W;
}
__device__ __forceinline__ bool sp_tile_interior(const SplitArgs &p, int z0, int y0, int x0, int TZ, int TY, int TX) {
    return z0 > 0 && z0 + TZ < p.D && y0 > 0 && y0 + TY < p.H && x0 > 0 && x0 + TX < p.W;
}

// ------------------------------------------------------------------------------------------------ the epilogue of the direct kernels
// ONE contract for conv3d_split_kernel, conv3d_split_strip_kernel, conv3d_split_wide_kernel (unet_split.hip).  Per output value: accumulator * scale (+ border-class bias) (+ polyphase partial) (ReLU), in this order, each step
// rounded to fp32; channel statistics of the stored values in fp64.
// kb / pb: NULL when the layer has no bias table / no partial; kv(), pv(): the value's bias / partial, evaluated only behind that test (in the generic
// path they are loads behind 64-bit index arithmetic).  Callables and pointers ON PURPOSE: with the two terms passed by value, or their presence as
// bools formed at the call, every kernel's epilogue was scheduled differently and the 64-wide instances' main loops with it.
template <class KV, class PV>
__device__ __forceinline__ float sp_out_value(float acc, float osc, const float *kb, KV kv, const float *pb, PV pv, int relu) {
    float v = __fmul_rn(acc, osc);
    if (kb) v = __fadd_rn(v, kv());
    if (pb) v = __fadd_rn(v, pv());
    if (relu) v = gn_relu(v);
    return v;
}
// output scale of channel n of sample b: the pack's weight scale times the sample's activation scale undone (exact powers of two)
__device__ __forceinline__ float sp_out_scale(const SplitArgs &p, int b, int n) {
    const float osn = p.out_scale[(int64_t)b * p.osc_bstride + n];
    return p.act_inv ? __fmul_rn(osn, p.act_inv[b]) : osn;
}
// NULL or channel n's column of sample b's kbias table (class stride Cout)
__device__ __forceinline__ const float *sp_kbias_col(const SplitArgs &p, int b, int n) { return p.kbias ? p.kbias + (int64_t)b * 64 * p.Cout + n : nullptr; }
// kbias class of voxel (gz, gy, gx)
__device__ __forceinline__ int sp_kbias_class(const SplitArgs &p, int gz, int gy, int gx) {
    return (sp_axis_mask(gz, p.D) * 4 + sp_axis_mask(gy, p.H)) * 4 + sp_axis_mask(gx, p.W);
}

// The generic (ragged-tile) store of ONE value: bounds, a 64-bit output address, the class lookup and the five-factor partial index per value.
__device__ __forceinline__ void sp_store_ragged(const SplitArgs &p, int b, int gz, int gy, int gx, int n, float acc, float osc, const float *kb, double &ssum,
                                                double &ssq) {
    if (gz < p.D && gy < p.H && gx < p.W) {
        const float v = sp_out_value(
            acc, osc, kb, [&] { return kb[(int64_t)sp_kbias_class(p, gz, gy, gx) * p.Cout]; }, p.partial,
            [&] { return p.partial[((((int64_t)b * (p.D >> 1) + (gz >> 1)) * (p.H >> 1) + (gy >> 1)) * (p.W >> 1) + (gx >> 1)) * (8 * p.Cout) + (((gz & 1) * 4 + (gy & 1) * 2 + (gx & 1)) * p.Cout + n)]; },
            p.relu);
        p.out[((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.Cout + n] = v;
        ssum += (double)v;
        ssq += (double)v * (double)v;
    }
}

// Epilogue of one 32 x 32 D fragment when the tile lies inside the volume and is active: lane (h, r) holds channel n and the 16 voxels
// (y = j, x = 4 h + k), q = 4 j + k, of one y half.  `ob` / `pb` point at (j, k) = (0, 0) of this lane; every other (j, k) is a
// workgroup-uniform element offset from there (the generic path above spends ~40 instructions per value, five of them quarter-rate
// integer multiplies, on 64-bit addresses and bounds: 9 % of the 128 -> 128 layer, 25 % of a 32 -> 32 one).  Same arithmetic, same
// order as the generic path, channel statistics accumulated q = 0 .. 15.  kb: sp_kbias_col; interior tiles (workgroup-uniform) add the one
// class-63 constant, tiles on a face of the volume look the class of each voxel up (gz: the fragment's plane; gy, gx: its first row / column,
// both even: the parity of voxel q is that of (j, k)).
// The x-strip kernel's fragment is the TRANSPOSE of this one (q walks (z, y) at one x) and keeps its own copy of this body around
// sp_out_value: with the two axes and their strides as compile-time traits of this function the strip kernel's main loop came out with
// another block order and 94 more lines of device code (profiles/conv_epilogue_isa_diff.txt), and the traits then served that one caller.
__device__ __forceinline__ void sp_store_frag_full(const SplitArgs &p, const f32x16 &val, float osc, float *ob, const float *pb, double &ssum, double &ssq,
                                                   const float *kb, bool interior, int gz, int gy, int gx) {
    const int64_t rs = (int64_t)p.W * p.Cout;
    float pv[16];
    float kv[16];
    if (kb) {
        if (interior) {
            const float k63 = kb[63 * (int64_t)p.Cout];
#pragma unroll
            for (int q = 0; q < 16; ++q) kv[q] = k63;
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) kv[q] = kb[(int64_t)sp_kbias_class(p, gz, gy + (q >> 2), gx + (q & 3)) * p.Cout];
        }
    }
    if (pb) {
        const int64_t prs = (int64_t)(p.W >> 1) * 8 * p.Cout;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int j = q >> 2, k = q & 3;
            pv[q] = pb[(j >> 1) * prs + (int64_t)((k >> 1) * 8 + (j & 1) * 2 + (k & 1)) * p.Cout];
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int j = q >> 2, k = q & 3;
        const float v = sp_out_value(val[q], osc, kb, [&] { return kv[q]; }, pb, [&] { return pv[q]; }, p.relu);
        ob[j * rs + (int64_t)k * p.Cout] = v;
        ssum += (double)v;
        ssq += (double)v * (double)v;
    }
}
// ob / pb of the call above: the output element of channel n at voxel (gz, gy, gx) of sample b / NULL or its entry of the polyphase partial
__device__ __forceinline__ float *sp_out_at(const SplitArgs &p, int b, int gz, int gy, int gx, int n) {
    return p.out + ((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.Cout + n;
}
__device__ __forceinline__ const float *sp_partial_at(const SplitArgs &p, int b, int gz, int gy, int gx, int n) {
    return p.partial ? p.partial + ((((int64_t)b * (p.D >> 1) + (gz >> 1)) * (p.H >> 1) + (gy >> 1)) * (p.W >> 1) + (gx >> 1)) * (8 * p.Cout) + (((gz & 1) * 4 + (gy & 1) * 2 + (gx & 1)) * p.Cout + n) : nullptr;
}

// Channel statistics of a 4-wave workgroup over NT * 32 channels from column COL0 of sample B (wave w: one row of each channel, lane (h, r) holds channel
// u * 32 + r in SSUM[u] / SSQ[u]): fold the lane halves, RED[sum | sq][wave][NT * 32] through LDS (8 * NT * 32 doubles), then one fp64 atomic pair per
// channel; the four waves' rows are added in the order 0 + 1 + 2 + 3 (the per-tile partials are the same in dense and occupancy-aware launches).  Uses
// the caller's tid, h, r.  A macro ON PURPOSE (as GN_WAVE_ARGMIN, device_prims.h): as an inlined function -- array references or pointers, the output
// address formed inside or outside -- the same text changed the block placement and the scratch use of conv3d_split_kernel<2, 3, false>'s MAIN LOOP.
// conv3d_split_wide_kernel keeps its own [cg][zs][64] form of this: with either form of the shared text its main loop was allocated differently
// (226 instead of 228 VGPRs, another schedule), and that kernel is 58 % of the UNet's FLOPs (profiles/conv_epilogue_isa_diff.txt).
#define SP_REDUCE_STATS(NT_, P, B, COL0, SSUM, SSQ, RED, WAVE)                                                                 \
    do {                                                                                                                       \
        constexpr int ct_ = (NT_) * 32;                                                                                        \
        double *const red_ = (RED);                                                                                            \
        _Pragma("unroll") for (int u = 0; u < (NT_); ++u) {                                                                    \
            const double s2 = SSUM[u] + __shfl_xor(SSUM[u], 32), q2 = SSQ[u] + __shfl_xor(SSQ[u], 32);                         \
            if (h == 0) { red_[(WAVE) * ct_ + u * 32 + r] = s2; red_[4 * ct_ + (WAVE) * ct_ + u * 32 + r] = q2; }              \
        }                                                                                                                      \
        __syncthreads();                                                                                                       \
        if (tid < ct_) {                                                                                                       \
            const double s4 = red_[tid] + red_[ct_ + tid] + red_[2 * ct_ + tid] + red_[3 * ct_ + tid];                         \
            const double q4 = red_[4 * ct_ + tid] + red_[5 * ct_ + tid] + red_[6 * ct_ + tid] + red_[7 * ct_ + tid];           \
            atomicAdd(&(P).osum[(int64_t)(B) * (P).Cout + (COL0) + tid], s4);                                                  \
            atomicAdd(&(P).osq[(int64_t)(B) * (P).Cout + (COL0) + tid], q4);                                                   \
        }                                                                                                                      \
    } while (0)

// LDS halo layout.  ds_read_b128 is serviced in four 16-lane groups that are NOT contiguous lane ranges ({0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same +32: MI355X_MICROARCH.md, LDS table); with the fragment's row r = (y = r>>3, x = r&7) a group is
// four runs of 4 x-consecutive voxels in 4 different halo rows, and 16-byte bank quads repeat every 256 B.  Two planes (P = 2):
// voxel = 64 B unpadded (x step = 4 quads) and ONE 16-byte pad per halo ROW (row pitch 41 quads, odd) -> every group touches 16
// distinct quads: conflict-free, and the halo shrinks to 39.4 KB.  (The earlier per-voxel pad, 80 B, was 3-way conflicted on every A
// read; found by enumerating the real lane groups: tools/dev/lds_bank_check.py.)  P = 3: 96-byte voxels + the row pad = 2-way (no
// conflict-free pitch exists; the per-voxel pad was 3-way).
template <int P, int HZ = GN_CONV_HZ> struct HaloLayout {
    static constexpr int VB = P * 32;                                      // bytes per voxel
    static constexpr int ROWP = GN_CONV_HX * VB + 16;                           // bytes per halo row
    static constexpr int BYTES = HZ * GN_CONV_HY * ROWP;
    __device__ static constexpr __forceinline__ int at(int hz, int hy, int hx) { return (hz * GN_CONV_HY + hy) * ROWP + hx * VB; }
};

// unet_wino.hip: launch of conv3d_split_wino_kernel<true> over `tiles` 4 x 8 x 8 tiles per sample (shape checks: conv3d_gcr_split_impl)
void gn_launch_conv3d_wino(const SplitArgs &p, int tiles, hipStream_t st);
// unet_wino32.hip: launch of conv3d_split_wino32pc_kernel<true> over `tiles8` 8 x 8 x 8 tiles per sample x Cout / 32 column blocks
void gn_launch_conv3d_wino32(const SplitArgs &p, int tiles8, hipStream_t st);

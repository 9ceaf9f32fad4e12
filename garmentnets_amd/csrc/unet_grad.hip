// unet_grad.hip -- backward kernels of the 3-D UNet's 'gcr' layers (GroupNorm -> Conv3d 3x3x3 -> ReLU) and the 2x2x2 max-pool, on the stored layout
// of the forward: channel-last [B][D][H][W][C] fp32, channel-padded widths (DESIGN.md "UNet gradients").  The final 1x1x1 convolution is a row GEMM:
// its backward is linear_grad.hip's.
//   gn_conv3d_bwd_weight     dW = sum over voxels of (GroupNorm-applied, virtually concatenated / upsampled input) x (ReLU-masked dy): implicit GEMM with
//                            K = B*D*H*W on v_mfma_f32_32x32x2_f32, split over K into partials, folded in a fixed order
//   gn_relu_mask             g = y > 0 ? dy : 0   (the data gradient then runs the FORWARD conv kernel on a flipped / transposed weight pack)
//   gn_groupnorm_bwd_stats / _coef / _apply    nn.GroupNorm's backward over the virtual concat, the x2 nearest upsampling's backward folded in
//   gn_maxpool3d_2_bwd       gradient to the winner of each window (ATen's scan), no index tensor
// Rule of the file (as grad.hip, losses.hip): NO float atomics; every sum has a fixed order, so identical calls give identical bits.
#include "common.h"

// ------------------------------------------------------------------------------------------------ conv weight gradient
// A workgroup owns a (32 input channels) x (NCO * 32 output channels) block of dW for ALL 27 taps and walks a chain of 4 x 8 x 8 spatial tiles.
// Per tile it stages once: the 6 x 10 x 10 halo of its 32 input channels with the GroupNorm affine applied on the way (x*a + d inside the volume, 0 in
// the padding; source 1 read at half resolution -- exactly the operand gn_conv3d_gcr forms) and the 256 voxels x NCO*32 channels of g = dy masked by
// y > 0.  Wave (kd, cu) of the 3 * NCO waves owns the 9 taps of plane kd for column block cu: 9 accumulators of 32 x 32 (144 registers), one MFMA
// 32x32x2 per tap and voxel pair -- lanes 0-31 feed voxel (z, y, x), lanes 32-63 voxel (z, y, x + 1), lane r channel r: both operands are one
// conflict-free 64-float LDS row read.  Each tap's sum runs over the voxels of the chain in tile order, voxel order inside a tile; the chain writes one
// partial [27][32][NCO*32]; conv3d_bwd_weight_fold_kernel adds the chains in ascending order (fp64) into the nn.Conv3d layout.
#define BW_CI 32
#define BW_TARGET_WORKGROUPS 512       /* chains x blocks: two rounds of the 256 CUs (a constant: the summation order must not depend on the device) */

struct BwArgs {
    const float *src0, *src1, *a, *d, *y, *dy;
    float *part;
    int C0, C1, B, D, H, W, Cout, Cin32;
    int tiles_z, tiles_y, tiles_x, ntiles, per_chain;
};

static int bw_chains(int B, int D, int H, int W, int Cin, int Cout, int *per_chain) {
    const int64_t ntiles = (int64_t)B * gn_cdiv(D, GN_CONV_TZ) * gn_cdiv(H, GN_CONV_TY) * gn_cdiv(W, GN_CONV_TX);
    const int nco = Cout % 64 == 0 ? 2 : 1;
    const int64_t blocks = gn_cdiv(Cin, BW_CI) * (Cout / (32 * nco));
    int64_t chains = gn_cdiv(BW_TARGET_WORKGROUPS, blocks);
    if (chains > ntiles) chains = ntiles;
    if (chains < 1) chains = 1;
    const int64_t per = gn_cdiv(ntiles, chains);
    if (per_chain) *per_chain = (int)per;
    return (int)gn_cdiv(ntiles, per);
}

template <int NCO>
__global__ __launch_bounds__(192 * NCO) void conv3d_bwd_weight_kernel(BwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float bw_smem[];
    float *halo = bw_smem;                          // [600 halo voxels][32 ci]
    float *gt = bw_smem + GN_CONV_HVOX * BW_CI;          // [NCO][256 voxels][32 co]
    constexpr int NT = 192 * NCO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
    const int kd = wave % 3, cu = wave / 3;
    const int Cin = p.C0 + p.C1;
    const int nco = p.Cout / (32 * NCO);
    const int ci0 = ((int)blockIdx.x / nco) * BW_CI, co0 = ((int)blockIdx.x % nco) * 32 * NCO;
    const int chain = blockIdx.y;
    const int D1 = p.D >> 1, H1 = p.H >> 1, W1 = p.W >> 1;

    f32x16 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[k][q] = 0.f;

    const int t_begin = chain * p.per_chain;
    int t_end = t_begin + p.per_chain;
    if (t_end > p.ntiles) t_end = p.ntiles;
    const int tiles_per_sample = p.tiles_z * p.tiles_y * p.tiles_x;
    for (int t = t_begin; t < t_end; ++t) {
        const int b = t / tiles_per_sample;
        int rem = t % tiles_per_sample;
        const int tz = rem % p.tiles_z; rem /= p.tiles_z;
        const int tx = rem % p.tiles_x;
        const int ty = rem / p.tiles_x;
        const int z0 = tz * GN_CONV_TZ, y0 = ty * GN_CONV_TY, x0 = tx * GN_CONV_TX;
        // ---- halo of 32 input channels, the forward's operand: fmul then fadd, zeros outside the volume and beyond the last channel
        for (int idx = tid; idx < GN_CONV_HVOX * (BW_CI / 4); idx += NT) {
            const int hv = idx >> 3, c4 = (idx & 7) * 4;
            const int c = ci0 + c4;
            const int hx = hv % GN_CONV_HX, hy = (hv / GN_CONV_HX) % GN_CONV_HY, hz = hv / (GN_CONV_HX * GN_CONV_HY);
            const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < Cin && gz >= 0 && gz < p.D && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                const float *sp;
                if (c >= p.C0) sp = p.src1 + ((((int64_t)b * D1 + (gz >> 1)) * H1 + (gy >> 1)) * W1 + (gx >> 1)) * p.C1 + (c - p.C0);
                else sp = p.src0 + ((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.C0 + c;
                const float4 xin = *reinterpret_cast<const float4 *>(sp);
                const float4 av = *reinterpret_cast<const float4 *>(p.a + (int64_t)b * Cin + c);
                const float4 dv = *reinterpret_cast<const float4 *>(p.d + (int64_t)b * Cin + c);
                v.x = __fadd_rn(__fmul_rn(xin.x, av.x), dv.x);
                v.y = __fadd_rn(__fmul_rn(xin.y, av.y), dv.y);
                v.z = __fadd_rn(__fmul_rn(xin.z, av.z), dv.z);
                v.w = __fadd_rn(__fmul_rn(xin.w, av.w), dv.w);
            }
            *reinterpret_cast<float4 *>(halo + hv * BW_CI + c4) = v;
        }
        // ---- g = dy masked by y > 0 (ReLU backward), zeros outside the volume
        for (int idx = tid; idx < NCO * GN_CONV_TVOX * 8; idx += NT) {
            const int cb = idx / (GN_CONV_TVOX * 8), rm = idx % (GN_CONV_TVOX * 8);
            const int vv = rm >> 3, c4 = (rm & 7) * 4;
            const int gz = z0 + (vv >> 6), gy = y0 + ((vv >> 3) & 7), gx = x0 + (vv & 7);
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gz < p.D && gy < p.H && gx < p.W) {
                const int64_t off = ((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.Cout + co0 + cb * 32 + c4;
                g = *reinterpret_cast<const float4 *>(p.dy + off);
                if (p.y) {
                    const float4 yv = *reinterpret_cast<const float4 *>(p.y + off);
                    g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f; g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
                }
            }
            *reinterpret_cast<float4 *>(gt + (cb * GN_CONV_TVOX + vv) * 32 + c4) = g;
        }
        __syncthreads();
        const float *gw = gt + cu * GN_CONV_TVOX * 32 + r;
#pragma unroll 2
        for (int pair = 0; pair < GN_CONV_TVOX / 2; ++pair) {
            const int vv = pair * 2 + h;
            const int z = vv >> 6, yy = (vv >> 3) & 7, x = vv & 7;
            const float gv = gw[vv * 32];
            const float *hb = halo + (((z + kd) * GN_CONV_HY + yy) * GN_CONV_HX + x) * BW_CI + r;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float av = hb[((k / 3) * GN_CONV_HX + (k % 3)) * BW_CI];
                acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, gv, acc[k], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // ---- one partial per chain: [chain][tap][Cin32][Cout]; accumulator q of lane (r, h) is row (q & 3) + 8 (q >> 2) + 4 h (ci), column r (co)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float *pp = p.part + (((int64_t)chain * 27 + kd * 9 + k) * p.Cin32 + ci0) * p.Cout + co0 + cu * 32 + r;
#pragma unroll
        for (int q = 0; q < 16; ++q) pp[(int64_t)((q & 3) + 8 * (q >> 2) + 4 * h) * p.Cout] = acc[k][q];
    }
}

// dW[co][ci][tap] = partials of chain 0, 1, 2, ... added in that order in fp64, rounded once
__global__ __launch_bounds__(256) void conv3d_bwd_weight_fold_kernel(const float *__restrict__ part, int chains, int Cin, int Cin32, int Cout,
                                                                     float *__restrict__ dw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)27 * Cin * Cout) return;
    const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), tap = (int)(i / ((int64_t)Cout * Cin));
    const int64_t stride = (int64_t)27 * Cin32 * Cout;
    const float *pp = part + ((int64_t)tap * Cin32 + ci) * Cout + co;
    double s = 0.0;
    for (int c = 0; c < chains; ++c) s += (double)pp[c * stride];
    dw[((int64_t)co * Cin + ci) * 27 + tap] = (float)s;
}

extern "C" size_t gn_conv3d_bwd_weight_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cout % 32 != 0) return 0;
    const int chains = bw_chains(B, D, H, W, Cin, Cout, nullptr);
    return (size_t)chains * 27 * (size_t)(gn_cdiv(Cin, BW_CI) * BW_CI) * Cout * sizeof(float);
}

extern "C" int gn_conv3d_bwd_weight(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d, const float *y, const float *dy,
                                    int B, int D, int H, int W, int Cout, void *ws, size_t ws_bytes, float *dw, void *stream) {
    GN_REQUIRE(B >= 0 && D > 0 && H > 0 && W > 0 && C0 > 0 && C1 >= 0 && Cout > 0, "gn_conv3d_bwd_weight: bad sizes");
    GN_REQUIRE(C0 % 4 == 0 && C1 % 4 == 0, "gn_conv3d_bwd_weight: channel counts must be multiples of 4 (C0=%d C1=%d)", C0, C1);
    GN_REQUIRE(Cout % 32 == 0, "gn_conv3d_bwd_weight: Cout=%d must be a multiple of 32", Cout);
    GN_REQUIRE(C1 == 0 || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "gn_conv3d_bwd_weight: upsampled source needs even dims");
    GN_REQUIRE((int64_t)B * gn_cdiv(D, GN_CONV_TZ) * gn_cdiv(H, GN_CONV_TY) * gn_cdiv(W, GN_CONV_TX) < ((int64_t)1 << 30), "gn_conv3d_bwd_weight: volume too large");
    const int Cin = C0 + C1;
    const size_t need = gn_conv3d_bwd_weight_workspace_bytes(B, D, H, W, Cin, Cout);
    GN_REQUIRE(ws_bytes >= need, "gn_conv3d_bwd_weight: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    hipStream_t st = gn_stream(stream);
    if (B == 0) {
        GN_REQUIRE(dw != nullptr, "gn_conv3d_bwd_weight: null pointer");
        GN_HIP(hipMemsetAsync(dw, 0, (size_t)27 * Cin * Cout * sizeof(float), st), "gn_conv3d_bwd_weight");
        return GN_OK;
    }
    GN_REQUIRE(src0 && a && d && dy && dw && ws && (C1 == 0 || src1), "gn_conv3d_bwd_weight: null pointer");
    BwArgs p;
    p.src0 = src0; p.src1 = src1; p.a = a; p.d = d; p.y = y; p.dy = dy; p.part = (float *)ws;
    p.C0 = C0; p.C1 = C1; p.B = B; p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.Cin32 = (int)gn_cdiv(Cin, BW_CI) * BW_CI;
    p.tiles_z = (int)gn_cdiv(D, GN_CONV_TZ); p.tiles_y = (int)gn_cdiv(H, GN_CONV_TY); p.tiles_x = (int)gn_cdiv(W, GN_CONV_TX);
    p.ntiles = B * p.tiles_z * p.tiles_y * p.tiles_x;
    const int chains = bw_chains(B, D, H, W, Cin, Cout, &p.per_chain);
    const int nco = Cout % 64 == 0 ? 2 : 1;
    const size_t lds = (size_t)(GN_CONV_HVOX * BW_CI + nco * GN_CONV_TVOX * 32) * sizeof(float);
    const dim3 grid((unsigned)((p.Cin32 / BW_CI) * (Cout / (32 * nco))), (unsigned)chains);
    if (nco == 2) {
        GN_HIP(hipFuncSetAttribute((const void *)conv3d_bwd_weight_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gn_conv3d_bwd_weight");
        hipLaunchKernelGGL(conv3d_bwd_weight_kernel<2>, grid, dim3(384), lds, st, p);
    } else {
        GN_HIP(hipFuncSetAttribute((const void *)conv3d_bwd_weight_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gn_conv3d_bwd_weight");
        hipLaunchKernelGGL(conv3d_bwd_weight_kernel<1>, grid, dim3(192), lds, st, p);
    }
    GN_LAUNCH_CHECK("gn_conv3d_bwd_weight");
    const int64_t n = (int64_t)27 * Cin * Cout;
    hipLaunchKernelGGL(conv3d_bwd_weight_fold_kernel, dim3((unsigned)gn_cdiv(n, 256)), dim3(256), 0, st, (const float *)ws, chains, Cin, p.Cin32, Cout, dw);
    GN_LAUNCH_CHECK("gn_conv3d_bwd_weight");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ ReLU mask
__global__ __launch_bounds__(256) void relu_mask_kernel(const float *__restrict__ y, const float *__restrict__ dy, int64_t n4, float *__restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 yv = reinterpret_cast<const float4 *>(y)[i];
    float4 v = reinterpret_cast<const float4 *>(dy)[i];
    v.x = yv.x > 0.f ? v.x : 0.f; v.y = yv.y > 0.f ? v.y : 0.f; v.z = yv.z > 0.f ? v.z : 0.f; v.w = yv.w > 0.f ? v.w : 0.f;
    reinterpret_cast<float4 *>(g)[i] = v;
}

extern "C" int gn_relu_mask(const float *y, const float *dy, int64_t n, float *g, void *stream) {
    GN_REQUIRE(n >= 0 && n % 4 == 0, "gn_relu_mask: bad sizes (n must be a non-negative multiple of 4)");
    if (n == 0) return GN_OK;
    GN_REQUIRE(y && dy && g, "gn_relu_mask: null pointer");
    hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)gn_cdiv(n / 4, 256)), dim3(256), 0, gn_stream(stream), y, dy, n / 4, g);
    GN_LAUNCH_CHECK("gn_relu_mask");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ GroupNorm backward
// dxn: the gradient at the conv's operand, [B][fine voxels][ldg] with this source's channels at column goff.  half: the source is the half-resolution
// one -- the 8 fine gradients of a coarse voxel are added first, fp32, in ascending (dz, dy, dx) order, dx fastest: ((((((g000 + g001) + g010) + g011) +
// g100) + g101) + g110) + g111 (gn_sum8: the ONE place that order is written).
__device__ __forceinline__ float4 gn_sum8(const float *__restrict__ dxn, int64_t b, int z, int y, int x, int Df, int Hf, int Wf, int ldg, int col) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 t = *reinterpret_cast<const float4 *>(
            dxn + ((((int64_t)b * Df + 2 * z + (k >> 2)) * Hf + 2 * y + ((k >> 1) & 1)) * Wf + 2 * x + (k & 1)) * ldg + col);
        if (k == 0) s = t;
        else { s.x = __fadd_rn(s.x, t.x); s.y = __fadd_rn(s.y, t.y); s.z = __fadd_rn(s.z, t.z); s.w = __fadd_rn(s.w, t.w); }
    }
    return s;
}

// stage 1: grid (chunks of 512 voxels of the source's own resolution, B).  Thread = (voxel group, 4 channels); fp64 per thread over its voxels in
// ascending order, the groups added in ascending order through LDS: part[b][chunk][2][C].  stage 2 adds the chunks in ascending order.
#define GB_VOX_PER_BLOCK 512
__global__ __launch_bounds__(256) void groupnorm_bwd_stats_kernel(const float *__restrict__ dxn, int ldg, int goff, const float *__restrict__ x, int C,
                                                                  int half, int D, int H, int W, double *__restrict__ part) {
    __shared__ double red[256][8];
    const int C4 = C >> 2, L = C4 < 256 ? C4 : 256, ngrp = 256 / L;
    const int b = blockIdx.y, tid = threadIdx.x, grp = tid / L;
    const int64_t V = (int64_t)D * H * W, v0 = (int64_t)blockIdx.x * GB_VOX_PER_BLOCK;
    int64_t v1 = v0 + GB_VOX_PER_BLOCK;
    if (v1 > V) v1 = V;
    double *po = part + ((int64_t)b * gridDim.x + blockIdx.x) * 2 * C;
    for (int cq = tid % L; cq < C4; cq += L) {          // (more than one trip only when C > 1024: then ngrp == 1 and no barrier is met)
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        if (grp < ngrp) {
            for (int64_t v = v0 + grp; v < v1; v += ngrp) {
                const float4 xv = *reinterpret_cast<const float4 *>(x + ((int64_t)b * V + v) * C + cq * 4);
                float4 g;
                if (half) g = gn_sum8(dxn, b, (int)(v / ((int64_t)H * W)), (int)((v / W) % H), (int)(v % W), 2 * D, 2 * H, 2 * W, ldg, goff + cq * 4);
                else g = *reinterpret_cast<const float4 *>(dxn + ((int64_t)b * V + v) * ldg + goff + cq * 4);
                s[0] += (double)g.x; s[1] += (double)g.y; s[2] += (double)g.z; s[3] += (double)g.w;
                q[0] += (double)g.x * (double)xv.x; q[1] += (double)g.y * (double)xv.y; q[2] += (double)g.z * (double)xv.z; q[3] += (double)g.w * (double)xv.w;
            }
        }
        if (ngrp == 1) {
            if (grp == 0) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { po[cq * 4 + k] = s[k]; po[C + cq * 4 + k] = q[k]; }
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[tid][k] = s[k]; red[tid][4 + k] = q[k]; }
        __syncthreads();
        if (tid < L) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                double t = 0.0;
                for (int g2 = 0; g2 < ngrp; ++g2) t += red[g2 * L + tid][k];
                po[(k >> 2) * C + tid * 4 + (k & 3)] = t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void groupnorm_bwd_stats_fold_kernel(const double *__restrict__ part, int chunks, int B, int C, double *__restrict__ s1,
                                                                       double *__restrict__ s2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * 2 * C) return;
    const int c = (int)(i % C), k = (int)((i / C) % 2), b = (int)(i / (2 * C));
    const double *pp = part + (int64_t)b * chunks * 2 * C + k * C + c;
    double t = 0.0;
    for (int ch = 0; ch < chunks; ++ch) t += pp[(int64_t)ch * 2 * C];
    (k ? s2 : s1)[(int64_t)b * C + c] = t;
}

extern "C" size_t gn_groupnorm_bwd_stats_workspace_bytes(int B, int64_t V, int C) {
    if (B <= 0 || V <= 0 || C <= 0) return 0;
    return (size_t)B * (size_t)gn_cdiv(V, GB_VOX_PER_BLOCK) * 2 * C * sizeof(double);
}

// x: the source as stored, [B][D][H][W][C] (its own resolution); dxn [B][fine][ldg], fine = (D, H, W) or, half != 0, (2D, 2H, 2W)
extern "C" int gn_groupnorm_bwd_stats(const float *dxn, int ldg, int goff, const float *x, int B, int D, int H, int W, int C, int half, void *ws,
                                      size_t ws_bytes, double *s1, double *s2, void *stream) {
    GN_REQUIRE(B >= 0 && D > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "gn_groupnorm_bwd_stats: bad sizes (C=%d must be a positive multiple of 4)", C);
    GN_REQUIRE(goff >= 0 && goff % 4 == 0 && ldg % 4 == 0 && ldg >= goff + C, "gn_groupnorm_bwd_stats: bad sizes (ldg=%d goff=%d C=%d)", ldg, goff, C);
    const int64_t V = (int64_t)D * H * W;
    const size_t need = gn_groupnorm_bwd_stats_workspace_bytes(B, V, C);
    GN_REQUIRE(ws_bytes >= need, "gn_groupnorm_bwd_stats: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    if (B == 0) return GN_OK;
    GN_REQUIRE(dxn && x && ws && s1 && s2, "gn_groupnorm_bwd_stats: null pointer");
    hipStream_t st = gn_stream(stream);
    const int chunks = (int)gn_cdiv(V, GB_VOX_PER_BLOCK);
    hipLaunchKernelGGL(groupnorm_bwd_stats_kernel, dim3((unsigned)chunks, B), dim3(256), 0, st, dxn, ldg, goff, x, C, half ? 1 : 0, D, H, W, (double *)ws);
    GN_LAUNCH_CHECK("gn_groupnorm_bwd_stats");
    hipLaunchKernelGGL(groupnorm_bwd_stats_fold_kernel, dim3((unsigned)gn_cdiv((int64_t)B * 2 * C, 256)), dim3(256), 0, st, (const double *)ws, chunks, B, C,
                       s1, s2);
    GN_LAUNCH_CHECK("gn_groupnorm_bwd_stats");
    return GN_OK;
}

// One block.  Samples in ascending order; per sample the group sums in ascending channel order (one thread per group, as the forward's affine kernel).
// With n = cpg * V0, mean / rstd of the group from the forward's (sum, sumsq) in fp64, t1 = sum dxn, t2 = sum dxn * x per channel:
//   A = sum_c gamma t1,  Bq = sum_c gamma (t2 - mean t1) rstd,   p = rstd gamma,  q = -rstd^2 Bq / n,  r = -rstd A / n + rstd^2 mean Bq / n
//   dgamma[c] = sum_b (t2 - mean t1) rstd,  dbeta[c] = sum_b t1.
struct GbCoefArgs {
    const double *t1_0, *t2_0, *t1_1, *t2_1, *sum0, *sq0, *sum1, *sq1;
    const float *gamma;
    float *p, *q, *r, *dgamma, *dbeta;
    int C0, S0, C1, S1, rep1, B, groups;
    int64_t V0;
    float eps;
};

__global__ __launch_bounds__(256) void groupnorm_bwd_coef_kernel(GbCoefArgs k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gb_smem[];
    const int C = k.C0 + k.C1, S = k.S0 + k.S1, cpg = C / k.groups, tid = threadIdx.x;
    double *ls = reinterpret_cast<double *>(gb_smem), *lq = ls + C, *t1 = lq + C, *t2 = t1 + C, *dg = t2 + C, *db = dg + C;
    double *gmean = db + C, *grstd = gmean + k.groups, *gA = grstd + k.groups, *gB = gA + k.groups;
    for (int c = tid; c < C; c += 256) { dg[c] = 0.0; db[c] = 0.0; }
    const double n = (double)cpg * (double)k.V0;
    for (int b = 0; b < k.B; ++b) {
        for (int c = tid; c < C; c += 256) {
            if (c < k.C0) {
                const int64_t o = (int64_t)b * k.S0 + c;
                ls[c] = k.sum0[o]; lq[c] = k.sq0[o]; t1[c] = k.t1_0[o]; t2[c] = k.t2_0[o];
            } else {
                const int64_t o = (int64_t)b * k.S1 + c - k.C0;
                ls[c] = k.rep1 * k.sum1[o]; lq[c] = k.rep1 * k.sq1[o]; t1[c] = k.t1_1[o]; t2[c] = k.t2_1[o];
            }
        }
        for (int j = tid; j < S; j += 256) {
            if ((j >= k.C0 && j < k.S0) || j >= k.S0 + k.C1) { k.p[(int64_t)b * S + j] = 0.f; k.q[(int64_t)b * S + j] = 0.f; k.r[(int64_t)b * S + j] = 0.f; }
        }
        __syncthreads();
        for (int g = tid; g < k.groups; g += 256) {
            double s = 0.0, q = 0.0;
            for (int c = g * cpg; c < (g + 1) * cpg; ++c) { s += ls[c]; q += lq[c]; }
            const double mean = s / n;
            double var = q / n - mean * mean;
            if (var < 0) var = 0;
            const double rstd = 1.0 / sqrt(var + (double)k.eps);
            double A = 0.0, Bq = 0.0;
            for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
                A += (double)k.gamma[c] * t1[c];
                Bq += (double)k.gamma[c] * (t2[c] - mean * t1[c]) * rstd;
            }
            gmean[g] = mean; grstd[g] = rstd; gA[g] = A; gB[g] = Bq;
        }
        __syncthreads();
        for (int c = tid; c < C; c += 256) {
            const int g = c / cpg;
            const double mean = gmean[g], rstd = grstd[g], A = gA[g], Bq = gB[g];
            const int64_t o = (int64_t)b * S + (c < k.C0 ? c : k.S0 + c - k.C0);
            k.p[o] = (float)(rstd * (double)k.gamma[c]);
            k.q[o] = (float)(-rstd * rstd * Bq / n);
            k.r[o] = (float)(-rstd * A / n + rstd * rstd * mean * Bq / n);
            dg[c] += (t2[c] - mean * t1[c]) * rstd;
            db[c] += t1[c];
        }
        __syncthreads();
    }
    for (int c = tid; c < C; c += 256) { k.dgamma[c] = (float)dg[c]; k.dbeta[c] = (float)db[c]; }
}

#define GB_COEF_MAX_LDS (160 * 1024)
extern "C" int gn_groupnorm_bwd_coef(const double *t1_0, const double *t2_0, const double *sum0, const double *sq0, int C0, int S0, int64_t V0,
                                     const double *t1_1, const double *t2_1, const double *sum1, const double *sq1, int C1, int S1, int64_t V1, int rep1,
                                     int B, int groups, float eps, const float *gamma, float *p, float *q, float *r, float *dgamma, float *dbeta,
                                     void *stream) {
    GN_REQUIRE(B >= 0 && groups > 0 && C0 > 0 && C1 >= 0 && S0 >= C0 && S1 >= C1 && (C0 + C1) % groups == 0 && V0 > 0, "gn_groupnorm_bwd_coef: bad sizes");
    GN_REQUIRE(C1 == 0 || (rep1 > 0 && V1 * rep1 == V0), "gn_groupnorm_bwd_coef: source 1 must cover the same voxels after replication");
    GN_REQUIRE((int64_t)S0 + S1 <= (int64_t)1 << 30, "gn_groupnorm_bwd_coef: bad sizes");
    const int C = C0 + C1;
    const size_t lds = ((size_t)6 * C + (size_t)4 * groups) * sizeof(double);
    GN_REQUIRE(lds <= GB_COEF_MAX_LDS, "gn_groupnorm_bwd_coef: %d channels in %d groups need %zu bytes of LDS (at most %d)", C, groups, lds, GB_COEF_MAX_LDS);
    GN_REQUIRE(gamma && dgamma && dbeta, "gn_groupnorm_bwd_coef: null pointer");
    GN_REQUIRE(B == 0 || (t1_0 && t2_0 && sum0 && sq0 && p && q && r && (C1 == 0 || (t1_1 && t2_1 && sum1 && sq1))), "gn_groupnorm_bwd_coef: null pointer");
    GbCoefArgs k;
    k.t1_0 = t1_0; k.t2_0 = t2_0; k.t1_1 = t1_1; k.t2_1 = t2_1; k.sum0 = sum0; k.sq0 = sq0; k.sum1 = sum1; k.sq1 = sq1; k.gamma = gamma;
    k.p = p; k.q = q; k.r = r; k.dgamma = dgamma; k.dbeta = dbeta;
    k.C0 = C0; k.S0 = S0; k.C1 = C1; k.S1 = S1; k.rep1 = C1 ? rep1 : 1; k.B = B; k.groups = groups; k.V0 = V0; k.eps = eps;
    GN_HIP(hipFuncSetAttribute((const void *)groupnorm_bwd_coef_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gn_groupnorm_bwd_coef");
    hipLaunchKernelGGL(groupnorm_bwd_coef_kernel, dim3(1), dim3(256), lds, gn_stream(stream), k);
    GN_LAUNCH_CHECK("gn_groupnorm_bwd_coef");
    return GN_OK;
}

// dx = dxn * p + x * q + r  (fma(dxn, p, fma(x, q, r))); half: dx[coarse] = fma(sum8(dxn), p, fma(x, 8 q, 8 r)).  accumulate: dx += that.
// p / q / r: [B][cs] rows, this source's channels at column coff.
__global__ __launch_bounds__(256) void groupnorm_bwd_apply_kernel(const float *__restrict__ dxn, int ldg, int goff, const float *__restrict__ x, int C,
                                                                  int half, int D, int H, int W, const float *__restrict__ p, const float *__restrict__ q,
                                                                  const float *__restrict__ r, int cs, int coff, int accumulate, int64_t n4,
                                                                  float *__restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int C4 = C >> 2;
    const int c = (int)(i % C4) * 4;
    const int64_t vox = i / C4, V = (int64_t)D * H * W, b = vox / V, v = vox % V;
    const float4 xv = reinterpret_cast<const float4 *>(x)[i];
    const float4 pv = *reinterpret_cast<const float4 *>(p + b * cs + coff + c);
    float4 qv = *reinterpret_cast<const float4 *>(q + b * cs + coff + c);
    float4 rv = *reinterpret_cast<const float4 *>(r + b * cs + coff + c);
    float4 g;
    if (half) {
        g = gn_sum8(dxn, b, (int)(v / ((int64_t)H * W)), (int)((v / W) % H), (int)(v % W), 2 * D, 2 * H, 2 * W, ldg, goff + c);
        qv.x = __fmul_rn(qv.x, 8.f); qv.y = __fmul_rn(qv.y, 8.f); qv.z = __fmul_rn(qv.z, 8.f); qv.w = __fmul_rn(qv.w, 8.f);
        rv.x = __fmul_rn(rv.x, 8.f); rv.y = __fmul_rn(rv.y, 8.f); rv.z = __fmul_rn(rv.z, 8.f); rv.w = __fmul_rn(rv.w, 8.f);
    } else {
        g = *reinterpret_cast<const float4 *>(dxn + vox * ldg + goff + c);
    }
    float4 o;
    o.x = __fmaf_rn(g.x, pv.x, __fmaf_rn(xv.x, qv.x, rv.x));
    o.y = __fmaf_rn(g.y, pv.y, __fmaf_rn(xv.y, qv.y, rv.y));
    o.z = __fmaf_rn(g.z, pv.z, __fmaf_rn(xv.z, qv.z, rv.z));
    o.w = __fmaf_rn(g.w, pv.w, __fmaf_rn(xv.w, qv.w, rv.w));
    if (accumulate) {
        const float4 e = reinterpret_cast<const float4 *>(dx)[i];
        o.x = __fadd_rn(e.x, o.x); o.y = __fadd_rn(e.y, o.y); o.z = __fadd_rn(e.z, o.z); o.w = __fadd_rn(e.w, o.w);
    }
    reinterpret_cast<float4 *>(dx)[i] = o;
}

extern "C" int gn_groupnorm_bwd_apply(const float *dxn, int ldg, int goff, const float *x, int B, int D, int H, int W, int C, int half, const float *p,
                                      const float *q, const float *r, int cs, int coff, int accumulate, float *dx, void *stream) {
    GN_REQUIRE(B >= 0 && D > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "gn_groupnorm_bwd_apply: bad sizes (C=%d must be a positive multiple of 4)", C);
    GN_REQUIRE(goff >= 0 && goff % 4 == 0 && ldg % 4 == 0 && ldg >= goff + C, "gn_groupnorm_bwd_apply: bad sizes (ldg=%d goff=%d C=%d)", ldg, goff, C);
    GN_REQUIRE(coff >= 0 && coff % 4 == 0 && cs % 4 == 0 && cs >= coff + C, "gn_groupnorm_bwd_apply: bad sizes (cs=%d coff=%d C=%d)", cs, coff, C);
    if (B == 0) return GN_OK;
    GN_REQUIRE(dxn && x && p && q && r && dx, "gn_groupnorm_bwd_apply: null pointer");
    const int64_t n4 = (int64_t)B * D * H * W * (C / 4);
    hipLaunchKernelGGL(groupnorm_bwd_apply_kernel, dim3((unsigned)gn_cdiv(n4, 256)), dim3(256), 0, gn_stream(stream), dxn, ldg, goff, x, C, half ? 1 : 0, D, H,
                       W, p, q, r, cs, coff, accumulate ? 1 : 0, n4, dx);
    GN_LAUNCH_CHECK("gn_groupnorm_bwd_apply");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ maxpool 2x2x2 backward
// The winner of a window is found again from the stored input by ATen's CPU scan (max_pool3d): (z, y, x) order, x fastest, a value replaces the
// running maximum when it is greater or a NaN -- the first of equal maxima wins, a NaN beats every number and a later NaN an earlier one.
// Every input voxel of an even volume is written: the winner gets the window's gradient, the other seven 0.
__global__ __launch_bounds__(256) void maxpool3d_2_bwd_kernel(const float *__restrict__ grad_out, const float *__restrict__ in, int D, int H, int W, int C,
                                                              int64_t n4, float *__restrict__ grad_in) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int C4 = C >> 2, Do = D >> 1, Ho = H >> 1, Wo = W >> 1;
    const int c = (int)(i % C4) * 4;
    int64_t v = i / C4;
    const int x = (int)(v % Wo); v /= Wo;
    const int y = (int)(v % Ho); v /= Ho;
    const int z = (int)(v % Do);
    const int64_t b = v / Do;
    const float4 g = reinterpret_cast<const float4 *>(grad_out)[i];
    float m[4];
    int w[4] = {0, 0, 0, 0};
    int64_t off[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        off[k] = ((((int64_t)b * D + 2 * z + (k >> 2)) * H + 2 * y + ((k >> 1) & 1)) * W + 2 * x + (k & 1)) * C + c;
        const float4 t = *reinterpret_cast<const float4 *>(in + off[k]);
        const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (k == 0) m[e] = tv[e];
            else if (tv[e] > m[e] || tv[e] != tv[e]) { m[e] = tv[e]; w[e] = k; }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        *reinterpret_cast<float4 *>(grad_in + off[k]) = make_float4(w[0] == k ? g.x : 0.f, w[1] == k ? g.y : 0.f, w[2] == k ? g.z : 0.f, w[3] == k ? g.w : 0.f);
}

extern "C" int gn_maxpool3d_2_bwd(const float *grad_out, const float *in, int B, int D, int H, int W, int C, float *grad_in, void *stream) {
    GN_REQUIRE(B >= 0 && D >= 2 && H >= 2 && W >= 2 && C > 0 && C % 4 == 0, "gn_maxpool3d_2_bwd: bad sizes");
    GN_REQUIRE(D % 2 == 0 && H % 2 == 0 && W % 2 == 0, "gn_maxpool3d_2_bwd: the volume (%d, %d, %d) must have even dims (every input voxel is written)", D, H, W);
    if (B == 0) return GN_OK;
    GN_REQUIRE(grad_out && in && grad_in, "gn_maxpool3d_2_bwd: null pointer");
    const int64_t n4 = (int64_t)B * (D / 2) * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(maxpool3d_2_bwd_kernel, dim3((unsigned)gn_cdiv(n4, 256)), dim3(256), 0, gn_stream(stream), grad_out, in, D, H, W, C, n4, grad_in);
    GN_LAUNCH_CHECK("gn_maxpool3d_2_bwd");
    return GN_OK;
}

// unet_grad_split.hip -- the f16x2 form of the UNet convolutions' backward (DESIGN.md "f16x2 backward of the UNet convolutions"): the 16-bit matrix
// cores under the same mathematical objects as unet_grad.hip's fp32 kernels.
//   gn_relu_mask_max             g = y > 0 ? dy : 0 as gn_relu_mask, and per sample the largest FINITE |g|, a power-of-two range scale 2^k[b] from it and
//                                its inverse: the operand scale of the data gradient (gn_conv3d_gcr_split on the flipped / transposed pack takes
//                                a[b][:] = 2^k[b], d = 0, act_inv[b] = 2^-k[b]) and the input of the weight gradient's launch-wide scale
//   gn_conv3d_bwd_weight_split   dW as gn_conv3d_bwd_weight: both operands split into two fp16 planes after a power-of-two scale, the products
//                                hi*hi, hi*lo, lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulation, chains of tiles folded in fp64 in ascending order
// Rule of the file (as unet_grad.hip): NO atomics; every sum has a fixed order, identical calls give identical bits.
#include "common.h"

// ------------------------------------------------------------------------------------------------ ReLU mask + per-sample maximum
// Stage 1: grid (blocks, B).  max |g| over the finite values a workgroup sees, as the bit pattern of a non-negative float (monotone as an unsigned
// integer; 0: nothing but zeros), one partial per workgroup: part[b][block].  Stage 2 takes the maximum of a sample's partials.  No atomics.
#define GS_MASK_BLOCKS 256       /* at most this many workgroups per sample in the masking pass (a grid-stride loop inside); stage 2 reads them with one thread each */
__global__ __launch_bounds__(256) void relu_mask_max_kernel(const float *__restrict__ y, const float *__restrict__ dy, int64_t n4, float *__restrict__ g,
                                                            unsigned *__restrict__ part) {
    __shared__ unsigned wmax[4];
    const int b = blockIdx.y;
    const float4 *yp = y ? reinterpret_cast<const float4 *>(y) + (int64_t)b * n4 : nullptr;
    const float4 *dp = reinterpret_cast<const float4 *>(dy) + (int64_t)b * n4;
    float4 *gp = reinterpret_cast<float4 *>(g) + (int64_t)b * n4;
    unsigned m = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = dp[i];
        if (yp) {
            const float4 yv = yp[i];
            v.x = yv.x > 0.f ? v.x : 0.f; v.y = yv.y > 0.f ? v.y : 0.f; v.z = yv.z > 0.f ? v.z : 0.f; v.w = yv.w > 0.f ? v.w : 0.f;
        }
        gp[i] = v;
        const unsigned u[4] = {__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu, __float_as_uint(v.z) & 0x7fffffffu,
                               __float_as_uint(v.w) & 0x7fffffffu};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (u[k] < 0x7f800000u && u[k] > m) m = u[k];          // finite values only: an Inf / NaN must not decide the scale
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned m01 = wmax[0] > wmax[1] ? wmax[0] : wmax[1], m23 = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
        part[(int64_t)b * gridDim.x + blockIdx.x] = m01 > m23 ? m01 : m23;
    }
}

// the exponent k with m * 2^k in [2^14, 2^15) (fp16's largest finite value is 65504 < 2^16; values down to 2^-17 of the maximum then keep a normal second
// plane), held to [-126, 126] so that 2^k and 2^-k are normal floats; m == 0 (an all-zero sample): k = 0
__device__ __forceinline__ int gs_range_exp(float m) {
    if (!(m > 0.f)) return 0;
    const int e = (int)((__float_as_uint(m) >> 23) & 0xff) - 127;         // (a subnormal maximum reads as 2^-127: k is clamped below)
    int k = 14 - e;
    if (k > 126) k = 126;
    if (k < -126) k = -126;
    return k;
}

// stage 2: one workgroup per sample: the maximum of its partials (nb <= 256: one per thread), then gmax[b], scale[b][0..C) = 2^k and inv[b] = 2^-k
__global__ __launch_bounds__(256) void relu_mask_scale_kernel(const unsigned *__restrict__ part, int nb, int C, float *__restrict__ gmax,
                                                              float *__restrict__ scale, float *__restrict__ inv) {
    __shared__ unsigned wmax[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    unsigned m = tid < nb ? part[(int64_t)b * nb + tid] : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    const unsigned m01 = wmax[0] > wmax[1] ? wmax[0] : wmax[1], m23 = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
    const float mf = __uint_as_float(m01 > m23 ? m01 : m23);
    if (tid == 0) gmax[b] = mf;
    if (!scale) return;
    const int k = gs_range_exp(mf);
    const float sc = ldexpf(1.f, k);
    for (int c = tid; c < C; c += 256) scale[(int64_t)b * C + c] = sc;
    if (tid == 0) inv[b] = ldexpf(1.f, -k);
}

extern "C" size_t gn_relu_mask_max_workspace_bytes(int B) { return B > 0 ? (size_t)B * GS_MASK_BLOCKS * sizeof(unsigned) : 0; }

extern "C" int gn_relu_mask_max(const float *y, const float *dy, int B, int64_t n, int C, float *g, float *gmax, float *scale, float *inv, void *ws,
                                size_t ws_bytes, void *stream) {
    GN_REQUIRE(B >= 0 && n >= 0 && n % 4 == 0 && C > 0, "gn_relu_mask_max: bad sizes (n, the values per sample, must be a non-negative multiple of 4)");
    GN_REQUIRE((scale == nullptr) == (inv == nullptr), "gn_relu_mask_max: scale [B][C] and inv [B] come together");
    GN_REQUIRE(ws_bytes >= gn_relu_mask_max_workspace_bytes(B), "gn_relu_mask_max: workspace too small (%zu < %zu bytes)", ws_bytes,
               gn_relu_mask_max_workspace_bytes(B));
    if (B == 0) return GN_OK;
    GN_REQUIRE(dy && g && gmax && ws, "gn_relu_mask_max: null pointer");
    hipStream_t st = gn_stream(stream);
    int64_t blocks = gn_cdiv(n / 4, 256 * 4);
    if (blocks > GS_MASK_BLOCKS) blocks = GS_MASK_BLOCKS;
    if (blocks < 1) blocks = 1;                                  // (n == 0: the one workgroup writes a zero partial)
    hipLaunchKernelGGL(relu_mask_max_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, y, dy, n / 4, g, (unsigned *)ws);
    GN_LAUNCH_CHECK("gn_relu_mask_max");
    hipLaunchKernelGGL(relu_mask_scale_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned *)ws, (int)blocks, C, gmax, scale, inv);
    GN_LAUNCH_CHECK("gn_relu_mask_max");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ conv weight gradient, f16x2
// Ownership as conv3d_bwd_weight_kernel: a workgroup owns a (32 input channels) x (NCO * 32 output channels) block of dW for all 27 taps and walks a chain
// of 4 x 8 x 8 tiles; wave (kd, cu) of the 3 * NCO waves holds the 9 taps of plane kd for column block cu in 9 accumulators of 32 x 32.
// K of v_mfma_f32_32x32x16_f16 is the VOXEL index while the volumes are channel-last, so both operands are staged as they arrive from HBM -- rows
// [voxel][32 channels] of fp16, 64 bytes each, one image per plane (hi, lo) -- and the fragments are taken with ds_read_b64_tr_b16: per 16-lane group a
// block of 4 voxel rows x 16 channels, delivered channel-on-the-lane.  Lane l = 16 grp + 4 q + p supplies row q, channels 16 (grp & 1) + 4 p .. + 3 of the
// block and receives channel 16 (grp & 1) + (l & 15) of the four voxels: two reads give the lane's 8 K values (voxels 8 h + 0..7 of the 16-voxel step,
// h = l >> 5).  A step is the 16 voxels (y = 2 s, 2 s + 1; x = 0..7) of one z: a tap shift is a ROW offset of the halo image (an instruction immediate),
// no shifted copy and no misaligned read.  Per step a wave takes 4 transposed reads for g (both planes, reused by its 9 taps), 36 for xn, 27 MFMAs.
// Conditions of the transposed read (they are conditions of this kernel): every lane address is a multiple of 8 bytes (rows of 64 B, channel offsets of
// 8 B, the dynamic LDS region 16-byte aligned, no static LDS in front of it); EXEC is all ones at every transposed read -- the workgroup is 192 or 384
// lanes, the reads sit in the tile / step loops whose bounds are workgroup-uniform, never under a lane-dependent branch; nothing is masked: every lane
// address lies inside the images (the halo image covers every tap shift).
// Banks (bank = (byte / 4) % 64, conflicts inside a 32-lane half): the half's 32 lanes address 4 CONSECUTIVE 64-byte rows (x .. x + 3 of one halo row;
// 4 consecutive tile voxels of g), each lane 8 bytes of its row: 256 contiguous bytes = the 64 banks once each, whatever the first row.  Conflict-free.
// LDS: halo 600 rows x 64 B x 2 planes = 76 800 B, g NCO x 256 rows x 64 B x 2 planes = 32 768 NCO B: 142 336 B (NCO = 2), 109 568 B (NCO = 1): one
// workgroup per CU.
// Scales: a chain may span samples, so ONE power of two per operand per launch.  xn: a, d arrive as gn_conv3d_gcr_split takes them -- multiplied by the
// sample's power of two 2^k[b] with x_inv[b] = 2^-k[b] (ops.groupnorm_affine(with_act_scale=True): the largest per-channel rms in [1, 2)) -- and the staged
// value is multiplied by x_inv[b] / max_b x_inv: exactly xn / X, X = max_b x_inv.  g is multiplied by 2^kg from the largest finite |g| of the batch
// (gs_range_exp).  The fold multiplies the fp64 sum by X * 2^-kg (exact) and rounds once.  An all-zero dy has kg = 0: exact zeros.  An Inf / NaN in g is
// an Inf / NaN in its fp16 planes (lo = Inf - Inf = NaN): every dW entry of that output channel is non-finite.
#define BWS_CI 32
#define BWS_TARGET_WORKGROUPS 512      /* chains x blocks, as BW_TARGET_WORKGROUPS of unet_grad.hip: a constant, the summation order must not depend on the device */
#define BWS_ROW 64                     /* bytes of one [voxel][32 channels] fp16 row */
#define BWS_HALO_BYTES (GN_CONV_HVOX * BWS_ROW)
#define BWS_G_BYTES (GN_CONV_TVOX * BWS_ROW)

struct BwsArgs {
    const float *src0, *src1, *a, *d, *y, *dy;
    const float *hdr;          // workspace header (bws_scales_kernel): [0] = 2^kg; [2..3] = the double X * 2^-kg; [4 + b] = x_inv[b] / X
    float *part;
    int C0, C1, B, D, H, W, Cout, Cin32;
    int tiles_z, tiles_y, tiles_x, ntiles, per_chain;
};

// the workspace: the header's 4 + B floats on 16 bytes, then from the next 256-byte boundary one partial [27][Cin32][Cout] per chain
struct BwsWs { float *hdr, *part; };
static BwsWs bws_ws(GnCarve &c, int B, int chains, int Cin, int Cout) {
    return {c.take<float>(4 + (size_t)B, 16), c.take<float>((size_t)chains * 27 * (size_t)(gn_cdiv(Cin, BWS_CI) * BWS_CI) * Cout, 256)};
}

static int bws_chains(int B, int D, int H, int W, int Cin, int Cout, int *per_chain) {
    const int64_t ntiles = (int64_t)B * gn_cdiv(D, GN_CONV_TZ) * gn_cdiv(H, GN_CONV_TY) * gn_cdiv(W, GN_CONV_TX);
    const int nco = Cout % 64 == 0 ? 2 : 1;
    const int64_t blocks = gn_cdiv(Cin, BWS_CI) * (Cout / (32 * nco));
    int64_t chains = gn_cdiv(BWS_TARGET_WORKGROUPS, blocks);
    if (chains > ntiles) chains = ntiles;
    if (chains < 1) chains = 1;
    const int64_t per = gn_cdiv(ntiles, chains);
    if (per_chain) *per_chain = (int)per;
    return (int)gn_cdiv(ntiles, per);
}

// one block: the launch-wide scales from the per-sample ones
__global__ __launch_bounds__(64) void bws_scales_kernel(const float *__restrict__ x_inv, const float *__restrict__ gmax, int B, float *__restrict__ hdr) {
    float X = x_inv ? 0.f : 1.f, gm = 0.f;
    for (int b = 0; b < B; ++b) {
        if (x_inv) X = fmaxf(X, x_inv[b]);
        gm = fmaxf(gm, gmax[b]);
    }
    const int kg = gs_range_exp(gm);
    if (threadIdx.x == 0) {
        hdr[0] = ldexpf(1.f, kg);
        *reinterpret_cast<double *>(hdr + 2) = (double)X * ldexp(1.0, -kg);
    }
    for (int b = threadIdx.x; b < B; b += 64) hdr[4 + b] = x_inv ? x_inv[b] / X : 1.f;
}

typedef short bws_v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) bws_v4i16 *bws_lds_v4;
// ds_read_b64_tr_b16 at LDS byte address `base + off` (off: a compile-time constant wherever the caller's is, so it becomes the instruction's immediate)
__device__ __forceinline__ uint2 bws_tr(__attribute__((address_space(3))) char *base, int off) {
    return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((bws_lds_v4)(base + off)));
}

template <int NCO>
__global__ __launch_bounds__(192 * NCO) void conv3d_bwd_weight_split_kernel(BwsArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bws_smem[];
    unsigned char *xh = bws_smem, *xl = xh + BWS_HALO_BYTES;                    // [600 halo voxels][32 ci] fp16, hi and lo plane
    unsigned char *gh = xl + BWS_HALO_BYTES, *gl = gh + NCO * BWS_G_BYTES;      // [NCO][256 voxels][32 co] fp16, hi and lo plane
    constexpr int NT = 192 * NCO;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r = lane & 31;
    const int kd = wave % 3, cu = wave / 3;
    const int Cin = p.C0 + p.C1;
    const int nco = p.Cout / (32 * NCO);
    const int ci0 = ((int)blockIdx.x / nco) * BWS_CI, co0 = ((int)blockIdx.x % nco) * 32 * NCO;
    const int chain = blockIdx.y;
    const int D1 = p.D >> 1, H1 = p.H >> 1, W1 = p.W >> 1;
    const float sg = p.hdr[0];

    f32x16 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[k][q] = 0.f;

    // the lane's part of every transposed-read address: row q of its group's block, channels 16 (grp & 1) + 4 p
    const int tq = (lane >> 2) & 3, tp = lane & 3, tcb = (lane >> 4) & 1;
    const int lane_x = ((kd * GN_CONV_HY + h) * GN_CONV_HX + tq) * BWS_ROW + tcb * 32 + tp * 8;
    const int lane_g = cu * BWS_G_BYTES + (8 * h + tq) * BWS_ROW + tcb * 32 + tp * 8;
    __attribute__((address_space(3))) char *lxh = (__attribute__((address_space(3))) char *)xh + lane_x;
    __attribute__((address_space(3))) char *lxl = (__attribute__((address_space(3))) char *)xl + lane_x;
    __attribute__((address_space(3))) char *lgh = (__attribute__((address_space(3))) char *)gh + lane_g;
    __attribute__((address_space(3))) char *lgl = (__attribute__((address_space(3))) char *)gl + lane_g;

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
        const float mx = p.hdr[4 + b];
        // ---- halo of 32 input channels: the forward's operand (fmul then fadd), times the launch scale, split into two fp16 planes; zeros outside the
        //      volume and beyond the last channel.  Four loads in flight per thread.
        for (int base = tid; base < GN_CONV_HVOX * (BWS_CI / 4); base += NT * 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * NT;
                const int hv = idx >> 3, c4 = (idx & 7) * 4;
                const int c = ci0 + c4;
                const int hx = hv % GN_CONV_HX, hy = (hv / GN_CONV_HX) % GN_CONV_HY, hz = hv / (GN_CONV_HX * GN_CONV_HY);
                const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx < GN_CONV_HVOX * (BWS_CI / 4) && c < Cin && gz >= 0 && gz < p.D && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                    const float *sp;
                    if (c >= p.C0) sp = p.src1 + ((((int64_t)b * D1 + (gz >> 1)) * H1 + (gy >> 1)) * W1 + (gx >> 1)) * p.C1 + (c - p.C0);
                    else sp = p.src0 + ((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.C0 + c;
                    const float4 xin = *reinterpret_cast<const float4 *>(sp);
                    const float4 av = *reinterpret_cast<const float4 *>(p.a + (int64_t)b * Cin + c);
                    const float4 dv = *reinterpret_cast<const float4 *>(p.d + (int64_t)b * Cin + c);
                    v[u].x = __fmul_rn(__fadd_rn(__fmul_rn(xin.x, av.x), dv.x), mx);
                    v[u].y = __fmul_rn(__fadd_rn(__fmul_rn(xin.y, av.y), dv.y), mx);
                    v[u].z = __fmul_rn(__fadd_rn(__fmul_rn(xin.z, av.z), dv.z), mx);
                    v[u].w = __fmul_rn(__fadd_rn(__fmul_rn(xin.w, av.w), dv.w), mx);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * NT;
                if (idx < GN_CONV_HVOX * (BWS_CI / 4)) {
                    uint2 pl[2];
                    split4<2, true>(v[u].x, v[u].y, v[u].z, v[u].w, pl);
                    *reinterpret_cast<uint2 *>(xh + idx * 8) = pl[0];          // (row hv, channels c4 .. c4 + 3: byte hv * 64 + c4 * 2 = idx * 8)
                    *reinterpret_cast<uint2 *>(xl + idx * 8) = pl[1];
                }
            }
        }
        // ---- g = dy masked by y > 0 (ReLU backward), times 2^kg, two fp16 planes; zeros outside the volume
        for (int base = tid; base < NCO * GN_CONV_TVOX * 8; base += NT * 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * NT;
                const int cb = idx / (GN_CONV_TVOX * 8), rm = idx % (GN_CONV_TVOX * 8);
                const int vv = rm >> 3, c4 = (rm & 7) * 4;
                const int gz = z0 + (vv >> 6), gy = y0 + ((vv >> 3) & 7), gx = x0 + (vv & 7);
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (idx < NCO * GN_CONV_TVOX * 8 && gz < p.D && gy < p.H && gx < p.W) {
                    const int64_t off = ((((int64_t)b * p.D + gz) * p.H + gy) * p.W + gx) * p.Cout + co0 + cb * 32 + c4;
                    float4 g = *reinterpret_cast<const float4 *>(p.dy + off);
                    if (p.y) {
                        const float4 yv = *reinterpret_cast<const float4 *>(p.y + off);
                        g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f; g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
                    }
                    v[u] = make_float4(__fmul_rn(g.x, sg), __fmul_rn(g.y, sg), __fmul_rn(g.z, sg), __fmul_rn(g.w, sg));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * NT;
                if (idx < NCO * GN_CONV_TVOX * 8) {
                    uint2 pl[2];
                    split4<2, true>(v[u].x, v[u].y, v[u].z, v[u].w, pl);
                    *reinterpret_cast<uint2 *>(gh + idx * 8) = pl[0];          // ([cb][voxel][32]: byte (cb * 256 + vv) * 64 + c4 * 2 = idx * 8)
                    *reinterpret_cast<uint2 *>(gl + idx * 8) = pl[1];
                }
            }
        }
        __syncthreads();
        // ---- 16 steps of 16 voxels: z = s >> 2, y = 2 (s & 3) + h, x = 0 .. 7 (the lane's two reads: x = 0..3 and 4..7)
#pragma unroll 2
        for (int s = 0; s < GN_CONV_TVOX / 16; ++s) {
            const int xo = ((s >> 2) * GN_CONV_HY + 2 * (s & 3)) * GN_CONV_HX * BWS_ROW, go = s * 16 * BWS_ROW;
            const uint2 g0 = bws_tr(lgh + go, 0), g1 = bws_tr(lgh + go, 4 * BWS_ROW);
            const uint2 e0 = bws_tr(lgl + go, 0), e1 = bws_tr(lgl + go, 4 * BWS_ROW);
            const uint4 ghi = make_uint4(g0.x, g0.y, g1.x, g1.y), glo = make_uint4(e0.x, e0.y, e1.x, e1.y);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int ko = ((k / 3) * GN_CONV_HX + (k % 3)) * BWS_ROW;
                const uint2 a0 = bws_tr(lxh + xo, ko), a1 = bws_tr(lxh + xo, ko + 4 * BWS_ROW);
                const uint2 c0 = bws_tr(lxl + xo, ko), c1 = bws_tr(lxl + xo, ko + 4 * BWS_ROW);
                const uint4 xhi = make_uint4(a0.x, a0.y, a1.x, a1.y), xlo = make_uint4(c0.x, c0.y, c1.x, c1.y);
                acc[k] = mfma16<true>(xlo, ghi, acc[k]);
                acc[k] = mfma16<true>(xhi, glo, acc[k]);
                acc[k] = mfma16<true>(xhi, ghi, acc[k]);
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

// dW[co][ci][tap] = (partials of chain 0, 1, 2, ... added in that order in fp64) * X * 2^-kg (exact), rounded once
__global__ __launch_bounds__(256) void conv3d_bwd_weight_split_fold_kernel(const float *__restrict__ part, const float *__restrict__ hdr, int chains, int Cin,
                                                                           int Cin32, int Cout, float *__restrict__ dw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)27 * Cin * Cout) return;
    const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), tap = (int)(i / ((int64_t)Cout * Cin));
    const int64_t stride = (int64_t)27 * Cin32 * Cout;
    const float *pp = part + ((int64_t)tap * Cin32 + ci) * Cout + co;
    double s = 0.0;
    for (int c = 0; c < chains; ++c) s += (double)pp[c * stride];
    dw[((int64_t)co * Cin + ci) * 27 + tap] = (float)(s * *reinterpret_cast<const double *>(hdr + 2));
}

extern "C" size_t gn_conv3d_bwd_weight_split_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cout % 32 != 0) return 0;
    return gn_carve_bytes(bws_ws, B, bws_chains(B, D, H, W, Cin, Cout, nullptr), Cin, Cout);
}

extern "C" int gn_conv3d_bwd_weight_split(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d, const float *x_inv,
                                          const float *y, const float *dy, const float *gmax, int B, int D, int H, int W, int Cout, void *ws,
                                          size_t ws_bytes, float *dw, void *stream) {
    GN_REQUIRE(B >= 0 && D > 0 && H > 0 && W > 0 && C0 > 0 && C1 >= 0 && Cout > 0, "gn_conv3d_bwd_weight_split: bad sizes");
    GN_REQUIRE(C0 % 4 == 0 && C1 % 4 == 0, "gn_conv3d_bwd_weight_split: channel counts must be multiples of 4 (C0=%d C1=%d)", C0, C1);
    GN_REQUIRE(Cout % 32 == 0, "gn_conv3d_bwd_weight_split: Cout=%d must be a multiple of 32", Cout);
    GN_REQUIRE(C1 == 0 || (D % 2 == 0 && H % 2 == 0 && W % 2 == 0), "gn_conv3d_bwd_weight_split: upsampled source needs even dims");
    GN_REQUIRE((int64_t)B * gn_cdiv(D, GN_CONV_TZ) * gn_cdiv(H, GN_CONV_TY) * gn_cdiv(W, GN_CONV_TX) < ((int64_t)1 << 30), "gn_conv3d_bwd_weight_split: volume too large");
    const int Cin = C0 + C1;
    const size_t need = gn_conv3d_bwd_weight_split_workspace_bytes(B, D, H, W, Cin, Cout);
    GN_REQUIRE(ws_bytes >= need, "gn_conv3d_bwd_weight_split: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    hipStream_t st = gn_stream(stream);
    if (B == 0) {
        GN_REQUIRE(dw != nullptr, "gn_conv3d_bwd_weight_split: null pointer");
        GN_HIP(hipMemsetAsync(dw, 0, (size_t)27 * Cin * Cout * sizeof(float), st), "gn_conv3d_bwd_weight_split");
        return GN_OK;
    }
    GN_REQUIRE(src0 && a && d && dy && gmax && dw && ws && (C1 == 0 || src1), "gn_conv3d_bwd_weight_split: null pointer");
    GN_REQUIRE(((uintptr_t)ws & 15) == 0, "gn_conv3d_bwd_weight_split: the workspace must be 16-byte aligned");
    BwsArgs p;
    const int chains = bws_chains(B, D, H, W, Cin, Cout, &p.per_chain);
    GnCarve c(ws);
    const auto [hdr, part] = bws_ws(c, B, chains, Cin, Cout);
    hipLaunchKernelGGL(bws_scales_kernel, dim3(1), dim3(64), 0, st, x_inv, gmax, B, hdr);
    GN_LAUNCH_CHECK("gn_conv3d_bwd_weight_split");
    p.src0 = src0; p.src1 = src1; p.a = a; p.d = d; p.y = y; p.dy = dy; p.hdr = hdr; p.part = part;
    p.C0 = C0; p.C1 = C1; p.B = B; p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.Cin32 = (int)gn_cdiv(Cin, BWS_CI) * BWS_CI;
    p.tiles_z = (int)gn_cdiv(D, GN_CONV_TZ); p.tiles_y = (int)gn_cdiv(H, GN_CONV_TY); p.tiles_x = (int)gn_cdiv(W, GN_CONV_TX);
    p.ntiles = B * p.tiles_z * p.tiles_y * p.tiles_x;
    const int nco = Cout % 64 == 0 ? 2 : 1;
    const size_t lds = (size_t)2 * BWS_HALO_BYTES + (size_t)2 * nco * BWS_G_BYTES;
    const dim3 grid((unsigned)((p.Cin32 / BWS_CI) * (Cout / (32 * nco))), (unsigned)chains);
    if (nco == 2) {
        GN_HIP(hipFuncSetAttribute((const void *)conv3d_bwd_weight_split_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gn_conv3d_bwd_weight_split");
        hipLaunchKernelGGL(conv3d_bwd_weight_split_kernel<2>, grid, dim3(384), lds, st, p);
    } else {
        GN_HIP(hipFuncSetAttribute((const void *)conv3d_bwd_weight_split_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "gn_conv3d_bwd_weight_split");
        hipLaunchKernelGGL(conv3d_bwd_weight_split_kernel<1>, grid, dim3(192), lds, st, p);
    }
    GN_LAUNCH_CHECK("gn_conv3d_bwd_weight_split");
    const int64_t n = (int64_t)27 * Cin * Cout;
    hipLaunchKernelGGL(conv3d_bwd_weight_split_fold_kernel, dim3((unsigned)gn_cdiv(n, 256)), dim3(256), 0, st, (const float *)p.part, (const float *)hdr, chains,
                       Cin, p.Cin32, Cout, dw);
    GN_LAUNCH_CHECK("gn_conv3d_bwd_weight_split");
    return GN_OK;
}

// weight_pack.hip -- the STATIC split-operand weight packs of the UNet's 3x3x3 convolutions, built on the device from the raw Conv3d weight
// [Cout][Cin][3][3][3]: gn_weight_pack_split (the direct kernels' pack, csrc/unet_split.hip), gn_weight_pack_split_wino (the Winograd F(2,3)-along-x
// pack, csrc/unet_wino.hip / unet_wino32.hip) and gn_weight_pack_upconv (the polyphase pack of csrc/upconv.hip).
//
// Why: the host builders (garmentnets_amd.ops.pack_conv_weight_split, pack_conv_weight_split_wino, polyphase_weights + pack_upconv_weight) copy the
// weight to the CPU -- a stream synchronisation -- transform it in torch and upload the result.  Inference does that once per model; training after every
// optimiser step, about a dozen times per step.  These kernels produce the same bits without a host round trip (tests/test_gpu_weight_pack.py), so a
// training step's forward stays on the stream.  The per-sample affine-in-weights packs have always been built on the device (conv_prep.hip).
//
// One workgroup per output row (polyphase: per row and parity class): the row maximum through the wave reductions of device_prims.h, then one thread per
// 16-byte fragment piece -- 8 input channels of one output channel, every plane.  The transformed (Winograd) and the merged (polyphase) weights exist in
// registers only.  The work is a few MB per layer: nothing here is tuned beyond that.
//
// Row scale (f16x2): 2^k with k from the EXPONENT FIELD of the row maximum m (frexp), m 2^k in [1, 2); 1 for a zero or non-finite maximum; k clamped to
// +-100 as conv_prep.hip's scales.  That is what the host builders document.  What they compute is exp2(-floor(log2(m))), and log2 rounds up to the
// integer for m a few ulps below a power of two (fp32: the first two ulps below 2^-4, the first four below 2^-10): there the host leaves the row maximum
// in [0.5, 1) and its out_scale is twice this file's.  Both are exact decompositions that out_scale undoes; everywhere else the two agree bit for bit.
#include "common.h"

#define WPACK_THREADS 256

// k of the row scale 2^k from the row maximum m
__device__ __forceinline__ int wpack_scale_exp(float m) {
    if (!(m > 0.f && m < INFINITY)) return 0;
    int e = 0;
    (void)frexpf(m, &e);                            // m = f 2^e, f in [0.5, 1)
    e = 1 - e;
    return e > 100 ? 100 : e < -100 ? -100 : e;
}

// max over the workgroup (WPACK_THREADS threads, all of them here), in every thread
__device__ __forceinline__ float wpack_block_max(float v) {
    __shared__ float wmax[WPACK_THREADS / GN_WAVE];
    const float m = gn_wave_max(v);
    if ((threadIdx.x & (GN_WAVE - 1)) == 0) wmax[threadIdx.x / GN_WAVE] = m;
    __syncthreads();
    return fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// eight fp32 values -> P planes of 8 x 16 bit (residual chain p = rn(r), r -= float(p); round to nearest even), one 16-byte store per plane,
// `stride` uint4 apart
template <int P, bool F16>
__device__ __forceinline__ void wpack_store8(float (&v)[8], uint4 *dst, int stride) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (F16) {
            f16x8 q;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                q[i] = (_Float16)v[i];
                v[i] = __fsub_rn(v[i], (float)q[i]);
            }
            dst[p * stride] = __builtin_bit_cast(uint4, q);
        } else {
            bf16x8 q;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                q[i] = (__bf16)v[i];
                v[i] = __fsub_rn(v[i], (float)q[i]);
            }
            dst[p * stride] = __builtin_bit_cast(uint4, q);
        }
    }
}

// zero steps behind the last slice (the conv kernels' fragment DMA runs ahead of the last step): row n's lanes of `steps` steps of P planes
template <int P>
__device__ __forceinline__ void wpack_zero_steps(uint4 *pack, int64_t first_step, int steps, int nblk, int blk, int r) {
    for (int it = threadIdx.x; it < steps * P * 2; it += WPACK_THREADS) {
        const int z = it / (P * 2), ph = it % (P * 2);
        pack[(((first_step + z) * nblk + blk) * (P * 2) + ph) * 32 + r] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// (a) the direct pack [c_n/16][27][Cout/32][P][h 2][r 32][8] + eight zero steps, of input channels [c_lo, c_lo + c_n).  SCALED: fp16 planes of w 2^k(row)
template <int P, bool F16, bool SCALED>
__global__ __launch_bounds__(WPACK_THREADS) void wpack_direct_kernel(const float *__restrict__ w, int Cin, int Cout, int c_lo, int c_n,
                                                                     uint4 *__restrict__ pack, float *__restrict__ out_scale) {
    const int n = blockIdx.x, blk = n >> 5, r = n & 31, nblk = Cout / 32, nsl = c_n / 16;
    const float *wr = w + ((int64_t)n * Cin + c_lo) * 27;
    int k = 0;
    if (SCALED) {
        float mx = 0.f;
        for (int i = threadIdx.x; i < c_n * 27; i += WPACK_THREADS) mx = fmaxf(mx, fabsf(wr[i]));
        k = wpack_scale_exp(wpack_block_max(mx));
    }
    const float rs = ldexpf(1.f, k);
    if (threadIdx.x == 0) out_scale[n] = ldexpf(1.f, -k);
    for (int it = threadIdx.x; it < nsl * 2 * 27; it += WPACK_THREADS) {
        const int tap = it % 27, sh = it / 27, h = sh & 1, S = sh >> 1;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __fmul_rn(wr[(S * 16 + 8 * h + i) * 27 + tap], rs);
        wpack_store8<P, F16>(v, pack + ((((int64_t)S * 27 + tap) * nblk + blk) * (P * 2) + h) * 32 + r, 64);
    }
    wpack_zero_steps<P>(pack, (int64_t)nsl * 27, 8, nblk, blk, r);
}

// the four Winograd F(2,3) positions of the taps (g0, g1, g2) along x, in fp64
__device__ __forceinline__ double wpack_wino_u(const float *g, int j) {
    const double g0 = (double)g[0], g1 = (double)g[1], g2 = (double)g[2];
    return j == 0 ? g0 : j == 1 ? 0.5 * (g0 + g1 + g2) : j == 2 ? 0.5 * (g0 - g1 + g2) : g2;
}

// (b) the Winograd pack [c_n/16][36 steps = (j * 3 + kd) * 3 + kh][Cout/32][2][h][r][8] + six zero steps: transform in fp64, row scale over the TRANSFORMED
// row, one rounding to fp32 after scaling, two fp16 planes.  The row maximum travels as fp32 rounded TOWARDS ZERO: the exponent of the fp64 maximum itself
// (round-to-nearest could carry a maximum just below a power of two over it)
__global__ __launch_bounds__(WPACK_THREADS) void wpack_wino_kernel(const float *__restrict__ w, int Cin, int Cout, int c_lo, int c_n,
                                                                   uint4 *__restrict__ pack, float *__restrict__ out_scale) {
    const int n = blockIdx.x, blk = n >> 5, r = n & 31, nblk = Cout / 32, nsl = c_n / 16;
    const float *wr = w + ((int64_t)n * Cin + c_lo) * 27;
    float mx = 0.f;
    for (int i = threadIdx.x; i < c_n * 9; i += WPACK_THREADS) {
        const float *g = wr + 3 * i;
        const double m = fmax(fmax(fabs((double)g[0]), fabs((double)g[2])), fmax(fabs(wpack_wino_u(g, 1)), fabs(wpack_wino_u(g, 2))));
        mx = fmaxf(mx, __double2float_rz(m));
    }
    const int k = wpack_scale_exp(wpack_block_max(mx));
    const double rs = ldexp(1.0, k);
    if (threadIdx.x == 0) out_scale[n] = ldexpf(1.f, -k);
    for (int it = threadIdx.x; it < nsl * 2 * 36; it += WPACK_THREADS) {
        const int step = it % 36, sh = it / 36, h = sh & 1, S = sh >> 1;
        const int j = step / 9, kdh = step % 9;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)(wpack_wino_u(wr + (S * 16 + 8 * h + i) * 27 + kdh * 3, j) * rs);
        wpack_store8<2, true>(v, pack + ((((int64_t)S * 36 + step) * nblk + blk) * 4 + h) * 32 + r, 64);
    }
    wpack_zero_steps<2>(pack, (int64_t)nsl * 36, 6, nblk, blk, r);
}

// coarse tap t = 4 iz + 2 iy + ix of parity class cls = 4 pz + 2 py + px, merged from the 27 fine taps wk [3][3][3] of one (output, input) channel pair: a
// fine tap d in {-1, 0, +1} of an even voxel lands on coarse offset {-1, 0, 0}, of an odd voxel on {0, 0, +1}, so per axis (p, i) collects the fine taps
// (0, 0): {0}   (0, 1): {1, 2}   (1, 0): {0, 1}   (1, 1): {2}.  Up to 8 weights summed in fp64, rounded to fp32 once
__device__ __forceinline__ float wpack_merged_tap(const float *wk, int cls, int t) {
    const int pz = cls >> 2, py = (cls >> 1) & 1, px = cls & 1, iz = t >> 2, iy = (t >> 1) & 1, ix = t & 1;
    const int z0 = iz ? 1 + pz : 0, z1 = iz ? 2 : pz, y0 = iy ? 1 + py : 0, y1 = iy ? 2 : py, x0 = ix ? 1 + px : 0, x1 = ix ? 2 : px;
    double acc = 0.0;
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) acc += (double)wk[(z * 3 + y) * 3 + x];
    return (float)acc;
}

// (c) the polyphase pack [C1/16][tap 8][class 8][Cout/32][2][h][r][8] of input channels [c0, Cin): one workgroup per (output row, class), its scale over
// the class's 8 merged taps of the row
template <bool F16>
__global__ __launch_bounds__(WPACK_THREADS) void wpack_upconv_kernel(const float *__restrict__ w, int Cin, int Cout, int c0, uint4 *__restrict__ pack,
                                                                     float *__restrict__ out_scale) {
    const int n = blockIdx.x, cls = blockIdx.y, blk = n >> 5, r = n & 31, nblk = Cout / 32, C1 = Cin - c0, nsl = C1 / 16;
    const float *wr = w + ((int64_t)n * Cin + c0) * 27;
    int k = 0;
    if (F16) {
        float mx = 0.f;
        for (int i = threadIdx.x; i < C1 * 8; i += WPACK_THREADS) mx = fmaxf(mx, fabsf(wpack_merged_tap(wr + (i >> 3) * 27, cls, i & 7)));
        k = wpack_scale_exp(wpack_block_max(mx));
    }
    const float rs = ldexpf(1.f, k);
    if (threadIdx.x == 0) out_scale[cls * Cout + n] = ldexpf(1.f, -k);
    for (int it = threadIdx.x; it < nsl * 2 * 8; it += WPACK_THREADS) {
        const int t = it & 7, sh = it >> 3, h = sh & 1, S = sh >> 1;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __fmul_rn(wpack_merged_tap(wr + (S * 16 + 8 * h + i) * 27, cls, t), rs);
        wpack_store8<2, F16>(v, pack + (((((int64_t)S * 8 + t) * 8 + cls) * nblk + blk) * 4 + h) * 32 + r, 64);
    }
}

static int wpack_planes(int mode) { return mode == GN_SPLIT_BF16X3 ? 3 : (mode == GN_SPLIT_BF16X2 || mode == GN_SPLIT_F16X2) ? 2 : 0; }

extern "C" size_t gn_weight_pack_split_bytes(int c_n, int Cout, int mode) {
    if (c_n <= 0 || Cout <= 0 || c_n % 16 || Cout % 32 || !wpack_planes(mode)) return 0;
    return ((size_t)(c_n / 16) * 27 + 8) * (Cout / 32) * wpack_planes(mode) * 1024;
}

extern "C" size_t gn_weight_pack_split_wino_bytes(int c_n, int Cout) {
    if (c_n <= 0 || Cout <= 0 || c_n % 16 || Cout % 32) return 0;
    return ((size_t)(c_n / 16) * 36 + 6) * (Cout / 32) * 2 * 1024;
}

extern "C" size_t gn_weight_pack_upconv_bytes(int C1, int Cout) {
    if (C1 <= 0 || Cout <= 0 || C1 % 16 || Cout % 32) return 0;
    return (size_t)(C1 / 16) * 64 * (Cout / 32) * 2 * 1024;
}

// the checks the three entries share: widths, the channel range inside the weight, buffers
static int wpack_check(const char *who, const float *w, int Cout, int Cin, int c_lo, int c_n, const void *pack, size_t pack_bytes, size_t need,
                       const float *out_scale) {
    GN_REQUIRE(Cout > 0 && Cin > 0 && c_n > 0 && c_n % 16 == 0 && Cout % 32 == 0, "%s: channels must be multiples of 16 (in) / 32 (out), got %d / %d", who,
               c_n, Cout);
    GN_REQUIRE(c_lo >= 0 && c_lo <= Cin - c_n, "%s: input channels [%d, %d) outside the weight's %d", who, c_lo, c_lo + c_n, Cin);
    GN_REQUIRE(w && pack && out_scale, "%s: null pointer", who);
    GN_REQUIRE(((uintptr_t)pack & 15) == 0, "%s: pack must be 16-byte aligned", who);
    GN_REQUIRE(pack_bytes >= need, "%s: pack buffer too small (%zu < %zu)", who, pack_bytes, need);
    return GN_OK;
}

extern "C" int gn_weight_pack_split(const float *w, int Cout, int Cin, int c_lo, int c_n, int mode, void *pack, size_t pack_bytes, float *out_scale,
                                    void *stream) {
    GN_REQUIRE(wpack_planes(mode), "gn_weight_pack_split: unknown split mode %d", mode);
    const int rc = wpack_check("gn_weight_pack_split", w, Cout, Cin, c_lo, c_n, pack, pack_bytes, gn_weight_pack_split_bytes(c_n, Cout, mode), out_scale);
    if (rc != GN_OK) return rc;
    hipStream_t st = gn_stream(stream);
    const dim3 grid((unsigned)Cout), block(WPACK_THREADS);
    if (mode == GN_SPLIT_F16X2) hipLaunchKernelGGL((wpack_direct_kernel<2, true, true>), grid, block, 0, st, w, Cin, Cout, c_lo, c_n, (uint4 *)pack, out_scale);
    else if (mode == GN_SPLIT_BF16X2) hipLaunchKernelGGL((wpack_direct_kernel<2, false, false>), grid, block, 0, st, w, Cin, Cout, c_lo, c_n, (uint4 *)pack, out_scale);
    else hipLaunchKernelGGL((wpack_direct_kernel<3, false, false>), grid, block, 0, st, w, Cin, Cout, c_lo, c_n, (uint4 *)pack, out_scale);
    GN_LAUNCH_CHECK("gn_weight_pack_split");
    return GN_OK;
}

extern "C" int gn_weight_pack_split_wino(const float *w, int Cout, int Cin, int c_lo, int c_n, void *pack, size_t pack_bytes, float *out_scale,
                                         void *stream) {
    const int rc = wpack_check("gn_weight_pack_split_wino", w, Cout, Cin, c_lo, c_n, pack, pack_bytes, gn_weight_pack_split_wino_bytes(c_n, Cout), out_scale);
    if (rc != GN_OK) return rc;
    hipLaunchKernelGGL(wpack_wino_kernel, dim3((unsigned)Cout), dim3(WPACK_THREADS), 0, gn_stream(stream), w, Cin, Cout, c_lo, c_n, (uint4 *)pack, out_scale);
    GN_LAUNCH_CHECK("gn_weight_pack_split_wino");
    return GN_OK;
}

extern "C" int gn_weight_pack_upconv(const float *w, int Cout, int Cin, int c0, int mode, void *pack, size_t pack_bytes, float *out_scale, void *stream) {
    GN_REQUIRE(mode == GN_SPLIT_F16X2 || mode == GN_SPLIT_BF16X2, "gn_weight_pack_upconv: the two-plane modes only, got %d", mode);
    GN_REQUIRE(c0 >= 0 && c0 < Cin, "gn_weight_pack_upconv: split point %d outside the weight's %d input channels", c0, Cin);
    const int rc = wpack_check("gn_weight_pack_upconv", w, Cout, Cin, c0, Cin - c0, pack, pack_bytes, gn_weight_pack_upconv_bytes(Cin - c0, Cout), out_scale);
    if (rc != GN_OK) return rc;
    hipStream_t st = gn_stream(stream);
    const dim3 grid((unsigned)Cout, 8u), block(WPACK_THREADS);
    if (mode == GN_SPLIT_F16X2) hipLaunchKernelGGL(wpack_upconv_kernel<true>, grid, block, 0, st, w, Cin, Cout, c0, (uint4 *)pack, out_scale);
    else hipLaunchKernelGGL(wpack_upconv_kernel<false>, grid, block, 0, st, w, Cin, Cout, c0, (uint4 *)pack, out_scale);
    GN_LAUNCH_CHECK("gn_weight_pack_upconv");
    return GN_OK;
}

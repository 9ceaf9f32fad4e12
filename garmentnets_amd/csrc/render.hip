// render.hip -- the training monitors' images: the z-buffered point splat of the reference's common/rendering_util.py and its colouring, every image of
// a batch in one launch each.
//
//   gn_render_points_batch   fp32 points -> uint32 index images: per pixel the index of the covering point nearest to the camera
//   gn_color_idx_batch       index images -> fp32 RGBA: a colour table or a scalar through viridis, the default colour elsewhere, then the overlay points
//
// The definitions ("Training monitors"; garmentnets_amd/visualize.py restates them in numpy, operation for operation):
//   camera     side 0 'front' (x, 1 - z, y), 1 'top' (x, 1 - y, 1 - z), 2 'left' (1 - y, 1 - z, x): cam[j] = sign_j * double(p[axis_j]) + t_j, one fp64
//              rounding per coordinate.  A point with a non-finite coordinate is not drawn.
//   pixel      clamp(trunc(cam * (S - 1)), 0, S - 1) in fp64: x from cam[0], y from cam[1]
//   footprint  off = -(k / 2); the point at (x, y) covers X in [max(x + off, 0), min(x + off + k - 1, S - 1)], and Y likewise
//   winner     the covering point with the smallest cam[2] (fp64); equal depths: the lowest index (the serial strict-< scan); +inf and NaN never win;
//              a pixel nobody covers holds 0xFFFFFFFF.  Indices count from the start of the image's own segment.
//
// Shape of the splat: a workgroup of 256 threads owns a 16 x 16 pixel tile of one image (blockIdx.z), a thread one pixel with (best_z, best_idx) in
// registers.  The image's points stream through LDS in tiles of 256: each staging thread does the camera transform and the footprint of ONE point, the
// points whose footprint misses the pixel tile are dropped there (ballot + popcount prefix inside a wave, the four wave counts through LDS: the kept
// points stay in ascending index), and in the scan every lane reads the same staged point (an LDS broadcast).  A pixel is written once by its owner:
// no atomics, so the image is a pure function of (points, side, k, S), whatever else the launch carries.
#include <math.h>

#include "common.h"
#include "viridis_lut.h"

#define RD_TILE 16
#define RD_BLOCK (RD_TILE * RD_TILE)
#define RD_WAVES (RD_BLOCK / GN_WAVE)
#define RD_NONE 0xFFFFFFFFu

// cam = (c[0], c[1], c[2]) of the fp32 point p seen from `side`; false: a non-finite coordinate or an unknown side (never drawn)
__device__ __forceinline__ bool rd_camera(const float *__restrict__ p, int side, double (&c)[3]) {
    const float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    if (side == 0) { c[0] = dx; c[1] = __dadd_rn(-dz, 1.0); c[2] = dy; }
    else if (side == 1) { c[0] = dx; c[1] = __dadd_rn(-dy, 1.0); c[2] = __dadd_rn(-dz, 1.0); }
    else if (side == 2) { c[0] = __dadd_rn(-dy, 1.0); c[1] = __dadd_rn(-dz, 1.0); c[2] = dx; }
    else return false;
    return true;
}

// clamp(trunc(c * (S - 1)), 0, S - 1) for a finite c
__device__ __forceinline__ int rd_pixel(double c, int S) {
    const double t = __dmul_rn(c, (double)(S - 1));
    return t <= 0.0 ? 0 : (t >= (double)(S - 1) ? S - 1 : (int)t);
}

// the covered interval [lo, hi] of a point at pixel coordinate v (0 <= v < S) under a k-wide footprint
__device__ __forceinline__ void rd_span(int v, int k, int S, int &lo, int &hi) {
    const int a = v - k / 2;
    lo = a < 0 ? 0 : a;
    hi = a + k - 1 > S - 1 ? S - 1 : a + k - 1;
}

// tab: per image (first point, end point, side, k) as int64
__global__ __launch_bounds__(RD_BLOCK) void render_points_batch_kernel(const float *__restrict__ points, const int64_t *__restrict__ tab, int S,
                                                                       uint32_t *__restrict__ out) {
    __shared__ double sz[RD_BLOCK];
    __shared__ uint32_t sx[RD_BLOCK], sy[RD_BLOCK], si[RD_BLOCK];       // (lo | hi << 16) of x and of y (S <= 4096), the point's index
    __shared__ int scnt[RD_WAVES];
    const int64_t *im = tab + 4 * (int64_t)blockIdx.z;
    const int64_t begin = im[0], end = im[1];
    const int side = (int)im[2], k = (int)im[3];
    const int tid = threadIdx.x, lane = tid & (GN_WAVE - 1), wave = tid / GN_WAVE;
    const int tx0 = blockIdx.x * RD_TILE, ty0 = blockIdx.y * RD_TILE;
    const int X = tx0 + (tid & (RD_TILE - 1)), Y = ty0 + tid / RD_TILE;
    double best = INFINITY;
    uint32_t best_idx = RD_NONE;
    for (int64_t c0 = begin; c0 < end; c0 += RD_BLOCK) {                 // block-uniform bounds: every thread reaches every barrier
        const int64_t j = c0 + tid;
        bool hit = false;
        double c[3];
        int xlo = 0, xhi = 0, ylo = 0, yhi = 0;
        if (j < end && rd_camera(points + 3 * j, side, c)) {
            rd_span(rd_pixel(c[0], S), k, S, xlo, xhi);
            rd_span(rd_pixel(c[1], S), k, S, ylo, yhi);
            hit = xlo <= tx0 + RD_TILE - 1 && xhi >= tx0 && ylo <= ty0 + RD_TILE - 1 && yhi >= ty0;
        }
        const unsigned long long mask = __ballot(hit);
        __syncthreads();                                                 // the previous tile's scan is over: the stage may be overwritten
        if (lane == 0) scnt[wave] = __popcll(mask);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RD_WAVES; ++w) {
            const int n = scnt[w];
            base += w < wave ? n : 0;
            total += n;
        }
        if (hit) {
            const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
            sz[slot] = c[2];
            sx[slot] = (uint32_t)xlo | ((uint32_t)xhi << 16);
            sy[slot] = (uint32_t)ylo | ((uint32_t)yhi << 16);
            si[slot] = (uint32_t)(j - begin);
        }
        __syncthreads();
        for (int s = 0; s < total; ++s) {                                // ascending index: a strict < keeps the first of equal depths
            const uint32_t px = sx[s], py = sy[s];
            const double z = sz[s];
            const bool in = X >= (int)(px & 0xffffu) && X <= (int)(px >> 16) && Y >= (int)(py & 0xffffu) && Y <= (int)(py >> 16);
            if (in && z < best) { best = z; best_idx = si[s]; }
        }
    }
    if (X < S && Y < S) out[((int64_t)blockIdx.z * S + Y) * S + X] = best_idx;
}

// ------------------------------------------------------------------------------------------------ colour
static __device__ const uint32_t rd_viridis[VIRIDIS_LUT_ENTRIES * 3] = VIRIDIS_LUT_BITS;

// matplotlib's Colormap.__call__ on float32: v = (x - lo) / (hi - lo), u = v * 256; entry trunc(u) (u == 256 -> 255), under -> 0, over -> 255, NaN -> 0 0 0 0
__device__ __forceinline__ float4 rd_viridis_of(float x, float lo, float hi) {
    const float u = __fmul_rn(__fdiv_rn(__fsub_rn(x, lo), __fsub_rn(hi, lo)), 256.f);
    if (u != u) return make_float4(0.f, 0.f, 0.f, 0.f);
    const int e = u < 0.f ? 0 : (u >= 256.f ? 255 : (int)u);
    return make_float4(__uint_as_float(rd_viridis[3 * e]), __uint_as_float(rd_viridis[3 * e + 1]), __uint_as_float(rd_viridis[3 * e + 2]), 1.f);
}

__global__ __launch_bounds__(256) void color_idx_batch_kernel(const uint32_t *__restrict__ idx_img, const GnColorImage *__restrict__ tab,
                                                              const float *__restrict__ colors, const float *__restrict__ values, int S,
                                                              float *__restrict__ out) {
    const GnColorImage &im = tab[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const int X = pix % S, Y = pix / S;
    const int64_t o = (int64_t)blockIdx.y * S * S + pix;
    const uint32_t idx = idx_img[o];
    float4 col = make_float4(im.default_color[0], im.default_color[1], im.default_color[2], im.default_color[3]);
    if (idx != RD_NONE && (int64_t)idx < im.count) {
        if (im.mode == GN_COLOR_TABLE) col = *reinterpret_cast<const float4 *>(colors + 4 * (im.offset + idx));
        else col = rd_viridis_of(values[im.offset + idx], im.vmin, im.vmax);
    }
    for (int v = 0; v < im.num_overlays; ++v) {                          // overlay_grip: a one-point image of this footprint, copied where its alpha > 0
        const GnOverlayPoint &g = im.overlay[v];
        double c[3];
        if (!(g.rgba[3] > 0.f) || !rd_camera(g.xyz, im.side, c) || !(c[2] < INFINITY)) continue;
        int xlo, xhi, ylo, yhi;
        rd_span(rd_pixel(c[0], S), g.kernel_size, S, xlo, xhi);
        rd_span(rd_pixel(c[1], S), g.kernel_size, S, ylo, yhi);
        if (X >= xlo && X <= xhi && Y >= ylo && Y <= yhi) col = make_float4(g.rgba[0], g.rgba[1], g.rgba[2], g.rgba[3]);
    }
    *reinterpret_cast<float4 *>(out + 4 * o) = col;
}

// ------------------------------------------------------------------------------------------------ C ABI
static int rd_check_size(const char *who, int I, int S) {
    GN_REQUIRE(S >= 1 && S <= GN_RENDER_MAX_SIZE, "%s: image size S=%d outside [1, %d]", who, S, GN_RENDER_MAX_SIZE);
    GN_REQUIRE(I >= 0 && I <= 65535, "%s: I=%d images outside [0, 65535]", who, I);
    return GN_OK;
}

extern "C" int gn_render_points_batch(const float *points, const int64_t *seg_host, const int32_t *side_host, const int32_t *kernel_size_host,
                                      const int64_t *tab, int I, int S, uint32_t *out, void *stream) {
    const int rc = rd_check_size("gn_render_points_batch", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(seg_host && side_host && kernel_size_host && tab && out, "gn_render_points_batch: null pointer");
    for (int i = 0; i < I; ++i) {
        const int64_t n = seg_host[i + 1] - seg_host[i];
        GN_REQUIRE(seg_host[i] >= 0 && n >= 0, "gn_render_points_batch: image %d: seg is not a non-decreasing CSR", i);
        GN_REQUIRE(n < (int64_t)RD_NONE, "gn_render_points_batch: image %d: a segment of %lld points (needs fewer than 2^32 - 1)", i, (long long)n);
        GN_REQUIRE(side_host[i] >= 0 && side_host[i] <= 2, "gn_render_points_batch: image %d: side=%d outside {0 front, 1 top, 2 left}", i, side_host[i]);
        GN_REQUIRE(kernel_size_host[i] >= 1 && kernel_size_host[i] <= S, "gn_render_points_batch: image %d: kernel_size k=%d outside [1, S=%d]", i,
                   kernel_size_host[i], S);
    }
    GN_REQUIRE(seg_host[I] == 0 || points, "gn_render_points_batch: null points");
    const unsigned tiles = (unsigned)gn_cdiv(S, RD_TILE);
    hipLaunchKernelGGL(render_points_batch_kernel, dim3(tiles, tiles, (unsigned)I), dim3(RD_BLOCK), 0, gn_stream(stream), points, tab, S, out);
    GN_LAUNCH_CHECK("gn_render_points_batch");
    return GN_OK;
}

extern "C" int gn_color_idx_batch(const uint32_t *idx_img, const GnColorImage *tab_host, const GnColorImage *tab, const float *colors, const float *values,
                                  int I, int S, float *out, void *stream) {
    const int rc = rd_check_size("gn_color_idx_batch", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(idx_img && tab_host && tab && out, "gn_color_idx_batch: null pointer");
    for (int i = 0; i < I; ++i) {
        const GnColorImage &g = tab_host[i];
        GN_REQUIRE(g.mode == GN_COLOR_TABLE || g.mode == GN_COLOR_VIRIDIS, "gn_color_idx_batch: image %d: unknown mode %d", i, g.mode);
        GN_REQUIRE(g.offset >= 0 && g.count >= 0, "gn_color_idx_batch: image %d: bad offset / count", i);
        GN_REQUIRE(g.count == 0 || (g.mode == GN_COLOR_TABLE ? colors : values) != nullptr, "gn_color_idx_batch: image %d: null colour source", i);
        GN_REQUIRE(g.side >= 0 && g.side <= 2, "gn_color_idx_batch: image %d: side=%d outside {0 front, 1 top, 2 left}", i, g.side);
        GN_REQUIRE(g.num_overlays >= 0 && g.num_overlays <= GN_RENDER_MAX_OVERLAYS, "gn_color_idx_batch: image %d: %d overlays (at most %d)", i,
                   g.num_overlays, GN_RENDER_MAX_OVERLAYS);
        for (int v = 0; v < g.num_overlays; ++v)
            GN_REQUIRE(g.overlay[v].kernel_size >= 1 && g.overlay[v].kernel_size <= S,
                       "gn_color_idx_batch: image %d: overlay %d: kernel_size k=%d outside [1, S=%d]", i, v, g.overlay[v].kernel_size, S);
    }
    hipLaunchKernelGGL(color_idx_batch_kernel, dim3((unsigned)gn_cdiv((int64_t)S * S, 256), (unsigned)I), dim3(256), 0, gn_stream(stream), idx_img, tab,
                       colors, values, S, out);
    GN_LAUNCH_CHECK("gn_color_idx_batch");
    return GN_OK;
}

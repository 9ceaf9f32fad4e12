// render.hip -- the training monitors' images: the z-buffered point splat of the reference's common/rendering_util.py and its colouring, every image of
// a batch in one launch each; below them the evaluation's mesh images, a triangle rasteriser behind the same camera ("mesh images"), and below those
// the dataset's input clouds, the same rasteriser behind a perspective camera and a compaction of its covered pixels ("point clouds from meshes").
//
//   gn_render_points_batch  fp32 points -> uint32 index images: per pixel the index of the covering point nearest to the camera
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

// The ballot compaction of a stage: -> this thread's slot among the block's kept items (kept: hit), which stay in ascending thread order; total: how many
// are kept.  It CONTAINS TWO __syncthreads(), so every thread of the block calls it, whatever its hit: the first ends the previous tile's scan (after it
// the stage may be overwritten), the second publishes the wave counts.  The caller writes its slot and places the third barrier before it scans.
__device__ __forceinline__ int rd_compact(bool hit, int lane, int wave, int (&scnt)[RD_WAVES], int &total) {
    const unsigned long long mask = __ballot(hit);
    __syncthreads();
    if (lane == 0) scnt[wave] = __popcll(mask);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < RD_WAVES; ++w) {
        const int n = scnt[w];
        base += w < wave ? n : 0;
        total += n;
    }
    return base + __popcll(mask & ((1ull << lane) - 1ull));
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
        int total;
        const int slot = rd_compact(hit, lane, wave, scnt, total);       // (two barriers inside)
        if (hit) {
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

// ------------------------------------------------------------------------------------------------ mesh images
//   gn_render_mesh_batch     fp32 vertices + int32 faces -> uint32 index images: per pixel the index of the covering face nearest to the camera
//   gn_color_mesh_batch      index images -> fp32 RGBA: the barycentric mix of the face's vertex colours times a headlight shade, the default colour elsewhere
//
// The definitions ("Mesh images"; visualize.py restates them in numpy, operation for operation):
//   screen     u = cam[0] * (S - 1), v = cam[1] * (S - 1) in fp64 (rd_camera, as the splat); fixed point fx = rint(u * 256), fy = rint(v * 256), half to
//              even; pixel (X, Y) is sampled at (256 X + 128, 256 Y + 128)
//   not drawn  a vertex index outside [0, V), a non-finite coordinate, |fx| or |fy| > 2^24 at a vertex, area2 == 0
//   two-sided  area2 = (bx - ax)(cy - ay) - (by - ay)(cx - ax) in int64; area2 < 0: b and c swap, with their depths and colours
//   coverage   w_a = E(b, c, p), w_b = E(c, a, p), w_c = E(a, b, p), E(p, q, r) = (qx - px)(ry - py) - (qy - py)(rx - px); covered iff every w is > 0,
//              or == 0 on an edge d = q - p with dy > 0 or (dy == 0 and dx < 0): a sample on a shared edge belongs to exactly one of its two faces
//   depth      z = ((w_a z_a + w_b z_b) + w_c z_c) / area2 in fp64, every operation rounded on its own
//   winner     the smallest z; equal depths: the lowest face index (strict < in ascending order); nobody: 0xFFFFFFFF
// Every product has factors below 2^26, so the int64 values stay below 2^53 and convert to fp64 exactly.
//
// Shape: the splat's.  A workgroup owns a 16 x 16 tile, a thread one pixel; the faces stream through LDS in tiles of 256, one face per staging thread
// (gather, camera, fixed point, the pixels whose samples lie in its bounding box), the ones that miss the tile dropped by the same ballot compaction.
struct MrFace {
    int x[3], y[3], v[3];                                                 // fixed-point screen coordinates and vertex indices, a b c after the swap
    double z[3];
    double cam[3][3];
};

// rint(c * (S - 1) * 256) as an int; false beyond 2^24 in magnitude
__device__ __forceinline__ bool mr_fixed(double c, int S, int &f) {
    const double r = rint(__dmul_rn(__dmul_rn(c, (double)(S - 1)), 256.0));
    if (!(fabs(r) <= 16777216.0)) return false;
    f = (int)r;
    return true;
}

// E(p, q, r): every difference fits an int, every product an int64
__device__ __forceinline__ long long mr_edge(int px, int py, int qx, int qy, int rx, int ry) {
    return (long long)(qx - px) * (long long)(ry - py) - (long long)(qy - py) * (long long)(rx - px);
}

// the directed edge p -> q owns the samples on it
__device__ __forceinline__ bool mr_owns(int px, int py, int qx, int qy) {
    const int dx = qx - px, dy = qy - py;
    return dy > 0 || (dy == 0 && dx < 0);
}

// the positive orientation of a face whose x, y, v, z and cam are filled in: area2 < 0 swaps b and c with everything they carry; false: area2 == 0
__device__ __forceinline__ bool mr_orient(MrFace &f) {
    const long long area2 = mr_edge(f.x[0], f.y[0], f.x[1], f.y[1], f.x[2], f.y[2]);
    if (area2 == 0) return false;
    if (area2 < 0) {
        int t = f.x[1]; f.x[1] = f.x[2]; f.x[2] = t;
        t = f.y[1]; f.y[1] = f.y[2]; f.y[2] = t;
        t = f.v[1]; f.v[1] = f.v[2]; f.v[2] = t;
        double d = f.z[1]; f.z[1] = f.z[2]; f.z[2] = d;
#pragma unroll
        for (int j = 0; j < 3; ++j) { d = f.cam[1][j]; f.cam[1][j] = f.cam[2][j]; f.cam[2][j] = d; }
    }
    return true;
}

// the face `idx` (three indices into the V vertices at `verts`) in positive orientation; false: never drawn
__device__ __forceinline__ bool mr_face(const float *__restrict__ verts, int64_t V, const int32_t *__restrict__ idx, int side, int S, MrFace &f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int v = idx[k];
        if (v < 0 || (int64_t)v >= V) return false;
        if (!rd_camera(verts + 3 * (int64_t)v, side, f.cam[k])) return false;
        if (!mr_fixed(f.cam[k][0], S, f.x[k]) || !mr_fixed(f.cam[k][1], S, f.y[k])) return false;
        f.z[k] = f.cam[k][2];
        f.v[k] = v;
    }
    return mr_orient(f);
}

// the weights of the sample (px, py) in the positively oriented face; false: not covered
__device__ __forceinline__ bool mr_cover(int ax, int ay, int bx, int by, int cx, int cy, int px, int py, long long &wa, long long &wb, long long &wc) {
    wa = mr_edge(bx, by, cx, cy, px, py);
    wb = mr_edge(cx, cy, ax, ay, px, py);
    wc = mr_edge(ax, ay, bx, by, px, py);
    return (wa > 0 || (wa == 0 && mr_owns(bx, by, cx, cy))) && (wb > 0 || (wb == 0 && mr_owns(cx, cy, ax, ay))) &&
           (wc > 0 || (wc == 0 && mr_owns(ax, ay, bx, by)));
}

// n = (B - A) x (C - A) on the camera coordinates of the (oriented) face
__device__ __forceinline__ void mr_normal(const MrFace &f, double &nx, double &ny, double &nz) {
    const double ux = __dsub_rn(f.cam[1][0], f.cam[0][0]), uy = __dsub_rn(f.cam[1][1], f.cam[0][1]), uz = __dsub_rn(f.cam[1][2], f.cam[0][2]);
    const double vx = __dsub_rn(f.cam[2][0], f.cam[0][0]), vy = __dsub_rn(f.cam[2][1], f.cam[0][1]), vz = __dsub_rn(f.cam[2][2], f.cam[0][2]);
    nx = __dsub_rn(__dmul_rn(uy, vz), __dmul_rn(uz, vy));
    ny = __dsub_rn(__dmul_rn(uz, vx), __dmul_rn(ux, vz));
    nz = __dsub_rn(__dmul_rn(ux, vy), __dmul_rn(uy, vx));
}

// What a rasteriser is made of besides the loop below: its table entry, how a face gets to the screen (face(): x, y, v, cam and the three staged values z),
// what the staged values give at a covered sample (value()) and which of two such values is nearer (nearer(); farthest() loses to every finite one).
struct MrOrtho {                                                          // the mesh images: the axis camera of `side`, the interpolated depth, smallest wins
    typedef GnMeshImage Image;
    static __device__ __forceinline__ bool face(const GnMeshImage &im, const float *__restrict__ iv, int64_t V, const int32_t *__restrict__ idx, int S,
                                                MrFace &f) {
        return mr_face(iv, V, idx, im.side, S, f);
    }
    static __device__ __forceinline__ double value(long long wa, long long wb, long long wc, double za, double zb, double zc) {
        const double num = __dadd_rn(__dadd_rn(__dmul_rn((double)wa, za), __dmul_rn((double)wb, zb)), __dmul_rn((double)wc, zc));
        return __ddiv_rn(num, (double)(wa + wb + wc));                    // the weights sum to area2
    }
    static __device__ __forceinline__ double farthest() { return INFINITY; }
    static __device__ __forceinline__ bool nearer(double z, double best) { return z < best; }
};

template <class P>
__device__ __forceinline__ void mr_raster(const float *__restrict__ verts, const int32_t *__restrict__ faces, const typename P::Image *__restrict__ tab,
                                          int S, uint32_t *__restrict__ out) {
    __shared__ double sz[3][RD_BLOCK];
    __shared__ int sx[3][RD_BLOCK], sy[3][RD_BLOCK];
    __shared__ uint32_t si[RD_BLOCK];
    __shared__ int scnt[RD_WAVES];
    const typename P::Image &im = tab[blockIdx.z];
    const int64_t begin = im.face_begin, end = im.face_end, V = im.vert_end - im.vert_begin;
    const float *iv = verts + 3 * im.vert_begin;
    const int tid = threadIdx.x, lane = tid & (GN_WAVE - 1), wave = tid / GN_WAVE;
    const int tx0 = blockIdx.x * RD_TILE, ty0 = blockIdx.y * RD_TILE;
    const int X = tx0 + (tid & (RD_TILE - 1)), Y = ty0 + tid / RD_TILE;
    const int px = 256 * X + 128, py = 256 * Y + 128;
    double best = P::farthest();
    uint32_t best_idx = RD_NONE;
    for (int64_t c0 = begin; c0 < end; c0 += RD_BLOCK) {                 // block-uniform bounds: every thread reaches every barrier
        const int64_t j = c0 + tid;
        bool hit = false;
        MrFace f;
        if (j < end && P::face(im, iv, V, faces + 3 * j, S, f)) {
            // the pixels whose samples 256 X + 128 lie within [min, max]: X from ceil((min - 128) / 256) to floor((max - 128) / 256)
            const int xlo = (min(f.x[0], min(f.x[1], f.x[2])) + 127) >> 8, xhi = (max(f.x[0], max(f.x[1], f.x[2])) - 128) >> 8;
            const int ylo = (min(f.y[0], min(f.y[1], f.y[2])) + 127) >> 8, yhi = (max(f.y[0], max(f.y[1], f.y[2])) - 128) >> 8;
            hit = xlo <= xhi && ylo <= yhi && xlo <= min(tx0 + RD_TILE, S) - 1 && xhi >= tx0 && ylo <= min(ty0 + RD_TILE, S) - 1 && yhi >= ty0;
        }
        int total;
        const int slot = rd_compact(hit, lane, wave, scnt, total);       // (two barriers inside)
        if (hit) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { sx[k][slot] = f.x[k]; sy[k][slot] = f.y[k]; sz[k][slot] = f.z[k]; }
            si[slot] = (uint32_t)(j - begin);
        }
        __syncthreads();
        for (int s = 0; s < total; ++s) {                                // ascending index: a strict comparison keeps the first of equal depths
            long long wa, wb, wc;
            if (!mr_cover(sx[0][s], sy[0][s], sx[1][s], sy[1][s], sx[2][s], sy[2][s], px, py, wa, wb, wc)) continue;
            const double z = P::value(wa, wb, wc, sz[0][s], sz[1][s], sz[2][s]);
            if (P::nearer(z, best)) { best = z; best_idx = si[s]; }
        }
    }
    if (X < S && Y < S) out[((int64_t)blockIdx.z * S + Y) * S + X] = best_idx;
}

// The winner's weights from its index: the colour / write passes store no weights, they rebuild face `idx` of the image (counted from its first face; iv, V:
// the image's vertices) under the policy P and cover the sample of pixel (X, Y) again.  false: not a face of the image, never drawn, or not covering --
// none of which an index image of mr_raster<P> holds.  A macro ON PURPOSE: as an inlined function template (references or the sample point passed, with
// or without __restrict__, one return or three) the same text took depth_cloud_write_kernel from 76 to 86 SGPRs.
#define MR_WINNER(P, im, iv, V, faces, idx, X, Y, S, f, wa, wb, wc)                                                              \
    ((int64_t)(idx) < (im).face_end - (im).face_begin && P::face(im, iv, V, (faces) + 3 * ((im).face_begin + (idx)), S, f) && \
     mr_cover((f).x[0], (f).y[0], (f).x[1], (f).y[1], (f).x[2], (f).y[2], 256 * (X) + 128, 256 * (Y) + 128, wa, wb, wc))

__global__ __launch_bounds__(RD_BLOCK) void render_mesh_batch_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                     const GnMeshImage *__restrict__ tab, int S, uint32_t *__restrict__ out) {
    mr_raster<MrOrtho>(verts, faces, tab, S, out);
}

__global__ __launch_bounds__(256) void color_mesh_batch_kernel(const uint32_t *__restrict__ idx_img, const float *__restrict__ verts,
                                                               const int32_t *__restrict__ faces, const float *__restrict__ colors,
                                                               const GnMeshImage *__restrict__ tab, int S, float *__restrict__ out) {
    const GnMeshImage &im = tab[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= S * S) return;
    const int X = pix % S, Y = pix / S;
    const int64_t o = (int64_t)blockIdx.y * S * S + pix;
    const uint32_t idx = idx_img[o];
    float4 col = make_float4(im.default_color[0], im.default_color[1], im.default_color[2], im.default_color[3]);
    MrFace f;
    long long wa, wb, wc;
    if (idx != RD_NONE && MR_WINNER(MrOrtho, im, verts + 3 * im.vert_begin, im.vert_end - im.vert_begin, faces, idx, X, Y, S, f, wa, wb, wc)) {
        const double area2 = (double)(wa + wb + wc);
        const float ba = (float)__ddiv_rn((double)wa, area2), bb = (float)__ddiv_rn((double)wb, area2), bc = (float)__ddiv_rn((double)wc, area2);
        const float4 ca = *reinterpret_cast<const float4 *>(colors + 4 * (im.vert_begin + f.v[0]));
        const float4 cb = *reinterpret_cast<const float4 *>(colors + 4 * (im.vert_begin + f.v[1]));
        const float4 cc = *reinterpret_cast<const float4 *>(colors + 4 * (im.vert_begin + f.v[2]));
        double nx, ny, nz;
        mr_normal(f, nx, ny, nz);
        const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(nx, nx), __dmul_rn(ny, ny)), __dmul_rn(nz, nz)));
        const double amb = (double)im.ambient;
        double shade = amb;
        if (len > 0.0 && len < INFINITY) shade = __dadd_rn(amb, __dmul_rn(__dsub_rn(1.0, amb), __ddiv_rn(fabs(nz), len)));
        const float sh = (float)shade;
        col.x = __fmul_rn(sh, __fadd_rn(__fadd_rn(__fmul_rn(ba, ca.x), __fmul_rn(bb, cb.x)), __fmul_rn(bc, cc.x)));
        col.y = __fmul_rn(sh, __fadd_rn(__fadd_rn(__fmul_rn(ba, ca.y), __fmul_rn(bb, cb.y)), __fmul_rn(bc, cc.y)));
        col.z = __fmul_rn(sh, __fadd_rn(__fadd_rn(__fmul_rn(ba, ca.z), __fmul_rn(bb, cb.z)), __fmul_rn(bc, cc.z)));
        col.w = 1.f;
    }
    *reinterpret_cast<float4 *>(out + 4 * o) = col;
}

// entry i of the two host CSRs; what: "image" or "mesh", whichever the CSRs count
static int mr_check_csr(const char *who, const char *what, const int64_t *vseg_host, const int64_t *fseg_host, int i) {
    GN_REQUIRE(vseg_host[i] >= 0 && vseg_host[i + 1] >= vseg_host[i], "%s: %s %d: vseg is not a non-decreasing CSR", who, what, i);
    GN_REQUIRE(fseg_host[i] >= 0 && fseg_host[i + 1] >= fseg_host[i], "%s: %s %d: fseg is not a non-decreasing CSR", who, what, i);
    return GN_OK;
}

static int mr_check(const char *who, const int64_t *vseg_host, const int64_t *fseg_host, const GnMeshImage *tab_host, int I) {
    for (int i = 0; i < I; ++i) {
        const GnMeshImage &g = tab_host[i];
        const int rc = mr_check_csr(who, "image", vseg_host, fseg_host, i);
        if (rc != GN_OK) return rc;
        GN_REQUIRE(g.vert_begin == vseg_host[i] && g.vert_end == vseg_host[i + 1] && g.face_begin == fseg_host[i] && g.face_end == fseg_host[i + 1],
                   "%s: image %d: the table's segments differ from vseg / fseg", who, i);
        GN_REQUIRE(g.face_end - g.face_begin < (int64_t)RD_NONE, "%s: image %d: a segment of %lld faces (needs fewer than 2^32 - 1)", who, i,
                   (long long)(g.face_end - g.face_begin));
        GN_REQUIRE(g.side >= 0 && g.side <= 2, "%s: image %d: side=%d outside {0 front, 1 top, 2 left}", who, i, g.side);
        GN_REQUIRE(g.ambient >= 0.f && g.ambient <= 1.f, "%s: image %d: ambient=%g outside [0, 1]", who, i, (double)g.ambient);
    }
    return GN_OK;
}

extern "C" int gn_render_mesh_batch(const float *verts, const int32_t *faces, const int64_t *vseg_host, const int64_t *fseg_host,
                                    const GnMeshImage *tab_host, const GnMeshImage *tab, int I, int S, uint32_t *out, void *stream) {
    int rc = rd_check_size("gn_render_mesh_batch", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(vseg_host && fseg_host && tab_host && tab && out, "gn_render_mesh_batch: null pointer");
    rc = mr_check("gn_render_mesh_batch", vseg_host, fseg_host, tab_host, I);
    if (rc != GN_OK) return rc;
    GN_REQUIRE(fseg_host[I] == 0 || (faces && (vseg_host[I] == 0 || verts)), "gn_render_mesh_batch: null verts / faces");
    const unsigned tiles = (unsigned)gn_cdiv(S, RD_TILE);
    hipLaunchKernelGGL(render_mesh_batch_kernel, dim3(tiles, tiles, (unsigned)I), dim3(RD_BLOCK), 0, gn_stream(stream), verts, faces, tab, S, out);
    GN_LAUNCH_CHECK("gn_render_mesh_batch");
    return GN_OK;
}

extern "C" int gn_color_mesh_batch(const uint32_t *idx_img, const float *verts, const int32_t *faces, const float *colors, const int64_t *vseg_host,
                                   const int64_t *fseg_host, const GnMeshImage *tab_host, const GnMeshImage *tab, int I, int S, float *out,
                                   void *stream) {
    int rc = rd_check_size("gn_color_mesh_batch", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(idx_img && vseg_host && fseg_host && tab_host && tab && out, "gn_color_mesh_batch: null pointer");
    rc = mr_check("gn_color_mesh_batch", vseg_host, fseg_host, tab_host, I);
    if (rc != GN_OK) return rc;
    GN_REQUIRE(fseg_host[I] == 0 || (faces && (vseg_host[I] == 0 || (verts && colors))), "gn_color_mesh_batch: null verts / faces / colors");
    hipLaunchKernelGGL(color_mesh_batch_kernel, dim3((unsigned)gn_cdiv((int64_t)S * S, 256), (unsigned)I), dim3(256), 0, gn_stream(stream), idx_img, verts,
                       faces, colors, tab, S, out);
    GN_LAUNCH_CHECK("gn_color_mesh_batch");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ point clouds from meshes
//   gn_depth_render_batch    fp32 vertices + int32 faces behind a perspective camera -> uint32 index images: per pixel the covering face nearest to it
//   gn_depth_cloud_offsets   index images -> the exclusive prefix sum of the covered pixels per image row, and the count per image
//   gn_depth_cloud_write     index images + those offsets -> point rows (position, NOCS label, colour) in raster order, image after image
//
// The definitions ("Point clouds from meshes"; garmentnets_amd/point_cloud.py restates them in numpy, operation for operation):
//   camera     cam[j] = ((R[j][0] x + R[j][1] y) + R[j][2] z) + t[j] in fp64 on the fp32 vertex, every operation rounded on its own
//   screen     u = (f * cam[0]) / cam[2] + c, v likewise; fx = rint(u * 256), fy = rint(v * 256), half to even; samples at (256 X + 128, 256 Y + 128)
//   not drawn  what the mesh images never draw, and a face with a vertex at cam[2] < near (no clipping)
//   two-sided, coverage, ownership   mr_orient, mr_cover, mr_owns: the mesh images' own
//   winner     i_k = 1 / z_k, q_k = double(w_k) * i_k, q = (q_a + q_b) + q_c, inv = q / double(area2); the LARGEST inv, equal ones: the lowest face index
//   point      b_k = q_k / q; ((b_a A + b_b B) + b_c C) per coordinate in fp64 on the fp32 corners, rounded once to fp32; the NOCS label likewise
//   colour     n = (B - A) x (C - A) on the camera coordinates, p = the camera coordinates of the fp32 point; nn = (nx nx + ny ny) + nz nz, pp and np
//              likewise, root = sqrt(nn * pp); shade = ambient + (1 - ambient) * (|np| / root), ambient where root is 0 or not finite;
//              rgb_c = uint8(clamp(rint((255 * float(shade)) * base_c), 0, 255)) in fp32, NaN -> 0
//   order      images back to back; within an image the covered pixels in raster order (Y, then X)
// Shape: the rasteriser is mr_raster with the three inverse depths staged in place of the three depths.  The compaction is three small kernels and has
// no atomics: a wave counts the covered pixels of one image row (ballot + popcount), ONE workgroup scans the I * S counts in place (a wave-shuffle scan
// per 256 counts, a running carry), and a wave writes its row's points at its offset, a lane's slot from the popcount of the covered lanes below it.
// The write pass recomputes the winner's weights from the face index, as color_mesh_batch_kernel does.
#define PC_ROWS (256 / GN_WAVE)                                           // image rows per workgroup of the count and the write pass
#define PC_SCAN_BLOCK 256

__device__ __forceinline__ bool pc_camera(const GnDepthImage &im, const float *__restrict__ p, double (&c)[3]) {
    const float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    const double dx = (double)x, dy = (double)y, dz = (double)z;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        c[j] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(im.R[3 * j], dx), __dmul_rn(im.R[3 * j + 1], dy)), __dmul_rn(im.R[3 * j + 2], dz)), im.t[j]);
    return true;
}

// rint(((f * a) / z + c) * 256) as an int; false beyond 2^24 in magnitude (or NaN)
__device__ __forceinline__ bool pc_fixed(const GnDepthImage &im, double a, double z, int &fx) {
    const double r = rint(__dmul_rn(__dadd_rn(__ddiv_rn(__dmul_rn(im.f, a), z), im.c), 256.0));
    if (!(fabs(r) <= 16777216.0)) return false;
    fx = (int)r;
    return true;
}

struct MrPersp {                                                          // the depth images: a free-standing pinhole, the inverse depth, largest wins
    typedef GnDepthImage Image;
    static __device__ __forceinline__ bool face(const GnDepthImage &im, const float *__restrict__ iv, int64_t V, const int32_t *__restrict__ idx, int S,
                                                MrFace &f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int v = idx[k];
            if (v < 0 || (int64_t)v >= V) return false;
            if (!pc_camera(im, iv + 3 * (int64_t)v, f.cam[k])) return false;
            if (!(f.cam[k][2] >= im.znear)) return false;                 // behind the near plane (or NaN): no clipping, the face is not drawn
            if (!pc_fixed(im, f.cam[k][0], f.cam[k][2], f.x[k]) || !pc_fixed(im, f.cam[k][1], f.cam[k][2], f.y[k])) return false;
            f.z[k] = __ddiv_rn(1.0, f.cam[k][2]);
            f.v[k] = v;
        }
        return mr_orient(f);
    }
    static __device__ __forceinline__ double value(long long wa, long long wb, long long wc, double ia, double ib, double ic) {
        const double q = __dadd_rn(__dadd_rn(__dmul_rn((double)wa, ia), __dmul_rn((double)wb, ib)), __dmul_rn((double)wc, ic));
        return __ddiv_rn(q, (double)(wa + wb + wc));
    }
    static __device__ __forceinline__ double farthest() { return -INFINITY; }
    static __device__ __forceinline__ bool nearer(double inv, double best) { return inv > best; }
};

__global__ __launch_bounds__(RD_BLOCK) void depth_render_batch_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                      const GnDepthImage *__restrict__ tab, int S, uint32_t *__restrict__ out) {
    mr_raster<MrPersp>(verts, faces, tab, S, out);
}

// row_off[row] = the covered pixels of image row `row` (rows = I * S of them), a wave per row
__global__ __launch_bounds__(256) void depth_cloud_count_kernel(const uint32_t *__restrict__ idx_img, int64_t rows, int S, int64_t *__restrict__ row_off) {
    const int lane = threadIdx.x & (GN_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * PC_ROWS + threadIdx.x / GN_WAVE;
    if (row >= rows) return;                                              // wave-uniform
    int n = 0;
    for (int x0 = 0; x0 < S; x0 += GN_WAVE) {
        const int X = x0 + lane;
        n += __popcll(__ballot(X < S && idx_img[row * S + X] != RD_NONE));
    }
    if (lane == 0) row_off[row] = n;
}

// counts -> exclusive offsets in place, the total at row_off[rows]; sizes[i] = the points of image i.  ONE workgroup.
__global__ __launch_bounds__(PC_SCAN_BLOCK) void depth_cloud_scan_kernel(int64_t *row_off, int64_t rows, int I, int S, int64_t *sizes) {
    __shared__ long long swave[PC_SCAN_BLOCK / GN_WAVE];
    const int tid = threadIdx.x, lane = tid & (GN_WAVE - 1), wave = tid / GN_WAVE;
    long long carry = 0;
    for (int64_t c0 = 0; c0 < rows; c0 += PC_SCAN_BLOCK) {                // block-uniform bounds: every thread reaches every barrier
        const int64_t i = c0 + tid;
        const long long v = i < rows ? (long long)row_off[i] : 0;
        long long x = v;                                                  // the inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < GN_WAVE; d <<= 1) {
            const long long y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        __syncthreads();                                                  // the previous chunk's wave sums are read
        if (lane == GN_WAVE - 1) swave[wave] = x;
        __syncthreads();
        long long base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PC_SCAN_BLOCK / GN_WAVE; ++w) {
            const long long n = swave[w];
            base += w < wave ? n : 0;
            total += n;
        }
        if (i < rows) row_off[i] = (int64_t)(carry + base + x - v);
        carry += total;
    }
    if (tid == 0) row_off[rows] = (int64_t)carry;
    __threadfence();
    __syncthreads();                                                      // this workgroup wrote every offset: they are visible to it
    for (int i = tid; i < I; i += PC_SCAN_BLOCK) sizes[i] = row_off[(int64_t)(i + 1) * S] - row_off[(int64_t)i * S];
}

__global__ __launch_bounds__(256) void depth_cloud_write_kernel(const uint32_t *__restrict__ idx_img, const float *__restrict__ verts,
                                                                const float *__restrict__ nocs, const int32_t *__restrict__ faces,
                                                                const GnDepthImage *__restrict__ tab, const int64_t *__restrict__ row_off, int64_t rows,
                                                                int S, int64_t N, float *__restrict__ point, float *__restrict__ nocs_out,
                                                                uint8_t *__restrict__ rgb) {
    const int lane = threadIdx.x & (GN_WAVE - 1);
    const int64_t row = (int64_t)blockIdx.x * PC_ROWS + threadIdx.x / GN_WAVE;
    if (row >= rows) return;                                              // wave-uniform
    const int64_t first = row_off[row];
    if (row_off[row + 1] == first) return;                                // an empty row costs two loads
    const GnDepthImage &im = tab[row / S];
    const int Y = (int)(row % S);
    const int64_t V = im.vert_end - im.vert_begin;
    const float *iv = verts + 3 * im.vert_begin, *in = nocs + 3 * im.vert_begin;
    int64_t done = 0;
    for (int x0 = 0; x0 < S; x0 += GN_WAVE) {
        const int X = x0 + lane;
        const uint32_t idx = X < S ? idx_img[row * S + X] : RD_NONE;
        const unsigned long long mask = __ballot(idx != RD_NONE);
        const int64_t slot = first + done + __popcll(mask & ((1ull << lane) - 1ull));
        done += __popcll(mask);
        if (idx == RD_NONE || slot < 0 || slot >= N) continue;
        float P[3] = {0.f, 0.f, 0.f}, L[3] = {0.f, 0.f, 0.f};
        uint8_t col[3] = {0, 0, 0};
        MrFace f;
        long long wa, wb, wc;
        if (MR_WINNER(MrPersp, im, iv, V, faces, idx, X, Y, S, f, wa, wb, wc)) {
            const double qa = __dmul_rn((double)wa, f.z[0]), qb = __dmul_rn((double)wb, f.z[1]), qc = __dmul_rn((double)wc, f.z[2]);
            const double q = __dadd_rn(__dadd_rn(qa, qb), qc);
            const double ba = __ddiv_rn(qa, q), bb = __ddiv_rn(qb, q), bc = __ddiv_rn(qc, q);
            const float *A = iv + 3 * (int64_t)f.v[0], *B = iv + 3 * (int64_t)f.v[1], *C = iv + 3 * (int64_t)f.v[2];
            const float *LA = in + 3 * (int64_t)f.v[0], *LB = in + 3 * (int64_t)f.v[1], *LC = in + 3 * (int64_t)f.v[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                P[c] = (float)__dadd_rn(__dadd_rn(__dmul_rn(ba, (double)A[c]), __dmul_rn(bb, (double)B[c])), __dmul_rn(bc, (double)C[c]));
                L[c] = (float)__dadd_rn(__dadd_rn(__dmul_rn(ba, (double)LA[c]), __dmul_rn(bb, (double)LB[c])), __dmul_rn(bc, (double)LC[c]));
            }
            double nx, ny, nz;
            mr_normal(f, nx, ny, nz);
            const double amb = (double)im.ambient;
            double shade = amb, p[3];                                     // p = the point seen from the camera
            if (pc_camera(im, P, p)) {
                const double nn = __dadd_rn(__dadd_rn(__dmul_rn(nx, nx), __dmul_rn(ny, ny)), __dmul_rn(nz, nz));
                const double pp = __dadd_rn(__dadd_rn(__dmul_rn(p[0], p[0]), __dmul_rn(p[1], p[1])), __dmul_rn(p[2], p[2]));
                const double np = __dadd_rn(__dadd_rn(__dmul_rn(nx, p[0]), __dmul_rn(ny, p[1])), __dmul_rn(nz, p[2]));
                const double root = __dsqrt_rn(__dmul_rn(nn, pp));
                if (root > 0.0 && root < INFINITY) shade = __dadd_rn(amb, __dmul_rn(__dsub_rn(1.0, amb), __ddiv_rn(fabs(np), root)));
            }
            const float sh = __fmul_rn(255.f, (float)shade);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r = rintf(__fmul_rn(sh, im.base_color[c]));
                col[c] = (uint8_t)(r >= 255.f ? 255.f : (r > 0.f ? r : 0.f));      // NaN -> 0
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            point[3 * slot + c] = P[c];
            nocs_out[3 * slot + c] = L[c];
            rgb[3 * slot + c] = col[c];
        }
    }
}

static int pc_check(const char *who, const int64_t *vseg_host, const int64_t *fseg_host, int M, const int32_t *mesh_host, const GnDepthImage *tab_host,
                    int I) {
    GN_REQUIRE(M >= 0, "%s: M=%d meshes", who, M);
    for (int m = 0; m < M; ++m) {
        const int rc = mr_check_csr(who, "mesh", vseg_host, fseg_host, m);
        if (rc != GN_OK) return rc;
        GN_REQUIRE(fseg_host[m + 1] - fseg_host[m] < (int64_t)RD_NONE, "%s: mesh %d: a segment of %lld faces (needs fewer than 2^32 - 1)", who, m,
                   (long long)(fseg_host[m + 1] - fseg_host[m]));
    }
    for (int i = 0; i < I; ++i) {
        const GnDepthImage &g = tab_host[i];
        const int m = mesh_host[i];
        GN_REQUIRE(m >= 0 && m < M, "%s: image %d: mesh=%d outside [0, M=%d)", who, i, m, M);
        GN_REQUIRE(g.vert_begin == vseg_host[m] && g.vert_end == vseg_host[m + 1] && g.face_begin == fseg_host[m] && g.face_end == fseg_host[m + 1],
                   "%s: image %d: the table's segments differ from vseg / fseg of mesh %d", who, i, m);
        for (int k = 0; k < 9; ++k) GN_REQUIRE(std::isfinite(g.R[k]), "%s: image %d: camera entry R[%d]=%g is not finite", who, i, k, g.R[k]);
        for (int k = 0; k < 3; ++k) GN_REQUIRE(std::isfinite(g.t[k]), "%s: image %d: camera entry t[%d]=%g is not finite", who, i, k, g.t[k]);
        GN_REQUIRE(std::isfinite(g.c), "%s: image %d: camera entry c=%g is not finite", who, i, g.c);
        GN_REQUIRE(std::isfinite(g.f) && g.f > 0.0, "%s: image %d: f=%g is not a positive finite focal length", who, i, g.f);
        GN_REQUIRE(std::isfinite(g.znear) && g.znear > 0.0, "%s: image %d: near=%g is not positive and finite", who, i, g.znear);
        GN_REQUIRE(g.ambient >= 0.f && g.ambient <= 1.f, "%s: image %d: ambient=%g outside [0, 1]", who, i, (double)g.ambient);
        for (int k = 0; k < 3; ++k)
            GN_REQUIRE(std::isfinite(g.base_color[k]), "%s: image %d: base_color[%d]=%g is not finite", who, i, k, (double)g.base_color[k]);
    }
    return GN_OK;
}

extern "C" int gn_depth_render_batch(const float *verts, const int32_t *faces, const int64_t *vseg_host, const int64_t *fseg_host, int M,
                                     const int32_t *mesh_host, const GnDepthImage *tab_host, const GnDepthImage *tab, int I, int S, uint32_t *out,
                                     void *stream) {
    int rc = rd_check_size("gn_depth_render_batch", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(vseg_host && fseg_host && mesh_host && tab_host && tab && out, "gn_depth_render_batch: null pointer");
    rc = pc_check("gn_depth_render_batch", vseg_host, fseg_host, M, mesh_host, tab_host, I);
    if (rc != GN_OK) return rc;
    GN_REQUIRE(fseg_host[M] == 0 || (faces && (vseg_host[M] == 0 || verts)), "gn_depth_render_batch: null verts / faces");
    const unsigned tiles = (unsigned)gn_cdiv(S, RD_TILE);
    hipLaunchKernelGGL(depth_render_batch_kernel, dim3(tiles, tiles, (unsigned)I), dim3(RD_BLOCK), 0, gn_stream(stream), verts, faces, tab, S, out);
    GN_LAUNCH_CHECK("gn_depth_render_batch");
    return GN_OK;
}

extern "C" int gn_depth_cloud_offsets(const uint32_t *idx_img, int I, int S, int64_t *row_off, int64_t *sizes, void *stream) {
    const int rc = rd_check_size("gn_depth_cloud_offsets", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(idx_img && row_off && sizes, "gn_depth_cloud_offsets: null pointer");
    const int64_t rows = (int64_t)I * S;
    hipLaunchKernelGGL(depth_cloud_count_kernel, dim3((unsigned)gn_cdiv(rows, PC_ROWS)), dim3(256), 0, gn_stream(stream), idx_img, rows, S, row_off);
    GN_LAUNCH_CHECK("gn_depth_cloud_offsets (count)");
    hipLaunchKernelGGL(depth_cloud_scan_kernel, dim3(1), dim3(PC_SCAN_BLOCK), 0, gn_stream(stream), row_off, rows, I, S, sizes);
    GN_LAUNCH_CHECK("gn_depth_cloud_offsets (scan)");
    return GN_OK;
}

extern "C" int gn_depth_cloud_write(const uint32_t *idx_img, const float *verts, const float *nocs, const int32_t *faces, const int64_t *vseg_host,
                                    const int64_t *fseg_host, int M, const int32_t *mesh_host, const GnDepthImage *tab_host, const GnDepthImage *tab,
                                    const int64_t *row_off, int I, int S, int64_t N, float *point, float *nocs_out, uint8_t *rgb, void *stream) {
    int rc = rd_check_size("gn_depth_cloud_write", I, S);
    if (rc != GN_OK) return rc;
    if (I == 0) return GN_OK;
    GN_REQUIRE(idx_img && vseg_host && fseg_host && mesh_host && tab_host && tab && row_off, "gn_depth_cloud_write: null pointer");
    rc = pc_check("gn_depth_cloud_write", vseg_host, fseg_host, M, mesh_host, tab_host, I);
    if (rc != GN_OK) return rc;
    GN_REQUIRE(N >= 0, "gn_depth_cloud_write: N=%lld rows", (long long)N);
    if (N == 0) return GN_OK;
    GN_REQUIRE(point && nocs_out && rgb, "gn_depth_cloud_write: null output");
    GN_REQUIRE(faces && verts && nocs, "gn_depth_cloud_write: null verts / nocs / faces");
    const int64_t rows = (int64_t)I * S;
    hipLaunchKernelGGL(depth_cloud_write_kernel, dim3((unsigned)gn_cdiv(rows, PC_ROWS)), dim3(256), 0, gn_stream(stream), idx_img, verts, nocs, faces, tab,
                       row_off, rows, S, N, point, nocs_out, rgb);
    GN_LAUNCH_CHECK("gn_depth_cloud_write");
    return GN_OK;
}

// grad.hip -- gradients of the point and grid operators (the third-party operators this library restates: torch_scatter.scatter, PointConv's gather +
// max aggregation, global_max_pool, knn_interpolate, F.grid_sample).  fp32 in / fp32 out.  The dense layers between them keep torch's own backward.
//
// Two families:
//  * selections (grid scatter max / min, segment max, global max pool): the gradient of an output element goes to ONE input element, the one whose
//    value is bit-equal to the forward's stored output; among equal values the lowest point / edge index.  NaN never wins.  A gather per input element.
//  * sums over an unordered set (sa_gather, knn_interpolate, the sampler's volume gradient): the inverse lists (destination -> the elements that
//    read it) are built once -- count, a range per destination, fill, then every element moves to its rank inside its range, so a range is in
//    ascending element index -- and ONE wavefront per destination adds its terms in that order: identical calls give identical bits, no float atomics.
//    (The integer atomics that count and hand out ranges only decide WHERE a range lives, never the order inside it.)
#include "common.h"
#include "inv_lists.h"
#include <limits.h>

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) && a == a; }

// ------------------------------------------------------------------------------------------------ ordered sums over the inverse lists (inv_lists.h)
// one wavefront per destination, channels over its lanes: out[key][ch] = sum over the range, ascending, of coef[e] * g[e / div][ch]  (coef NULL: 1).
// A destination nobody reads gets 0: the kernel writes every row of out.
__global__ __launch_bounds__(256) void ordered_sum_kernel(InvWs w, int64_t nkeys, const float *__restrict__ coef, int div, const float *__restrict__ g,
                                                          int ldg, int C, float *__restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63;
    const int64_t key = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (key >= nkeys) return;
    const int k = w.cnt[key];
    const int32_t *list = w.sorted + (k ? w.start[key] : 0);
    for (int ch = lane; ch < C; ch += 64) {
        float acc = 0.f;
        for (int i = 0; i < k; ++i) {
            const int e = list[i];
            const float t = g[(int64_t)(e / div) * ldg + ch];
            acc = __fadd_rn(acc, coef ? __fmul_rn(coef[e], t) : t);
        }
        out[key * ldo + ch] = acc;
    }
}

static int ordered_sum(InvWs w, int64_t nkeys, const float *coef, int div, const float *g, int ldg, int C, float *out, int ldo, hipStream_t st) {
    hipLaunchKernelGGL(ordered_sum_kernel, dim3((unsigned)gn_cdiv(nkeys, 4)), dim3(256), 0, st, w, nkeys, coef, div, g, ldg, C, out, ldo);
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ grid scatter
// max / min: every occupied cell gets an owner point (which one only decides where the cell's winner row lives), every point whose value is bit-equal
// to the cell's stored value bids its index for (owner, channel) with an integer atomicMin -- order-independent -- and the gather hands the cell's
// gradient to the point that holds the bid.
__global__ __launch_bounds__(256) void gsb_bid_kernel(const float *__restrict__ src, int lds, const float *__restrict__ vol, const int32_t *__restrict__ flat_idx,
                                                      int64_t N, int C, int c_real, const int32_t *__restrict__ owner_of, int32_t *__restrict__ win) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N || owner_of[p] < 0) return;
    const float *v = vol + (int64_t)flat_idx[p] * C;
    int32_t *wr = win + (int64_t)owner_of[p] * C;
    for (int ch = lane; ch < c_real; ch += 64)
        if (same_bits(src[p * lds + ch], v[ch])) atomicMin(&wr[ch], (int)p);
}

__global__ __launch_bounds__(256) void gsb_select_kernel(const float *__restrict__ grad_vol, const int32_t *__restrict__ flat_idx, int64_t N, int C, int c_real,
                                                         const int32_t *__restrict__ owner_of, const int32_t *__restrict__ win,
                                                         float *__restrict__ grad_src, int ldg) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N) return;
    const int o = owner_of[p];
    const float *g = grad_vol + (int64_t)(o < 0 ? 0 : flat_idx[p]) * C;
    for (int ch = lane; ch < C; ch += 64)
        grad_src[p * ldg + ch] = (o >= 0 && ch < c_real && win[(int64_t)o * C + ch] == (int)p) ? g[ch] : 0.f;
}

__global__ __launch_bounds__(256) void gsb_count_kernel(const int32_t *__restrict__ flat_idx, int64_t N, int64_t cells, int32_t *__restrict__ count) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    const int64_t cell = flat_idx[p];
    if (cell >= 0 && cell < cells) atomicAdd(&count[cell], 1);
}

// sum: the cell's gradient; mean (count != NULL): divided by the cell's point count
__global__ __launch_bounds__(256) void gsb_spread_kernel(const float *__restrict__ grad_vol, const int32_t *__restrict__ flat_idx, int64_t N, int C, int c_real,
                                                         int64_t cells, const int32_t *__restrict__ count, float *__restrict__ grad_src, int ldg) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= N) return;
    const int64_t cell = flat_idx[p];
    const bool in = cell >= 0 && cell < cells;
    const float *g = grad_vol + (in ? cell : 0) * C;
    const float c = (in && count) ? (float)count[cell] : 1.f;
    for (int ch = lane; ch < C; ch += 64) grad_src[p * ldg + ch] = (in && ch < c_real) ? __fdiv_rn(g[ch], c) : 0.f;
}

// count [cells] (max / min / mean), owner_of [N] and the bids win [N][C] (max / min); sum needs nothing
struct GsbWs { int32_t *count, *owner_of, *win; };
static GsbWs gsb_ws(GnCarve &c, int64_t N, int C, int64_t cells, int reduce) {
    const bool sel = reduce == GN_REDUCE_MAX || reduce == GN_REDUCE_MIN;
    return {c.take<int32_t>(sel || reduce == GN_REDUCE_MEAN ? (size_t)cells : 0), c.take<int32_t>(sel ? (size_t)N : 0), c.take<int32_t>(sel ? (size_t)N * C : 0)};
}

extern "C" size_t gn_grid_scatter_bwd_workspace_bytes(int64_t N, int C, int64_t cells, int reduce) {
    return N <= 0 ? 0 : gn_carve_bytes(gsb_ws, N, C, cells, reduce);
}

extern "C" int gn_grid_scatter_bwd(const float *grad_vol, const float *vol, const float *src, int lds, const int32_t *flat_idx, int64_t N, int C, int c_real,
                                   int64_t cells, int reduce, void *ws, size_t ws_bytes, float *grad_src, int ldg, void *stream) {
    GN_REQUIRE(reduce != GN_REDUCE_MUL, "gn_grid_scatter_bwd: reduce 'mul' has no gradient here (it divides by zero at a zero factor)");
    GN_REQUIRE(reduce >= GN_REDUCE_MAX && reduce <= GN_REDUCE_MIN, "gn_grid_scatter_bwd: bad reduce code");
    GN_REQUIRE(N >= 0 && C > 0 && cells >= 0 && ldg >= C, "gn_grid_scatter_bwd: bad sizes");
    GN_REQUIRE(c_real > 0 && c_real <= C, "gn_grid_scatter_bwd: c_real must be in [1, C]");
    GN_REQUIRE(N < (int64_t)0x7fffffff, "gn_grid_scatter_bwd: more than 2^31-2 points");
    if (N == 0) return GN_OK;                       // (needs no workspace)
    GnCarve c(ws);
    const auto [count, owner_of, win] = gsb_ws(c, N, C, cells, reduce);
    GN_REQUIRE(c.off <= ws_bytes && (ws || !c.off), "gn_grid_scatter_bwd: workspace too small (gn_grid_scatter_bwd_workspace_bytes)");
    const bool sel = reduce == GN_REDUCE_MAX || reduce == GN_REDUCE_MIN;
    GN_REQUIRE(grad_vol && flat_idx && grad_src && (!sel || (vol && src && lds >= c_real)), "gn_grid_scatter_bwd: null pointer");
    hipStream_t st = gn_stream(stream);
    const dim3 grid((unsigned)gn_cdiv(N, 4)), block(256), pts((unsigned)gn_cdiv(N, 256));
    if (sel) {
        GN_HIP(hipMemsetAsync(count, 0, (size_t)cells * sizeof(int32_t), st), "gn_grid_scatter_bwd(memset count)");
        GN_HIP(hipMemsetAsync(win, 0x7f, (size_t)N * C * sizeof(int32_t), st), "gn_grid_scatter_bwd(memset bids)");   // 0x7f7f7f7f > any point index
        hipLaunchKernelGGL(cell_owner_kernel<true>, pts, block, 0, st, flat_idx, N, cells, count, owner_of, (int32_t *)nullptr);
        hipLaunchKernelGGL(gsb_bid_kernel, grid, block, 0, st, src, lds, vol, flat_idx, N, C, c_real, owner_of, win);
        hipLaunchKernelGGL(gsb_select_kernel, grid, block, 0, st, grad_vol, flat_idx, N, C, c_real, owner_of, win, grad_src, ldg);
    } else {
        if (reduce == GN_REDUCE_MEAN) {
            GN_HIP(hipMemsetAsync(count, 0, (size_t)cells * sizeof(int32_t), st), "gn_grid_scatter_bwd(memset count)");
            hipLaunchKernelGGL(gsb_count_kernel, pts, block, 0, st, flat_idx, N, cells, count);
        }
        hipLaunchKernelGGL(gsb_spread_kernel, grid, block, 0, st, grad_vol, flat_idx, N, C, c_real, cells, reduce == GN_REDUCE_MEAN ? count : nullptr,
                           grad_src, ldg);
    }
    GN_LAUNCH_CHECK("gn_grid_scatter_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ segment max
// one thread per (centre, channel): the slots in ascending order, the first valid one that holds the stored maximum takes the gradient
__global__ __launch_bounds__(256) void segment_max_bwd_kernel(const float *__restrict__ grad_out, int ldg, const float *__restrict__ out, int ldo,
                                                              const float *__restrict__ in, int ldi, const int32_t *__restrict__ slot_src, int S, int C,
                                                              float *__restrict__ grad_in, int ldgi) {
    const int c = blockIdx.x;
    for (int ch = threadIdx.x; ch < C; ch += blockDim.x) {
        const float o = out[(int64_t)c * ldo + ch], g = grad_out[(int64_t)c * ldg + ch];
        bool found = false;
        for (int s = 0; s < S; ++s) {
            const int64_t row = (int64_t)c * S + s;
            const bool win = !found && slot_src[row] >= 0 && same_bits(in[row * ldi + ch], o);
            grad_in[row * ldgi + ch] = win ? g : 0.f;
            found |= win;
        }
    }
}

extern "C" int gn_segment_max_bwd(const float *grad_out, int ldg, const float *out, int ldo, const float *in, int ldi, const int32_t *slot_src, int M, int S,
                                  int C, float *grad_in, int ldgi, void *stream) {
    GN_REQUIRE(M >= 0 && S > 0 && C > 0 && ldg >= C && ldo >= C && ldi >= C && ldgi >= C, "gn_segment_max_bwd: bad sizes");
    if (M == 0) return GN_OK;
    GN_REQUIRE(grad_out && out && in && slot_src && grad_in, "gn_segment_max_bwd: null pointer");
    const int threads = C >= 256 ? 256 : (C >= 128 ? 128 : 64);
    hipLaunchKernelGGL(segment_max_bwd_kernel, dim3(M), dim3(threads), 0, gn_stream(stream), grad_out, ldg, out, ldo, in, ldi, slot_src, S, C, grad_in, ldgi);
    GN_LAUNCH_CHECK("gn_segment_max_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ global max pool
// grid (B, channel tiles of 64), 16 row groups x 64 channels as the forward: each group finds the lowest of ITS rows that holds the stored maximum,
// LDS takes the lowest of the 16, then every group writes its rows (the gradient at the winner, 0 elsewhere)
#define GMB_GROUPS 16
__global__ __launch_bounds__(64 * GMB_GROUPS) void global_max_bwd_kernel(const float *__restrict__ grad_out, int ldg, const float *__restrict__ out, int ldo,
                                                                        const float *__restrict__ in, int ldi, const int32_t *__restrict__ ptr, int C,
                                                                        float *__restrict__ grad_in, int ldgi) {
    __shared__ int part[GMB_GROUPS][64];
    const int b = blockIdx.x, l = threadIdx.x & 63, ch = blockIdx.y * 64 + l, g = threadIdx.x >> 6;
    const int s = ptr[b], e = ptr[b + 1];
    int win = INT_MAX;
    if (ch < C) {
        const float o = out[(int64_t)b * ldo + ch];
        for (int r = s + g; r < e; r += GMB_GROUPS)
            if (same_bits(in[(int64_t)r * ldi + ch], o)) { win = r; break; }
    }
    part[g][l] = win;
    __syncthreads();
    if (ch >= C) return;
#pragma unroll
    for (int k = 0; k < GMB_GROUPS; ++k) win = min(win, part[k][l]);
    const float go = grad_out[(int64_t)b * ldg + ch];
    for (int r = s + g; r < e; r += GMB_GROUPS) grad_in[(int64_t)r * ldgi + ch] = r == win ? go : 0.f;
}

extern "C" int gn_global_max_pool_bwd(const float *grad_out, int ldg, const float *out, int ldo, const float *in, int ldi, const int32_t *ptr, int B, int C,
                                      float *grad_in, int ldgi, void *stream) {
    GN_REQUIRE(B >= 0 && C > 0 && ldg >= C && ldo >= C && ldi >= C && ldgi >= C, "gn_global_max_pool_bwd: bad sizes");
    if (B == 0) return GN_OK;
    GN_REQUIRE(grad_out && out && in && ptr && grad_in, "gn_global_max_pool_bwd: null pointer");
    hipLaunchKernelGGL(global_max_bwd_kernel, dim3(B, (unsigned)gn_cdiv(C, 64)), dim3(64 * GMB_GROUPS), 0, gn_stream(stream), grad_out, ldg, out, ldo, in, ldi,
                       ptr, C, grad_in, ldgi);
    GN_LAUNCH_CHECK("gn_global_max_pool_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ SA gather
// grad_x[j] = the sum of the feature part of the edge rows whose source is j (slot_src: gn_sa_gather's record of every row's source after the
// self-loop rule, -1 = an empty slot), in ascending row index.  Positions are data: no gradient.
extern "C" size_t gn_sa_gather_bwd_workspace_bytes(int64_t rows, int64_t n_points) { return (rows < 0 || n_points <= 0) ? 0 : gn_carve_bytes(inv_ws, n_points, rows); }

extern "C" int gn_sa_gather_bwd(const float *grad_edge, int lde, const int32_t *slot_src, int64_t rows, int C, int64_t n_points, void *ws, size_t ws_bytes,
                                float *grad_x, int ldgx, void *stream) {
    GN_REQUIRE(rows >= 0 && rows < (int64_t)0x7fffffff && n_points >= 0 && n_points < (int64_t)0x7fffffff && C > 0 && lde >= C && ldgx >= C,
               "gn_sa_gather_bwd: bad sizes");
    if (n_points == 0) return GN_OK;
    GnCarve c(ws);
    const InvWs w = inv_ws(c, n_points, rows);
    GN_REQUIRE(ws && c.off <= ws_bytes, "gn_sa_gather_bwd: workspace too small (gn_sa_gather_bwd_workspace_bytes)");
    GN_REQUIRE(grad_x && (rows == 0 || (grad_edge && slot_src)), "gn_sa_gather_bwd: null pointer");
    hipStream_t st = gn_stream(stream);
    const int rc = inv_build(slot_src, rows, n_points, w, st, "gn_sa_gather_bwd");
    if (rc != GN_OK) return rc;
    ordered_sum(w, n_points, nullptr, 1, grad_edge, lde, C, grad_x, ldgx, st);
    GN_LAUNCH_CHECK("gn_sa_gather_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ kNN interpolate
// The neighbours gn_knn_interpolate / _any use, written out: one wavefront per query and one pass per neighbour; pass r finds the smallest (d2, index)
// key strictly greater than pass r-1's (the forward kernels' ascending (d2, index) order, the same gn_sqdist3).  nbr [Nq][k] (-1 past an example's
// sources), d2 [Nq][k] (0 there).
__global__ __launch_bounds__(256) void knn_neighbours_kernel(const float *__restrict__ ps, const int32_t *__restrict__ ptr_s, const float *__restrict__ pq,
                                                             const int32_t *__restrict__ ptr_q, int B, int Nq, int k, int32_t *__restrict__ nbr,
                                                             float *__restrict__ d2) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= Nq) return;
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (ptr_q[mid] <= q) lo = mid; else hi = mid;
    }
    const int s = ptr_s[lo], e = ptr_s[lo + 1];
    const float qx = pq[3 * (size_t)q], qy = pq[3 * (size_t)q + 1], qz = pq[3 * (size_t)q + 2];
    float pd = -1.f;
    int pj = -1, r = 0;
    for (; r < k; ++r) {
        float v = 3.4e38f;
        int i = INT_MAX;
        for (int j = s + lane; j < e; j += 64) {
            const float d = gn_sqdist3(ps[3 * (size_t)j], ps[3 * (size_t)j + 1], ps[3 * (size_t)j + 2], qx, qy, qz);
            if ((d > pd || (d == pd && j > pj)) && d < v) { v = d; i = j; }
        }
        GN_WAVE_ARGMIN(v, i)
        if (i == INT_MAX) break;
        pd = v;
        pj = i;
        if (lane == 0) { nbr[(size_t)q * k + r] = i; d2[(size_t)q * k + r] = v; }
    }
    for (int t = r + lane; t < k; t += 64) { nbr[(size_t)q * k + t] = -1; d2[(size_t)q * k + t] = 0.f; }
}

extern "C" int gn_knn_neighbours(const float *ps, const int32_t *ptr_s, const float *pq, const int32_t *ptr_q, int B, int Nq, int k, int32_t *nbr, float *d2,
                                 void *stream) {
    GN_REQUIRE(k >= 1 && B >= 0 && Nq >= 0, "gn_knn_neighbours: bad sizes (k must be >= 1)");
    if (Nq == 0) return GN_OK;
    GN_REQUIRE(B > 0 && ps && ptr_s && pq && ptr_q && nbr && d2, "gn_knn_neighbours: null pointer");
    hipLaunchKernelGGL(knn_neighbours_kernel, dim3((unsigned)gn_cdiv(Nq, 4)), dim3(256), 0, gn_stream(stream), ps, ptr_s, pq, ptr_q, B, Nq, k, nbr, d2);
    GN_LAUNCH_CHECK("gn_knn_neighbours");
    return GN_OK;
}

// coef[q][r] = w / sum of the query's w, w = 1 / max(d2, 1e-16), the sum in the forward's order
__global__ __launch_bounds__(256) void knn_coef_kernel(const int32_t *__restrict__ nbr, const float *__restrict__ d2, int Nq, int k, float *__restrict__ coef) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Nq) return;
    float wsum = 0.f;
    for (int r = 0; r < k; ++r)
        if (nbr[(size_t)q * k + r] >= 0) wsum = __fadd_rn(wsum, __fdiv_rn(1.0f, fmaxf(d2[(size_t)q * k + r], 1e-16f)));
    for (int r = 0; r < k; ++r)
        coef[(size_t)q * k + r] = nbr[(size_t)q * k + r] >= 0 ? __fdiv_rn(__fdiv_rn(1.0f, fmaxf(d2[(size_t)q * k + r], 1e-16f)), wsum) : 0.f;
}

// the inverse lists over the Nq k neighbour slots, keyed by the source, then coef [Nq][k]
struct KnnBwdWs { InvWs inv; float *coef; };
static KnnBwdWs knn_bwd_ws(GnCarve &c, int64_t Nq, int k, int64_t Ns) { return {inv_ws(c, Ns, Nq * k), c.take<float>((size_t)(Nq * k))}; }

extern "C" size_t gn_knn_interpolate_bwd_workspace_bytes(int64_t Nq, int k, int64_t Ns) {
    return (Nq < 0 || k < 1 || Ns <= 0) ? 0 : gn_carve_bytes(knn_bwd_ws, Nq, k, Ns);
}

extern "C" int gn_knn_interpolate_bwd(const int32_t *nbr, const float *d2, int Nq, int k, const float *grad_y, int ldg, int Ns, int C, void *ws, size_t ws_bytes,
                                      float *grad_xs, int ldgx, void *stream) {
    GN_REQUIRE(k >= 1 && Nq >= 0 && Ns >= 0 && C > 0 && ldg >= C && ldgx >= C && (int64_t)Nq * k < (int64_t)0x7fffffff, "gn_knn_interpolate_bwd: bad sizes");
    if (Ns == 0) return GN_OK;
    GnCarve c(ws);
    const auto [w, coef] = knn_bwd_ws(c, Nq, k, Ns);
    GN_REQUIRE(ws && c.off <= ws_bytes, "gn_knn_interpolate_bwd: workspace too small (gn_knn_interpolate_bwd_workspace_bytes)");
    GN_REQUIRE(grad_xs && (Nq == 0 || (nbr && d2 && grad_y)), "gn_knn_interpolate_bwd: null pointer");
    hipStream_t st = gn_stream(stream);
    const int64_t n = (int64_t)Nq * k;
    if (Nq > 0) hipLaunchKernelGGL(knn_coef_kernel, dim3((unsigned)gn_cdiv(Nq, 256)), dim3(256), 0, st, nbr, d2, Nq, k, coef);
    const int rc = inv_build(nbr, n, Ns, w, st, "gn_knn_interpolate_bwd");
    if (rc != GN_OK) return rc;
    ordered_sum(w, Ns, coef, k, grad_y, ldg, C, grad_xs, ldgx, st);
    GN_LAUNCH_CHECK("gn_knn_interpolate_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ trilinear sampler
// The forward's arithmetic (gn_tri_src_index / gn_tri_cell, device_prims.h; query component 0 indexes the LAST volume axis); mx, my, mz: the `moving` flags.
struct TriCorners : GnTriCell {
    float mx, my, mz;
};
__device__ __forceinline__ TriCorners tri_corners(const float *__restrict__ q, int D, int H, int W) {
    TriCorners t;
    const float ix = gn_tri_src_index(q[0], W, &t.mx), iy = gn_tri_src_index(q[1], H, &t.my), iz = gn_tri_src_index(q[2], D, &t.mz);
    static_cast<GnTriCell &>(t) = gn_tri_cell(ix, iy, iz);
    return t;
}

// one thread per query: its eight (voxel, weight) elements, element index (b M + m) 8 + corner; a corner beyond the border: key -1
__global__ __launch_bounds__(256) void tri_elements_kernel(const float *__restrict__ query, int64_t BM, int64_t M, int D, int H, int W,
                                                           int32_t *__restrict__ keys, float *__restrict__ wgt) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= BM) return;
    const TriCorners t = tri_corners(query + r * 3, D, H, W);
    const int64_t b = r / M;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
        const int xx = t.x0 + dx, yy = t.y0 + dy, zz = t.z0 + dz;
        const bool ok = xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D;
        keys[r * 8 + c] = ok ? (int32_t)(((b * D + zz) * H + yy) * (int64_t)W + xx) : -1;
        wgt[r * 8 + c] = gn_tri_weight(t, c);
    }
}

// one wavefront per query, channels over the lanes, a fixed butterfly over the lanes at the end: deterministic
__global__ __launch_bounds__(256) void tri_grad_query_kernel(const float *__restrict__ vol, int64_t vol_bs, int D, int H, int W, int C,
                                                             const float *__restrict__ query, int64_t BM, int64_t M, const float *__restrict__ grad_rows,
                                                             int ldg, float *__restrict__ grad_query) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= BM) return;
    const TriCorners t = tri_corners(query + r * 3, D, H, W);
    const float *v = vol + (r / M) * vol_bs;
    const float *g = grad_rows + r * ldg;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int ch = lane; ch < C; ch += 64) {
        const float go = g[ch];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            const int xx = t.x0 + dx, yy = t.y0 + dy, zz = t.z0 + dz;
            if (xx >= 0 && xx < W && yy >= 0 && yy < H && zz >= 0 && zz < D) {
                const float p = __fmul_rn(v[(((int64_t)zz * H + yy) * W + xx) * C + ch], go);
                const float tx = __fmul_rn(__fmul_rn(p, t.wy[dy]), t.wz[dz]), ty = __fmul_rn(__fmul_rn(p, t.wx[dx]), t.wz[dz]),
                            tz = __fmul_rn(__fmul_rn(p, t.wx[dx]), t.wy[dy]);
                gx = dx ? __fadd_rn(gx, tx) : __fsub_rn(gx, tx);
                gy = dy ? __fadd_rn(gy, ty) : __fsub_rn(gy, ty);
                gz = dz ? __fadd_rn(gz, tz) : __fsub_rn(gz, tz);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        gx = __fadd_rn(gx, __shfl_xor(gx, off));
        gy = __fadd_rn(gy, __shfl_xor(gy, off));
        gz = __fadd_rn(gz, __shfl_xor(gz, off));
    }
    if (lane == 0) {
        // d(index) / d(query) = size - 1 (the query is in [0, 1]: 2 q - 1, then (. + 1) / 2 (size - 1))
        grad_query[r * 3] = __fmul_rn(__fmul_rn(t.mx, (float)(W - 1)), gx);
        grad_query[r * 3 + 1] = __fmul_rn(__fmul_rn(t.my, (float)(H - 1)), gy);
        grad_query[r * 3 + 2] = __fmul_rn(__fmul_rn(t.mz, (float)(D - 1)), gz);
    }
}

// the inverse lists over the n = 8 B M corner elements, keyed by the voxel, then the elements' keys [n] and weights [n]
struct TriBwdWs { InvWs inv; int32_t *keys; float *wgt; };
static TriBwdWs tri_bwd_ws(GnCarve &c, int64_t n, int64_t vox) { return {inv_ws(c, vox, n), c.take<int32_t>((size_t)n), c.take<float>((size_t)n)}; }

extern "C" size_t gn_trilinear_sample_bwd_workspace_bytes(int B, int64_t M, int D, int H, int W) {
    const int64_t n = (int64_t)B * M * 8, vox = (int64_t)B * D * H * W;
    return (B <= 0 || M < 0 || vox <= 0) ? 0 : gn_carve_bytes(tri_bwd_ws, n, vox);
}

// grad_rows: (B M) rows of ldg floats; vol / grad_vol: B dense channel-last volumes (D, H, W, C); grad_vol or grad_query may be NULL (not asked for)
extern "C" int gn_trilinear_sample_bwd(const float *grad_rows, int ldg, const float *vol, int B, int D, int H, int W, int C, const float *query, int64_t M,
                                       void *ws, size_t ws_bytes, float *grad_vol, float *grad_query, void *stream) {
    GN_REQUIRE(B >= 0 && D > 0 && H > 0 && W > 0 && C > 0 && M >= 0 && ldg >= C, "gn_trilinear_sample_bwd: bad sizes");
    const int64_t BM = (int64_t)B * M, vox = (int64_t)B * D * H * W;
    GN_REQUIRE(BM * 8 < (int64_t)0x7fffffff && vox < (int64_t)0x7fffffff, "gn_trilinear_sample_bwd: more than 2^31-2 corner elements or voxels");
    if (B == 0 || (!grad_vol && !grad_query)) return GN_OK;
    GN_REQUIRE(BM == 0 || (grad_rows && query), "gn_trilinear_sample_bwd: null pointer");
    hipStream_t st = gn_stream(stream);
    if (grad_vol) {
        const int64_t n = BM * 8;
        GnCarve c(ws);
        const auto [w, keys, wgt] = tri_bwd_ws(c, n, vox);
        GN_REQUIRE(ws && c.off <= ws_bytes, "gn_trilinear_sample_bwd: workspace too small (gn_trilinear_sample_bwd_workspace_bytes)");
        if (BM > 0) hipLaunchKernelGGL(tri_elements_kernel, dim3((unsigned)gn_cdiv(BM, 256)), dim3(256), 0, st, query, BM, M, D, H, W, keys, wgt);
        const int rc = inv_build(keys, n, vox, w, st, "gn_trilinear_sample_bwd");
        if (rc != GN_OK) return rc;
        ordered_sum(w, vox, wgt, 8, grad_rows, ldg, C, grad_vol, C, st);
    }
    if (grad_query && BM > 0) {
        GN_REQUIRE(vol != nullptr, "gn_trilinear_sample_bwd: grad_query needs the volume");
        hipLaunchKernelGGL(tri_grad_query_kernel, dim3((unsigned)gn_cdiv(BM, 4)), dim3(256), 0, st, vol, (int64_t)D * H * W * C, D, H, W, C, query, BM, M,
                           grad_rows, ldg, grad_query);
    }
    GN_LAUNCH_CHECK("gn_trilinear_sample_bwd");
    return GN_OK;
}

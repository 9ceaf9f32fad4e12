// inv_lists.h -- ordered inverse lists and the owner election, for grid.hip (reduce = mul) and grad.hip (the ordered sums).
// The inverse lists (destination key -> the elements that belong to it) are a counting sort keyed by the destination: count, a range per key handed
// out from one counter, the elements in arrival order, then every element moves to its rank inside its range, so a range is in ascending element
// index.  The integer atomics that count and hand out ranges only decide WHERE a range lives, never the order inside it.
// Everything here is static: each translation unit that includes the header gets its own kernels.
#pragma once
#include "common.h"

struct InvWs {
    int32_t *cnt, *start, *cursor, *total, *lst, *sorted;      // [nkeys] x 3, [1], [n] x 2
};
// (cnt, start, cursor and total stay back to back: inv_build zeroes them with one fill)
static InvWs inv_ws(GnCarve &c, int64_t nkeys, int64_t n) {
    return {c.take<int32_t>(nkeys), c.take<int32_t>(nkeys), c.take<int32_t>(nkeys), c.take<int32_t>(1), c.take<int32_t>(n), c.take<int32_t>(n)};
}

// keys[e] outside [0, nkeys): the element belongs to no destination (an empty slot, a corner beyond the border)
static __global__ __launch_bounds__(256) void inv_count_kernel(const int32_t *__restrict__ keys, int64_t n, int64_t nkeys, InvWs w) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int k = keys[e];
    if (k >= 0 && k < nkeys) atomicAdd(&w.cnt[k], 1);
}
static __global__ __launch_bounds__(256) void inv_start_kernel(int64_t nkeys, InvWs w) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nkeys || w.cnt[k] == 0) return;
    w.start[k] = atomicAdd(w.total, w.cnt[k]);
}
static __global__ __launch_bounds__(256) void inv_list_kernel(const int32_t *__restrict__ keys, int64_t n, int64_t nkeys, InvWs w) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int k = keys[e];
    if (k >= 0 && k < nkeys) w.lst[w.start[k] + atomicAdd(&w.cursor[k], 1)] = (int)e;
}
// every element finds its rank in its destination's range (how many of the range's elements have a lower index: O(range) per element)
static __global__ __launch_bounds__(256) void inv_rank_kernel(const int32_t *__restrict__ keys, int64_t n, int64_t nkeys, InvWs w) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int k = keys[e];
    if (k < 0 || k >= nkeys) return;
    const int base = w.start[k], c = w.cnt[k];
    int rank = 0;
    for (int i = 0; i < c; ++i) rank += w.lst[base + i] < (int)e;
    w.sorted[base + rank] = (int)e;
}

// the lists from counts the caller already has in w.cnt (w.start, w.cursor and w.total zeroed; any layout): three launches
static void inv_build_counted(const int32_t *keys, int64_t n, int64_t nkeys, InvWs w, hipStream_t st) {
    const dim3 block(256), ge((unsigned)gn_cdiv(n, 256)), gk((unsigned)gn_cdiv(nkeys, 256));
    hipLaunchKernelGGL(inv_start_kernel, gk, block, 0, st, nkeys, w);
    hipLaunchKernelGGL(inv_list_kernel, ge, block, 0, st, keys, n, nkeys, w);
    hipLaunchKernelGGL(inv_rank_kernel, ge, block, 0, st, keys, n, nkeys, w);
}

// w = inv_ws(...): zero, count, build
static int inv_build(const int32_t *keys, int64_t n, int64_t nkeys, InvWs w, hipStream_t st, const char *who) {
    GN_HIP(hipMemsetAsync(w.cnt, 0, (size_t)(3 * nkeys + 1) * sizeof(int32_t), st), who);
    if (n == 0) return GN_OK;
    hipLaunchKernelGGL(inv_count_kernel, dim3((unsigned)gn_cdiv(n, 256)), dim3(256), 0, st, keys, n, nkeys, w);
    inv_build_counted(keys, n, nkeys, w, st);
    return GN_OK;
}

// Every occupied cell gets an OWNER point: the first atomicCAS on the zeroed count workspace (which point wins only decides where the cell's
// partial results live).  owner_of[p] = the owner of p's cell; npts (or NULL) [N] zeroed: the owner's entry counts its cell's points.
// CHECKED: a flat_idx outside [0, cells) belongs to no cell, owner_of[p] = -1 (a gradient call may be handed such points; the forward's
// indices come from gn_grid_features, which clamps).
template <bool CHECKED>
static __global__ __launch_bounds__(256) void cell_owner_kernel(const int32_t *__restrict__ flat_idx, int64_t N, int64_t cells, int32_t *__restrict__ count,
                                                                int32_t *__restrict__ owner_of, int32_t *__restrict__ npts) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    const int64_t cell = flat_idx[p];
    if (CHECKED && (cell < 0 || cell >= cells)) { owner_of[p] = -1; return; }
    const int old = atomicCAS(&count[cell], 0, (int)p + 1);
    const int owner = old == 0 ? (int)p : old - 1;
    owner_of[p] = owner;
    if (npts) atomicAdd(&npts[owner], 1);
}

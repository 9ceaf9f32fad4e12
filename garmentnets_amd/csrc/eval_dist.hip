// eval_dist.hip -- the all-pairs searches of the evaluation metrics (eval.py), fp64, brute force.
//
//   gn_nearest_neighbor_f64_batch  exact 1-NN (scipy cKDTree.query(k=1)) -- chamfer, hybrid chamfer, gradient threshold
//   gn_point_mesh_sqdist_batch     unsigned squared point-to-triangle-mesh distance (libigl point_mesh_squared_distance,
//                                  what igl.hausdorff calls in both directions)
//   gn_distance_field_batch        the same distance at every node of a (D, H, W) lattice over the unit cube, B meshes in one launch: the
//                                  distance, signed-distance and occupancy training targets (garmentnets_amd/distance.py)
//
// The first two take a pairs table so that one launch serves every (query set, reference set) pair of a sample: blockIdx.y = pair,
// blockIdx.x = a block of 256 queries (one per thread), blocks past the pair's query count leave at once.  The reference set
// streams through LDS in SoA tiles; every lane reads the same LDS element at a time (a broadcast).  The library is built with
// -ffp-contract=off and the per-pair arithmetic below has no fma: every distance is the plain-rounded expression written here.
// ed_dot3, pm_stage_tile / pm_load / pm_sqdist and ED_BLOCK / PM_TILE live in mesh_pair.h (query_targets.hip runs the same core).
#include "mesh_pair.h"

#define NN64_TILE 256

// ((dx*dx + dy*dy) + dz*dz): the summation order of cKDTree's squared Euclidean distance (4-way accumulators, all zero for 3-D,
// then the scalar tail), so the distances are the ones scipy returns before its sqrt
__device__ __forceinline__ double ed_sqdist3(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
    double s = __dmul_rn(dx, dx);
    s = __dadd_rn(s, __dmul_rn(dy, dy));
    return __dadd_rn(s, __dmul_rn(dz, dz));
}

__global__ __launch_bounds__(ED_BLOCK) void nn_f64_batch_kernel(const double *__restrict__ q, const double *__restrict__ ref,
                                                                const int64_t *__restrict__ pairs, int32_t *__restrict__ idx,
                                                                double *__restrict__ d2) {
    __shared__ double sx[NN64_TILE], sy[NN64_TILE], sz[NN64_TILE];
    const int64_t *pr = pairs + 4 * (int64_t)blockIdx.y;
    const int64_t q_off = pr[0], nq = pr[1], r_off = pr[2], nr = pr[3];
    const int64_t i0 = (int64_t)blockIdx.x * ED_BLOCK;
    if (i0 >= nq) return;                                   // block-uniform: no barrier is skipped by part of the block
    const int64_t i = i0 + threadIdx.x;
    const bool live = i < nq;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) { const double *p = q + 3 * (q_off + i); qx = p[0]; qy = p[1]; qz = p[2]; }
    double best = __longlong_as_double(0x7ff0000000000000LL);    // +inf
    int bi = -1;
    const double *r = ref + 3 * r_off;
    for (int64_t t0 = 0; t0 < nr; t0 += NN64_TILE) {
        const int n = (int)((nr - t0) < NN64_TILE ? (nr - t0) : NN64_TILE);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += ED_BLOCK) {
            const double *p = r + 3 * (t0 + j);
            sx[j] = p[0]; sy[j] = p[1]; sz[j] = p[2];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double d = ed_sqdist3(qx, qy, qz, sx[j], sy[j], sz[j]);
            if (d < best) { best = d; bi = (int)(t0 + j); }          // strict: ties keep the lowest index
        }
    }
    if (live) { idx[q_off + i] = bi; d2[q_off + i] = best; }
}

extern "C" int gn_nearest_neighbor_f64_batch(const double *query, const double *ref, const int64_t *pairs, int P, int64_t max_nq, int32_t *idx,
                                             double *d2, void *stream) {
    GN_REQUIRE(P >= 0 && P <= 65535 && max_nq >= 0 && max_nq < INT32_MAX, "gn_nearest_neighbor_f64_batch: bad sizes (P=%d, max_nq=%lld)", P,
               (long long)max_nq);
    if (P == 0 || max_nq == 0) return GN_OK;
    GN_REQUIRE(query && pairs && idx && d2, "gn_nearest_neighbor_f64_batch: null pointer");
    hipLaunchKernelGGL(nn_f64_batch_kernel, dim3((unsigned)gn_cdiv(max_nq, ED_BLOCK), (unsigned)P), dim3(ED_BLOCK), 0, gn_stream(stream), query, ref,
                       pairs, idx, d2);
    GN_LAUNCH_CHECK("gn_nearest_neighbor_f64_batch");
    return GN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- point -> mesh
// The staged triangle (PM_* planes), pm_stage_tile, pm_load and pm_sqdist: mesh_pair.h.
__global__ __launch_bounds__(ED_BLOCK) void point_mesh_sqdist_batch_kernel(const double *__restrict__ q, const double *__restrict__ verts,
                                                                           const int32_t *__restrict__ faces, const int64_t *__restrict__ pairs,
                                                                           int32_t *__restrict__ face_idx, double *__restrict__ d2,
                                                                           int64_t *__restrict__ bad) {
    __shared__ double tri[PM_NCONST][PM_TILE];
    const int64_t *pr = pairs + 6 * (int64_t)blockIdx.y;
    const int64_t q_off = pr[0], nq = pr[1], v_off = pr[2], nv = pr[3], f_off = pr[4], nf = pr[5];
    const int32_t *F = faces + 3 * f_off;
    const double *V = verts + 3 * v_off;
    const int64_t i0 = (int64_t)blockIdx.x * ED_BLOCK;
    if (i0 >= nq) {
        // a pair without queries still has its faces checked (once, by its first block): the wrapper raises on any bad index
        if (blockIdx.x == 0)
            for (int64_t f = threadIdx.x; f < nf; f += ED_BLOCK)
                for (int k = 0; k < 3; ++k)
                    if (F[3 * f + k] < 0 || F[3 * f + k] >= nv) *bad = 1;
        return;
    }
    const int64_t i = i0 + threadIdx.x;
    const bool live = i < nq;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) { const double *p = q + 3 * (q_off + i); qx = p[0]; qy = p[1]; qz = p[2]; }
    double best = __longlong_as_double(0x7ff0000000000000LL);    // +inf
    int bi = -1;
    for (int64_t t0 = 0; t0 < nf; t0 += PM_TILE) {
        const int n = (int)((nf - t0) < PM_TILE ? (nf - t0) : PM_TILE);
        __syncthreads();
        pm_stage_tile(tri, V, nv, F, t0, n, bad);
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double d = pm_sqdist(pm_load(tri, j), qx, qy, qz);
            if (d < best) { best = d; bi = (int)(t0 + j); }          // strict: ties keep the lowest face index
        }
    }
    if (live) {
        if (isnan(qx) || isnan(qy) || isnan(qz)) best = __longlong_as_double(0x7ff8000000000000LL);   // a NaN query has no distance
        face_idx[q_off + i] = bi;
        d2[q_off + i] = best;
    }
}

// The lattice form: every node of a (D, H, W) lattice over the unit cube against each of B meshes (blockIdx.y), the nodes formed here as
// winding_field_batch_kernel forms them.  A thread owns DF_QPT nodes in registers, a workgroup DF_SPAN consecutive ones; each broadcast read of
// a staged triangle serves all DF_QPT.  Every node scans the faces in index order with the strict `<` of the kernel above and is written by its
// one owner: no atomics, no cross-thread reduction, and (face_idx, d2) are the bits gn_point_mesh_sqdist_batch gives at the lattice points.
#define DF_QPT 4
#define DF_SPAN (ED_BLOCK * DF_QPT)

__global__ __launch_bounds__(ED_BLOCK) void distance_field_batch_kernel(const double *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                        const int64_t *__restrict__ mesh_csr, int D, int H, int W,
                                                                        int32_t *__restrict__ face_idx, double *__restrict__ d2,
                                                                        int64_t *__restrict__ bad) {
    __shared__ double tri[PM_NCONST][PM_TILE];
    const int64_t *m = mesh_csr + 2 * (int64_t)blockIdx.y;
    const int64_t v_off = m[0], nv = m[2] - m[0], f_off = m[1], nf = m[3] - m[1];
    const int32_t *F = faces + 3 * f_off;
    const double *V = verts + 3 * v_off;
    const int64_t nq = (int64_t)D * H * W;
    const int64_t i0 = (int64_t)blockIdx.x * DF_SPAN;        // < nq: the grid has cdiv(nq, DF_SPAN) blocks along x
    const double sd = (double)(D - 1), sh = (double)(H - 1), sw = (double)(W - 1);
    double qx[DF_QPT], qy[DF_QPT], qz[DF_QPT], best[DF_QPT];
    int bi[DF_QPT];
#pragma unroll
    for (int k = 0; k < DF_QPT; ++k) {
        const int64_t i = i0 + k * ED_BLOCK + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0;
        best[k] = __longlong_as_double(0x7ff0000000000000LL);    // +inf
        bi[k] = -1;
        if (i < nq) {                                        // node (id, ih, iw) is the point (id / (D-1), ih / (H-1), iw / (W-1))
            const int iw = (int)(i % W), ih = (int)((i / W) % H), id = (int)(i / ((int64_t)W * H));
            qx[k] = __ddiv_rn((double)id, sd); qy[k] = __ddiv_rn((double)ih, sh); qz[k] = __ddiv_rn((double)iw, sw);
        }
    }
    for (int64_t t0 = 0; t0 < nf; t0 += PM_TILE) {
        const int n = (int)((nf - t0) < PM_TILE ? (nf - t0) : PM_TILE);
        __syncthreads();
        pm_stage_tile(tri, V, nv, F, t0, n, bad);
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const PmTri T = pm_load(tri, j);
#pragma unroll
            for (int k = 0; k < DF_QPT; ++k) {
                const double d = pm_sqdist(T, qx[k], qy[k], qz[k]);
                if (d < best[k]) { best[k] = d; bi[k] = (int)(t0 + j); }      // strict: ties keep the lowest face index
            }
        }
    }
    const int64_t o = (int64_t)blockIdx.y * nq;
#pragma unroll
    for (int k = 0; k < DF_QPT; ++k) {
        const int64_t i = i0 + k * ED_BLOCK + threadIdx.x;
        if (i < nq) { face_idx[o + i] = bi[k]; d2[o + i] = best[k]; }
    }
}

extern "C" int gn_point_mesh_sqdist_batch(const double *query, const double *verts, const int32_t *faces, const int64_t *pairs, int P, int64_t max_nq,
                                          int32_t *face_idx, double *d2, int64_t *bad, void *stream) {
    GN_REQUIRE(P >= 0 && P <= 65535 && max_nq >= 0 && max_nq < INT32_MAX, "gn_point_mesh_sqdist_batch: bad sizes (P=%d, max_nq=%lld)", P,
               (long long)max_nq);
    if (P == 0) return GN_OK;
    GN_REQUIRE(pairs && bad, "gn_point_mesh_sqdist_batch: null pointer");
    hipLaunchKernelGGL(point_mesh_sqdist_batch_kernel, dim3((unsigned)(max_nq > 0 ? gn_cdiv(max_nq, ED_BLOCK) : 1), (unsigned)P), dim3(ED_BLOCK), 0,
                       gn_stream(stream), query, verts, faces, pairs, face_idx, d2, bad);
    GN_LAUNCH_CHECK("gn_point_mesh_sqdist_batch");
    return GN_OK;
}

extern "C" int gn_distance_field_batch(const double *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int D, int H, int W,
                                       int32_t *face_idx, double *d2, int64_t *bad, void *stream) {
    GN_REQUIRE(B >= 0 && B <= 65535, "gn_distance_field_batch: B=%d outside [0, 65535]", B);
    GN_REQUIRE(D >= 2 && H >= 2 && W >= 2 && (int64_t)D * H * W < INT32_MAX,
               "gn_distance_field_batch: lattice (%d, %d, %d): every axis needs >= 2 nodes and D*H*W < 2^31", D, H, W);
    if (B == 0) return GN_OK;
    GN_REQUIRE(mesh_csr && face_idx && d2 && bad, "gn_distance_field_batch: null pointer");
    hipLaunchKernelGGL(distance_field_batch_kernel, dim3((unsigned)gn_cdiv((int64_t)D * H * W, DF_SPAN), (unsigned)B), dim3(ED_BLOCK), 0,
                       gn_stream(stream), verts, faces, mesh_csr, D, H, W, face_idx, d2, bad);
    GN_LAUNCH_CHECK("gn_distance_field_batch");
    return GN_OK;
}

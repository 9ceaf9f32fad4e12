// winding.hip -- the generalised winding number of a triangle mesh, fp64, all pairs: the training target of the WNF stage
// (volume/nocs_winding_number_field, volume/sim_nocs_winding_number_field) built on the device.
//
//   gn_winding_number_batch   arbitrary query points against their own mesh, P (query set, mesh) pairs in one launch
//   gn_winding_field_batch    every node of a (D, H, W) lattice over the unit cube against each of B meshes, float32 out
//
// Both run wn_accumulate below.  The definition ("Winding numbers"): per (query q, face (v0, v1, v2)), with a = v0 - q, b = v1 - q,
// c = v2 - q, the Van Oosterom-Strackee solid angle omega = 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) in the operation
// order written in wn_omega; w(q) = (0 + omega_0 + omega_1 + ...) / (4 pi), the faces in index order.  No fma anywhere (the library is built
// with -ffp-contract=off and every operation below is an explicit _rn intrinsic): the two arguments of atan2 are the plain-rounded expressions
// of the numpy restatement (garmentnets_amd/winding.py), bit for bit.
//
// Shape: a thread owns WN_QPT queries (registers), a workgroup WN_BLOCK * WN_QPT of them; blockIdx.y = pair / mesh.  The faces stream through
// LDS in tiles of WN_TILE as RESOLVED vertex coordinates, SoA (9 planes), gathered once per tile; in the pair loop every lane reads the same
// LDS element (a broadcast) and each read serves WN_QPT queries.  Every query adds its faces in index order into its own register and is
// written by its one owner: no atomics, no cross-thread reduction, so w(q) is a pure function of (q, mesh) -- whatever the launch geometry,
// the other pairs of the table, or the tile size.
// wn_omega / wn_accumulate / wn_check_faces and the WN_* sizes live in mesh_pair.h (query_targets.hip runs the same core).
#include "mesh_pair.h"

__global__ __launch_bounds__(WN_BLOCK) void winding_number_batch_kernel(const double *__restrict__ q, const double *__restrict__ verts,
                                                                        const int32_t *__restrict__ faces, const int64_t *__restrict__ pairs,
                                                                        double *__restrict__ out, int64_t *__restrict__ bad) {
    __shared__ double tri[9][WN_TILE];
    const int64_t *pr = pairs + 6 * (int64_t)blockIdx.y;
    const int64_t q_off = pr[0], nq = pr[1], v_off = pr[2], nv = pr[3], f_off = pr[4], nf = pr[5];
    const int32_t *F = faces + 3 * f_off;
    const double *V = verts + 3 * v_off;
    const int64_t i0 = (int64_t)blockIdx.x * WN_SPAN;
    if (i0 >= nq) {                                          // block-uniform: no barrier is skipped by part of the block
        if (blockIdx.x == 0) wn_check_faces(F, nf, nv, bad);
        return;
    }
    double qx[WN_QPT], qy[WN_QPT], qz[WN_QPT], acc[WN_QPT];
#pragma unroll
    for (int k = 0; k < WN_QPT; ++k) {
        const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0;
        acc[k] = 0.0;
        if (i < nq) { const double *p = q + 3 * (q_off + i); qx[k] = p[0]; qy[k] = p[1]; qz[k] = p[2]; }
    }
    wn_accumulate(tri, V, nv, F, nf, qx, qy, qz, acc, bad);
#pragma unroll
    for (int k = 0; k < WN_QPT; ++k) {
        const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
        if (i < nq) out[q_off + i] = __ddiv_rn(acc[k], WN_FOUR_PI);
    }
}

__global__ __launch_bounds__(WN_BLOCK) void winding_field_batch_kernel(const double *__restrict__ verts, const int32_t *__restrict__ faces,
                                                                       const int64_t *__restrict__ mesh_csr, int D, int H, int W,
                                                                       float *__restrict__ out, int64_t *__restrict__ bad) {
    __shared__ double tri[9][WN_TILE];
    const int64_t *m = mesh_csr + 2 * (int64_t)blockIdx.y;
    const int64_t v_off = m[0], nv = m[2] - m[0], f_off = m[1], nf = m[3] - m[1];
    const int32_t *F = faces + 3 * f_off;
    const double *V = verts + 3 * v_off;
    const int64_t nq = (int64_t)D * H * W;
    const int64_t i0 = (int64_t)blockIdx.x * WN_SPAN;        // < nq: the grid has cdiv(nq, WN_SPAN) blocks along x
    const double sd = (double)(D - 1), sh = (double)(H - 1), sw = (double)(W - 1);
    double qx[WN_QPT], qy[WN_QPT], qz[WN_QPT], acc[WN_QPT];
#pragma unroll
    for (int k = 0; k < WN_QPT; ++k) {
        const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0;
        acc[k] = 0.0;
        if (i < nq) {                                        // node (id, ih, iw) is the point (id / (D-1), ih / (H-1), iw / (W-1))
            const int iw = (int)(i % W), ih = (int)((i / W) % H), id = (int)(i / ((int64_t)W * H));
            qx[k] = __ddiv_rn((double)id, sd); qy[k] = __ddiv_rn((double)ih, sh); qz[k] = __ddiv_rn((double)iw, sw);
        }
    }
    wn_accumulate(tri, V, nv, F, nf, qx, qy, qz, acc, bad);
    float *o = out + (int64_t)blockIdx.y * nq;
#pragma unroll
    for (int k = 0; k < WN_QPT; ++k) {
        const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
        if (i < nq) o[i] = __double2float_rn(__ddiv_rn(acc[k], WN_FOUR_PI));      // rounded to float once
    }
}

extern "C" int gn_winding_number_batch(const double *query, const double *verts, const int32_t *faces, const int64_t *pairs, int P, int64_t max_nq,
                                       double *out, int64_t *bad, void *stream) {
    GN_REQUIRE(P >= 0 && P <= 65535 && max_nq >= 0 && max_nq < INT32_MAX, "gn_winding_number_batch: bad sizes (P=%d, max_nq=%lld)", P,
               (long long)max_nq);
    if (P == 0) return GN_OK;
    GN_REQUIRE(pairs && bad, "gn_winding_number_batch: null pointer");
    GN_REQUIRE(max_nq == 0 || (query && out), "gn_winding_number_batch: null query / out with max_nq=%lld", (long long)max_nq);
    hipLaunchKernelGGL(winding_number_batch_kernel, dim3((unsigned)(max_nq > 0 ? gn_cdiv(max_nq, WN_SPAN) : 1), (unsigned)P), dim3(WN_BLOCK), 0,
                       gn_stream(stream), query, verts, faces, pairs, out, bad);
    GN_LAUNCH_CHECK("gn_winding_number_batch");
    return GN_OK;
}

extern "C" int gn_winding_field_batch(const double *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int D, int H, int W, float *out,
                                      int64_t *bad, void *stream) {
    GN_REQUIRE(B >= 0 && B <= 65535, "gn_winding_field_batch: B=%d outside [0, 65535]", B);
    GN_REQUIRE(D >= 2 && H >= 2 && W >= 2 && (int64_t)D * H * W < INT32_MAX,
               "gn_winding_field_batch: lattice (%d, %d, %d): every axis needs >= 2 nodes and D*H*W < 2^31", D, H, W);
    if (B == 0) return GN_OK;
    GN_REQUIRE(mesh_csr && out && bad, "gn_winding_field_batch: null pointer");
    hipLaunchKernelGGL(winding_field_batch_kernel, dim3((unsigned)gn_cdiv((int64_t)D * H * W, WN_SPAN), (unsigned)B), dim3(WN_BLOCK), 0,
                       gn_stream(stream), verts, faces, mesh_csr, D, H, W, out, bad);
    GN_LAUNCH_CHECK("gn_winding_field_batch");
    return GN_OK;
}

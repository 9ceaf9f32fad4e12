// query_targets.hip -- the second stage's training target at arbitrary query points, from the garment's mesh alone (DESIGN.md "Exact volume targets"):
// the generalised winding number and / or the squared distance to the mesh, fp64, all pairs, and the float32 target of the dataset's volume_group made
// of them.  The shape "few queries, many faces" of a training batch: B x M queries (24 x 6000), ~10 000 faces each.
//
//   gn_query_targets_batch     B query sets (B, M, 3) fp32 against B meshes through the CSR table of gn_winding_field_batch (fp32 vertices)
//   gn_resident_query_targets  the same launches on the meshes of a resident store, one garment per slots[b] (csrc/resident.hip)
//
// Definition (garmentnets_amd/targets.py restates it in numpy).  A query's fp32 coordinates and the fp32 vertices are widened exactly.  The faces are cut
// into chunks of QT_FACE_CHUNK consecutive faces.  w: every chunk's solid angles (wn_omega) are added in face order from 0, the chunk sums are added in
// ascending chunk order from 0, the total is divided by 4 pi -- winding.py's sum with one change of order, and its very bits when F <= QT_FACE_CHUNK.
// (d2, face_idx): the strict `<` minimum of pm_sqdist in face order inside a chunk, then over the chunks in ascending order: the lowest face index still
// wins, so both are gn_point_mesh_sqdist_batch's bits for every F.  The per-pair cores are mesh_pair.h's, shared with winding.hip and eval_dist.hip.
//
// Shape: grid = (blocks of QT_SPAN queries, face chunks, garments).  partial kernel: a thread owns QT_QPT queries in registers, a workgroup QT_SPAN; its
// chunk streams through LDS in tiles of PM_TILE faces (a broadcast read per lane, serving the thread's QT_QPT queries); ONE partial (w_c, d2_c, face_c) per
// (query, chunk) goes to the workspace.  fold kernel: one thread per query adds / compares its partials in ascending chunk order and writes the target.  No
// atomics, one writer per value: identical calls give identical bits and a query's result does not depend on B, M, the grid or its neighbours.
#include "mesh_pair.h"

#define QT_FACE_CHUNK GN_QT_FACE_CHUNK
#define QT_QPT WN_QPT
#define QT_SPAN (WN_BLOCK * QT_QPT)
#define QT_FOLD_WG 256

static_assert(WN_TILE == PM_TILE && WN_BLOCK == ED_BLOCK, "the two cores share one LDS tile and one workgroup");
static_assert(QT_FACE_CHUNK % PM_TILE == 0, "a chunk is a whole number of LDS tiles");

// where the B meshes are: a CSR table (gn_query_targets_batch) or a resident store's meta rows through slots (gn_resident_query_targets)
struct QtMeshes {
    const float *verts;              // [sum V][3]
    const int32_t *faces;            // [sum F][3], vertex numbers within the mesh
    const int64_t *csr;              // [B + 1][2] = {v_off, f_off}, or NULL
    const int64_t *meta;             // GnResidentStore.meta
    const int32_t *slots;            // [B]
    int64_t total_verts;             // rows of the store's vertex arrays (the end of the last sample's)
    int32_t n;                       // samples of the store
};
struct QtMesh {
    const float *V;
    const int32_t *F;
    int64_t nv, nf;
};

__device__ __forceinline__ bool qt_mesh(const QtMeshes &ms, int b, QtMesh &m) {
    int64_t v_off, f_off;
    if (ms.csr != nullptr) {
        const int64_t *r = ms.csr + 2 * (int64_t)b;
        v_off = r[0]; f_off = r[1]; m.nv = r[2] - r[0]; m.nf = r[3] - r[1];
    } else {
        const int slot = ms.slots[b];
        if (slot < 0 || slot >= ms.n) return false;                  // (a slot outside the store writes nothing, as the gn_resident_* entries)
        const int64_t *r = ms.meta + (int64_t)slot * GN_RESIDENT_META;
        v_off = r[GN_RESIDENT_VERT_OFF]; f_off = r[GN_RESIDENT_FACE_OFF]; m.nf = r[GN_RESIDENT_NUM_FACES];
        m.nv = (slot + 1 < ms.n ? r[GN_RESIDENT_META + GN_RESIDENT_VERT_OFF] : ms.total_verts) - v_off;
    }
    m.V = ms.verts + 3 * v_off;
    m.F = ms.faces + 3 * f_off;
    return true;
}

__device__ __forceinline__ bool qt_needs_w(int kind) { return kind != GN_QT_DISTANCE; }
__device__ __forceinline__ bool qt_needs_d(int kind) { return kind == GN_QT_DISTANCE || kind == GN_QT_SIGNED_DISTANCE; }

// the QT_QPT queries of this thread, widened exactly: query i0 + k * WN_BLOCK + threadIdx.x of the garment's M (zeros past the end: never written)
__device__ __forceinline__ void qt_load_queries(const float *__restrict__ q, int64_t i0, int M, double (&qx)[QT_QPT], double (&qy)[QT_QPT], double (&qz)[QT_QPT]) {
#pragma unroll
    for (int k = 0; k < QT_QPT; ++k) {
        const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0;
        if (i < M) { const float *p = q + 3 * i; qx[k] = (double)p[0]; qy[k] = (double)p[1]; qz[k] = (double)p[2]; }
    }
}

// partials of chunk blockIdx.y of garment blockIdx.z for QT_SPAN queries: ws_w / ws_d2 / ws_face [B][C][M].  amdgpu_waves_per_eu(4, 4): the <true, true> form
// lands one register past the 128-VGPR step without it (129, 3 waves per SIMD); held to 4 waves it takes 127 and spills no vector register.
template <bool NEED_W, bool NEED_D>
__global__ __launch_bounds__(WN_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void query_targets_partial_kernel(QtMeshes ms, const float *__restrict__ query, int M, int C, double *__restrict__ ws_w,
                                                                         double *__restrict__ ws_d2, int32_t *__restrict__ ws_face, int64_t *__restrict__ bad) {
    __shared__ double tri[NEED_D ? (int)PM_NCONST : 9][PM_TILE];
    const int b = blockIdx.z, c = blockIdx.y;
    QtMesh m;
    if (!qt_mesh(ms, b, m)) return;
    if (m.nf > (int64_t)C * QT_FACE_CHUNK) {                         // max_nf promised fewer faces: flagged, the mesh is not walked
        if (threadIdx.x == 0) bad[1] = 1;
        return;
    }
    const int64_t c0 = (int64_t)c * QT_FACE_CHUNK;
    if (c0 >= m.nf) return;                                          // block-uniform: no barrier is skipped by part of the block
    const int64_t left = m.nf - c0;
    const int nc = (int)(left < QT_FACE_CHUNK ? left : QT_FACE_CHUNK);
    const int32_t *F = m.F + 3 * c0;
    const int64_t i0 = (int64_t)blockIdx.x * QT_SPAN;
    if (i0 >= M) {                                                   // no queries (M == 0): the faces are still checked
        if (blockIdx.x == 0) wn_check_faces(F, nc, m.nv, bad);
        return;
    }
    const int64_t o = ((int64_t)b * C + c) * M;
    if (NEED_W) {
        double qx[QT_QPT], qy[QT_QPT], qz[QT_QPT], acc[QT_QPT];
        qt_load_queries(query + 3 * (int64_t)b * M, i0, M, qx, qy, qz);
#pragma unroll
        for (int k = 0; k < QT_QPT; ++k) acc[k] = 0.0;
        wn_accumulate(tri, m.V, m.nv, F, (int64_t)nc, qx, qy, qz, acc, bad);
#pragma unroll
        for (int k = 0; k < QT_QPT; ++k) {
            const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
            if (i < M) ws_w[o + i] = acc[k];
        }
    }
    if (NEED_D) {                                                    // (the thread's queries are read again: the two passes share no registers)
        double qx[QT_QPT], qy[QT_QPT], qz[QT_QPT], best[QT_QPT];
        int bi[QT_QPT];
        qt_load_queries(query + 3 * (int64_t)b * M, i0, M, qx, qy, qz);
#pragma unroll
        for (int k = 0; k < QT_QPT; ++k) {
            best[k] = __longlong_as_double(0x7ff0000000000000LL);    // +inf
            bi[k] = -1;
        }
        for (int t0 = 0; t0 < nc; t0 += PM_TILE) {
            const int n = (nc - t0) < PM_TILE ? (nc - t0) : PM_TILE;
            __syncthreads();
            pm_stage_tile(tri, m.V, m.nv, F, (int64_t)t0, n, bad);
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                const PmTri T = pm_load(tri, j);
#pragma unroll
                for (int k = 0; k < QT_QPT; ++k) {
                    const double d = pm_sqdist(T, qx[k], qy[k], qz[k]);
                    if (d < best[k]) { best[k] = d; bi[k] = (int)(c0 + t0 + j); }      // strict: ties keep the lowest face index
                }
            }
        }
#pragma unroll
        for (int k = 0; k < QT_QPT; ++k) {
            const int64_t i = i0 + k * WN_BLOCK + threadIdx.x;
            if (i < M) { ws_d2[o + i] = best[k]; ws_face[o + i] = bi[k]; }
        }
    }
}

// np.clip: a NaN stays a NaN
__device__ __forceinline__ double qt_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ float qt_clipf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the float32 target of `kind` from (w, d2): distance.py's rules at a point, then data_io's tsdf_clip_value and volume_absolute_value steps
__device__ __forceinline__ float qt_target(int kind, double w, double d2, int use_clip, float tsdf_clip, int absolute) {
    const float w32 = __double2float_rn(w);
    float v;
    if (kind == GN_QT_WINDING) {
        v = w32;
    } else if (kind == GN_QT_DISTANCE) {
        v = __double2float_rn(__dsqrt_rn(d2));
    } else if (kind == GN_QT_SIGNED_DISTANCE) {
        const double sign = qt_clip(__dsub_rn(1.0, __dmul_rn(2.0, (double)w32)), -1.0, 1.0);
        v = __double2float_rn(__dmul_rn(sign, __dsqrt_rn(d2)));
    } else {
        v = w32 > 0.5f ? 1.0f : 0.0f;
    }
    if (use_clip) v = qt_clipf(__fdiv_rn(v, tsdf_clip), -1.0f, 1.0f);
    if (absolute) v = fabsf(v);
    return v;
}

// one thread per query: its partials in ascending chunk order -> w, (d2, face_idx), the target
__global__ __launch_bounds__(QT_FOLD_WG) void query_targets_fold_kernel(QtMeshes ms, const float *__restrict__ query, int M, int C, int kind, int use_clip,
                                                                        float tsdf_clip, int absolute, const double *__restrict__ ws_w,
                                                                        const double *__restrict__ ws_d2, const int32_t *__restrict__ ws_face,
                                                                        float *__restrict__ target, double *__restrict__ w_out, double *__restrict__ d2_out,
                                                                        int32_t *__restrict__ face_out) {
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * QT_FOLD_WG + threadIdx.x;
    QtMesh m;
    if (i >= M || !qt_mesh(ms, b, m) || m.nf > (int64_t)C * QT_FACE_CHUNK) return;
    const int nchunks = (int)((m.nf + QT_FACE_CHUNK - 1) / QT_FACE_CHUNK);
    const int64_t o = (int64_t)b * M + i;
    double w = 0.0, best = __longlong_as_double(0x7ff0000000000000LL);   // an empty mesh: w = 0, d2 = +inf
    int bi = -1;
    if (qt_needs_w(kind)) {
        double total = 0.0;
        for (int c = 0; c < nchunks; ++c) total = __dadd_rn(total, ws_w[((int64_t)b * C + c) * M + i]);
        w = __ddiv_rn(total, WN_FOUR_PI);
        if (w_out != nullptr) w_out[o] = w;
    }
    if (qt_needs_d(kind)) {
        for (int c = 0; c < nchunks; ++c) {
            const double d = ws_d2[((int64_t)b * C + c) * M + i];
            if (d < best) { best = d; bi = ws_face[((int64_t)b * C + c) * M + i]; }
        }
        const float *p = query + 3 * o;
        if (isnan(p[0]) || isnan(p[1]) || isnan(p[2])) best = __longlong_as_double(0x7ff8000000000000LL);   // a NaN query has no distance
        if (d2_out != nullptr) d2_out[o] = best;
        if (face_out != nullptr) face_out[o] = bi;
    }
    target[o] = qt_target(kind, w, best, use_clip, tsdf_clip, absolute);
}

static int64_t qt_chunks(int64_t max_nf) { return max_nf > 0 ? gn_cdiv(max_nf, QT_FACE_CHUNK) : 1; }
static bool qt_kind_ok(int kind) { return kind >= GN_QT_WINDING && kind <= GN_QT_OCCUPANCY; }
static bool qt_host_needs_w(int kind) { return kind != GN_QT_DISTANCE; }
static bool qt_host_needs_d(int kind) { return kind == GN_QT_DISTANCE || kind == GN_QT_SIGNED_DISTANCE; }

extern "C" int gn_query_targets_face_chunk(void) { return QT_FACE_CHUNK; }

// the partials, [B][chunks][M] each: d2 and face for the kinds that fold a distance, w for those that fold a winding number (the doubles first, the
// int32 face numbers last: every part aligned).  A part the kind does not need is empty; the kernels never touch its pointer.
struct QtWs { double *d2, *w; int32_t *face; };
static QtWs qt_ws(GnCarve &c, int B, int64_t M, int64_t max_nf, int kind) {
    const size_t n = (size_t)B * (size_t)qt_chunks(max_nf) * (size_t)M;
    return {c.take<double>(qt_host_needs_d(kind) ? n : 0), c.take<double>(qt_host_needs_w(kind) ? n : 0), c.take<int32_t>(qt_host_needs_d(kind) ? n : 0)};
}

extern "C" size_t gn_query_targets_workspace_bytes(int B, int64_t M, int64_t max_nf, int kind) {
    return (B <= 0 || M <= 0 || max_nf < 0 || !qt_kind_ok(kind)) ? 0 : gn_carve_bytes(qt_ws, B, M, max_nf, kind);
}

// the workspace check and the two launches of both entries (every other argument checked by the caller)
static int qt_launch(const char *who, const QtMeshes &ms, const float *query, int B, int64_t M, int64_t max_nf, int kind, int use_clip, float tsdf_clip,
                     int absolute, void *ws, size_t ws_bytes, float *target, double *w, double *d2, int32_t *face_idx, int64_t *bad, void *stream) {
    GnCarve c(ws);
    const auto [ws_d2, ws_w, ws_face] = qt_ws(c, B, M, max_nf, kind);
    GN_REQUIRE(c.off == 0 || (ws && ws_bytes >= c.off), "%s: short workspace (%zu bytes, %zu needed)", who, ws ? ws_bytes : (size_t)0, c.off);
    const int64_t C = qt_chunks(max_nf);
    const bool need_w = qt_host_needs_w(kind), need_d = qt_host_needs_d(kind);
    const dim3 grid((unsigned)(M > 0 ? gn_cdiv(M, QT_SPAN) : 1), (unsigned)C, (unsigned)B);
    hipStream_t st = gn_stream(stream);
    if (need_w && need_d)
        hipLaunchKernelGGL((query_targets_partial_kernel<true, true>), grid, dim3(WN_BLOCK), 0, st, ms, query, (int)M, (int)C, ws_w, ws_d2, ws_face, bad);
    else if (need_w)
        hipLaunchKernelGGL((query_targets_partial_kernel<true, false>), grid, dim3(WN_BLOCK), 0, st, ms, query, (int)M, (int)C, ws_w, ws_d2, ws_face, bad);
    else
        hipLaunchKernelGGL((query_targets_partial_kernel<false, true>), grid, dim3(WN_BLOCK), 0, st, ms, query, (int)M, (int)C, ws_w, ws_d2, ws_face, bad);
    GN_LAUNCH_CHECK(who);
    if (M == 0) return GN_OK;
    hipLaunchKernelGGL(query_targets_fold_kernel, dim3((unsigned)gn_cdiv(M, QT_FOLD_WG), (unsigned)B), dim3(QT_FOLD_WG), 0, st, ms, query, (int)M, (int)C, kind,
                       use_clip, tsdf_clip, absolute, ws_w, ws_d2, ws_face, target, w, d2, face_idx);
    GN_LAUNCH_CHECK(who);
    return GN_OK;
}

extern "C" int gn_query_targets_batch(const float *query, const float *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int64_t M, int64_t max_nf,
                                      int kind, int use_clip, float tsdf_clip, int absolute, void *ws, size_t ws_bytes, float *target, double *w, double *d2,
                                      int32_t *face_idx, int64_t *bad, void *stream) {
    GN_REQUIRE(B >= 0 && B <= 65535 && M >= 0 && M < INT32_MAX && max_nf >= 0 && qt_chunks(max_nf) <= 65535,
               "gn_query_targets_batch: bad sizes (B=%d, M=%lld, max_nf=%lld): B <= 65535, M < 2^31, max_nf <= 65535 * %d", B, (long long)M, (long long)max_nf,
               QT_FACE_CHUNK);
    GN_REQUIRE(qt_kind_ok(kind), "gn_query_targets_batch: unknown kind %d", kind);
    if (B == 0) return GN_OK;
    GN_REQUIRE(mesh_csr && bad, "gn_query_targets_batch: null pointer (mesh_csr / bad)");
    GN_REQUIRE(max_nf == 0 || (verts && faces), "gn_query_targets_batch: null pointer (verts / faces with max_nf=%lld)", (long long)max_nf);
    GN_REQUIRE(M == 0 || (query && target), "gn_query_targets_batch: null pointer (query / target with M=%lld)", (long long)M);
    const QtMeshes ms = {verts, faces, mesh_csr, nullptr, nullptr, 0, 0};
    return qt_launch("gn_query_targets_batch", ms, query, B, M, max_nf, kind, use_clip, tsdf_clip, absolute, ws, ws_bytes, target, w, d2, face_idx, bad, stream);
}

extern "C" int gn_resident_query_targets(const GnResidentStore *store, const int32_t *slots, int B, int64_t M, int task_space, int64_t total_verts,
                                         int64_t max_nf, int kind, int use_clip, float tsdf_clip, int absolute, const float *query, void *ws, size_t ws_bytes,
                                         float *value, int64_t *bad, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && M >= 1 && M < INT32_MAX && max_nf >= 1 && qt_chunks(max_nf) <= 65535 && total_verts >= 0,
               "gn_resident_query_targets: 1 <= B <= 65535 garments of 1 <= M < 2^31 queries, 1 <= max_nf <= 65535 * %d", QT_FACE_CHUNK);
    GN_REQUIRE(qt_kind_ok(kind), "gn_resident_query_targets: unknown kind %d", kind);
    GN_REQUIRE(store->meta && store->faces && slots && query && value && bad, "gn_resident_query_targets: null pointer");
    const float *verts = task_space ? store->task_verts : store->nocs_verts;
    GN_REQUIRE(verts != nullptr, "gn_resident_query_targets: the store holds no %s vertices", task_space ? "task-space" : "NOCS");
    const QtMeshes ms = {verts, store->faces, nullptr, store->meta, slots, total_verts, store->n};
    return qt_launch("gn_resident_query_targets", ms, query, B, M, max_nf, kind, use_clip, tsdf_clip, absolute, ws, ws_bytes, value, nullptr, nullptr, nullptr, bad, stream);
}

// resident.hip -- gn_resident_*: a training batch assembled on the device from the resident dataset (garmentnets_amd/io/resident.py, DESIGN.md
// "Resident dataset").  The raw samples live in a few packed device arrays (GnResidentStore); the host draws every random number (io/dataset.py
// SeededDraws) and uploads them; these kernels do what GarmentInputDataset.__getitem__ and collate() do with them, in numpy's operation order:
//   gn_resident_points      the selected rows of the cloud -> x, y, pos (noise, rotation) and the batch vector
//   gn_resident_garment     the per-garment fields: nearest selected point to the grip vertex (segmented arg-min), grip points, bookkeeping
//   gn_resident_volume      volume queries (uniform | near the NOCS mesh) and the garment's own volume there (trilinear, ATen's CPU order)
//   gn_resident_volume_queries  those queries alone (exact targets: gn_resident_query_targets of query_targets.hip takes the values from the mesh)
//   gn_resident_surface     points of the garment mesh in query space and their targets
//   gn_resident_mc_surface  points of the marching-cubes mesh and their on-surface flag
//
// One garment per blockIdx.y, its resident sample from the device index table `slots`; the launch count does not depend on B.  No atomics; every
// value has one writer and a fixed operation order (explicit _rn intrinsics, no contraction): identical calls give identical bits.
#include "common.h"

#pragma clang fp contract(off)

#define RES_WG 256

__device__ __forceinline__ const int64_t *res_meta(const GnResidentStore &s, const int32_t *slots, int b) {
    const int slot = slots[b];
    return (slot < 0 || slot >= s.n) ? nullptr : s.meta + (int64_t)slot * GN_RESIDENT_META;
}

// numpy's (p @ R.T)[j] for one row: (x * R[j][0] + y * R[j][1]) + z * R[j][2], every step rounded
__device__ __forceinline__ float res_rot32(const float *R, int j, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x, R[j * 3]), __fmul_rn(y, R[j * 3 + 1])), __fmul_rn(z, R[j * 3 + 2]));
}
__device__ __forceinline__ float res_rot64(const float *R, int j, double x, double y, double z) {
    return (float)__dadd_rn(__dadd_rn(__dmul_rn(x, (double)R[j * 3]), __dmul_rn(y, (double)R[j * 3 + 1])), __dmul_rn(z, (double)R[j * 3 + 2]));
}
// ((q - pivot) @ R.T + pivot) about TASK_SPACE_PIVOT = (0.5, 0.5, 0)
__device__ __forceinline__ void res_pivot_rot(const float *R, float q[3]) {
    const float dx = __fsub_rn(q[0], 0.5f), dy = __fsub_rn(q[1], 0.5f), dz = __fsub_rn(q[2], 0.0f);
    q[0] = __fadd_rn(res_rot32(R, 0, dx, dy, dz), 0.5f);
    q[1] = __fadd_rn(res_rot32(R, 1, dx, dy, dz), 0.5f);
    q[2] = __fadd_rn(res_rot32(R, 2, dx, dy, dz), 0.0f);
}

// mesh_sample_barycentric on given draws: the face is the upper bound of its uniform in the fp64 CDF (RandomState.choice's searchsorted side="right");
// u, v reflected when u + v >= 1; w = 1 - (u + v)
struct ResPick {
    int face;
    double bc[3];
};
__device__ __forceinline__ ResPick res_pick(const double *__restrict__ cdf, int nf, double fu, double u, double v) {
    int lo = 0, hi = nf;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= fu) lo = mid + 1; else hi = mid;
    }
    ResPick p;
    p.face = lo < nf ? lo : nf - 1;
    if (__dadd_rn(u, v) >= 1.0) {
        u = __dsub_rn(1.0, u);
        v = __dsub_rn(1.0, v);
    }
    p.bc[0] = u;
    p.bc[1] = v;
    p.bc[2] = __dsub_rn(1.0, __dadd_rn(u, v));
    return p;
}
// barycentric_interpolation: acc32 = float(double(acc32) + bc_i * double(v_i)), i = 0, 1, 2; `vals` rows of `width` floats, column c
__device__ __forceinline__ float res_bary(const float *__restrict__ vals, int width, int c, const int32_t *__restrict__ tri, const ResPick &p) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) acc = (float)__dadd_rn((double)acc, __dmul_rn(p.bc[i], (double)vals[(int64_t)tri[i] * width + c]));
    return acc;
}

// ------------------------------------------------------------------------------------------------ points
__global__ __launch_bounds__(RES_WG) void resident_points_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int P, const int32_t *__restrict__ sel,
                                                                 const double *__restrict__ noise, const float *__restrict__ rot, float *__restrict__ x,
                                                                 float *__restrict__ y, float *__restrict__ pos, int64_t *__restrict__ batch) {
    const int b = blockIdx.y, i = blockIdx.x * RES_WG + threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (i >= P || m == nullptr) return;
    int64_t r = sel[(int64_t)b * P + i];
    if (r < 0 || r >= m[GN_RESIDENT_PC_LEN]) r = 0;               // (the host draws indices of the stored cloud; never read outside it)
    const int64_t src = (m[GN_RESIDENT_PC_OFF] + r) * 3, dst = ((int64_t)b * P + i) * 3;
    const float px = s.pc_sim[src], py = s.pc_sim[src + 1], pz = s.pc_sim[src + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        x[dst + c] = __fdiv_rn((float)s.pc_rgb[src + c], 255.0f);
        y[dst + c] = s.pc_nocs[src + c];
    }
    batch[(int64_t)b * P + i] = b;
    const float *R = rot == nullptr ? nullptr : rot + (int64_t)b * 9;
    if (noise != nullptr) {                                        // numpy promotes pos + jitter to fp64; the rotation then runs in fp64
        const double *nz = noise + dst;
        const double dx = __dadd_rn((double)px, nz[0]), dy = __dadd_rn((double)py, nz[1]), dz = __dadd_rn((double)pz, nz[2]);
        if (R != nullptr) {
#pragma unroll
            for (int j = 0; j < 3; ++j) pos[dst + j] = res_rot64(R, j, dx, dy, dz);
        } else {
            pos[dst] = (float)dx;
            pos[dst + 1] = (float)dy;
            pos[dst + 2] = (float)dz;
        }
    } else if (R != nullptr) {
#pragma unroll
        for (int j = 0; j < 3; ++j) pos[dst + j] = res_rot32(R, j, px, py, pz);
    } else {
        pos[dst] = px;
        pos[dst + 1] = py;
        pos[dst + 2] = pz;
    }
}

extern "C" int gn_resident_points(const GnResidentStore *store, const int32_t *slots, int B, int P, const int32_t *sel, const double *noise, const float *rot,
                                  float *x, float *y, float *pos, int64_t *batch, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && P >= 1, "gn_resident_points: 1 <= B <= 65535 garments of P >= 1 points");
    GN_REQUIRE(store->pc_sim && store->pc_nocs && store->pc_rgb && store->meta && slots && sel && x && y && pos && batch, "gn_resident_points: null pointer");
    hipLaunchKernelGGL(resident_points_kernel, dim3((unsigned)gn_cdiv(P, RES_WG), (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, P, sel, noise,
                       rot, x, y, pos, batch);
    GN_LAUNCH_CHECK("gn_resident_points");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ per-garment fields
// one workgroup per garment: np.argmin(np.linalg.norm(pos - grip, axis=1)) over the selected, un-noised, un-rotated rows: fp32
// sqrt((dx*dx + dy*dy) + dz*dz), the first index of the minimum
__global__ __launch_bounds__(RES_WG) void resident_garment_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int P, const int32_t *__restrict__ sel,
                                                                  const float *__restrict__ rot, int64_t *__restrict__ grip_pc_idx, float *__restrict__ sim_grip,
                                                                  float *__restrict__ nocs_grip, int64_t *__restrict__ scale_bits, int64_t *__restrict__ dataset_idx,
                                                                  float *__restrict__ aabb, float *__restrict__ rot_out) {
    __shared__ float sv[RES_WG];
    __shared__ int si[RES_WG];
    const int b = blockIdx.y, t = threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (m == nullptr) return;
    const float *g = s.grip + (int64_t)slots[b] * 6;
    float best = INFINITY;
    int arg = P;
    for (int i = t; i < P; i += RES_WG) {
        int64_t r = sel[(int64_t)b * P + i];
        if (r < 0 || r >= m[GN_RESIDENT_PC_LEN]) r = 0;
        const float *p = s.pc_sim + (m[GN_RESIDENT_PC_OFF] + r) * 3;
        const float d = (float)__dsqrt_rn((double)gn_sqdist3(p[0], p[1], p[2], g[0], g[1], g[2]));     // correctly rounded fp32 root (losses.hip)
        if (d < best || arg == P) {
            best = d;
            arg = i;
        }
    }
    sv[t] = best;
    si[t] = arg;
    __syncthreads();
    for (int off = RES_WG / 2; off >= 1; off >>= 1) {
        if (t < off) {
            const float ov = sv[t + off];
            const int oi = si[t + off];
            if (oi < P && (si[t] == P || ov < sv[t] || (ov == sv[t] && oi < si[t]))) {
                sv[t] = ov;
                si[t] = oi;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        grip_pc_idx[b] = si[0];
        scale_bits[b] = m[GN_RESIDENT_SCALE_BITS];
        dataset_idx[b] = m[GN_RESIDENT_DATASET_IDX];
    }
    const float *R = rot == nullptr ? nullptr : rot + (int64_t)b * 9;
    if (t < 3) {
        sim_grip[b * 3 + t] = R == nullptr ? g[t] : res_rot32(R, t, g[0], g[1], g[2]);
        nocs_grip[b * 3 + t] = g[3 + t];
    }
    if (t < 6) aabb[b * 6 + t] = s.aabb[t];
    if (t < 9) rot_out[b * 9 + t] = R == nullptr ? (t % 4 == 0 ? 1.f : 0.f) : R[t];
}

extern "C" int gn_resident_garment(const GnResidentStore *store, const int32_t *slots, int B, int P, const int32_t *sel, const float *rot, int64_t *grip_pc_idx,
                                   float *sim_grip, float *nocs_grip, int64_t *scale_bits, int64_t *dataset_idx, float *aabb, float *rot_out, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && P >= 1, "gn_resident_garment: 1 <= B <= 65535 garments of P >= 1 points");
    GN_REQUIRE(store->pc_sim && store->meta && store->grip && store->aabb && slots && sel && grip_pc_idx && sim_grip && nocs_grip && scale_bits && dataset_idx &&
                   aabb && rot_out, "gn_resident_garment: null pointer");
    hipLaunchKernelGGL(resident_garment_kernel, dim3(1, (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, P, sel, rot, grip_pc_idx, sim_grip,
                       nocs_grip, scale_bits, dataset_idx, aabb, rot_out);
    GN_LAUNCH_CHECK("gn_resident_garment");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ volume targets
// dataset.nocs_grid_sample for one point: fp32, coordinate ((2q - 1) + 1) / 2 * (size - 1) clipped to [0, size - 1]; corner weight (w_W * w_H) * w_D; the
// eight corners added to 0 in (D, H, W) bit order, those past the far face skipped
__device__ __forceinline__ float res_trilinear(const float *__restrict__ vol, int D, int H, int W, const float q[3]) {
    const int n[3] = {D, H, W};
    int lo[3];
    float w[3][2];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float top = (float)(n[ax] - 1);
        float c = __fmul_rn(__fdiv_rn(__fadd_rn(__fsub_rn(__fmul_rn(2.0f, q[ax]), 1.0f), 1.0f), 2.0f), top);
        c = fminf(top, fmaxf(c, 0.0f));
        const float f0 = floorf(c);
        lo[ax] = (int)f0;
        w[ax][0] = __fsub_rn(__fadd_rn(f0, 1.0f), c);
        w[ax][1] = __fsub_rn(c, f0);
    }
    float out = 0.f;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int b0 = (corner >> 2) & 1, b1 = (corner >> 1) & 1, b2 = corner & 1;
        const int i0 = lo[0] + b0, i1 = lo[1] + b1, i2 = lo[2] + b2;
        if (i0 > D - 1 || i1 > H - 1 || i2 > W - 1) continue;
        const float wt = __fmul_rn(__fmul_rn(w[2][b2], w[1][b1]), w[0][b0]);
        out = __fadd_rn(out, __fmul_rn(vol[((int64_t)i0 * H + i1) * W + i2], wt));
    }
    return out;
}

// volume query i of garment b (its meta row m): the first n_uniform are the uploaded uniform points; the others a point of the NOCS mesh plus noise (fp64),
// rounded to fp32, clipped to [0, 1].  Shared by resident_volume_kernel and resident_volume_queries_kernel: the two form the same bits.
__device__ __forceinline__ void res_volume_query(const GnResidentStore &s, const int64_t *m, int b, int i, int M, int n_uniform, const float *__restrict__ uniform,
                                                 const double *__restrict__ face_u, const double *__restrict__ uv, const double *__restrict__ noise, float q[3]) {
    if (i < n_uniform) {
        const float *u = uniform + ((int64_t)b * n_uniform + i) * 3;
        q[0] = u[0];
        q[1] = u[1];
        q[2] = u[2];
    } else {                                                       // a point of the NOCS mesh plus noise (fp64), rounded to fp32, clipped to [0, 1]
        const int64_t j = (int64_t)b * (M - n_uniform) + (i - n_uniform);
        const ResPick p = res_pick(s.cdf_nocs + m[GN_RESIDENT_FACE_OFF], (int)m[GN_RESIDENT_NUM_FACES], face_u[j], uv[j * 2], uv[j * 2 + 1]);
        const int32_t *tri = s.faces + (m[GN_RESIDENT_FACE_OFF] + p.face) * 3;
        const float *verts = s.nocs_verts + m[GN_RESIDENT_VERT_OFF] * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (float)__dadd_rn((double)res_bary(verts, 3, c, tri, p), noise[j * 3 + c]);
            q[c] = fminf(fmaxf(v, 0.0f), 1.0f);
        }
    }
}

__global__ __launch_bounds__(RES_WG) void resident_volume_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int M, int n_uniform,
                                                                 const float *__restrict__ uniform, const double *__restrict__ face_u,
                                                                 const double *__restrict__ uv, const double *__restrict__ noise, const float *__restrict__ rot,
                                                                 int occupancy, float *__restrict__ query, float *__restrict__ value) {
    const int b = blockIdx.y, i = blockIdx.x * RES_WG + threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (i >= M || m == nullptr) return;
    float q[3];
    res_volume_query(s, m, b, i, M, n_uniform, uniform, face_u, uv, noise, q);
    float v = res_trilinear(s.volume + (int64_t)slots[b] * s.D * s.H * s.W, s.D, s.H, s.W, q);
    if (occupancy) v = v > 0.1f ? 1.0f : 0.0f;
    if (rot != nullptr) res_pivot_rot(rot + (int64_t)b * 9, q);    // after the values are taken
    const int64_t o = (int64_t)b * M + i;
    query[o * 3] = q[0];
    query[o * 3 + 1] = q[1];
    query[o * 3 + 2] = q[2];
    value[o] = v;
}

extern "C" int gn_resident_volume(const GnResidentStore *store, const int32_t *slots, int B, int M, int n_uniform, const float *uniform, const double *face_u,
                                  const double *uv, const double *noise, const float *rot, int occupancy, float *query, float *value, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && M >= 1 && n_uniform >= 0 && n_uniform <= M, "gn_resident_volume: 1 <= B <= 65535, 0 <= n_uniform <= M");
    GN_REQUIRE(store->volume && store->meta && store->D >= 1 && store->H >= 1 && store->W >= 1 && slots && query && value, "gn_resident_volume: no resident volume");
    GN_REQUIRE(n_uniform == 0 || uniform != nullptr, "gn_resident_volume: the uniform points are required");
    GN_REQUIRE(n_uniform == M || (face_u && uv && noise && store->cdf_nocs && store->faces && store->nocs_verts),
               "gn_resident_volume: near-surface queries need face_u, uv, noise and the resident NOCS mesh with its CDF");
    hipLaunchKernelGGL(resident_volume_kernel, dim3((unsigned)gn_cdiv(M, RES_WG), (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, M, n_uniform,
                       uniform, face_u, uv, noise, rot, occupancy, query, value);
    GN_LAUNCH_CHECK("gn_resident_volume");
    return GN_OK;
}

// the queries of gn_resident_volume alone: `plain` (optional) before the turn, what gn_resident_query_targets (query_targets.hip) evaluates the mesh's own
// field at; `query` as the batch carries them (turned about the pivot when rot is given)
__global__ __launch_bounds__(RES_WG) void resident_volume_queries_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int M, int n_uniform,
                                                                         const float *__restrict__ uniform, const double *__restrict__ face_u,
                                                                         const double *__restrict__ uv, const double *__restrict__ noise, const float *__restrict__ rot,
                                                                         float *__restrict__ plain, float *__restrict__ query) {
    const int b = blockIdx.y, i = blockIdx.x * RES_WG + threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (i >= M || m == nullptr) return;
    float q[3];
    res_volume_query(s, m, b, i, M, n_uniform, uniform, face_u, uv, noise, q);
    const int64_t o = (int64_t)b * M + i;
    if (plain != nullptr) {
        plain[o * 3] = q[0];
        plain[o * 3 + 1] = q[1];
        plain[o * 3 + 2] = q[2];
    }
    if (rot != nullptr) res_pivot_rot(rot + (int64_t)b * 9, q);
    query[o * 3] = q[0];
    query[o * 3 + 1] = q[1];
    query[o * 3 + 2] = q[2];
}

extern "C" int gn_resident_volume_queries(const GnResidentStore *store, const int32_t *slots, int B, int M, int n_uniform, const float *uniform,
                                          const double *face_u, const double *uv, const double *noise, const float *rot, float *plain, float *query,
                                          void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && M >= 1 && n_uniform >= 0 && n_uniform <= M,
               "gn_resident_volume_queries: 1 <= B <= 65535, 0 <= n_uniform <= M");
    GN_REQUIRE(store->meta && slots && query && plain != query, "gn_resident_volume_queries: null pointer (or plain == query)");
    GN_REQUIRE(n_uniform == 0 || uniform != nullptr, "gn_resident_volume_queries: the uniform points are required");
    GN_REQUIRE(n_uniform == M || (face_u && uv && noise && store->cdf_nocs && store->faces && store->nocs_verts),
               "gn_resident_volume_queries: near-surface queries need face_u, uv, noise and the resident NOCS mesh with its CDF");
    hipLaunchKernelGGL(resident_volume_queries_kernel, dim3((unsigned)gn_cdiv(M, RES_WG), (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, M,
                       n_uniform, uniform, face_u, uv, noise, rot, plain, query);
    GN_LAUNCH_CHECK("gn_resident_volume_queries");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ mesh targets
// query <- the mesh the faces are drawn on (NOCS vertices; in task space the normalised simulation vertices), target <- the other space's vertices.
// rot_mode: 0 none, 1 the target rotates (simulation space), 2 the query turns about the pivot (task space)
__global__ __launch_bounds__(RES_WG) void resident_surface_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int M, const double *__restrict__ face_u,
                                                                  const double *__restrict__ uv, int task_space, const float *__restrict__ rot,
                                                                  float *__restrict__ query, float *__restrict__ target) {
    const int b = blockIdx.y, i = blockIdx.x * RES_WG + threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (i >= M || m == nullptr) return;
    const int64_t o = (int64_t)b * M + i;
    const double *cdf = (task_space ? s.cdf_task : s.cdf_nocs) + m[GN_RESIDENT_FACE_OFF];
    const ResPick p = res_pick(cdf, (int)m[GN_RESIDENT_NUM_FACES], face_u[o], uv[o * 2], uv[o * 2 + 1]);
    const int32_t *tri = s.faces + (m[GN_RESIDENT_FACE_OFF] + p.face) * 3;
    const float *qv = (task_space ? s.task_verts : s.nocs_verts) + m[GN_RESIDENT_VERT_OFF] * 3;
    const float *tv = (task_space ? s.nocs_verts : s.sim_verts) + m[GN_RESIDENT_VERT_OFF] * 3;
    float q[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[c] = res_bary(qv, 3, c, tri, p);
        g[c] = res_bary(tv, 3, c, tri, p);
    }
    if (rot != nullptr) {
        const float *R = rot + (int64_t)b * 9;
        if (task_space) {
            res_pivot_rot(R, q);
        } else {
            const float gx = g[0], gy = g[1], gz = g[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) g[j] = res_rot32(R, j, gx, gy, gz);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        query[o * 3 + c] = q[c];
        target[o * 3 + c] = g[c];
    }
}

extern "C" int gn_resident_surface(const GnResidentStore *store, const int32_t *slots, int B, int M, const double *face_u, const double *uv, int task_space,
                                   const float *rot, float *query, float *target, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && M >= 1, "gn_resident_surface: 1 <= B <= 65535 garments of M >= 1 points");
    GN_REQUIRE(store->meta && store->faces && store->nocs_verts && slots && face_u && uv && query && target, "gn_resident_surface: null pointer");
    GN_REQUIRE(task_space ? (store->cdf_task && store->task_verts) : (store->cdf_nocs && store->sim_verts),
               "gn_resident_surface: the store holds no %s mesh table", task_space ? "task-space" : "NOCS");
    hipLaunchKernelGGL(resident_surface_kernel, dim3((unsigned)gn_cdiv(M, RES_WG), (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, M, face_u, uv,
                       task_space, rot, query, target);
    GN_LAUNCH_CHECK("gn_resident_surface");
    return GN_OK;
}

__global__ __launch_bounds__(RES_WG) void resident_mc_surface_kernel(GnResidentStore s, const int32_t *__restrict__ slots, int M, const double *__restrict__ face_u,
                                                                     const double *__restrict__ uv, float *__restrict__ query, float *__restrict__ on_surf) {
    const int b = blockIdx.y, i = blockIdx.x * RES_WG + threadIdx.x;
    const int64_t *m = res_meta(s, slots, b);
    if (i >= M || m == nullptr) return;
    const int64_t o = (int64_t)b * M + i;
    const ResPick p = res_pick(s.cdf_mc + m[GN_RESIDENT_MC_FACE_OFF], (int)m[GN_RESIDENT_NUM_MC_FACES], face_u[o], uv[o * 2], uv[o * 2 + 1]);
    const int32_t *tri = s.mc_faces + (m[GN_RESIDENT_MC_FACE_OFF] + p.face) * 3;
    const float *verts = s.mc_verts + m[GN_RESIDENT_MC_VERT_OFF] * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) query[o * 3 + c] = res_bary(verts, 3, c, tri, p);
    on_surf[o] = res_bary(s.mc_flags + m[GN_RESIDENT_MC_VERT_OFF], 1, 0, tri, p) > 0.5f ? 1.0f : 0.0f;
}

extern "C" int gn_resident_mc_surface(const GnResidentStore *store, const int32_t *slots, int B, int M, const double *face_u, const double *uv, float *query,
                                      float *on_surf, void *stream) {
    GN_REQUIRE(store != nullptr && B >= 1 && B <= 65535 && M >= 1, "gn_resident_mc_surface: 1 <= B <= 65535 garments of M >= 1 points");
    GN_REQUIRE(store->meta && store->mc_verts && store->mc_faces && store->mc_flags && store->cdf_mc && slots && face_u && uv && query && on_surf,
               "gn_resident_mc_surface: the store holds no marching-cubes mesh");
    hipLaunchKernelGGL(resident_mc_surface_kernel, dim3((unsigned)gn_cdiv(M, RES_WG), (unsigned)B), dim3(RES_WG), 0, gn_stream(stream), *store, slots, M, face_u,
                       uv, query, on_surf);
    GN_LAUNCH_CHECK("gn_resident_mc_surface");
    return GN_OK;
}

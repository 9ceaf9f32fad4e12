// mesh_pair.h -- the per-(query, face) device cores of the all-pairs mesh kernels, fp64, no fma: the solid angle of winding.hip (wn_*) and the squared
// point-to-triangle distance of eval_dist.hip (pm_*).  winding.hip, eval_dist.hip, query_targets.hip and cloth.hip (pm_closest, the vertex-face contacts
// of garmentnets_amd/cloth.py) include this file, so that one definition serves every kernel that is held to garmentnets_amd/winding.py and
// garmentnets_amd/distance.py.  The vertex type is a template parameter: the dataset
// preparation entries read fp64 vertices, the training-target entries the stored fp32 ones, widened exactly.
#pragma once
#include <math.h>

#include "common.h"

// ---------------------------------------------------------------------------------------------------------------- winding number
#define WN_BLOCK 256
#define WN_QPT 4
#define WN_TILE 128
#define WN_SPAN (WN_BLOCK * WN_QPT)
#define WN_FOUR_PI 12.566370614359172             /* 4 * M_PI (a power-of-two multiple: exact) */

__device__ __forceinline__ double wn_dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

// the solid angle of the triangle (v0, v1, v2) seen from q
__device__ __forceinline__ double wn_omega(double qx, double qy, double qz, double v0x, double v0y, double v0z, double v1x, double v1y, double v1z,
                                           double v2x, double v2y, double v2z) {
    const double ax = __dsub_rn(v0x, qx), ay = __dsub_rn(v0y, qy), az = __dsub_rn(v0z, qz);
    const double bx = __dsub_rn(v1x, qx), by = __dsub_rn(v1y, qy), bz = __dsub_rn(v1z, qz);
    const double cx = __dsub_rn(v2x, qx), cy = __dsub_rn(v2y, qy), cz = __dsub_rn(v2z, qz);
    const double la = __dsqrt_rn(wn_dot3(ax, ay, az, ax, ay, az));
    const double lb = __dsqrt_rn(wn_dot3(bx, by, bz, bx, by, bz));
    const double lc = __dsqrt_rn(wn_dot3(cx, cy, cz, cx, cy, cz));
    const double crx = __dsub_rn(__dmul_rn(by, cz), __dmul_rn(bz, cy));
    const double cry = __dsub_rn(__dmul_rn(bz, cx), __dmul_rn(bx, cz));
    const double crz = __dsub_rn(__dmul_rn(bx, cy), __dmul_rn(by, cx));
    const double num = wn_dot3(ax, ay, az, crx, cry, crz);
    const double dab = wn_dot3(ax, ay, az, bx, by, bz), dbc = wn_dot3(bx, by, bz, cx, cy, cz), dca = wn_dot3(cx, cy, cz, ax, ay, az);
    double den = __dadd_rn(__dmul_rn(__dmul_rn(la, lb), lc), __dmul_rn(dab, lc));
    den = __dadd_rn(den, __dmul_rn(dbc, la));
    den = __dadd_rn(den, __dmul_rn(dca, lb));
    return __dmul_rn(2.0, atan2(num, den));
}

// acc[k] += omega(q[k], face) over the nf faces of one mesh, in face order.  Called by the whole workgroup (it holds barriers).  A face with an
// index outside [0, nv) sets *bad and is staged as three coincident points: its numerator is an exact zero, so it adds +-0.
template <typename VT>
__device__ __forceinline__ void wn_accumulate(double (*tri)[WN_TILE], const VT *__restrict__ V, int64_t nv, const int32_t *__restrict__ F, int64_t nf,
                                              const double (&qx)[WN_QPT], const double (&qy)[WN_QPT], const double (&qz)[WN_QPT],
                                              double (&acc)[WN_QPT], int64_t *__restrict__ bad) {
    for (int64_t t0 = 0; t0 < nf; t0 += WN_TILE) {
        const int n = (int)((nf - t0) < WN_TILE ? (nf - t0) : WN_TILE);
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += WN_BLOCK) {
            double p[9];
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                const int32_t vi = F[3 * (t0 + j) + k];
                const bool in = vi >= 0 && vi < nv;
                ok = ok && in;
                for (int c = 0; c < 3; ++c) p[3 * k + c] = in ? (double)V[3 * (int64_t)vi + c] : 0.0;     // out of range: flagged, never read
            }
            if (!ok) *bad = 1;
            for (int c = 0; c < 9; ++c) tri[c][j] = ok ? p[c] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double v0x = tri[0][j], v0y = tri[1][j], v0z = tri[2][j];
            const double v1x = tri[3][j], v1y = tri[4][j], v1z = tri[5][j];
            const double v2x = tri[6][j], v2y = tri[7][j], v2z = tri[8][j];
#pragma unroll
            for (int k = 0; k < WN_QPT; ++k)
                acc[k] = __dadd_rn(acc[k], wn_omega(qx[k], qy[k], qz[k], v0x, v0y, v0z, v1x, v1y, v1z, v2x, v2y, v2z));
        }
    }
}

// a pair / mesh that no workgroup walks still has its face indices checked (by its first workgroup): the wrapper raises on any bad index
__device__ __forceinline__ void wn_check_faces(const int32_t *__restrict__ F, int64_t nf, int64_t nv, int64_t *__restrict__ bad) {
    for (int64_t f = threadIdx.x; f < 3 * nf; f += WN_BLOCK)
        if (F[f] < 0 || F[f] >= nv) *bad = 1;
}

// ---------------------------------------------------------------------------------------------------------------- point -> mesh
#define ED_BLOCK 256
#define PM_TILE 128

__device__ __forceinline__ double ed_dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}

// Per staged triangle (v0, v1, v2): v0, e0 = v1 - v0, e1 = v2 - v0, v1, e2 = v2 - v1, the Gram entries a = e0.e0, b = e0.e1,
// c = e1.e1, 1 / det (det = a c - b b; 0 when det <= 0) and the reciprocal squared lengths of the three edges (0 for a zero-length edge).
enum { PM_V0X, PM_V0Y, PM_V0Z, PM_E0X, PM_E0Y, PM_E0Z, PM_E1X, PM_E1Y, PM_E1Z, PM_V1X, PM_V1Y, PM_V1Z, PM_E2X, PM_E2Y, PM_E2Z,
       PM_A, PM_B, PM_C, PM_IDET, PM_IA, PM_IC, PM_IE2, PM_NCONST };

__device__ __forceinline__ double pm_rcp_or_zero(double x) { return x > 0.0 ? 1.0 / x : 0.0; }

// squared distance from w (the query relative to the segment's start) to the segment start + t dir, t = clamp(w.dir / |dir|^2, 0, 1)
__device__ __forceinline__ double pm_seg(double wx, double wy, double wz, double dx, double dy, double dz, double wd, double inv_len2) {
    const double t = fmin(fmax(__dmul_rn(wd, inv_len2), 0.0), 1.0);
    const double rx = __dsub_rn(wx, __dmul_rn(t, dx)), ry = __dsub_rn(wy, __dmul_rn(t, dy)), rz = __dsub_rn(wz, __dmul_rn(t, dz));
    return ed_dot3(rx, ry, rz, rx, ry, rz);
}

// Stage the faces t0 .. t0 + n - 1 of the mesh (V, nv, F) into `tri`: the PM_NCONST constants of each.  Called by the whole workgroup of ED_BLOCK
// threads between two barriers.  A face index outside [0, nv) sets *bad and is never dereferenced (a zero vertex stands in).
template <typename VT>
__device__ __forceinline__ void pm_stage_tile(double (*tri)[PM_TILE], const VT *__restrict__ V, int64_t nv, const int32_t *__restrict__ F, int64_t t0,
                                              int n, int64_t *__restrict__ bad) {
    for (int j = threadIdx.x; j < n; j += ED_BLOCK) {
        double p[3][3];
        for (int k = 0; k < 3; ++k) {
            const int32_t vi = F[3 * (t0 + j) + k];
            p[k][0] = p[k][1] = p[k][2] = 0.0;
            if (vi >= 0 && vi < nv) {
                p[k][0] = (double)V[3 * (int64_t)vi]; p[k][1] = (double)V[3 * (int64_t)vi + 1]; p[k][2] = (double)V[3 * (int64_t)vi + 2];
            } else {
                *bad = 1;                                   // out of range: flagged, never read
            }
        }
        const double e0x = __dsub_rn(p[1][0], p[0][0]), e0y = __dsub_rn(p[1][1], p[0][1]), e0z = __dsub_rn(p[1][2], p[0][2]);
        const double e1x = __dsub_rn(p[2][0], p[0][0]), e1y = __dsub_rn(p[2][1], p[0][1]), e1z = __dsub_rn(p[2][2], p[0][2]);
        const double e2x = __dsub_rn(p[2][0], p[1][0]), e2y = __dsub_rn(p[2][1], p[1][1]), e2z = __dsub_rn(p[2][2], p[1][2]);
        const double a = ed_dot3(e0x, e0y, e0z, e0x, e0y, e0z), b = ed_dot3(e0x, e0y, e0z, e1x, e1y, e1z);
        const double c = ed_dot3(e1x, e1y, e1z, e1x, e1y, e1z), l2 = ed_dot3(e2x, e2y, e2z, e2x, e2y, e2z);
        const double det = __dsub_rn(__dmul_rn(a, c), __dmul_rn(b, b));
        tri[PM_V0X][j] = p[0][0]; tri[PM_V0Y][j] = p[0][1]; tri[PM_V0Z][j] = p[0][2];
        tri[PM_E0X][j] = e0x; tri[PM_E0Y][j] = e0y; tri[PM_E0Z][j] = e0z;
        tri[PM_E1X][j] = e1x; tri[PM_E1Y][j] = e1y; tri[PM_E1Z][j] = e1z;
        tri[PM_V1X][j] = p[1][0]; tri[PM_V1Y][j] = p[1][1]; tri[PM_V1Z][j] = p[1][2];
        tri[PM_E2X][j] = e2x; tri[PM_E2Y][j] = e2y; tri[PM_E2Z][j] = e2z;
        tri[PM_A][j] = a; tri[PM_B][j] = b; tri[PM_C][j] = c;
        tri[PM_IDET][j] = pm_rcp_or_zero(det);
        tri[PM_IA][j] = pm_rcp_or_zero(a); tri[PM_IC][j] = pm_rcp_or_zero(c); tri[PM_IE2][j] = pm_rcp_or_zero(l2);
    }
}

// one staged triangle in registers: every lane reads the same LDS elements (a broadcast); a thread that owns several queries reads it once for all
struct PmTri { double k[PM_NCONST]; };

__device__ __forceinline__ PmTri pm_load(const double (*tri)[PM_TILE], int j) {
    PmTri t;
#pragma unroll
    for (int c = 0; c < PM_NCONST; ++c) t.k[c] = tri[c][j];
    return t;
}

// the squared distance from q to the staged triangle T: the per-pair arithmetic of every distance kernel (no fma, the operation order written here)
__device__ __forceinline__ double pm_sqdist(const PmTri &T, double qx, double qy, double qz) {
    const double wx = __dsub_rn(qx, T.k[PM_V0X]), wy = __dsub_rn(qy, T.k[PM_V0Y]), wz = __dsub_rn(qz, T.k[PM_V0Z]);
    const double e0x = T.k[PM_E0X], e0y = T.k[PM_E0Y], e0z = T.k[PM_E0Z];
    const double e1x = T.k[PM_E1X], e1y = T.k[PM_E1Y], e1z = T.k[PM_E1Z];
    const double d0 = ed_dot3(wx, wy, wz, e0x, e0y, e0z), d1 = ed_dot3(wx, wy, wz, e1x, e1y, e1z);
    // the three clamped segment distances (a zero-length edge clamps to its start point: degenerate triangles land here)
    const double s0 = pm_seg(wx, wy, wz, e0x, e0y, e0z, d0, T.k[PM_IA]);
    const double s1 = pm_seg(wx, wy, wz, e1x, e1y, e1z, d1, T.k[PM_IC]);
    const double ux = __dsub_rn(qx, T.k[PM_V1X]), uy = __dsub_rn(qy, T.k[PM_V1Y]), uz = __dsub_rn(qz, T.k[PM_V1Z]);
    const double e2x = T.k[PM_E2X], e2y = T.k[PM_E2Y], e2z = T.k[PM_E2Z];
    const double s2 = pm_seg(ux, uy, uz, e2x, e2y, e2z, ed_dot3(ux, uy, uz, e2x, e2y, e2z), T.k[PM_IE2]);
    // the projection onto the plane in barycentric form: w = s e0 + t e1 + (normal part)
    const double a = T.k[PM_A], b = T.k[PM_B], c = T.k[PM_C], idet = T.k[PM_IDET];
    const double s = __dmul_rn(__dsub_rn(__dmul_rn(c, d0), __dmul_rn(b, d1)), idet);
    const double t = __dmul_rn(__dsub_rn(__dmul_rn(a, d1), __dmul_rn(b, d0)), idet);
    const double rx = __dsub_rn(__dsub_rn(wx, __dmul_rn(s, e0x)), __dmul_rn(t, e1x));
    const double ry = __dsub_rn(__dsub_rn(wy, __dmul_rn(s, e0y)), __dmul_rn(t, e1y));
    const double rz = __dsub_rn(__dsub_rn(wz, __dmul_rn(s, e0z)), __dmul_rn(t, e1z));
    const double plane = ed_dot3(rx, ry, rz, rx, ry, rz);
    const bool inside = idet > 0.0 && s >= 0.0 && t >= 0.0 && __dadd_rn(s, t) <= 1.0;
    // the segment distances stay in the minimum when the projection is inside: on a sliver (det nearly cancelled) s and t are
    // noise, `plane` is then only an upper bound and an edge can be closer
    const double seg = fmin(fmin(s0, s1), s2);
    return inside ? fmin(plane, seg) : seg;
}

// the PM_NCONST constants of the triangle (p0, p1, p2) in registers: pm_stage_tile's expressions, for a kernel that meets a triangle once
__device__ __forceinline__ PmTri pm_tri_of(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3]) {
    PmTri T;
    const double e0x = __dsub_rn(p1[0], p0[0]), e0y = __dsub_rn(p1[1], p0[1]), e0z = __dsub_rn(p1[2], p0[2]);
    const double e1x = __dsub_rn(p2[0], p0[0]), e1y = __dsub_rn(p2[1], p0[1]), e1z = __dsub_rn(p2[2], p0[2]);
    const double e2x = __dsub_rn(p2[0], p1[0]), e2y = __dsub_rn(p2[1], p1[1]), e2z = __dsub_rn(p2[2], p1[2]);
    const double a = ed_dot3(e0x, e0y, e0z, e0x, e0y, e0z), b = ed_dot3(e0x, e0y, e0z, e1x, e1y, e1z);
    const double c = ed_dot3(e1x, e1y, e1z, e1x, e1y, e1z), l2 = ed_dot3(e2x, e2y, e2z, e2x, e2y, e2z);
    const double det = __dsub_rn(__dmul_rn(a, c), __dmul_rn(b, b));
    T.k[PM_V0X] = p0[0]; T.k[PM_V0Y] = p0[1]; T.k[PM_V0Z] = p0[2];
    T.k[PM_E0X] = e0x; T.k[PM_E0Y] = e0y; T.k[PM_E0Z] = e0z;
    T.k[PM_E1X] = e1x; T.k[PM_E1Y] = e1y; T.k[PM_E1Z] = e1z;
    T.k[PM_V1X] = p1[0]; T.k[PM_V1Y] = p1[1]; T.k[PM_V1Z] = p1[2];
    T.k[PM_E2X] = e2x; T.k[PM_E2Y] = e2y; T.k[PM_E2Z] = e2z;
    T.k[PM_A] = a; T.k[PM_B] = b; T.k[PM_C] = c;
    T.k[PM_IDET] = pm_rcp_or_zero(det);
    T.k[PM_IA] = pm_rcp_or_zero(a); T.k[PM_IC] = pm_rcp_or_zero(c); T.k[PM_IE2] = pm_rcp_or_zero(l2);
    return T;
}

// pm_seg, which also returns what it squares (r) and the clamped parameter
__device__ __forceinline__ double pm_seg_closest(double wx, double wy, double wz, double dx, double dy, double dz, double wd, double inv_len2,
                                                 double (&r)[3], double &u) {
    u = fmin(fmax(__dmul_rn(wd, inv_len2), 0.0), 1.0);
    r[0] = __dsub_rn(wx, __dmul_rn(u, dx)); r[1] = __dsub_rn(wy, __dmul_rn(u, dy)); r[2] = __dsub_rn(wz, __dmul_rn(u, dz));
    return ed_dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
}

// pm_sqdist, which also names the winner (cloth.py "Vertex-face contacts", point_triangle): the squared distance (the bits of pm_sqdist), r = q - the
// closest point as the winner computes it, bary the closest point's weights on (v0, v1, v2).  The plane wins when the projection is inside and
// plane <= min(s0, s1, s2); otherwise the first of s0, s1, s2 that equals the minimum.
__device__ __forceinline__ double pm_closest(const PmTri &T, double qx, double qy, double qz, double (&r)[3], double (&bary)[3]) {
    const double wx = __dsub_rn(qx, T.k[PM_V0X]), wy = __dsub_rn(qy, T.k[PM_V0Y]), wz = __dsub_rn(qz, T.k[PM_V0Z]);
    const double e0x = T.k[PM_E0X], e0y = T.k[PM_E0Y], e0z = T.k[PM_E0Z];
    const double e1x = T.k[PM_E1X], e1y = T.k[PM_E1Y], e1z = T.k[PM_E1Z];
    const double d0 = ed_dot3(wx, wy, wz, e0x, e0y, e0z), d1 = ed_dot3(wx, wy, wz, e1x, e1y, e1z);
    double r0[3], r1[3], r2[3], u0, u1, u2;
    const double s0 = pm_seg_closest(wx, wy, wz, e0x, e0y, e0z, d0, T.k[PM_IA], r0, u0);
    const double s1 = pm_seg_closest(wx, wy, wz, e1x, e1y, e1z, d1, T.k[PM_IC], r1, u1);
    const double ux = __dsub_rn(qx, T.k[PM_V1X]), uy = __dsub_rn(qy, T.k[PM_V1Y]), uz = __dsub_rn(qz, T.k[PM_V1Z]);
    const double e2x = T.k[PM_E2X], e2y = T.k[PM_E2Y], e2z = T.k[PM_E2Z];
    const double s2 = pm_seg_closest(ux, uy, uz, e2x, e2y, e2z, ed_dot3(ux, uy, uz, e2x, e2y, e2z), T.k[PM_IE2], r2, u2);
    const double a = T.k[PM_A], b = T.k[PM_B], c = T.k[PM_C], idet = T.k[PM_IDET];
    const double s = __dmul_rn(__dsub_rn(__dmul_rn(c, d0), __dmul_rn(b, d1)), idet);
    const double t = __dmul_rn(__dsub_rn(__dmul_rn(a, d1), __dmul_rn(b, d0)), idet);
    const double rx = __dsub_rn(__dsub_rn(wx, __dmul_rn(s, e0x)), __dmul_rn(t, e1x));
    const double ry = __dsub_rn(__dsub_rn(wy, __dmul_rn(s, e0y)), __dmul_rn(t, e1y));
    const double rz = __dsub_rn(__dsub_rn(wz, __dmul_rn(s, e0z)), __dmul_rn(t, e1z));
    const double plane = ed_dot3(rx, ry, rz, rx, ry, rz);
    const bool inside = idet > 0.0 && s >= 0.0 && t >= 0.0 && __dadd_rn(s, t) <= 1.0;
    const double seg = fmin(fmin(s0, s1), s2);
    if (inside && plane <= seg) {
        r[0] = rx; r[1] = ry; r[2] = rz;
        bary[0] = __dsub_rn(__dsub_rn(1.0, s), t); bary[1] = s; bary[2] = t;
        return plane;
    }
    if (s0 == seg) {
        r[0] = r0[0]; r[1] = r0[1]; r[2] = r0[2];
        bary[0] = __dsub_rn(1.0, u0); bary[1] = u0; bary[2] = 0.0;
    } else if (s1 == seg) {
        r[0] = r1[0]; r[1] = r1[1]; r[2] = r1[2];
        bary[0] = __dsub_rn(1.0, u1); bary[1] = 0.0; bary[2] = u1;
    } else {
        r[0] = r2[0]; r[1] = r2[1]; r[2] = r2[2];
        bary[0] = 0.0; bary[1] = __dsub_rn(1.0, u2); bary[2] = u2;
    }
    return seg;
}

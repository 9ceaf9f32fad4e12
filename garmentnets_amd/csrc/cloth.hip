// cloth.hip -- the hanging garment: small-step XPBD over point masses and distance constraints, fp64, no fma: mesh/cloth_verts built on the device.
//
//   gn_cloth_simulate_batch            B ragged garments, `substeps` substeps each, in launches of at most max_substeps_per_launch
//   gn_cloth_contact_lists             the vertex-vertex contact lists of B garments through a hashed uniform grid (and contact_travel)
//   gn_cloth_simulate_contacts_batch   gn_cloth_simulate_batch with the contact pass of those lists after the last colour
//   gn_cloth_face_contact_lists        the vertex-face contact lists of B garments over all (vertex, face) pairs (at the end of this file)
//   gn_cloth_simulate_face_contacts_batch   gn_cloth_simulate_contacts_batch with the face entries of those lists inside the same gather
//
// The definition is garmentnets_amd/cloth.py's ("Hanging garments"); cloth_substeps below is its substep, operation for operation: the
// library is built with -ffp-contract=off and every operation is an explicit _rn intrinsic, so x and v are the bits of cloth.simulate_reference.
//
// Shape: ONE workgroup owns ONE garment for the whole launch, so nothing is ever handed to another workgroup and there is no device-scope
// synchronisation.  A thread owns the vertices tid, tid + T, ... in the per-vertex passes and the constraints c0 + tid, c0 + tid + T, ... of a
// colour.  No two constraints of a colour share a vertex (the host's colouring), so inside a colour every position has one reader-writer: no atomics,
// and which thread projects which constraint cannot change a bit.  Barriers: one after the prediction pass and one after every colour; every thread
// reaches every one of them -- each loop bound is a launch argument or a table entry that the whole workgroup reads alike, and nothing returns early.
// (The velocity pass of a substep and the prediction pass of the next touch only the thread's own vertices: no barrier between them.)
//
// Contacts (cloth_substeps<true>): after the last colour's barrier a thread gathers, for its own vertices, the corrections of its list entries from
// the positions the sweep left (reads of any vertex, a write to the thread's own row of the corr workspace only), ONE more barrier says "all reads
// done", and the thread adds relax * corr to its own vertices.  The velocity pass that follows reads only what the same thread wrote, and the next
// reader of a foreign position is the next substep's first colour, behind the prediction pass's barrier: the second barrier the plan allowed for
// ("writes done") is that one.  A Jacobi gather: one writer per position, no atomics, the order of the additions fixed by the list.
// Face entries (cloth_substeps<true, true>): in the same gather, after the vertex entries of the vertex and into the same sum, the entries of its
// face list: the triangle's constants from P (pm_tri_of), the closest point (pm_closest), the vertex's mass-weighted share; the face's corners get
// no reaction, so the one-writer rule and the barriers are those of the vertex entries.
//
// Contact lists (cl_contact_* below): many workgroups per garment; a uniform grid of cells of edge `cell` (a little above r) hashed into `buckets`
// buckets per garment, filled by count, scan, fill (a thread per vertex); the query (a wave per vertex) scans the 27 neighbouring cells, keeps the
// candidates that really lie in the scanned cell (so two cells that share a bucket only cost time), applies the predicate of the definition and
// places every partner by its rank among those found.  The result is the brute-force set of cloth.contact_lists_reference: DESIGN.md argues the
// cell edge.
//
// Storage: the working positions p of a garment live in LDS when 24 V bytes fit the launch's dynamic LDS (the wrapper's budget), otherwise in the
// garment's rows of x in global memory (L2-resident at these sizes; the waves of a workgroup share their CU's L1, and __syncthreads() is the
// workgroup-scope release / acquire between a colour's stores and the next colour's loads).  x_prev needs no storage of its own: v is dead between the
// prediction pass and the velocity pass, so its rows hold x_prev meanwhile.  Both paths run the same cloth_substeps and give the same bits, as does
// every workgroup size: the result is a pure function of (garment, constants, substeps).
#include <type_traits>

#include "common.h"
#include "mesh_pair.h"

#define CL_MAX_BLOCK 1024
#define CL_MAX_LDS (160 * 1024)

struct ClothArgs {
    double *x, *v;                          // [*][3] in / out
    const double *w;                        // [*] inverse masses
    const int32_t *pairs;                   // [*][2] vertex indices relative to the garment's first vertex, grouped by colour
    const double *l0, *alpha_t;             // [*] per constraint
    const int64_t *csr;                     // [B + 1][3] = {v_off, c_off, k_off}
    const int64_t *colour_off;              // garment b: colour_off[k_off[b] .. k_off[b + 1] - 1], relative to c_off[b], K_b + 1 entries
    int64_t *bad;
    double h, inv_h, hgx, hgy, hgz, damp;
    int substeps, lds_bytes;
};

#define CL_MAX_LIST 64                      // the longest contact list a vertex can have (cloth.COLLISION_MAX_LIST_CAP)
#define CL_GATHER 8                         // list entries the contact pass fetches at a time
#define CL_DIAG 4                           // int64 per garment: {contact_overflow, contact_max_list, contact_active, bits of the largest travel^2}

// what the contact pass reads beside ClothArgs: the lists of gn_cloth_contact_lists
struct ClothArgsContacts : ClothArgs {
    const int32_t *list_j;                  // [*][K] partner indices relative to the garment's first vertex, ascending
    const double *list_tm2;                 // [*][K] min(t2, rest2) of the entry
    const int32_t *list_n;                  // [*] entries of the row
    double *corr;                           // [*][3] workspace: a vertex's correction between the gather and its application
    int64_t *diag;                          // [B][CL_DIAG]
    double relax;
    int K;
};
#define CL_FACE_MAX_LIST 32                 // the longest face-contact list a vertex can have (cloth.FACE_MAX_LIST_CAP)
#define CL_FACE_DIAG 3                      // int64 per garment: {face_contact_overflow, face_contact_max_list, face_contact_active}

// what the face entries of the contact pass read beside ClothArgsContacts: the lists of gn_cloth_face_contact_lists
struct ClothArgsFaces : ClothArgsContacts {
    const int32_t *faces;                   // [*][3] vertex indices relative to the garment's first vertex
    const int64_t *fcsr;                    // [B + 1] the garment's first face
    const int32_t *flist_f;                 // [*][Kf] face indices relative to the garment's first face, ascending
    const double *flist_tm2;                // [*][Kf] min(tf2, the rest d2) of the entry
    const int32_t *flist_n;                 // [*] entries of the row
    int64_t *fdiag;                         // [B][CL_FACE_DIAG]
    int Kf;
};
template <bool CONTACTS, bool FACES = false>
using ClothArgsOf = std::conditional_t<FACES, ClothArgsFaces, std::conditional_t<CONTACTS, ClothArgsContacts, ClothArgs>>;

__device__ __forceinline__ double cl_sq(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}
__device__ __forceinline__ long long cl_wave_sum(long long v) {
    for (int m = GN_WAVE / 2; m; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ unsigned long long cl_wave_max(unsigned long long v) {
    for (int m = GN_WAVE / 2; m; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// P: the working positions of the garment (LDS or global), vb: its rows of v.  Called by the whole workgroup (it holds barriers).  CONTACTS: v_off is
// the garment's first row of the lists and of corr, diag its CL_DIAG counters.  FACES (with CONTACTS): b is the garment, the face entries follow the
// vertex entries of a vertex in the same corr.
template <bool CONTACTS, bool FACES = false>
__device__ __forceinline__ void cloth_substeps(double *P, double *vb, const double *__restrict__ w, const int32_t *__restrict__ ij,
                                               const double *__restrict__ l0, const double *__restrict__ at, const int64_t *__restrict__ coff, int ncol,
                                               int V, const ClothArgsOf<CONTACTS, FACES> &a, int64_t v_off = 0, int64_t *diag = nullptr, int b = 0) {
    const int T = blockDim.x;
    long long active = 0;
    [[maybe_unused]] long long face_active = 0;
    for (int s = 0; s < a.substeps; ++s) {
        for (int i = threadIdx.x; i < V; i += T) {
            if (!(w[i] > 0.0)) continue;                     // held or massless: stays where it is
            double *p = P + 3 * (int64_t)i, *q = vb + 3 * (int64_t)i;
            const double vx = __dmul_rn(__dadd_rn(q[0], a.hgx), a.damp), vy = __dmul_rn(__dadd_rn(q[1], a.hgy), a.damp),
                         vz = __dmul_rn(__dadd_rn(q[2], a.hgz), a.damp);
            const double x0 = p[0], x1 = p[1], x2 = p[2];
            q[0] = x0; q[1] = x1; q[2] = x2;                 // x_prev, kept in v's rows until the velocity pass
            p[0] = __dadd_rn(x0, __dmul_rn(a.h, vx)); p[1] = __dadd_rn(x1, __dmul_rn(a.h, vy)); p[2] = __dadd_rn(x2, __dmul_rn(a.h, vz));
        }
        __syncthreads();
        for (int k = 0; k < ncol; ++k) {
            const int64_t c1 = coff[k + 1];
            for (int64_t c = coff[k] + threadIdx.x; c < c1; c += T) {
                const int32_t i = ij[2 * c], j = ij[2 * c + 1];
                if (i < 0 || i >= V || j < 0 || j >= V) { *a.bad = 1; continue; }          // flagged, never dereferenced
                double *pi = P + 3 * (int64_t)i, *pj = P + 3 * (int64_t)j;
                const double ix = pi[0], iy = pi[1], iz = pi[2], jx = pj[0], jy = pj[1], jz = pj[2];
                const double dx = __dsub_rn(ix, jx), dy = __dsub_rn(iy, jy), dz = __dsub_rn(iz, jz);
                const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
                const double wi = w[i], wj = w[j];
                const double sum = __dadd_rn(__dadd_rn(wi, wj), at[c]);
                if (len == 0.0 || sum == 0.0) continue;
                const double dl = __ddiv_rn(-__dsub_rn(len, l0[c]), sum);
                const double nx = __ddiv_rn(dx, len), ny = __ddiv_rn(dy, len), nz = __ddiv_rn(dz, len);
                const double ai = __dmul_rn(wi, dl), aj = __dmul_rn(wj, dl);
                pi[0] = __dadd_rn(ix, __dmul_rn(ai, nx)); pi[1] = __dadd_rn(iy, __dmul_rn(ai, ny)); pi[2] = __dadd_rn(iz, __dmul_rn(ai, nz));
                pj[0] = __dsub_rn(jx, __dmul_rn(aj, nx)); pj[1] = __dsub_rn(jy, __dmul_rn(aj, ny)); pj[2] = __dsub_rn(jz, __dmul_rn(aj, nz));
            }
            __syncthreads();
        }
        if constexpr (CONTACTS) {
            const int32_t *lj = a.list_j + v_off * a.K, *ln = a.list_n + v_off;
            const double *lt = a.list_tm2 + v_off * a.K;
            double *corr = a.corr + 3 * v_off;
            for (int i = threadIdx.x; i < V; i += T) {       // gather: reads any vertex, writes the thread's own rows of corr
                const double wi = w[i];
                if (!(wi > 0.0)) continue;
                const double *p = P + 3 * (int64_t)i;
                const double px = p[0], py = p[1], pz = p[2];
                int n = ln[i];
                n = n < 0 ? 0 : (n > a.K ? a.K : n);
                double cx = 0.0, cy = 0.0, cz = 0.0;
                for (int k0 = 0; k0 < n; k0 += CL_GATHER) {  // CL_GATHER entries fetched together: a row is read in a few round trips, not n
                    int32_t js[CL_GATHER];
                    double ts[CL_GATHER];
#pragma unroll
                    for (int u = 0; u < CL_GATHER; ++u) {
                        const int k = min(k0 + u, n - 1);
                        js[u] = lj[(int64_t)i * a.K + k]; ts[u] = lt[(int64_t)i * a.K + k];
                    }
#pragma unroll
                    for (int u = 0; u < CL_GATHER; ++u) {      // in list order
                        if (k0 + u >= n) break;
                        const int32_t j = js[u];
                        if (j < 0 || j >= V) { *a.bad = 1; continue; }                         // flagged, never dereferenced
                        const double *q = P + 3 * (int64_t)j;
                        const double dx = __dsub_rn(px, q[0]), dy = __dsub_rn(py, q[1]), dz = __dsub_rn(pz, q[2]);
                        const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
                        const double tm2 = ts[u];
                        if (!(d2 < tm2 && d2 > 0.0)) continue;
                        const double len = __dsqrt_rn(d2), tmin = __dsqrt_rn(tm2);
                        const double dl = __ddiv_rn(__dsub_rn(tmin, len), __dadd_rn(wi, w[j]));
                        const double ai = __dmul_rn(wi, dl);
                        cx = __dadd_rn(cx, __dmul_rn(ai, __ddiv_rn(dx, len)));
                        cy = __dadd_rn(cy, __dmul_rn(ai, __ddiv_rn(dy, len)));
                        cz = __dadd_rn(cz, __dmul_rn(ai, __ddiv_rn(dz, len)));
                        ++active;
                    }
                }
                if constexpr (FACES) {                       // the face entries, after the vertex entries and in list order
                    const int64_t f_off = a.fcsr[b];
                    const int F = (int)(a.fcsr[b + 1] - f_off);
                    const int32_t *fc = a.faces + 3 * f_off;
                    const int32_t *ff = a.flist_f + (v_off + i) * a.Kf;
                    const double *ft = a.flist_tm2 + (v_off + i) * a.Kf;
                    int nf = a.flist_n[v_off + i];
                    nf = nf < 0 ? 0 : (nf > a.Kf ? a.Kf : nf);
                    for (int k = 0; k < nf; ++k) {
                        const int32_t f = ff[k];
                        const double tm2 = ft[k];
                        if (f < 0 || f >= F) { *a.bad = 1; continue; }                             // flagged, never dereferenced
                        const int32_t ia = fc[3 * (int64_t)f], ib = fc[3 * (int64_t)f + 1], ic = fc[3 * (int64_t)f + 2];
                        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) { *a.bad = 1; continue; }
                        const double *qa = P + 3 * (int64_t)ia, *qb = P + 3 * (int64_t)ib, *qc = P + 3 * (int64_t)ic;
                        const double p0[3] = {qa[0], qa[1], qa[2]}, p1[3] = {qb[0], qb[1], qb[2]}, p2[3] = {qc[0], qc[1], qc[2]};
                        const PmTri tri = pm_tri_of(p0, p1, p2);
                        double r[3], bary[3];
                        const double d2 = pm_closest(tri, px, py, pz, r, bary);
                        if (!(d2 < tm2 && d2 > 0.0)) continue;
                        const double len = __dsqrt_rn(d2), tmin = __dsqrt_rn(tm2);
                        const double sum = __dadd_rn(__dadd_rn(wi, __dadd_rn(__dmul_rn(__dmul_rn(bary[0], bary[0]), w[ia]),
                                                                             __dmul_rn(__dmul_rn(bary[1], bary[1]), w[ib]))),
                                                     __dmul_rn(__dmul_rn(bary[2], bary[2]), w[ic]));
                        const double dl = __ddiv_rn(__dsub_rn(tmin, len), sum);
                        const double ai = __dmul_rn(wi, dl);
                        cx = __dadd_rn(cx, __dmul_rn(ai, __ddiv_rn(r[0], len)));
                        cy = __dadd_rn(cy, __dmul_rn(ai, __ddiv_rn(r[1], len)));
                        cz = __dadd_rn(cz, __dmul_rn(ai, __ddiv_rn(r[2], len)));
                        ++face_active;
                    }
                }
                corr[3 * (int64_t)i] = cx; corr[3 * (int64_t)i + 1] = cy; corr[3 * (int64_t)i + 2] = cz;
            }
            __syncthreads();                                 // all reads done
            for (int i = threadIdx.x; i < V; i += T) {
                if (!(w[i] > 0.0)) continue;
                double *p = P + 3 * (int64_t)i;
                const double *c = corr + 3 * (int64_t)i;
                p[0] = __dadd_rn(p[0], __dmul_rn(a.relax, c[0])); p[1] = __dadd_rn(p[1], __dmul_rn(a.relax, c[1]));
                p[2] = __dadd_rn(p[2], __dmul_rn(a.relax, c[2]));
            }
        }
        for (int i = threadIdx.x; i < V; i += T) {
            if (!(w[i] > 0.0)) continue;
            const double *p = P + 3 * (int64_t)i;
            double *q = vb + 3 * (int64_t)i;
            q[0] = __dmul_rn(__dsub_rn(p[0], q[0]), a.inv_h); q[1] = __dmul_rn(__dsub_rn(p[1], q[1]), a.inv_h);
            q[2] = __dmul_rn(__dsub_rn(p[2], q[2]), a.inv_h);
        }
    }
    if constexpr (CONTACTS) {
        active = cl_wave_sum(active);                        // every lane is here: nothing above returns
        if ((threadIdx.x & (GN_WAVE - 1)) == 0 && active) atomicAdd((unsigned long long *)(diag + 2), (unsigned long long)active);
    }
    if constexpr (FACES) {
        face_active = cl_wave_sum(face_active);
        if ((threadIdx.x & (GN_WAVE - 1)) == 0 && face_active)
            atomicAdd((unsigned long long *)(a.fdiag + CL_FACE_DIAG * (int64_t)b + 2), (unsigned long long)face_active);
    }
}

template <bool CONTACTS, bool FACES = false>
__global__ __launch_bounds__(CL_MAX_BLOCK) void cloth_simulate_batch_kernel(ClothArgsOf<CONTACTS, FACES> a) {
    extern __shared__ __attribute__((aligned(16))) double cl_pos[];
    const int64_t *m = a.csr + 3 * (int64_t)blockIdx.x;
    const int64_t v_off = m[0], c_off = m[1], k_off = m[2];
    const int V = (int)(m[3] - v_off), ncol = (int)(m[5] - k_off) - 1;
    const int64_t C = m[4] - c_off;
    const int32_t *ij = a.pairs + 2 * c_off;
    const int64_t *coff = a.colour_off + k_off;
    double *xb = a.x + 3 * v_off, *vb = a.v + 3 * v_off;
    const double *w = a.w + v_off;
    int64_t *diag = nullptr;
    if constexpr (CONTACTS) diag = a.diag + CL_DIAG * (int64_t)blockIdx.x;
    // every index of the table is checked whatever the substep count: the wrapper raises on the flag
    for (int64_t c = threadIdx.x; c < 2 * C; c += blockDim.x)
        if (ij[c] < 0 || ij[c] >= V) *a.bad = 1;
    if constexpr (FACES) {
        const int64_t f_off = a.fcsr[blockIdx.x], F = a.fcsr[blockIdx.x + 1] - f_off;
        for (int64_t c = threadIdx.x; c < 3 * F; c += blockDim.x)
            if (a.faces[3 * f_off + c] < 0 || a.faces[3 * f_off + c] >= V) *a.bad = 1;
    }
    if ((int64_t)V * 24 <= (int64_t)a.lds_bytes) {           // workgroup-uniform: V and lds_bytes are the same for every thread
        for (int i = threadIdx.x; i < 3 * V; i += blockDim.x) cl_pos[i] = xb[i];
        __syncthreads();
        cloth_substeps<CONTACTS, FACES>(cl_pos, vb, w, ij, a.l0 + c_off, a.alpha_t + c_off, coff, ncol, V, a, v_off, diag, (int)blockIdx.x);
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * V; i += blockDim.x) xb[i] = cl_pos[i];
    } else {
        cloth_substeps<CONTACTS, FACES>(xb, vb, w, ij, a.l0 + c_off, a.alpha_t + c_off, coff, ncol, V, a, v_off, diag, (int)blockIdx.x);
    }
}

// the checks and launches both solver entries share; `name` is the entry's for the messages
template <bool CONTACTS, bool FACES = false>
static int cloth_launch(const char *name, ClothArgsOf<CONTACTS, FACES> &a, int B, int64_t total_verts, int64_t total_constraints, int64_t substeps,
                        int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block, void *stream) {
    GN_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d outside [0, 65535]", name, B);
    GN_REQUIRE(total_verts >= 0 && total_verts < INT32_MAX && total_constraints >= 0 && total_constraints < INT32_MAX,
               "%s: %lld vertices, %lld constraints: each table must stay below 2^31 rows", name, (long long)total_verts, (long long)total_constraints);
    GN_REQUIRE(substeps >= 0 && max_substeps_per_launch >= 1, "%s: substeps=%lld, max_substeps_per_launch=%d", name, (long long)substeps,
               max_substeps_per_launch);
    GN_REQUIRE(block >= GN_WAVE && block <= CL_MAX_BLOCK && block % GN_WAVE == 0, "%s: block=%d: a multiple of %d in [%d, %d]", name, block, GN_WAVE,
               GN_WAVE, CL_MAX_BLOCK);
    GN_REQUIRE(lds_bytes >= 0 && lds_bytes <= CL_MAX_LDS, "%s: lds_bytes=%d outside [0, %d]", name, lds_bytes, CL_MAX_LDS);
    if (B == 0) return GN_OK;
    GN_REQUIRE(a.csr && a.colour_off && a.bad && consts_host, "%s: null pointer", name);
    GN_REQUIRE(total_verts == 0 || (a.x && a.v && a.w), "%s: null x / v / w", name);
    GN_REQUIRE(total_constraints == 0 || (a.pairs && a.l0 && a.alpha_t), "%s: null constraint table", name);
    for (int k = 0; k < 6; ++k)
        GN_REQUIRE(consts_host[k] == consts_host[k] && fabs(consts_host[k]) <= 1.7976931348623157e308, "%s: step constant %d is not finite", name, k);
    a.h = consts_host[0]; a.inv_h = consts_host[1]; a.hgx = consts_host[2]; a.hgy = consts_host[3]; a.hgz = consts_host[4]; a.damp = consts_host[5];
    a.lds_bytes = lds_bytes;
    GN_HIP(hipFuncSetAttribute((const void *)cloth_simulate_batch_kernel<CONTACTS, FACES>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes), name);
    // a launch with substeps == 0 still checks the table
    int64_t left = substeps;
    do {
        a.substeps = (int)(left < max_substeps_per_launch ? left : max_substeps_per_launch);
        hipLaunchKernelGGL((cloth_simulate_batch_kernel<CONTACTS, FACES>), dim3((unsigned)B), dim3((unsigned)block), (size_t)lds_bytes, gn_stream(stream), a);
        GN_LAUNCH_CHECK(name);
        left -= a.substeps;
    } while (left > 0);
    return GN_OK;
}

extern "C" int gn_cloth_simulate_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0, const double *alpha_t,
                                       const int64_t *csr, const int64_t *colour_off, int B, int64_t total_verts, int64_t total_constraints,
                                       int64_t substeps, int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block,
                                       int64_t *bad, void *stream) {
    ClothArgs a;
    a.x = x; a.v = v; a.w = w; a.pairs = pairs; a.l0 = l0; a.alpha_t = alpha_t; a.csr = csr; a.colour_off = colour_off; a.bad = bad;
    return cloth_launch<false>("gn_cloth_simulate_batch", a, B, total_verts, total_constraints, substeps, max_substeps_per_launch, consts_host,
                               lds_bytes, block, stream);
}

static bool cl_finite(double v) { return v == v && fabs(v) <= 1.7976931348623157e308; }

extern "C" int gn_cloth_simulate_contacts_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0, const double *alpha_t,
                                                const int64_t *csr, const int64_t *colour_off, int B, int64_t total_verts, int64_t total_constraints,
                                                int64_t substeps, int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block,
                                                int64_t *bad, const int32_t *list_j, const double *list_tm2, const int32_t *list_n, int K,
                                                const double *collision_host, double *corr, int64_t *diag, void *stream) {
    const char *name = "gn_cloth_simulate_contacts_batch";
    GN_REQUIRE(K >= 1 && K <= CL_MAX_LIST, "%s: K=%d outside [1, %d]", name, K, CL_MAX_LIST);
    GN_REQUIRE(collision_host, "%s: null collision constants", name);
    GN_REQUIRE(cl_finite(collision_host[3]) && collision_host[3] > 0.0 && collision_host[3] <= 1.0, "%s: collision constant 3 (relax) is not in (0, 1]",
               name);
    GN_REQUIRE(B == 0 || diag, "%s: null diag", name);
    GN_REQUIRE(B == 0 || total_verts == 0 || (list_j && list_tm2 && list_n && corr), "%s: null list / corr", name);
    ClothArgsContacts a;
    a.x = x; a.v = v; a.w = w; a.pairs = pairs; a.l0 = l0; a.alpha_t = alpha_t; a.csr = csr; a.colour_off = colour_off; a.bad = bad;
    a.list_j = list_j; a.list_tm2 = list_tm2; a.list_n = list_n; a.corr = corr; a.diag = diag; a.relax = collision_host[3]; a.K = K;
    return cloth_launch<true>(name, a, B, total_verts, total_constraints, substeps, max_substeps_per_launch, consts_host, lds_bytes, block, stream);
}

// ------------------------------------------------------------------------------------------------ contact lists
#define CL_CELL_CLAMP 1073741824.0          // 2^30: a cell index and its neighbours fit int32; clamping is monotone, so it never separates neighbours
#define CL_BIN_BLOCK 256
#define CL_QUERY_BLOCK GN_WAVE
#define CL_QUERY_CAP 256                    // partners of a vertex the query holds in LDS
#define CL_SCAN_BLOCK 1024
enum { CL_LISTS_TRAVEL = 1, CL_LISTS_BUILD = 2 };

struct ContactArgs {
    const double *x, *x0;                   // [*][3] positions now, start pose
    double *x_ref;                          // [*][3] positions at the last build
    const int64_t *csr;                     // the solver's [B + 1][3]; only v_off is read
    int32_t *cell;                          // [*][4] per vertex: its cell and its bucket
    int32_t *count, *start, *cursor;        // [B][buckets]
    int32_t *items;                         // [*] the vertices of a garment grouped by bucket
    int32_t *list_j, *list_n, *list_total;
    double *list_tm2;
    int64_t *diag;
    double t2, r2, edge;
    int K, buckets, flags;
};

__device__ __forceinline__ int cl_cell_of(double x, double edge) {
    double q = __ddiv_rn(x, edge);
    q = fmin(fmax(q, -CL_CELL_CLAMP), CL_CELL_CLAMP);        // a NaN lands on -2^30: still a cell
    return (int)floor(q);
}
__device__ __forceinline__ int cl_bucket_of(int cx, int cy, int cz, int buckets) {
    return (int)((((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u)) & (uint32_t)(buckets - 1));
}

// grid (chunks of the largest garment, B).  Travel against x_ref, then x_ref = x, the vertex's cell and the bucket counts.
__global__ __launch_bounds__(CL_BIN_BLOCK) void cl_contact_bin_kernel(ContactArgs a) {
    const int b = blockIdx.y;
    const int64_t v_off = a.csr[3 * (int64_t)b];
    const int V = (int)(a.csr[3 * (int64_t)(b + 1)] - v_off);
    const int i = blockIdx.x * CL_BIN_BLOCK + threadIdx.x;
    unsigned long long far = 0;                              // bits of a double >= 0: ordered as the doubles are
    if (i < V) {
        const int64_t g = v_off + i;
        const double px = a.x[3 * g], py = a.x[3 * g + 1], pz = a.x[3 * g + 2];
        if (a.flags & CL_LISTS_TRAVEL) far = (unsigned long long)__double_as_longlong(cl_sq(px, py, pz, a.x_ref[3 * g], a.x_ref[3 * g + 1], a.x_ref[3 * g + 2]));
        if (a.flags & CL_LISTS_BUILD) {
            a.x_ref[3 * g] = px; a.x_ref[3 * g + 1] = py; a.x_ref[3 * g + 2] = pz;
            const int cx = cl_cell_of(px, a.edge), cy = cl_cell_of(py, a.edge), cz = cl_cell_of(pz, a.edge);
            const int bk = cl_bucket_of(cx, cy, cz, a.buckets);
            a.cell[4 * g] = cx; a.cell[4 * g + 1] = cy; a.cell[4 * g + 2] = cz; a.cell[4 * g + 3] = bk;
            atomicAdd(a.count + (int64_t)b * a.buckets + bk, 1);
        }
    }
    if (a.flags & CL_LISTS_TRAVEL) {                         // every lane: the flag is the launch's
        far = cl_wave_max(far);
        if ((threadIdx.x & (GN_WAVE - 1)) == 0 && far) atomicMax((unsigned long long *)(a.diag + CL_DIAG * (int64_t)b + 3), far);
    }
}

// grid B: the exclusive scan of a garment's bucket counts -> start and cursor
__global__ __launch_bounds__(CL_SCAN_BLOCK) void cl_contact_scan_kernel(ContactArgs a) {
    __shared__ int part[2][CL_SCAN_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * a.buckets;
    const int per = (a.buckets + CL_SCAN_BLOCK - 1) / CL_SCAN_BLOCK;
    const int k0 = min(threadIdx.x * per, a.buckets), k1 = min(k0 + per, a.buckets);
    int sum = 0;
    for (int k = k0; k < k1; ++k) sum += a.count[base + k];
    int cur = 0;
    part[0][threadIdx.x] = sum;
    __syncthreads();
    for (int step = 1; step < CL_SCAN_BLOCK; step <<= 1) {   // inclusive scan, ping-pong
        const int val = part[cur][threadIdx.x] + (threadIdx.x >= step ? part[cur][threadIdx.x - step] : 0);
        part[cur ^ 1][threadIdx.x] = val;
        cur ^= 1;
        __syncthreads();
    }
    int run = part[cur][threadIdx.x] - sum;
    for (int k = k0; k < k1; ++k) {
        a.start[base + k] = run;
        a.cursor[base + k] = run;
        run += a.count[base + k];
    }
}

// grid as the bin kernel: the vertices of a garment grouped by bucket (the order inside a bucket does not reach the result: the lists are sorted)
__global__ __launch_bounds__(CL_BIN_BLOCK) void cl_contact_fill_kernel(ContactArgs a) {
    const int b = blockIdx.y;
    const int64_t v_off = a.csr[3 * (int64_t)b];
    const int V = (int)(a.csr[3 * (int64_t)(b + 1)] - v_off);
    const int i = blockIdx.x * CL_BIN_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int pos = atomicAdd(a.cursor + (int64_t)b * a.buckets + a.cell[4 * (v_off + i) + 3], 1);
    if (pos >= 0 && pos < V) a.items[v_off + pos] = i;
}

// slot s of the bucket of cell (ex, ey, ez), scanned for vertex i: the index of the vertex there when it is a partner of the definition, else -1
struct ContactQuery {
    int i, V;
    int64_t v_off;
    double px, py, pz, rx, ry, rz;                          // x_i and x0_i
};
__device__ __forceinline__ int cl_partner(const ContactArgs &a, const ContactQuery &q, int s, int s1, int ex, int ey, int ez) {
    if (s >= s1) return -1;
    const int j = a.items[q.v_off + s];
    if (j == q.i || j < 0 || j >= q.V) return -1;
    const int32_t *cj = a.cell + 4 * (q.v_off + j);
    if (cj[0] != ex || cj[1] != ey || cj[2] != ez) return -1;                              // another cell of the same bucket
    const double *p = a.x + 3 * (q.v_off + j);
    if (!(cl_sq(q.px, q.py, q.pz, p[0], p[1], p[2]) <= a.r2)) return -1;
    const double *p0 = a.x0 + 3 * (q.v_off + j);
    if (!(cl_sq(q.rx, q.ry, q.rz, p0[0], p0[1], p0[2]) > 0.0)) return -1;                  // tm2 = min(t2, rest2) > 0 iff rest2 > 0 (t2 > 0)
    return j;
}
__device__ __forceinline__ void cl_write_entry(const ContactArgs &a, const ContactQuery &q, int k, int j) {
    const double *p0 = a.x0 + 3 * (q.v_off + j);
    a.list_j[(q.v_off + q.i) * a.K + k] = j;
    a.list_tm2[(q.v_off + q.i) * a.K + k] = fmin(a.t2, cl_sq(q.rx, q.ry, q.rz, p0[0], p0[1], p0[2]));
}

// grid (the most vertices of a garment, B), ONE wave per vertex: the lanes share the slots of the 27 buckets, the partners found go to LDS, and an
// entry's place in the list is its rank among them (the indices are distinct).  More than CL_QUERY_CAP partners: the K smallest are drawn one after
// the other by scanning the buckets again -- slow, exact, and only for a vertex with hundreds of vertices within r.
__global__ __launch_bounds__(CL_QUERY_BLOCK) void cl_contact_query_kernel(ContactArgs a) {
    __shared__ int32_t found[CL_QUERY_CAP];
    const int b = blockIdx.y, lane = threadIdx.x;
    ContactQuery q;
    q.v_off = a.csr[3 * (int64_t)b];
    q.V = (int)(a.csr[3 * (int64_t)(b + 1)] - q.v_off);
    q.i = blockIdx.x;
    if (q.i >= q.V) return;                                  // the whole workgroup: nobody is left waiting at the barrier below
    const int64_t g = q.v_off + q.i;
    q.px = a.x[3 * g]; q.py = a.x[3 * g + 1]; q.pz = a.x[3 * g + 2];
    q.rx = a.x0[3 * g]; q.ry = a.x0[3 * g + 1]; q.rz = a.x0[3 * g + 2];
    int ex = 0, ey = 0, ez = 0, s0 = 0, s1 = 0;              // lane c < 27: cell c of the neighbourhood and the slots of its bucket
    if (lane < 27) {
        ex = a.cell[4 * g] + lane % 3 - 1; ey = a.cell[4 * g + 1] + (lane / 3) % 3 - 1; ez = a.cell[4 * g + 2] + lane / 9 - 1;
        const int64_t at = (int64_t)b * a.buckets + cl_bucket_of(ex, ey, ez, a.buckets);
        s0 = max(a.start[at], 0); s1 = min(a.cursor[at], q.V);
    }
    const int K = a.K;
    int total = 0;
    for (int c = 0; c < 27; ++c) {
        const int c0 = __shfl(s0, c), c1 = __shfl(s1, c), fx = __shfl(ex, c), fy = __shfl(ey, c), fz = __shfl(ez, c);
        for (int s = c0; s < c1; s += GN_WAVE) {             // wave-uniform bounds
            const int j = cl_partner(a, q, s + lane, c1, fx, fy, fz);
            const unsigned long long hit = __ballot(j >= 0);
            const int at = total + __popcll(hit & ((1ull << lane) - 1ull));
            if (j >= 0 && at < CL_QUERY_CAP) found[at] = j;
            total += __popcll(hit);
        }
    }
    const int n = min(total, K);
    __syncthreads();                                         // one wave: the hand-over of `found` from the lanes that wrote it
    if (total <= CL_QUERY_CAP) {
        for (int e = lane; e < total; e += GN_WAVE) {
            const int j = found[e];
            int rank = 0;
            for (int o = 0; o < total; ++o) rank += found[o] < j;
            if (rank < K) cl_write_entry(a, q, rank, j);
        }
    } else {
        int prev = -1;
        for (int k = 0; k < n; ++k) {                        // the smallest partner above the last one drawn
            int best = INT32_MAX;
            for (int c = 0; c < 27; ++c) {
                const int c0 = __shfl(s0, c), c1 = __shfl(s1, c), fx = __shfl(ex, c), fy = __shfl(ey, c), fz = __shfl(ez, c);
                for (int s = c0; s < c1; s += GN_WAVE) {
                    const int j = cl_partner(a, q, s + lane, c1, fx, fy, fz);
                    if (j > prev && j < best) best = j;
                }
            }
            best = gn_wave_min(best);
            if (lane == 0 && best < q.V) cl_write_entry(a, q, k, best);
            prev = best;
        }
    }
    for (int k = n + lane; k < K; k += GN_WAVE) {
        a.list_j[g * K + k] = -1;
        a.list_tm2[g * K + k] = 0.0;
    }
    if (lane == 0) {
        a.list_n[g] = n;
        a.list_total[g] = total;
        int64_t *d = a.diag + CL_DIAG * (int64_t)b;
        if (total > n) atomicAdd((unsigned long long *)d, (unsigned long long)(total - n));
        if ((int64_t)total > d[1]) atomicMax((unsigned long long *)(d + 1), (unsigned long long)total);     // d[1] only grows: a stale read costs an atomic
    }
}

extern "C" int gn_cloth_contact_buckets(int max_verts) {
    int64_t nb = 64;
    while (nb < 2 * (int64_t)max_verts) nb <<= 1;
    return max_verts < 0 || nb > (1 << 30) ? 0 : (int)nb;
}

// cell [*][4] int32, items [*] int32, x_ref [*][3] fp64, count / start / cursor [B][buckets] int32, each part on a 256-byte boundary
// (the last one padded to it as well)
static void cl_contact_ws(GnCarve &c, int64_t total_verts, int B, int buckets, ContactArgs &a) {
    const size_t nv = (size_t)total_verts, table = (size_t)B * (size_t)buckets;
    a.cell = c.take<int32_t>(4 * nv, 256);
    a.items = c.take<int32_t>(nv, 256);
    a.x_ref = c.take<double>(3 * nv, 256);
    a.count = c.take<int32_t>(table, 256);
    a.start = c.take<int32_t>(table, 256);
    a.cursor = c.take<int32_t>(table, 256);
    c.align(256);
}

extern "C" size_t gn_cloth_contact_workspace_bytes(int64_t total_verts, int B, int buckets) {
    ContactArgs a;
    return (total_verts < 0 || B < 0 || buckets < 0) ? 0 : gn_carve_bytes(cl_contact_ws, total_verts, B, buckets, a);
}

extern "C" int gn_cloth_contact_lists(const double *x, const double *x0, const int64_t *csr, int B, int64_t total_verts, int max_verts, int buckets,
                                      const double *collision_host, int K, int flags, void *workspace, size_t workspace_bytes, int32_t *list_j,
                                      double *list_tm2, int32_t *list_n, int32_t *list_total, int64_t *diag, void *stream) {
    const char *name = "gn_cloth_contact_lists";
    GN_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d outside [0, 65535]", name, B);
    GN_REQUIRE(total_verts >= 0 && total_verts < INT32_MAX / CL_MAX_LIST, "%s: %lld vertices: the lists must stay below 2^31 entries", name,
               (long long)total_verts);
    GN_REQUIRE(max_verts >= 0 && max_verts <= total_verts, "%s: max_verts=%d outside [0, %lld]", name, max_verts, (long long)total_verts);
    GN_REQUIRE(K >= 1 && K <= CL_MAX_LIST, "%s: K=%d outside [1, %d]", name, K, CL_MAX_LIST);
    GN_REQUIRE(flags >= 1 && flags <= 3, "%s: flags=%d: 1 (travel), 2 (build) or 3", name, flags);
    GN_REQUIRE(buckets >= 64 && (buckets & (buckets - 1)) == 0 && buckets >= gn_cloth_contact_buckets(max_verts) && gn_cloth_contact_buckets(max_verts),
               "%s: buckets=%d: a power of two of at least max(64, 2 max_verts)", name, buckets);
    GN_REQUIRE(collision_host, "%s: null collision constants", name);
    for (int k = 0; k < 3; ++k)
        GN_REQUIRE(cl_finite(collision_host[k]) && collision_host[k] > 0.0, "%s: collision constant %d is not finite and positive", name, k);
    GN_REQUIRE(collision_host[2] * collision_host[2] > collision_host[1], "%s: the cell edge %g does not exceed r = sqrt(%g)", name, collision_host[2],
               collision_host[1]);
    if (B == 0 || total_verts == 0) return GN_OK;
    GN_REQUIRE(x && x0 && csr && diag && workspace, "%s: null pointer", name);
    GN_REQUIRE(!(flags & CL_LISTS_BUILD) || (list_j && list_tm2 && list_n && list_total), "%s: null list", name);
    ContactArgs a;
    GnCarve c(workspace);
    cl_contact_ws(c, total_verts, B, buckets, a);
    GN_REQUIRE(workspace_bytes >= c.off, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, c.off);
    a.x = x; a.x0 = x0; a.csr = csr; a.list_j = list_j; a.list_tm2 = list_tm2; a.list_n = list_n; a.list_total = list_total; a.diag = diag;
    a.t2 = collision_host[0]; a.r2 = collision_host[1]; a.edge = collision_host[2]; a.K = K; a.buckets = buckets; a.flags = flags;
    hipStream_t st = gn_stream(stream);
    const dim3 per_vertex((unsigned)gn_cdiv(max_verts, CL_BIN_BLOCK), (unsigned)B);
    if (max_verts == 0) return GN_OK;
    if (flags & CL_LISTS_BUILD) GN_HIP(hipMemsetAsync(a.count, 0, 4 * (size_t)B * (size_t)buckets, st), name);
    hipLaunchKernelGGL(cl_contact_bin_kernel, per_vertex, dim3(CL_BIN_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    if (!(flags & CL_LISTS_BUILD)) return GN_OK;
    hipLaunchKernelGGL(cl_contact_scan_kernel, dim3((unsigned)B), dim3(CL_SCAN_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(cl_contact_fill_kernel, per_vertex, dim3(CL_BIN_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(cl_contact_query_kernel, dim3((unsigned)max_verts, (unsigned)B), dim3(CL_QUERY_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ vertex-face contacts
// Face-contact lists (cloth.py "Vertex-face contacts"): all (vertex, face) pairs of a garment, no search structure.  cl_face_hits_kernel: grid
// (blocks of CL_FACE_BLOCK vertices, face chunks, B); a workgroup stages the triangle constants of its chunk's faces from the CURRENT x in LDS tiles
// (pm_stage_tile) and every thread walks them for its one vertex, so inside a chunk a vertex meets the faces in ascending order; a face within rf
// that the vertex is no corner of has its tm2 evaluated from x0 and, when that is positive, becomes a hit: the first Kf hits of the (vertex, chunk)
// are kept, all are counted.  cl_face_concat_kernel (a thread per vertex) strings the chunks' hits together in chunk order -- ascending f -- cuts
// at Kf and counts the rest.  The chunks only spread one garment over the machine: the lists do not depend on their number.
#define CL_FACE_BLOCK ED_BLOCK              // pm_stage_tile's workgroup
#define CL_FACE_MAX_CHUNKS 1024

struct FaceListArgs {
    const double *x, *x0;                   // [*][3] positions now, start pose
    const int64_t *csr;                     // the solver's [B + 1][3]; only v_off is read
    const int32_t *faces;                   // [*][3]
    const int64_t *fcsr;                    // [B + 1]
    int32_t *hit_f, *hit_n;                 // [*][chunks][Kf], [*][chunks]
    double *hit_tm2;                        // [*][chunks][Kf]
    int32_t *list_f, *list_n, *list_total;
    double *list_tm2;
    int64_t *fdiag, *bad;
    double tf2, rf2;
    int Kf, chunks;
};

__global__ __launch_bounds__(CL_FACE_BLOCK) void cl_face_hits_kernel(FaceListArgs a) {
    __shared__ double tri[PM_NCONST][PM_TILE];
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int64_t v_off = a.csr[3 * (int64_t)b], f_off = a.fcsr[b];
    const int V = (int)(a.csr[3 * (int64_t)(b + 1)] - v_off);
    const int64_t F = a.fcsr[b + 1] - f_off;
    if ((int64_t)blockIdx.x * CL_FACE_BLOCK >= V) return;    // the whole workgroup: nobody is left waiting at a barrier below
    const int64_t per = (F + a.chunks - 1) / a.chunks;       // faces per chunk of this garment
    const int64_t f0 = chunk * per, f1 = f0 + per < F ? f0 + per : F;
    const int i = blockIdx.x * CL_FACE_BLOCK + threadIdx.x;
    const bool own = i < V;
    const double *xb = a.x + 3 * v_off, *x0b = a.x0 + 3 * v_off;
    const int32_t *fc = a.faces + 3 * f_off;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (own) { qx = xb[3 * (int64_t)i]; qy = xb[3 * (int64_t)i + 1]; qz = xb[3 * (int64_t)i + 2]; }
    const int64_t slot = (v_off + i) * a.chunks + chunk;     // read only when own
    int n = 0;
    for (int64_t t0 = f0; t0 < f1; t0 += PM_TILE) {          // workgroup-uniform bounds
        const int m = (int)(f1 - t0 < PM_TILE ? f1 - t0 : PM_TILE);
        __syncthreads();
        pm_stage_tile(tri, xb, (int64_t)V, fc, t0, m, a.bad);
        __syncthreads();
        if (!own) continue;
        for (int j = 0; j < m; ++j) {
            const PmTri T = pm_load(tri, j);
            if (!(pm_sqdist(T, qx, qy, qz) <= a.rf2)) continue;
            const int64_t f = t0 + j;
            const int32_t ia = fc[3 * f], ib = fc[3 * f + 1], ic = fc[3 * f + 2];
            if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;     // flagged by the staging, never dereferenced
            if (ia == i || ib == i || ic == i) continue;                                   // a corner of the face, by index
            double p[3][3];
            const int32_t cs[3] = {ia, ib, ic};
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[k][c] = x0b[3 * (int64_t)cs[k] + c];
            const PmTri R = pm_tri_of(p[0], p[1], p[2]);
            const double tm2 = fmin(a.tf2, pm_sqdist(R, x0b[3 * (int64_t)i], x0b[3 * (int64_t)i + 1], x0b[3 * (int64_t)i + 2]));
            if (!(tm2 > 0.0)) continue;
            if (n < a.Kf) {
                a.hit_f[slot * a.Kf + n] = (int32_t)f;
                a.hit_tm2[slot * a.Kf + n] = tm2;
            }
            ++n;
        }
    }
    if (own) a.hit_n[slot] = n;
}

// grid (blocks of CL_FACE_BLOCK vertices, B): a thread per vertex
__global__ __launch_bounds__(CL_FACE_BLOCK) void cl_face_concat_kernel(FaceListArgs a) {
    const int b = blockIdx.y;
    const int64_t v_off = a.csr[3 * (int64_t)b];
    const int V = (int)(a.csr[3 * (int64_t)(b + 1)] - v_off);
    const int i = blockIdx.x * CL_FACE_BLOCK + threadIdx.x;
    if (i >= V) return;
    const int64_t g = v_off + i;
    const int Kf = a.Kf;
    int n = 0;
    long long total = 0;
    for (int c = 0; c < a.chunks; ++c) {
        const int64_t slot = g * a.chunks + c;
        int h = a.hit_n[slot];
        h = h < 0 ? 0 : h;
        total += h;
        const int kept = h < Kf ? h : Kf;
        for (int k = 0; k < kept && n < Kf; ++k, ++n) {
            a.list_f[g * Kf + n] = a.hit_f[slot * Kf + k];
            a.list_tm2[g * Kf + n] = a.hit_tm2[slot * Kf + k];
        }
    }
    for (int k = n; k < Kf; ++k) {
        a.list_f[g * Kf + k] = -1;
        a.list_tm2[g * Kf + k] = 0.0;
    }
    a.list_n[g] = n;
    a.list_total[g] = (int32_t)(total < INT32_MAX ? total : INT32_MAX);
    int64_t *d = a.fdiag + CL_FACE_DIAG * (int64_t)b;        // integer sums and maxima: the order of the atomics cannot reach the result
    if (total > n) atomicAdd((unsigned long long *)d, (unsigned long long)(total - n));
    if (total > d[1]) atomicMax((unsigned long long *)(d + 1), (unsigned long long)total);
}

static int cl_face_constants(const char *name, const double *face_host, const double *collision_host, int Kf) {
    GN_REQUIRE(Kf >= 1 && Kf <= CL_FACE_MAX_LIST, "%s: Kf=%d outside [1, %d]", name, Kf, CL_FACE_MAX_LIST);
    GN_REQUIRE(face_host, "%s: null face constants", name);
    for (int k = 0; k < 2; ++k)
        GN_REQUIRE(cl_finite(face_host[k]) && face_host[k] > 0.0, "%s: face constant %d is not finite and positive", name, k);
    GN_REQUIRE(collision_host, "%s: face constants need the vertex contacts' constants (null collision constants)", name);
    return GN_OK;
}

extern "C" int gn_cloth_face_contact_lists(const double *x, const double *x0, const int64_t *csr, const int32_t *faces, const int64_t *fcsr, int B,
                                           int64_t total_verts, int64_t total_faces, int max_verts, const double *face_host,
                                           const double *collision_host, int Kf, int chunks, int32_t *hit_f, double *hit_tm2, int64_t hit_entries,
                                           int32_t *hit_n, int64_t hit_rows, int32_t *list_f, double *list_tm2, int64_t list_entries, int32_t *list_n,
                                           int32_t *list_total, int64_t list_rows, int64_t *fdiag, int64_t fdiag_rows, int64_t *bad, void *stream) {
    const char *name = "gn_cloth_face_contact_lists";
    GN_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d outside [0, 65535]", name, B);
    GN_REQUIRE(chunks >= 1 && chunks <= CL_FACE_MAX_CHUNKS, "%s: chunks=%d outside [1, %d]", name, chunks, CL_FACE_MAX_CHUNKS);
    if (int rc = cl_face_constants(name, face_host, collision_host, Kf)) return rc;
    GN_REQUIRE(total_verts >= 0 && total_verts < INT32_MAX / CL_MAX_LIST && total_faces >= 0 && total_faces < INT32_MAX / 3,
               "%s: %lld vertices, %lld faces: the tables must stay below 2^31 entries", name, (long long)total_verts, (long long)total_faces);
    GN_REQUIRE(max_verts >= 0 && max_verts <= total_verts, "%s: max_verts=%d outside [0, %lld]", name, max_verts, (long long)total_verts);
    GN_REQUIRE(hit_entries >= total_verts * chunks * Kf && hit_rows >= total_verts * chunks,
               "%s: hit buffers of %lld entries and %lld rows, %lld and %lld needed", name, (long long)hit_entries, (long long)hit_rows,
               (long long)(total_verts * chunks * Kf), (long long)(total_verts * chunks));
    GN_REQUIRE(list_entries >= total_verts * Kf && list_rows >= total_verts, "%s: lists of %lld entries and %lld rows, %lld and %lld needed", name,
               (long long)list_entries, (long long)list_rows, (long long)(total_verts * Kf), (long long)total_verts);
    GN_REQUIRE(fdiag_rows >= B, "%s: fdiag of %lld rows, %d needed", name, (long long)fdiag_rows, B);
    if (B == 0 || total_verts == 0 || max_verts == 0) return GN_OK;
    GN_REQUIRE(x && x0 && csr && fcsr && fdiag && bad && (total_faces == 0 || faces), "%s: null pointer", name);
    GN_REQUIRE(hit_f && hit_tm2 && hit_n && list_f && list_tm2 && list_n && list_total, "%s: null list", name);
    FaceListArgs a;
    a.x = x; a.x0 = x0; a.csr = csr; a.faces = faces; a.fcsr = fcsr; a.hit_f = hit_f; a.hit_tm2 = hit_tm2; a.hit_n = hit_n; a.list_f = list_f;
    a.list_tm2 = list_tm2; a.list_n = list_n; a.list_total = list_total; a.fdiag = fdiag; a.bad = bad; a.tf2 = face_host[0]; a.rf2 = face_host[1];
    a.Kf = Kf; a.chunks = chunks;
    hipStream_t st = gn_stream(stream);
    const unsigned vb = (unsigned)gn_cdiv(max_verts, CL_FACE_BLOCK);
    hipLaunchKernelGGL(cl_face_hits_kernel, dim3(vb, (unsigned)chunks, (unsigned)B), dim3(CL_FACE_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    hipLaunchKernelGGL(cl_face_concat_kernel, dim3(vb, (unsigned)B), dim3(CL_FACE_BLOCK), 0, st, a);
    GN_LAUNCH_CHECK(name);
    return GN_OK;
}

extern "C" int gn_cloth_simulate_face_contacts_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0,
                                                     const double *alpha_t, const int64_t *csr, const int64_t *colour_off, int B, int64_t total_verts,
                                                     int64_t total_constraints, int64_t substeps, int max_substeps_per_launch,
                                                     const double *consts_host, int lds_bytes, int block, int64_t *bad, const int32_t *list_j,
                                                     const double *list_tm2, const int32_t *list_n, int K, const double *collision_host, double *corr,
                                                     int64_t *diag, const int32_t *faces, const int64_t *fcsr, int64_t total_faces,
                                                     const int32_t *flist_f, const double *flist_tm2, int64_t flist_entries, const int32_t *flist_n,
                                                     int64_t flist_rows, int Kf, const double *face_host, int64_t *fdiag, int64_t fdiag_rows,
                                                     void *stream) {
    const char *name = "gn_cloth_simulate_face_contacts_batch";
    GN_REQUIRE(K >= 1 && K <= CL_MAX_LIST, "%s: K=%d outside [1, %d]", name, K, CL_MAX_LIST);
    if (int rc = cl_face_constants(name, face_host, collision_host, Kf)) return rc;
    GN_REQUIRE(cl_finite(collision_host[3]) && collision_host[3] > 0.0 && collision_host[3] <= 1.0, "%s: collision constant 3 (relax) is not in (0, 1]",
               name);
    GN_REQUIRE(total_faces >= 0 && total_faces < INT32_MAX / 3, "%s: %lld faces: the table must stay below 2^31 entries", name, (long long)total_faces);
    GN_REQUIRE(total_verts < 0 || (flist_entries >= total_verts * Kf && flist_rows >= total_verts),
               "%s: face lists of %lld entries and %lld rows, %lld and %lld needed", name, (long long)flist_entries, (long long)flist_rows,
               (long long)(total_verts * Kf), (long long)total_verts);
    GN_REQUIRE(fdiag_rows >= B, "%s: fdiag of %lld rows, %d needed", name, (long long)fdiag_rows, B);
    GN_REQUIRE(B == 0 || (diag && fdiag && fcsr), "%s: null diag / fdiag / fcsr", name);
    GN_REQUIRE(B == 0 || total_verts == 0 || (list_j && list_tm2 && list_n && corr && flist_f && flist_tm2 && flist_n), "%s: null list / corr", name);
    GN_REQUIRE(B == 0 || total_faces == 0 || faces, "%s: null faces", name);
    ClothArgsFaces a;
    a.x = x; a.v = v; a.w = w; a.pairs = pairs; a.l0 = l0; a.alpha_t = alpha_t; a.csr = csr; a.colour_off = colour_off; a.bad = bad;
    a.list_j = list_j; a.list_tm2 = list_tm2; a.list_n = list_n; a.corr = corr; a.diag = diag; a.relax = collision_host[3]; a.K = K;
    a.faces = faces; a.fcsr = fcsr; a.flist_f = flist_f; a.flist_tm2 = flist_tm2; a.flist_n = flist_n; a.fdiag = fdiag; a.Kf = Kf;
    return cloth_launch<true, true>(name, a, B, total_verts, total_constraints, substeps, max_substeps_per_launch, consts_host, lds_bytes, block,
                                    stream);
}

// optim.hip -- gn_adam_step: torch.optim.Adam's update of every tensor of a device table in one launch (garmentnets_amd/optim.py FusedAdam);
//              gn_grad_pack: every gradient of a device table into one flat buffer in one launch (garmentnets_amd/parallel.py GradientReducer), below
//
// A workgroup owns one GN_ADAM_CHUNK-element chunk of one tensor (binary search of its number in the entries' first-workgroup column).  Each element of
// p, g, exp_avg, exp_avg_sq is read once and the three results written once: float4 where all four pointers of the tensor are 16-byte aligned (a chunk
// starts a multiple of GN_ADAM_CHUNK elements in, so the alignment holds for every chunk), scalars elsewhere and on the tail.  adam_element is the one
// arithmetic of both paths: the result of an element does not depend on the path it took.  No atomics.
#include "common.h"

#pragma clang fp contract(off)

#define ADAM_WG 256
#define ADAM_MAX_GRID (1 << 20)   // workgroups per launch; a longer table is split over launches

struct AdamHyperArg {
    GnAdamHyper h[GN_ADAM_MAX_HYPER];
};

// torch/optim/adam.py _single_tensor_adam, in fp64 of the fp32 operands, each stored value rounded once:
//   g += wd * p;  m = m + (g - m) * (1 - b1);  v = v * b2 + (1 - b2) * g * g;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
__device__ __forceinline__ void adam_element(float &p, float g32, float &m32, float &v32, const GnAdamHyper &h) {
    double g = (double)g32;
    if (h.weight_decay != 0.0) g += h.weight_decay * (double)p;
    const double m = (double)m32 + (g - (double)m32) * (1.0 - h.beta1);
    const double v = (double)v32 * h.beta2 + (1.0 - h.beta2) * g * g;
    const double denom = sqrt(v) / h.bias_correction2_sqrt + h.eps;
    p = (float)((double)p - (h.lr / h.bias_correction1) * (m / denom));
    m32 = (float)m;
    v32 = (float)v;
}

__global__ __launch_bounds__(ADAM_WG) void adam_step_kernel(const GnAdamEntry *__restrict__ table, int n, int64_t blk_base, int64_t nblocks, AdamHyperArg hy) {
    const int64_t b = blk_base + blockIdx.x;
    if (b >= nblocks) return;
    int lo = 0, hi = n - 1;                       // the last entry whose blk0 <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const GnAdamEntry e = table[lo];
    const GnAdamHyper &h = hy.h[e.hyper];
    const int64_t start = (b - e.blk0) * GN_ADAM_CHUNK;
    if (start >= e.numel) return;
    const int64_t len64 = e.numel - start;
    const int len = len64 < GN_ADAM_CHUNK ? (int)len64 : GN_ADAM_CHUNK;
    float *p = e.p + start, *m = e.exp_avg + start, *v = e.exp_avg_sq + start;
    const float *g = e.g + start;
    const bool aligned = (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.exp_avg | (uintptr_t)e.exp_avg_sq) & 15) == 0;
    int done = 0;
    if (aligned) {
        const int nvec = len >> 2;
        for (int i = threadIdx.x; i < nvec; i += ADAM_WG) {
            float4 pp = reinterpret_cast<float4 *>(p)[i], mm = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
            const float4 gg = reinterpret_cast<const float4 *>(g)[i];
            adam_element(pp.x, gg.x, mm.x, vv.x, h);
            adam_element(pp.y, gg.y, mm.y, vv.y, h);
            adam_element(pp.z, gg.z, mm.z, vv.z, h);
            adam_element(pp.w, gg.w, mm.w, vv.w, h);
            reinterpret_cast<float4 *>(p)[i] = pp;
            reinterpret_cast<float4 *>(m)[i] = mm;
            reinterpret_cast<float4 *>(v)[i] = vv;
        }
        done = nvec << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += ADAM_WG) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_element(pp, g[i], mm, vv, h);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

extern "C" int gn_adam_step(const GnAdamEntry *table, int n, int64_t nblocks, const GnAdamHyper *hyper_host, int nhyper, void *stream) {
    GN_REQUIRE(n >= 0 && nblocks >= 0, "gn_adam_step: negative counts");
    if (n == 0 || nblocks == 0) return GN_OK;
    GN_REQUIRE(table != nullptr, "gn_adam_step: the device table is required");
    GN_REQUIRE(hyper_host != nullptr && nhyper >= 1 && nhyper <= GN_ADAM_MAX_HYPER, "gn_adam_step: 1..%d hyper-parameter sets", GN_ADAM_MAX_HYPER);
    AdamHyperArg hy = {};
    for (int i = 0; i < nhyper; ++i) {
        const GnAdamHyper &h = hyper_host[i];
        GN_REQUIRE(h.bias_correction1 > 0.0 && h.bias_correction2_sqrt > 0.0, "gn_adam_step: set %d: the bias corrections must be positive (step >= 1, betas < 1)", i);
        hy.h[i] = h;
    }
    hipStream_t st = gn_stream(stream);
    for (int64_t base = 0; base < nblocks; base += ADAM_MAX_GRID) {
        const int64_t grid = nblocks - base < ADAM_MAX_GRID ? nblocks - base : ADAM_MAX_GRID;
        hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)grid), dim3(ADAM_WG), 0, st, table, n, base, nblocks, hy);
    }
    GN_LAUNCH_CHECK("gn_adam_step");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ gn_grad_pack
// Every gradient of a device table into one flat buffer, divided by the world size, in one launch (garmentnets_amd/parallel.py GradientReducer): the
// buffer is what ONE collective then sums.  A workgroup owns one GN_ADAM_CHUNK slice of one tensor, found as adam_step_kernel finds its own.  A slice
// of flat starts 16-byte aligned (dst_off % 4 == 0, the chunk a multiple of 4), so every store is a float4, the one that holds a tensor's tail and its
// zero pad included.  The loads are float4 where the slice of the SOURCE starts 16-byte aligned and written element by element elsewhere (a gradient that
// is a view at an odd element offset: nothing there assumes more than a float's alignment; gfx950 serves dword-aligned wide loads, and the compiler is
// free to form them); the tail's vector is loaded element by element either way.  world == 1 copies the bits; otherwise the value is
// __fdiv_rn(g, world), one rounding, whatever the path.  No atomics, one writer per element; no store reaches flat_numel or beyond.
__device__ __forceinline__ float4 pack_scale(float4 v, float w, bool copy) {
    if (copy) return v;
    return make_float4(__fdiv_rn(v.x, w), __fdiv_rn(v.y, w), __fdiv_rn(v.z, w), __fdiv_rn(v.w, w));
}

__global__ __launch_bounds__(ADAM_WG) void grad_pack_kernel(const GnPackEntry *__restrict__ table, int n, int64_t blk_base, int64_t nblocks,
                                                            float *__restrict__ flat, int64_t flat_numel, float world) {
    const int64_t b = blk_base + blockIdx.x;
    if (b >= nblocks) return;
    int lo = 0, hi = n - 1;                       // the last entry whose blk0 <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    const GnPackEntry e = table[lo];
    const int64_t start = (b - e.blk0) * GN_ADAM_CHUNK;
    if (b < e.blk0 || start >= e.numel || e.dst_off < 0 || (e.dst_off & 3)) return;
    const int64_t len64 = e.numel - start;
    const int len = len64 < GN_ADAM_CHUNK ? (int)len64 : GN_ADAM_CHUNK;
    const int64_t dst0 = e.dst_off + start;
    const int nvec = (len + 3) >> 2;              // the tail's vector carries the zero pad
    const int64_t room = flat_numel - dst0;       // floats of flat from this slice on (a table that points past the buffer writes nothing there)
    const float *src = e.src == nullptr ? nullptr : static_cast<const float *>(e.src) + start;
    const bool wide = (((uintptr_t)src) & 15) == 0;
    const bool copy = world == 1.0f;
    float4 *dst = reinterpret_cast<float4 *>(flat + dst0);
    for (int i = threadIdx.x; i < nvec; i += ADAM_WG) {
        const int at = i << 2;
        if ((int64_t)at + 4 > room) return;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src != nullptr) {
            if (at + 4 <= len) {
                if (wide) {
                    v = reinterpret_cast<const float4 *>(src)[i];
                } else {
                    v = make_float4(src[at], src[at + 1], src[at + 2], src[at + 3]);
                }
            } else {
                v.x = src[at];
                if (at + 1 < len) v.y = src[at + 1];
                if (at + 2 < len) v.z = src[at + 2];
            }
            v = pack_scale(v, world, copy);
        }
        dst[i] = v;
    }
}

extern "C" int gn_grad_pack(const GnPackEntry *table, int n_entries, int64_t n_blocks, float *flat, int64_t flat_numel, int world, void *stream) {
    GN_REQUIRE(table != nullptr && flat != nullptr, "gn_grad_pack: the device table and the flat buffer are required");
    GN_REQUIRE(n_entries >= 1, "gn_grad_pack: n_entries must be at least 1, got %d", n_entries);
    GN_REQUIRE(world >= 1, "gn_grad_pack: world must be at least 1, got %d", world);
    GN_REQUIRE(n_blocks >= 1 && n_blocks < ((int64_t)1 << 31), "gn_grad_pack: n_blocks must lie in [1, 2^31), got %lld", (long long)n_blocks);
    GN_REQUIRE(flat_numel >= 0 && (flat_numel & 3) == 0, "gn_grad_pack: flat_numel must be a multiple of 4, got %lld", (long long)flat_numel);
    GN_REQUIRE((((uintptr_t)flat) & 15) == 0, "gn_grad_pack: flat must be 16-byte aligned");
    hipStream_t st = gn_stream(stream);
    for (int64_t base = 0; base < n_blocks; base += ADAM_MAX_GRID) {
        const int64_t grid = n_blocks - base < ADAM_MAX_GRID ? n_blocks - base : ADAM_MAX_GRID;
        hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)grid), dim3(ADAM_WG), 0, st, table, n_entries, base, n_blocks, flat, flat_numel, (float)world);
    }
    GN_LAUNCH_CHECK("gn_grad_pack");
    return GN_OK;
}

// common.h -- shared helpers for the gfx950 kernels of libgarmentnets_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/garmentnets_hip.h"

#define GN_WAVE 64

// This library is written for ONE target: gfx950 (MI355X, CDNA4) with the ROCm 7 toolchain (clang >= 20).  The kernels use its instructions directly
// (v_mfma_f32_32x32x16_f16, global_load_lds_dwordx4, v_fma_mix_f32, v_maximum3_f32 through __builtin_elementwise_maximum) and there is no other code
// path: the Makefile's HIPCC / ARCH overrides exist for a differently installed ROCm, not for another architecture -- say so at compile time.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libgarmentnets_hip.so is gfx950-only (MI355X): build with --offload-arch=gfx950"
#endif
#if !defined(__has_builtin) || !__has_builtin(__builtin_elementwise_maximum)
#error "libgarmentnets_hip.so needs the ROCm 7 hipcc (clang >= 20: __builtin_elementwise_maximum)"
#endif

// gn_grid_scatter's reduce codes (include/garmentnets_hip.h)
enum { GN_REDUCE_MAX = 0, GN_REDUCE_MEAN = 1, GN_REDUCE_SUM = 2, GN_REDUCE_MIN = 3, GN_REDUCE_MUL = 4 };

void gn_set_error(const char *fmt, ...);

#define GN_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            gn_set_error(__VA_ARGS__);   \
            return GN_EINVAL;            \
        }                                \
    } while (0)

#define GN_LAUNCH_CHECK(name)                                                        \
    do {                                                                             \
        hipError_t e__ = hipGetLastError();                                          \
        if (e__ != hipSuccess) {                                                     \
            gn_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));     \
            return GN_ELAUNCH;                                                       \
        }                                                                            \
    } while (0)

#define GN_HIP(call, name)                                                           \
    do {                                                                             \
        hipError_t e__ = (call);                                                     \
        if (e__ != hipSuccess) {                                                     \
            gn_set_error("%s: %s", name, hipGetErrorString(e__));                    \
            return GN_ELAUNCH;                                                       \
        }                                                                            \
    } while (0)

// the launch stream of a C-ABI call.  A non-null stream also selects the device: kernels, memsets and function attributes of this
// call go to the device the stream lives on (hipSetDevice when it differs from the thread's current one), so a caller working on
// cuda:N only has to pass a stream of that device (ops._stream takes it from the tensors).  The null stream means "current device".
hipStream_t gn_stream(void *s);
// name of the kernel variant the last gn_conv3d_* call of this thread launched (bench.py labels its roofline with it)
void gn_note_kernel(const char *name);
static inline int64_t gn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// zero a pair of fp64 statistics buffers (sum, sumsq: n values each) that a kernel accumulates into with atomics: ONE fill when the caller laid them out back
// to back (ops._stats_buffers does) -- a fill is ~5 us of stream time, and a 32^3 UNet layer is not much longer than that
static inline hipError_t gn_zero_stats(double *sum, double *sumsq, size_t n, hipStream_t st) {
    if (sumsq == sum + n) return hipMemsetAsync(sum, 0, 2 * n * sizeof(double), st);
    hipError_t e = hipMemsetAsync(sum, 0, n * sizeof(double), st);
    return e != hipSuccess ? e : hipMemsetAsync(sumsq, 0, n * sizeof(double), st);
}

// A workspace layout is written ONCE, as a function over this cursor that returns the parts in order (a braced list evaluates left to right).  Host
// only.  With a null base the walk only measures (every part comes back null) -- that is the gn_*_workspace_bytes entry; with the caller's pointer it
// hands out the parts.  Either way `off` ends as the byte count.  Alignments are of the OFFSET: the base is expected on the layout's largest one.
struct GnCarve {
    char *base;
    size_t off = 0;
    explicit GnCarve(void *ws = nullptr) : base(static_cast<char *>(ws)) {}
    void align(size_t a) { off = (off + a - 1) / a * a; }
    void pad(size_t bytes) { off += bytes; }                // slack behind the parts that a size has always included
    template <class T> T *take(size_t n, size_t a = alignof(T)) {
        align(a);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};
// the byte count of a layout: its carve function walked on a null base
template <class F, class... A> static size_t gn_carve_bytes(F carve, A &&...shape) {
    GnCarve c;
    carve(c, shape...);
    return c.off;
}

// squared distance in the pinned operation order ((dx*dx + dy*dy) + dz*dz), fp32, no FMA contraction
// (the library is compiled with -ffp-contract=off; the intrinsics make it explicit).
__device__ __forceinline__ float gn_sqdist3(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    float s = __fmul_rn(dx, dx);
    s = __fadd_rn(s, __fmul_rn(dy, dy));
    s = __fadd_rn(s, __fmul_rn(dz, dz));
    return s;
}

// ReLU with torch's NaN behaviour (relu(NaN) = NaN).  fmaxf(v, 0) would return 0 for a NaN and turn an upstream overflow
// (e.g. an activation beyond the fp16 range in the split-operand kernels) into a silently wrong finite result.
// IEEE 754-2019 maximum(v, 0) -- NaN-propagating -- is ONE gfx950 instruction (v_maximum3_f32 v, v, 0, 0); the C form `v < 0 ? 0 : v`
// compiled to v_cmp_ngt_f32 + 2 hazard wait states on vcc + v_cndmask_b32 per value (the largest VALU item of the decoder MLPs'
// layer hand-over).  Same values; the only bit that can differ is the sign of a zero (maximum(-0, +0) = +0, the C form kept -0).
__device__ __forceinline__ float gn_relu(float v) { return __builtin_elementwise_maximum(v, 0.f); }

// vector types, reductions, float orders, MFMA / plane split, LDS DMA, sampler arithmetic, tile geometry
#include "device_prims.h"

// device_prims.h -- the leaf device helpers every gfx950 kernel file shares (included through common.h): vector types, DPP and shuffle
// reductions, order-preserving float encodings, the 16-bit MFMA wrapper and the exact plane split, the global -> LDS DMA and its
// wait counts, the trilinear sampler's index arithmetic and the conv tile geometry.  ONE definition each: a kernel file that needs
// a variant adds it here, next to its relatives, with the reason.  tools/isa_diff.py shows what a change here does to every kernel.
#pragma once

// ------------------------------------------------------------------------------------------------ vector types
typedef float f32x2 __attribute__((ext_vector_type(2)));       // v_pk_*_f32 operands
typedef float f32x4 __attribute__((ext_vector_type(4)));       // a dwordx4 the compiler may keep in any four registers (HIP's float4 is a struct)
typedef float f32x16 __attribute__((ext_vector_type(16)));     // the accumulator of a 32x32 MFMA
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));    // the A / B operand of v_mfma_f32_32x32x16_f16
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------ reductions
// DPP controls of the four steps that reduce a 16-lane row in place
#define GN_DPP_QUAD_XOR1 0xB1        // quad_perm [1,0,3,2]
#define GN_DPP_QUAD_XOR2 0x4E        // quad_perm [2,3,0,1]
#define GN_DPP_ROW_HALF_MIRROR 0x141
#define GN_DPP_ROW_MIRROR 0x140
template <int CTRL>
__device__ __forceinline__ int gn_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL>
__device__ __forceinline__ float gn_dpp(float v) { return __int_as_float(gn_dpp<CTRL>(__float_as_int(v))); }

// v = op(v, partner) over the N <= 16 values replicated with period N along every 16-lane DPP row, log2(N) steps in the FIXED order quad xor 1,
// quad xor 2, row_half_mirror, row_mirror: every lane ends up with the result, and a float sum is deterministic (the fp32 decoder's output sum
// rests on that order).  N = 16: the whole row.
template <int N, class T, class Op>
__device__ __forceinline__ T gn_row_reduce(T v, Op op) {
    v = op(v, gn_dpp<GN_DPP_QUAD_XOR1>(v));
    v = op(v, gn_dpp<GN_DPP_QUAD_XOR2>(v));
    if (N > 4) v = op(v, gn_dpp<GN_DPP_ROW_HALF_MIRROR>(v));
    if (N > 8) v = op(v, gn_dpp<GN_DPP_ROW_MIRROR>(v));
    return v;
}
template <int N = 16>
__device__ __forceinline__ float gn_row_max(float v) { return gn_row_reduce<N>(v, [](float a, float b) { return fmaxf(a, b); }); }
template <int N = 16>
__device__ __forceinline__ int gn_row_min(int v) { return gn_row_reduce<N>(v, [](int a, int b) { return min(a, b); }); }
__device__ __forceinline__ float gn_row_sum(float v) { return gn_row_reduce<16>(v, [](float a, float b) { return a + b; }); }
// max over the 32 lanes of each lane half (every lane of the half ends up with it): rows 0|1 and 2|3
__device__ __forceinline__ float gn_half_max(float v) { v = gn_row_max(v); return fmaxf(v, __shfl_xor(v, 16)); }
// the whole wave: the four row results meet through readlanes (wave-uniform result)
__device__ __forceinline__ float gn_wave_max(float v) {
    const int iv = __float_as_int(gn_row_max(v));
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(iv, 0)), __int_as_float(__builtin_amdgcn_readlane(iv, 16))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(iv, 32)), __int_as_float(__builtin_amdgcn_readlane(iv, 48))));
}
__device__ __forceinline__ int gn_wave_min(int v) {
    v = gn_row_min(v);
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// arg-min of (value, index) keys over the wave, in place in the lvalues V (float) and I (int) of every lane: the smaller value wins, equal values
// go to the LOWEST index.  A macro ON PURPOSE: as an inlined function (reference or by-value form) the same text changed the register allocation
// of all nine kNN kernels that use it.
#define GN_WAVE_ARGMIN(V, I)                                                  \
    _Pragma("unroll") for (int off_ = 32; off_ >= 1; off_ >>= 1) {            \
        const float ov_ = __shfl_xor(V, off_);                                \
        const int oi_ = __shfl_xor(I, off_);                                  \
        if (ov_ < (V) || (ov_ == (V) && oi_ < (I))) { (V) = ov_; (I) = oi_; } \
    }

// ------------------------------------------------------------------------------------------------ float orders for integer atomics
// Two conventions, NOT interchangeable -- each site's memset / empty test depends on its own:
//  * gn_ord_* (unsigned compare): the code is monotone in x and lies strictly between 0 and ~0 for every non-NaN float.  A NaN of EITHER sign
//    takes the extreme code of its side (gn_ord_enc_min: 0 for an atomicMin, gn_ord_enc_max: ~0 for an atomicMax), wins, and gn_ord_dec turns it
//    back into a NaN: numpy.min / numpy.max, torch's amin / amax.  The isosurface value range uses them as they are.  The grid scatter runs
//    atomicMax on gn_ord_enc_max(x) for 'max' and on ~gn_ord_enc_min(x) for 'min' (gn_ord_dec_inv undoes the complement): both are > 0 for
//    every float, a NaN included (~0 either way), so a zero-filled volume still reads as "empty".
//  * gn_sord_* (sa_fused's LDS max, SIGNED compare): an involution on the bit pattern, enc(-inf) is the smallest code; nothing means "empty".
__device__ __forceinline__ float gn_ord_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }
// gn_ord_dec(~e), written out: (e's top bit clear: ~e has it set)
__device__ __forceinline__ float gn_ord_dec_inv(unsigned e) { return __uint_as_float((e & 0x80000000u) ? e : (~e & 0x7fffffffu)); }
__device__ __forceinline__ unsigned gn_ord_enc_min(float v) { const unsigned e = __float_as_uint(v); return v != v ? 0u : ((e & 0x80000000u) ? ~e : (e | 0x80000000u)); }
__device__ __forceinline__ unsigned gn_ord_enc_max(float v) { const unsigned e = __float_as_uint(v); return v != v ? 0xffffffffu : ((e & 0x80000000u) ? ~e : (e | 0x80000000u)); }
__device__ __forceinline__ int gn_sord_enc(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float gn_sord_dec(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// ------------------------------------------------------------------------------------------------ 16-bit matrix operands
// Exact residual of an fp32 value r against one half of a packed fp16 pair h2 in ONE instruction: v_fma_mix_f32 reads the fp16 half in place,
// fma(f32(h), -1, r) = r - f32(h) with one rounding -- of a value that IS representable when h = fp16_rn(r) or any fp16 within the split's range (the
// difference has at most 13 significant bits), so the result is bit-identical to v_cvt_f32_f16 + v_sub_f32 (hipcc's selection for the C
// expression: two instructions per value; the plane split is the largest VALU item of every f16x2 kernel).  Not volatile: schedulable, removable.
__device__ __forceinline__ float gn_resid_lo(unsigned h2, float r) {
    float o;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(o) : "v"(h2), "v"(r));
    return o;
}
__device__ __forceinline__ float gn_resid_hi(unsigned h2, float r) {
    float o;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(o) : "v"(h2), "v"(r));
    return o;
}

// four floats -> P 16-bit planes (exact residual chain x = x1 + x2 [+ x3], xi = fp16_rn / bf16_rn of the running residual), each plane
// packed as 4 x 16 bit = uint2.  v_cvt_pk_bf16_f32 rounds to nearest even like the host-side pack of the weights.
// The staging step AROUND it (affine, zero padding after the affine, this split, the store of P planes) is written out at each of its four sites in
// unet_split.hip ON PURPOSE: as one inlined function called from the three generic sites it changed 10 of 12 kernels inside their main loops
// (conv3d_split_wide_kernel<2, true> 228 -> 232 VGPRs, conv3d_split_kernel<2, 2, *> +115 / +118 instructions, <2, 3, false> +370).
template <int P, bool F16>
__device__ __forceinline__ void split4(float r0, float r1, float r2, float r3, uint2 (&out)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const f32x2 lo = {r0, r1}, hi = {r2, r3};
        if (F16) {
            const f16x2 blo = __builtin_convertvector(lo, f16x2), bhi = __builtin_convertvector(hi, f16x2);
            out[i].x = __builtin_bit_cast(unsigned, blo);
            out[i].y = __builtin_bit_cast(unsigned, bhi);
            if (i + 1 < P) {
                r0 = gn_resid_lo(out[i].x, r0); r1 = gn_resid_hi(out[i].x, r1); r2 = gn_resid_lo(out[i].y, r2); r3 = gn_resid_hi(out[i].y, r3);
            }
            continue;
        }
        const bf16x2 blo = __builtin_convertvector(lo, bf16x2), bhi = __builtin_convertvector(hi, bf16x2);
        out[i].x = __builtin_bit_cast(unsigned, blo);
        out[i].y = __builtin_bit_cast(unsigned, bhi);
        if (i + 1 < P) {
            r0 = __fsub_rn(r0, __uint_as_float(out[i].x << 16));
            r1 = __fsub_rn(r1, __uint_as_float(out[i].x & 0xffff0000u));
            r2 = __fsub_rn(r2, __uint_as_float(out[i].y << 16));
            r3 = __fsub_rn(r3, __uint_as_float(out[i].y & 0xffff0000u));
        }
    }
}
// the two-value, two-plane fp16 form (the decoder splits accumulator register pairs in place)
__device__ __forceinline__ void split2(float a, float b, unsigned &p1, unsigned &p2) {
    const f32x2 v = {a, b};
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    const f32x2 res = {gn_resid_lo(p1, a), gn_resid_hi(p1, b)};
    p2 = __builtin_bit_cast(unsigned, __builtin_convertvector(res, f16x2));
}

template <bool F16>
__device__ __forceinline__ f32x16 mfma16(const uint4 &a, const uint4 &b, const f32x16 &c) {
    if (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------------ global -> LDS DMA and wait counts
// 16 bytes per lane global -> LDS (m0 = LDS byte address of the wave's 1-KB destination, wave-uniform; lane i lands at + 16 i), issued from
// inline asm ON PURPOSE: hipcc (ROCm 7.2) guards every ds_read that follows a __builtin_amdgcn_global_load_lds with s_waitcnt vmcnt(0) (it
// cannot prove the read does not alias the DMA's LDS destination), which drains a multi-stage ring at every step.  Slot reuse is made safe by
// hand instead -- a counted s_waitcnt vmcnt(N) + s_barrier at the stage hand-over -- and a user must not use m0 otherwise.  Measured on the
// split decoder (262144 rows): 0.165 ms with the asm DMA, 0.201 ms with the builtin.
__device__ __forceinline__ void gn_glds16(const void *g, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_addr) : "memory");
}
// the same with a wave-uniform base in SGPRs and a 32-bit per-lane byte offset: no 64-bit VALU address arithmetic per piece
__device__ __forceinline__ void gn_glds16_s(const void *sbase, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
// a wave's four 1-KB pieces of one stage in one statement: ONE scalar base and ONE m0 value, the pieces told apart by the instruction's immediate
// offset -- which the hardware adds to the global AND to the LDS address (LLVM's llvm.amdgcn.global.load.lds: "imm offset (applied to both global
// and LDS address)"), and both step by 1024 from piece to piece.  Four statements with four bases made hipcc keep 72 address pairs in SGPRs across
// the split decoder's tile loop and spill them into VGPR lanes: 79 - 130 v_readlane_b32 per tile in the VALU stream of a VALU-issue-bound kernel.
__device__ __forceinline__ void gn_glds16x4_s(const void *sbase, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:3072" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
// (two pieces: the share of one of EIGHT waves in a 16-KB stage)
__device__ __forceinline__ void gn_glds16x2_s(const void *sbase, unsigned voff, unsigned lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:1024" ::"v"(voff), "s"(sbase), "s"(lds_addr) : "memory");
}
// s_waitcnt immediates (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] = 7 (no wait) | lgkmcnt[11:8] | vmcnt_hi[15:14])
#define GN_WAIT_VM_LGKM0(N) __builtin_amdgcn_s_waitcnt(((N) & 15) | 0x70 | (((N) >> 4) << 14))           // vmcnt(N) lgkmcnt(0)
#define GN_WAIT_VM_ONLY(N) __builtin_amdgcn_s_waitcnt(((N) & 15) | 0x70 | 0xF00 | (((N) >> 4) << 14))    // vmcnt(N) alone (lgkmcnt field = 15: no wait)
#define GN_WAIT_ALL() GN_WAIT_VM_LGKM0(0)                                                               // vmcnt(0) lgkmcnt(0)

// ------------------------------------------------------------------------------------------------ trilinear sampler
// F.grid_sample(mode='bilinear', padding_mode='border', align_corners=True) in ATen's operation order (grid_sampler_3d: unnormalise -> clip ->
// floor, weights as differences), pinned with __f*_rn: the forward kernels (decode.hip, decode_split.hip) and the backward (grad.hip) are
// compared bit for bit, so this is the ONLY place the arithmetic is written.
// source index of query coordinate q in [0, 1] on an axis of `size` voxels: qn = 2q - 1; ((qn + 1) / 2) (size - 1); clipped to [0, size - 1].
// *moving (the backward's mask, ATen's clip_coordinates_set_grad): 0 where the coordinate was clamped (x <= 0 or x >= size - 1), else 1.
__device__ __forceinline__ float gn_tri_src_index(float q, int size, float *moving = nullptr) {
    const float qn = __fsub_rn(__fmul_rn(2.0f, q), 1.0f);
    const float x = __fmul_rn(__fdiv_rn(__fadd_rn(qn, 1.0f), 2.0f), (float)(size - 1));
    if (moving) *moving = (x > 0.0f && x < (float)(size - 1)) ? 1.f : 0.f;
    return fminf((float)(size - 1), fmaxf(x, 0.0f));
}
// the cell of source index (ix, iy, iz): lower corner and, per axis, the weights of the lower ([0] = (x0 + 1) - x) and upper ([1] = x - x0) corner.
// Corner c = dx + 2 dy + 4 dz (ATen's order tnw, tne, tsw, tse, bnw, bne, bsw, bse) weighs (wx[dx] * wy[dy]) * wz[dz].
struct GnTriCell {
    int x0, y0, z0;
    float wx[2], wy[2], wz[2];
};
__device__ __forceinline__ GnTriCell gn_tri_cell(float ix, float iy, float iz) {
    GnTriCell t;
    const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
    t.x0 = (int)fx0; t.y0 = (int)fy0; t.z0 = (int)fz0;
    t.wx[1] = __fsub_rn(ix, fx0); t.wx[0] = __fsub_rn(__fadd_rn(fx0, 1.0f), ix);
    t.wy[1] = __fsub_rn(iy, fy0); t.wy[0] = __fsub_rn(__fadd_rn(fy0, 1.0f), iy);
    t.wz[1] = __fsub_rn(iz, fz0); t.wz[0] = __fsub_rn(__fadd_rn(fz0, 1.0f), iz);
    return t;
}
__device__ __forceinline__ float gn_tri_weight(const GnTriCell &t, int c) { return __fmul_rn(__fmul_rn(t.wx[c & 1], t.wy[(c >> 1) & 1]), t.wz[c >> 2]); }

// ------------------------------------------------------------------------------------------------ conv tile geometry
// the 3x3x3 convolutions (fp32: unet.hip, split-operand: unet_split.hip / unet_wino.hip, backward: unet_grad.hip) work on output tiles of
// 4 x 8 x 8 voxels (z, y, x) staged with a one-voxel halo
#define GN_CONV_TZ 4
#define GN_CONV_TY 8
#define GN_CONV_TX 8
#define GN_CONV_HZ (GN_CONV_TZ + 2)
#define GN_CONV_HY (GN_CONV_TY + 2)
#define GN_CONV_HX (GN_CONV_TX + 2)
#define GN_CONV_HVOX (GN_CONV_HZ * GN_CONV_HY * GN_CONV_HX)
#define GN_CONV_TVOX (GN_CONV_TZ * GN_CONV_TY * GN_CONV_TX)

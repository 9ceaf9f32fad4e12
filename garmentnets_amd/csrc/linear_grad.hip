// linear_grad.hip -- backward of the MLP blocks  r = relu(x W^T + b),  y = fadd(fmul(r, sc), sh)  (components/mlp.py: MLPStack, HipLinear; DESIGN.md
// "MLP gradients").  No float atomics: every sum has a fixed order that depends on the shapes alone, identical calls give identical bits.
//
//   gn_linear_act_bwd     the epilogue's backward, one pass over dy and the saved r: g = r > 0 ? dy * sc : 0 and three fp64 column sums
//   gn_linear_bwd_weight  dW[n][k] = sum_m g[m][n] x[m][k] on the fp32 matrix cores
//   gn_row_affine         y = fadd(fmul(r, sc[n]), sh[n]): gn_linear's BatchNorm epilogue as a kernel of its own (the differentiable forward keeps r)
//   (dX = g W is gn_linear on the transposed weight pack: no kernel here)
//   gn_col_moments / gn_col_dots / gn_bn_train_bwd   train-mode BatchNorm (batch statistics): fp64 column reductions of one shared kernel, at the end
//
// The weight gradient.  v_mfma_f32_32x32x2_f32 (linear.hip's instruction; exact fp32, a k-ordered fma chain): D(32x32) += A(32x2) B(2x32), operand A:
// lane l holds A[l&31][l>>5], operand B: lane l holds B[l>>5][l&31], D: lane l, reg r -> column l&31, row (r&3)+8*(r>>2)+4*(l>>5).  The reduction
// index is the ROW m of the two row-major operands, so lane l feeds g[m + (l>>5)][n0 + (l&31)] as A and x[m + (l>>5)][k0 + (l&31)] as B: each half-wave
// reads 32 consecutive floats of one staged row -- conflict-free ds_read_b32 at any row stride, no transposed tile -- and D is dW[n0 + row][k0 + column].
// Block = 256 threads = 4 waves; a workgroup owns a BN x BK block of dW (128 x 128, narrower for small N / K) and walks ONE chunk of
// GN_LINEAR_BWD_CHUNK_ROWS rows in 16-row stages (g and x row tiles through LDS, the next stage prefetched into registers, as linear_kernel does).
// Per element of dW the chunk is one fp32 fma chain over its rows in ascending order; the partial of chunk c goes to ws[c][N][K] with plain stores
// and a fold launch adds the chunks in fp64 and rounds once.
#include "common.h"

#define LG_R GN_LINEAR_BWD_CHUNK_ROWS
#define LG_RT 16                        /* rows per LDS stage */
#define LG_FOLD_RUNS 8                  /* the folds cut the chunks into 8 contiguous runs (a constant: the order must not depend on the device) */
#define LG_FOLD_OUTS (256 / LG_FOLD_RUNS)
static_assert(LG_R % LG_RT == 0, "a chunk is whole stages");

// ------------------------------------------------------------------------------------------------ the ordered fold of per-chunk partials
// part[chunks][total] -> the sum over the chunks of output o = 32 * block + (tid & 31), fp64.  Thread (run = tid >> 5) adds its contiguous run of
// ceil(chunks / 8) chunks in ascending order; run 0's thread then adds the eight run sums in ascending order and gets the result (the others get 0):
// ascending chunk order throughout, with that fixed association.  (One thread per output walking every chunk is the same sum 8 x slower: at 1.56 M rows
// x 64 x 64 there are 3047 chunks over 4096 outputs, 16 workgroups' worth of serial loads.)
template <class T>
__device__ __forceinline__ double lg_fold(const T *__restrict__ part, int chunks, int64_t total, int64_t o, double (*red)[LG_FOLD_OUTS]) {
    const int run = threadIdx.x / LG_FOLD_OUTS, per = (chunks + LG_FOLD_RUNS - 1) / LG_FOLD_RUNS;
    const int c0 = run * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    double s = 0.0;
    if (o < total) {
#pragma unroll 4
        for (int c = c0; c < c1; ++c) s += (double)part[(int64_t)c * total + o];
    }
    red[run][threadIdx.x % LG_FOLD_OUTS] = s;
    __syncthreads();
    if (run != 0) return 0.0;
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < LG_FOLD_RUNS; ++k) t += red[k][threadIdx.x];
    return t;
}

// ------------------------------------------------------------------------------------------------ epilogue backward
// grid (chunks of GN_LINEAR_ACT_CHUNK_ROWS rows, blocks of 64 columns); thread = (row group tid >> 6, column tid & 63): its rows m0 + group, + 4, ... in
// ascending order, fp64; the four groups added in ascending order through LDS: part[chunk][3][N].  The fold adds the chunks (lg_fold).
#define LA_ROWS GN_LINEAR_ACT_CHUNK_ROWS
#define LA_COLS 64
__global__ __launch_bounds__(256) void linear_act_bwd_kernel(const float *dy, int lddy, const float *__restrict__ r, int ldr, const float *__restrict__ sc,
                                                             int64_t M, int N, float *g, int ldg, double *__restrict__ part) {
    __shared__ double red[4][3][LA_COLS];
    const int col = threadIdx.x & (LA_COLS - 1), grp = threadIdx.x / LA_COLS, n = blockIdx.y * LA_COLS + col;
    const int64_t m0 = (int64_t)blockIdx.x * LA_ROWS;
    const int64_t m1 = m0 + LA_ROWS < M ? m0 + LA_ROWS : M;
    double s[3] = {0.0, 0.0, 0.0};
    if (n < N) {
        const float scv = sc ? sc[n] : 1.f;
#pragma unroll 4
        for (int64_t m = m0 + grp; m < m1; m += 4) {
            const float d = dy[m * lddy + n];
            float gv = __fmul_rn(d, scv);
            if (r) {
                const float rv = r[m * ldr + n];
                gv = rv > 0.f ? gv : 0.f;                        // gn_relu_mask's rule: a NaN in r takes no gradient
                s[2] += (double)d * (double)rv;                  // (exact: two 24-bit significands)
            }
            if (g) g[m * ldg + n] = gv;
            s[0] += (double)gv;
            s[1] += (double)d;
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) red[grp][j][col] = s[j];
    __syncthreads();
    if (grp == 0 && n < N) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            part[((int64_t)blockIdx.x * 3 + j) * N + n] = ((red[0][j][col] + red[1][j][col]) + red[2][j][col]) + red[3][j][col];
    }
}

__global__ __launch_bounds__(256) void linear_act_bwd_fold_kernel(const double *__restrict__ part, int chunks, int N, double *__restrict__ sums) {
    __shared__ double red[LG_FOLD_RUNS][LG_FOLD_OUTS];
    const int64_t total = 3 * (int64_t)N, o = (int64_t)blockIdx.x * LG_FOLD_OUTS + threadIdx.x % LG_FOLD_OUTS;
    const double t = lg_fold(part, chunks, total, o, red);
    if (threadIdx.x < LG_FOLD_OUTS && o < total) sums[o] = t;
}

extern "C" size_t gn_linear_act_bwd_workspace_bytes(int64_t M, int N) {
    if (M <= 0 || N <= 0) return 0;
    return (size_t)gn_cdiv(M, LA_ROWS) * 3 * (size_t)N * sizeof(double);
}

extern "C" int gn_linear_act_bwd(const float *dy, int lddy, const float *r, int ldr, const float *sc, int64_t M, int N, float *g, int ldg, void *ws,
                                 size_t ws_bytes, double *sums, void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && lddy >= N && (!r || ldr >= N) && (!g || ldg >= N), "gn_linear_act_bwd: bad sizes M=%lld N=%d (lddy=%d ldr=%d ldg=%d)",
               (long long)M, N, lddy, ldr, ldg);
    const size_t need = gn_linear_act_bwd_workspace_bytes(M, N);
    GN_REQUIRE(ws_bytes >= need, "gn_linear_act_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    GN_REQUIRE(sums != nullptr, "gn_linear_act_bwd: null pointer");
    GN_REQUIRE(g || (!r && !sc), "gn_linear_act_bwd: null pointer (g may be NULL only when there is neither a mask nor a scale: g is dy then)");
    hipStream_t st = gn_stream(stream);
    const int chunks = (int)gn_cdiv(M, LA_ROWS);
    if (chunks > 0) {
        GN_REQUIRE(dy && ws, "gn_linear_act_bwd: null pointer");
        hipLaunchKernelGGL(linear_act_bwd_kernel, dim3((unsigned)chunks, (unsigned)gn_cdiv(N, LA_COLS)), dim3(256), 0, st, dy, lddy, r, ldr, sc, M, N, g, ldg,
                           (double *)ws);
        GN_LAUNCH_CHECK("gn_linear_act_bwd");
    }
    hipLaunchKernelGGL(linear_act_bwd_fold_kernel, dim3((unsigned)gn_cdiv(3 * (int64_t)N, LG_FOLD_OUTS)), dim3(256), 0, st, (const double *)ws, chunks, N, sums);
    GN_LAUNCH_CHECK("gn_linear_act_bwd");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ weight gradient
template <int COLS>
struct RowTile {
    static constexpr int NV = (LG_RT * (COLS / 4) + 255) / 256;  // float4 per thread
    float4 v[NV];
};

// rows [row0, row0 + 16) x columns [c0, c0 + COLS) of the row-major P (ld) into registers; rows from row_end on and columns from C on are zeros and
// are not read (the float4 load is taken only where all four columns exist)
template <int COLS, bool ALIGNED>
__device__ __forceinline__ void row_tile_load(RowTile<COLS> &t, const float *__restrict__ P, int ld, int64_t row0, int64_t row_end, int c0, int C) {
#pragma unroll
    for (int i = 0; i < RowTile<COLS>::NV; ++i) {
        const int idx = threadIdx.x + i * 256;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < LG_RT * (COLS / 4)) {
            const int64_t row = row0 + idx / (COLS / 4);
            const int c = c0 + (idx % (COLS / 4)) * 4;
            if (row < row_end && c < C) {
                const float *p = P + row * ld + c;
                if (ALIGNED && c + 3 < C) {
                    v = *reinterpret_cast<const float4 *>(p);
                } else {
                    v.x = p[0];
                    if (c + 1 < C) v.y = p[1];
                    if (c + 2 < C) v.z = p[2];
                    if (c + 3 < C) v.w = p[3];
                }
            }
        }
        t.v[i] = v;
    }
}

template <int COLS>
__device__ __forceinline__ void row_tile_store(const RowTile<COLS> &t, float *__restrict__ lds) {
#pragma unroll
    for (int i = 0; i < RowTile<COLS>::NV; ++i) {
        const int idx = threadIdx.x + i * 256;
        if (idx < LG_RT * (COLS / 4)) *reinterpret_cast<float4 *>(lds + idx * 4) = t.v[i];      // row-major [16][COLS]: idx * 4 = row * COLS + column
    }
}

template <int WAVES_N, int WAVES_K, int TN, int TK, bool ALIGNED>
__global__ __launch_bounds__(256) void linear_bwd_weight_kernel(const float *__restrict__ G, int ldg, const float *__restrict__ X, int ldx, int64_t M, int N,
                                                                int K, float *__restrict__ part) {
    static_assert(WAVES_N * WAVES_K == 4, "4 waves per block");
    constexpr int BN = WAVES_N * TN * 32, BK = WAVES_K * TK * 32;
    __shared__ __attribute__((aligned(16))) float Gs[LG_RT * BN];
    __shared__ __attribute__((aligned(16))) float Xs[LG_RT * BK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wn = wave / WAVES_K, wk = wave % WAVES_K;
    const int64_t m0 = (int64_t)blockIdx.x * LG_R;
    const int64_t m1 = m0 + LG_R < M ? m0 + LG_R : M;
    const int n0 = blockIdx.y * BN, k0 = blockIdx.z * BK;

    f32x16 acc[TN][TK];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int u = 0; u < TK; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][u][r] = 0.f;

    RowTile<BN> rg;
    RowTile<BK> rx;
    row_tile_load<BN, ALIGNED>(rg, G, ldg, m0, m1, n0, N);
    row_tile_load<BK, ALIGNED>(rx, X, ldx, m0, m1, k0, K);
    row_tile_store<BN>(rg, Gs);
    row_tile_store<BK>(rx, Xs);
    __syncthreads();
    const int stages = (int)((m1 - m0 + LG_RT - 1) / LG_RT);
    const int aoff = (lane >> 5) * BN + wn * TN * 32 + (lane & 31);      // the half-wave's row of the pair, 32 consecutive floats
    const int boff = (lane >> 5) * BK + wk * TK * 32 + (lane & 31);
    for (int s = 0; s < stages; ++s) {
        if (s + 1 < stages) {
            row_tile_load<BN, ALIGNED>(rg, G, ldg, m0 + (int64_t)(s + 1) * LG_RT, m1, n0, N);
            row_tile_load<BK, ALIGNED>(rx, X, ldx, m0 + (int64_t)(s + 1) * LG_RT, m1, k0, K);
        }
#pragma unroll
        for (int pr = 0; pr < LG_RT / 2; ++pr) {
            float a[TN], b[TK];
#pragma unroll
            for (int t = 0; t < TN; ++t) a[t] = Gs[aoff + pr * 2 * BN + t * 32];
#pragma unroll
            for (int u = 0; u < TK; ++u) b[u] = Xs[boff + pr * 2 * BK + u * 32];
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int u = 0; u < TK; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
        __syncthreads();
        if (s + 1 < stages) {
            row_tile_store<BN>(rg, Gs);
            row_tile_store<BK>(rx, Xs);
        }
        __syncthreads();
    }
    float *__restrict__ po = part + (int64_t)blockIdx.x * N * K;
#pragma unroll
    for (int u = 0; u < TK; ++u) {
        const int k = k0 + (wk * TK + u) * 32 + (lane & 31);
        if (k >= K) continue;
#pragma unroll
        for (int t = 0; t < TN; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + (wn * TN + t) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < N) po[(int64_t)n * K + k] = acc[t][u][r];
            }
        }
    }
}

__global__ __launch_bounds__(256) void linear_bwd_weight_fold_kernel(const float *__restrict__ part, int chunks, int N, int K, float *__restrict__ dW, int lddw) {
    __shared__ double red[LG_FOLD_RUNS][LG_FOLD_OUTS];
    const int64_t total = (int64_t)N * K, o = (int64_t)blockIdx.x * LG_FOLD_OUTS + threadIdx.x % LG_FOLD_OUTS;
    const double t = lg_fold(part, chunks, total, o, red);
    if (threadIdx.x < LG_FOLD_OUTS && o < total) dW[(o / K) * lddw + o % K] = (float)t;
}

extern "C" size_t gn_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (size_t)gn_cdiv(M, LG_R) * (size_t)N * (size_t)K * sizeof(float);
}

extern "C" int gn_linear_bwd_weight(const float *g, int ldg, const float *x, int ldx, int64_t M, int N, int K, void *ws, size_t ws_bytes, float *dW, int lddw,
                                    void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && K > 0 && ldg >= N && ldx >= K && lddw >= K, "gn_linear_bwd_weight: bad sizes M=%lld N=%d K=%d (ldg=%d ldx=%d lddw=%d)",
               (long long)M, N, K, ldg, ldx, lddw);
    const size_t need = gn_linear_bwd_weight_workspace_bytes(M, N, K);
    GN_REQUIRE(ws_bytes >= need, "gn_linear_bwd_weight: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    GN_REQUIRE(dW != nullptr && (M == 0 || (g && x && ws)), "gn_linear_bwd_weight: null pointer");
    hipStream_t st = gn_stream(stream);
    const int64_t chunks = gn_cdiv(M, LG_R);
    GN_REQUIRE(chunks <= 0x7fffffff, "gn_linear_bwd_weight: bad sizes (too many row chunks)");
    if (chunks > 0) {
        const bool aligned = (ldg % 4 == 0) && (ldx % 4 == 0) && (((uintptr_t)g | (uintptr_t)x) % 16 == 0);
#define LG_LAUNCH(WN, WK, TN, TK)                                                                                                                   \
    do {                                                                                                                                            \
        constexpr int BN = WN * TN * 32, BK = WK * TK * 32;                                                                                         \
        dim3 grid((unsigned)chunks, (unsigned)gn_cdiv(N, BN), (unsigned)gn_cdiv(K, BK));                                                            \
        GN_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "gn_linear_bwd_weight: bad sizes (N=%d K=%d: too many blocks)", N, K);                       \
        if (aligned) hipLaunchKernelGGL((linear_bwd_weight_kernel<WN, WK, TN, TK, true>), grid, dim3(256), 0, st, g, ldg, x, ldx, M, N, K, (float *)ws); \
        else hipLaunchKernelGGL((linear_bwd_weight_kernel<WN, WK, TN, TK, false>), grid, dim3(256), 0, st, g, ldg, x, ldx, M, N, K, (float *)ws);   \
    } while (0)
        if (N <= 32) LG_LAUNCH(1, 4, 1, 1);                      // 32 x 128: the decoder heads (N = 1, 3)
        else if (K <= 32) LG_LAUNCH(4, 1, 1, 1);                 // 128 x 32
        else if (N <= 64 || K <= 64) LG_LAUNCH(2, 2, 1, 1);      // 64 x 64: the first set abstraction
        else LG_LAUNCH(2, 2, 2, 2);                              // 128 x 128
#undef LG_LAUNCH
        GN_LAUNCH_CHECK("gn_linear_bwd_weight");
    }
    hipLaunchKernelGGL(linear_bwd_weight_fold_kernel, dim3((unsigned)gn_cdiv((int64_t)N * K, LG_FOLD_OUTS)), dim3(256), 0, st, (const float *)ws, (int)chunks, N,
                       K, dW, lddw);
    GN_LAUNCH_CHECK("gn_linear_bwd_weight");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ row affine
__global__ __launch_bounds__(256) void row_affine_kernel(const float *r, int ldr, const float *__restrict__ sc, const float *__restrict__ sh, int64_t M, int N,
                                                         float *y, int ldy) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * N) return;
    const int64_t m = i / N;
    const int n = (int)(i % N);
    y[m * ldy + n] = __fadd_rn(__fmul_rn(r[m * ldr + n], sc[n]), sh[n]);      // gn_linear's epilogue: fmul then fadd, not an fma
}

extern "C" int gn_row_affine(const float *r, int ldr, const float *sc, const float *sh, int64_t M, int N, float *y, int ldy, void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && ldr >= N && ldy >= N && M <= ((int64_t)1 << 39) / N, "gn_row_affine: bad sizes M=%lld N=%d (ldr=%d ldy=%d)", (long long)M, N,
               ldr, ldy);
    if (M == 0) return GN_OK;
    GN_REQUIRE(r && sc && sh && y, "gn_row_affine: null pointer");
    hipLaunchKernelGGL(row_affine_kernel, dim3((unsigned)gn_cdiv(M * N, 256)), dim3(256), 0, gn_stream(stream), r, ldr, sc, sh, M, N, y, ldy);
    GN_LAUNCH_CHECK("gn_row_affine");
    return GN_OK;
}

// ------------------------------------------------------------------------------------------------ train-mode BatchNorm: column reductions
// y = (r - mean) * inv * gamma + beta with the batch's own mean and biased variance over the M rows (DESIGN.md "Train-mode BatchNorm").  One kernel, four
// per-element terms: each adds J fp64 values per (row, column) and folds them like linear_act_bwd_kernel -- chunks of GN_LINEAR_ACT_CHUNK_ROWS rows, then
// lg_fold over the chunks.  Thread map: cw = the power of two >= N, at most 64, columns per workgroup (thread = (row group tid / cw, column tid % cw)), so
// a wave reads 64 / cw whole rows of a narrow matrix (the decoder head's N = 1: 64 consecutive rows) and 64 consecutive columns of a wide one.  A thread
// adds its rows m0 + group, + 256 / cw, ... in ascending order; the 256 / cw groups are then added by a halving tree through LDS (group p += group p + h,
// h = groups / 2 ... 1): an order that depends on (M, N) alone.
enum { CS_SUM, CS_M2, CS_DOTS, CS_BN };
//   CS_SUM   a          -> sum a                                                      (the mean's numerator; converting a float is exact)
//   CS_M2    a, p[n]    -> sum (a - p[n])^2                                           (p: the column mean)
//   CS_DOTS  a, b       -> sum a, sum a * b                                           (products of two 24-bit significands: exact)
//   CS_BN    a, b, p    -> g = b > 0 ? (float)(p[0][n] a + p[1][n] b + p[2][n]) : 0, sum g   (a = dy, b = r; g may be a: each element is read, then written, by one thread)
template <int T>
__global__ __launch_bounds__(256) void col_sums_kernel(const float *a, int lda, const float *__restrict__ b, int ldb, const double *__restrict__ p, int64_t M,
                                                       int N, int cw, float *g, int ldg, double *__restrict__ part) {
    constexpr int J = T == CS_DOTS ? 2 : 1;
    __shared__ double red[J][256];
    const int col = threadIdx.x & (cw - 1), grp = threadIdx.x / cw, groups = 256 / cw, n = blockIdx.y * cw + col;
    const int64_t m0 = (int64_t)blockIdx.x * LA_ROWS;
    const int64_t m1 = m0 + LA_ROWS < M ? m0 + LA_ROWS : M;
    double s[J] = {};
    if (n < N) {
        const double p0 = T == CS_M2 || T == CS_BN ? p[n] : 0.0, p1 = T == CS_BN ? p[N + n] : 0.0, p2 = T == CS_BN ? p[2 * (int64_t)N + n] : 0.0;
#pragma unroll 4
        for (int64_t m = m0 + grp; m < m1; m += groups) {
            const float av = a[m * lda + n];
            if (T == CS_SUM) {
                s[0] += (double)av;
            } else if (T == CS_M2) {
                const double d = (double)av - p0;
                s[0] += d * d;
            } else {
                const float bv = b[m * ldb + n];
                if (T == CS_DOTS) {
                    s[0] += (double)av;
                    s[J - 1] += (double)av * (double)bv;
                } else {
                    const float gv = bv > 0.f ? (float)((p0 * (double)av + p1 * (double)bv) + p2) : 0.f;      // gn_relu_mask's rule: a NaN in r takes no gradient
                    g[m * ldg + n] = gv;
                    s[0] += (double)gv;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) red[j][threadIdx.x] = s[j];
    __syncthreads();
    for (int h = groups >> 1; h >= 1; h >>= 1) {
        if (grp < h) {
#pragma unroll
            for (int j = 0; j < J; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + h * cw];
        }
        __syncthreads();
    }
    if (grp == 0 && n < N) {
#pragma unroll
        for (int j = 0; j < J; ++j) part[((int64_t)blockIdx.x * J + j) * N + n] = red[j][col];
    }
}

// sums[o] = (the chunks of part[chunks][total] in lg_fold's order) / div
__global__ __launch_bounds__(256) void col_sums_fold_kernel(const double *__restrict__ part, int chunks, int64_t total, double div, double *__restrict__ sums) {
    __shared__ double red[LG_FOLD_RUNS][LG_FOLD_OUTS];
    const int64_t o = (int64_t)blockIdx.x * LG_FOLD_OUTS + threadIdx.x % LG_FOLD_OUTS;
    const double t = lg_fold(part, chunks, total, o, red);
    if (threadIdx.x < LG_FOLD_OUTS && o < total) sums[o] = t / div;
}

static size_t col_sums_bytes(int64_t M, int N, int J) { return M <= 0 || N <= 0 ? 0 : (size_t)gn_cdiv(M, LA_ROWS) * J * (size_t)N * sizeof(double); }

// one reduction: the chunk launch (none when M == 0) and the fold of its J * N outputs
template <int T>
static int col_sums_run(const char *who, const float *a, int lda, const float *b, int ldb, const double *p, int64_t M, int N, float *g, int ldg, double *ws,
                        double div, double *sums, hipStream_t st) {
    constexpr int J = T == CS_DOTS ? 2 : 1;
    const int chunks = (int)gn_cdiv(M, LA_ROWS);
    int cw = LA_COLS;
    while (cw / 2 >= N) cw /= 2;
    if (chunks > 0) {
        hipLaunchKernelGGL(col_sums_kernel<T>, dim3((unsigned)chunks, (unsigned)gn_cdiv(N, cw)), dim3(256), 0, st, a, lda, b, ldb, p, M, N, cw, g, ldg, ws);
        GN_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(col_sums_fold_kernel, dim3((unsigned)gn_cdiv(J * (int64_t)N, LG_FOLD_OUTS)), dim3(256), 0, st, (const double *)ws, chunks, J * (int64_t)N,
                       div, sums);
    GN_LAUNCH_CHECK(who);
    return GN_OK;
}

// what the three entries refuse alike: the grid is (chunks, ceil(N / 64)) at most
#define CS_GRID_OK(M, N) (gn_cdiv(M, LA_ROWS) <= 0x7fffffff && gn_cdiv(N, LA_COLS) <= 65535)

extern "C" size_t gn_col_moments_workspace_bytes(int64_t M, int N) { return col_sums_bytes(M, N, 1); }

extern "C" int gn_col_moments(const float *r, int ldr, int64_t M, int N, void *ws, size_t ws_bytes, double *moments, void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && ldr >= N && CS_GRID_OK(M, N), "gn_col_moments: bad sizes M=%lld N=%d (ldr=%d)", (long long)M, N, ldr);
    const size_t need = gn_col_moments_workspace_bytes(M, N);
    GN_REQUIRE(ws_bytes >= need, "gn_col_moments: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    GN_REQUIRE(moments != nullptr && (M == 0 || (r && ws)), "gn_col_moments: null pointer");
    hipStream_t st = gn_stream(stream);
    // two passes: the mean first, then the squares of the differences from it (the second launch reads the first fold's result: stream order)
    const int rc = col_sums_run<CS_SUM>("gn_col_moments", r, ldr, nullptr, 0, nullptr, M, N, nullptr, 0, (double *)ws, M > 0 ? (double)M : 1.0, moments, st);
    if (rc != GN_OK) return rc;
    return col_sums_run<CS_M2>("gn_col_moments", r, ldr, nullptr, 0, moments, M, N, nullptr, 0, (double *)ws, 1.0, moments + N, st);
}

extern "C" size_t gn_col_dots_workspace_bytes(int64_t M, int N) { return col_sums_bytes(M, N, 2); }

extern "C" int gn_col_dots(const float *dy, int lddy, const float *r, int ldr, int64_t M, int N, void *ws, size_t ws_bytes, double *dots, void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && lddy >= N && ldr >= N && CS_GRID_OK(M, N), "gn_col_dots: bad sizes M=%lld N=%d (lddy=%d ldr=%d)", (long long)M, N, lddy, ldr);
    const size_t need = gn_col_dots_workspace_bytes(M, N);
    GN_REQUIRE(ws_bytes >= need, "gn_col_dots: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    GN_REQUIRE(dots != nullptr && (M == 0 || (dy && r && ws)), "gn_col_dots: null pointer");
    return col_sums_run<CS_DOTS>("gn_col_dots", dy, lddy, r, ldr, nullptr, M, N, nullptr, 0, (double *)ws, 1.0, dots, gn_stream(stream));
}

extern "C" size_t gn_bn_train_bwd_workspace_bytes(int64_t M, int N) { return col_sums_bytes(M, N, 1); }

extern "C" int gn_bn_train_bwd(const float *dy, int lddy, const float *r, int ldr, const double *coef, int64_t M, int N, float *g, int ldg, void *ws,
                               size_t ws_bytes, double *sum_g, void *stream) {
    GN_REQUIRE(M >= 0 && N > 0 && lddy >= N && ldr >= N && ldg >= N && CS_GRID_OK(M, N), "gn_bn_train_bwd: bad sizes M=%lld N=%d (lddy=%d ldr=%d ldg=%d)",
               (long long)M, N, lddy, ldr, ldg);
    const size_t need = gn_bn_train_bwd_workspace_bytes(M, N);
    GN_REQUIRE(ws_bytes >= need, "gn_bn_train_bwd: workspace too small (%zu < %zu bytes)", ws_bytes, need);
    GN_REQUIRE(sum_g != nullptr && (M == 0 || (dy && r && coef && g && ws)), "gn_bn_train_bwd: null pointer");
    return col_sums_run<CS_BN>("gn_bn_train_bwd", dy, lddy, r, ldr, coef, M, N, g, ldg, (double *)ws, 1.0, sum_g, gn_stream(stream));
}

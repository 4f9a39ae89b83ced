// The 128 x 128 f64 output tile of one workgroup of 4 waves on the matrix cores (k_gram of kgram.hip, k_chol_tile of chol.hip):
// 64 x 64 per wave as 4 x 4 v_mfma_f64_16x16x4_f64 tiles; both operands go through LDS in chunks of 16 k-columns, double-buffered
// (the next chunk is loaded into registers while the current one is multiplied, one barrier per chunk).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

typedef double t128_v2d __attribute__((ext_vector_type(2)));
typedef double t128_v4d __attribute__((ext_vector_type(4)));

#define T128_T 128     // output tile edge
#define T128_KB 16     // k-columns per staged chunk
#define T128_LD 144    // LDS row stride (doubles): 128 + 16 (consecutive k-rows 32 banks apart, as k_syrk)
constexpr size_t T128_LDS_BYTES = sizeof(double) * 4 * T128_KB * T128_LD;   // 73 728 B: two workgroups per CU

// linear index b of a tile of a triangle -> (lo <= hi): hi (hi + 1) / 2 <= b < (hi + 1)(hi + 2) / 2
__device__ __forceinline__ void t128_tri(int64_t b, int64_t &lo, int64_t &hi)
{
    int64_t t = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > b) --t;
    while ((t + 1) * (t + 2) / 2 <= b) ++t;
    hi = t; lo = b - t * (t + 1) / 2;
}

// acc = sum over nch chunks of A B', A the operand along the MFMA's rows (j), B the one along its columns (i, the contiguous direction
// of the output): acc[mj][ni][reg] belongs to j = 64 qj + 16 mj + (lane >> 4) + 4 reg, i = 64 qi + 16 ni + (lane & 15) of the tile,
// qj = wave >> 1, qi = wave & 1.  lda(k, c) / ldb(k, c): rows c, c + 1 of the tile's k-column k of the operand (c = 2 lane).
// lds: 4 * T128_KB * T128_LD doubles, 16-byte aligned.  Ends behind a barrier: the caller may reuse lds at once.
template <class LA, class LB>
__device__ __forceinline__ void t128_mma(double *lds, int nch, LA lda, LB ldb, t128_v4d (&acc)[4][4])
{
    double *As = lds;                                // [2][T128_KB][T128_LD]
    double *Bs = lds + 2 * T128_KB * T128_LD;        // [2][T128_KB][T128_LD]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int qj = wv >> 1, qi = wv & 1;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = t128_v4d{0.0, 0.0, 0.0, 0.0};
    t128_v2d va[4], vb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int k = k0 + wv * 4 + it;
            va[it] = lda(k, 2 * lane);
            vb[it] = ldb(k, 2 * lane);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = wv * 4 + it;
            *reinterpret_cast<t128_v2d *>(As + (buf * T128_KB + row) * T128_LD + 2 * lane) = va[it];
            *reinterpret_cast<t128_v2d *>(Bs + (buf * T128_KB + row) * T128_LD + 2 * lane) = vb[it];
        }
    };
    load(0);
    stage(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) load((ch + 1) * T128_KB);
        const double *A = As + buf * T128_KB * T128_LD, *B = Bs + buf * T128_KB * T128_LD;
#pragma unroll
        for (int kk = 0; kk < T128_KB / 4; ++kk) {
            const int krow = 4 * kk + (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = A[krow * T128_LD + 64 * qj + 16 * u + (lane & 15)];
                b[u] = B[krow * T128_LD + 64 * qi + 16 * u + (lane & 15)];
            }
#pragma unroll
            for (int mj = 0; mj < 4; ++mj)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mj][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mj], b[ni], acc[mj][ni], 0, 0, 0);
        }
        if (ch + 1 < nch) stage(buf ^ 1);
        __syncthreads();
    }
}

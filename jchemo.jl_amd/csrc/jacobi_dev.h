// Parallel cyclic Jacobi eigensolver of one workgroup (NTH threads) on a small symmetric matrix: shared by the small-state
// kernels (smallstate.hip) and the kpca Rayleigh-Ritz / orthonormalisation kernels (kpca.hip).
#pragma once
#include "jch_internal.h"
// Parallel cyclic Jacobi on the symmetric q x q matrix in A0 (LDS, ld = lda).  On return the eigenvalues are
// on the diagonal of the returned buffer and V holds the eigenvectors (columns).  Two syncs per round.
template <int NTH = 256>
__device__ static void jacobi_eig(int q, int lda, double *&A0, double *&A1, double *&V0, double *&V1, double *cs,
                                  int *partner, int *flag)
{
    const int m = (q + 1) & ~1;  // even number of players; index q (if odd) is a bye
    const int tid = threadIdx.x;
    for (int e = tid; e < q * q; e += NTH) {
        const int i = e / q, j = e % q;
        V0[i * lda + j] = (i == j) ? 1.0 : 0.0;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        for (int round = 0; round < m - 1; ++round) {
            // ---- step 1: one thread per pair computes its rotation
            if (tid < m / 2) {
                int a, b;
                if (tid == 0) { a = m - 1; b = round; }
                else { a = (round + tid) % (m - 1); b = (round - tid + (m - 1)) % (m - 1); }
                if (a > b) { const int t = a; a = b; b = t; }
                double c = 1.0, s = 0.0;
                if (b < q) {
                    const double app = A0[a * lda + a], aqq = A0[b * lda + b], apq = A0[a * lda + b];
                    if (fabs(apq) > 1e-290 && fabs(apq) > 1e-17 * sqrt(fabs(app * aqq))) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        *flag = 1;  // benign race: any rotation this sweep sets it
                    }
                    partner[a] = b; partner[b] = a;
                    // role: +1 for the lower index (p), -1 for the higher (q)
                    cs[2 * a] = c; cs[2 * a + 1] = s;
                    cs[2 * b] = c; cs[2 * b + 1] = -s;
                } else if (a < q) {  // bye
                    partner[a] = a;
                    cs[2 * a] = 1.0; cs[2 * a + 1] = 0.0;
                }
            }
            __syncthreads();
            // ---- step 2: A1 = J' A0 J, V1 = V0 J   (for index i with partner i': Jcol_i = c e_i + s_i e_i',
            //      with s_i = +s for the lower index (new_p = c*x_p - s*x_q) -> encoded so that
            //      new_i = c * x_i - sgn * s * x_partner, sgn carried in cs[2i+1])
            for (int e = tid; e < q * q; e += NTH) {
                const int i = e / q, j = e % q;
                const int ip = partner[i], jp = partner[j];
                const double ci = cs[2 * i], si = cs[2 * i + 1], cj = cs[2 * j], sj = cs[2 * j + 1];
                // row op on rows (i, ip) evaluated at columns j and jp
                const double rij = ci * A0[i * lda + j] - si * A0[ip * lda + j];
                const double rijp = ci * A0[i * lda + jp] - si * A0[ip * lda + jp];
                A1[i * lda + j] = cj * rij - sj * rijp;
                V1[i * lda + j] = cj * V0[i * lda + j] - sj * V0[i * lda + jp];
            }
            __syncthreads();
            double *t = A0; A0 = A1; A1 = t;
            t = V0; V0 = V1; V1 = t;
        }
        const int any = *flag;
        __syncthreads();
        if (tid == 0) *flag = 0;
        __syncthreads();
        if (!any) break;
    }
}

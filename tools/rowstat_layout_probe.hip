// Standalone probe for jch_rows_standardize: how many rows should a wave hold?  The row statistics need each row
// two or three times; one thread per row (64 rows x p x 8 B per wave) keeps 2 GB in flight chip-wide at p = 500, far beyond the
// 256 MiB Infinity Cache, so every pass comes from HBM.  R rows x C column phases per wave (R * C = 64; runs of 8 R bytes per
// column, the statistics finished by log2(C) __shfl_xor) hold C times fewer rows; dynamic LDS that nothing uses limits the
// workgroups per CU further (20 / 40 / 64 KiB: at most 8 / 4 / 2 of 256 threads).  In place on n x p doubles (default 1e6 x 500),
// refilled before every launch, medians of 5 after a warm-up, next to a same-size device-to-device copy.
// hipcc --offload-arch=gfx950 -O3 tools/rowstat_layout_probe.hip -o tools/rowstat_layout_probe && tools/rowstat_layout_probe [n p]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
#define U 8

__global__ void k_fill(double *X, int64_t n, int64_t p)
{
    const int64_t tot = n * p;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e % n, j = e / n;
        uint64_t h = (uint64_t)e * 0x9E3779B97F4A7C15ull; h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        X[e] = (double)(h >> 11) * (1.0 / 9007199254740992.0) + 50.0 * (double)(i % 7) + 0.001 * (double)j;
    }
}

__global__ __launch_bounds__(256) void k_simple(const double *X, int64_t n, int64_t p, int64_t ldx, double *out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *x = X + i; double *o = out + i;
    double s = 0.0;
#pragma unroll U
    for (int64_t j = 0; j < p; ++j) s += x[j * ldx];
    const double mean = s / (double)p;
    double ss = 0.0;
#pragma unroll U
    for (int64_t j = 0; j < p; ++j) { const double d = x[j * ldx] - mean; ss += d * d; }
    const double sd = sqrt(ss / (double)p);
#pragma unroll U
    for (int64_t j = 0; j < p; ++j) o[j * ldo] = (x[j * ldx] - mean) / sd;
}

// R rows x C phases per wave, R * C == 64; a block of NT threads
template <int R, int C, int NT>
__global__ __launch_bounds__(NT) void k_narrow(const double *X, int64_t n, int64_t p, int64_t ldx, double *out, int64_t ldo)
{
    extern __shared__ double pad_[];   // occupancy limiter only
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane % R, c = lane / R;
    int64_t i = ((int64_t)blockIdx.x * (NT / 64) + w) * R + r;
    const bool live = i < n;
    if (!live) i = n - 1;
    const double *x = X + i + (int64_t)c * ldx; double *o = out + i + (int64_t)c * ldo;
    const int64_t cnt = (p - c + C - 1) / C;   // columns c, c + C, ...
    const int64_t sx = ldx * C, so = ldo * C;
    double s = 0.0;
#pragma unroll U
    for (int64_t t = 0; t < cnt; ++t) s += x[t * sx];
#pragma unroll
    for (int m = R; m < 64; m <<= 1) s += __shfl_xor(s, m);
    const double mean = s / (double)p;
    double ss = 0.0;
#pragma unroll U
    for (int64_t t = 0; t < cnt; ++t) { const double d = x[t * sx] - mean; ss += d * d; }
#pragma unroll
    for (int m = R; m < 64; m <<= 1) ss += __shfl_xor(ss, m);
    const double sd = sqrt(ss / (double)p);
    if (!live) return;
#pragma unroll U
    for (int64_t t = 0; t < cnt; ++t) o[t * so] = (x[t * sx] - mean) / sd;
}

static float med(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? atoll(argv[1]) : 1000000, p = argc > 2 ? atoll(argv[2]) : 500;
    double *X, *B, *Ref;
    CK(hipMalloc(&X, sizeof(double) * n * p)); CK(hipMalloc(&B, sizeof(double) * n * p)); CK(hipMalloc(&Ref, sizeof(double) * n * p));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipStream_t st = 0;
    auto timeit = [&](const char *name, auto fn, bool keepref, bool cmp) {
        std::vector<float> ts;
        for (int it = 0; it < 6; ++it) {
            k_fill<<<4096, 256, 0, st>>>(X, n, p);
            CK(hipEventRecord(e0, st)); fn(); CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1)); if (it) ts.push_back(ms);
        }
        const float m = med(ts);
        printf("%-28s n=%lld p=%lld  %.3f ms  %.2f TB/s (2np8)\n", name, (long long)n, (long long)p, m, 2.0 * n * p * 8 / (m * 1e-3) / 1e12);
        if (keepref) CK(hipMemcpy(Ref, X, sizeof(double) * n * p, hipMemcpyDeviceToDevice));
        if (cmp) {   // compare a sample with the simple kernel's result
            const int64_t cnt = std::min<int64_t>(n * p, 1 << 22);
            std::vector<double> a(cnt), b(cnt);
            CK(hipMemcpy(a.data(), X + (n * p - cnt), sizeof(double) * cnt, hipMemcpyDeviceToHost));
            CK(hipMemcpy(b.data(), Ref + (n * p - cnt), sizeof(double) * cnt, hipMemcpyDeviceToHost));
            double mx = 0; for (int64_t k = 0; k < cnt; ++k) mx = std::max(mx, fabs(a[k] - b[k]));
            printf("    max |diff to simple| over the last %lld elements: %.3e\n", (long long)cnt, mx);
        }
        fflush(stdout);
    };
    timeit("copy d2d", [&] { CK(hipMemcpyAsync(B, X, sizeof(double) * n * p, hipMemcpyDeviceToDevice, st)); }, false, false);
    timeit("simple 256", [&] { k_simple<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(X, n, p, n, X, n); }, true, false);
    const size_t lds[] = {0, 20 << 10, 40 << 10, 64 << 10};   // blocks per CU limited to all / 8 / 4 / 2 (160 KiB of LDS)
    for (size_t l : lds) {
        char nm[64];
        snprintf(nm, sizeof nm, "narrow 16x4 nt256 lds%zuK", l >> 10);
        if (l > (48 << 10)) CK(hipFuncSetAttribute((const void *)k_narrow<16, 4, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l));
        timeit(nm, [&] { k_narrow<16, 4, 256><<<(unsigned)((n + 63) / 64), 256, l, st>>>(X, n, p, n, X, n); }, false, true);
    }
    for (size_t l : lds) {
        char nm[64];
        snprintf(nm, sizeof nm, "narrow 32x2 nt256 lds%zuK", l >> 10);
        if (l > (48 << 10)) CK(hipFuncSetAttribute((const void *)k_narrow<32, 2, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l));
        timeit(nm, [&] { k_narrow<32, 2, 256><<<(unsigned)((n + 127) / 128), 256, l, st>>>(X, n, p, n, X, n); }, false, true);
    }
    for (size_t l : lds) {
        char nm[64];
        snprintf(nm, sizeof nm, "narrow 8x8 nt256 lds%zuK", l >> 10);
        if (l > (48 << 10)) CK(hipFuncSetAttribute((const void *)k_narrow<8, 8, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l));
        timeit(nm, [&] { k_narrow<8, 8, 256><<<(unsigned)((n + 31) / 32), 256, l, st>>>(X, n, p, n, X, n); }, false, true);
    }
    timeit("copy d2d (again)", [&] { CK(hipMemcpyAsync(B, X, sizeof(double) * n * p, hipMemcpyDeviceToDevice, st)); }, false, false);
    return 0;
}

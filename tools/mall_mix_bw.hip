// Standalone probe: can a FIXED slice of a streamed buffer stay resident in the 256 MiB Infinity Cache from launch to launch
// when the slice is read with default-policy loads and everything else with non-temporal ones?  ("resident slice")
// hipcc --offload-arch=gfx950 -O3 tools/mall_mix_bw.hip -o tools/mall_mix_bw && tools/mall_mix_bw
//
// Access shape of k_sweep_v2: wave w of W = 4 * blocks waves reads the 32 KB groups w, w + W, w + 2W, ... with 16-byte loads, two
// groups in flight.  A set of waves spread evenly over the global wave index (hence over blocks and XCDs) reads its groups with plain
// loads, every other wave with __builtin_nontemporal_load; the set is sized so that its groups make up S MiB.  25 launches back to
// back per setting, each between its own pair of events; launch 1 is reported apart from launches 2-25.  The cache is flushed (a
// 512 MiB memset) before every setting.  `st=1`: every wave also stores 64 B per group (the sweep's T column: 8 MB per launch at 4 GiB).
//
// `tools/mall_mix_bw tstage` ("T column through LDS"): only the store modes, 4 GiB, 208 blocks, S = 0 and 128 MiB —
// st=0 read-only, st=1 the direct store, st=2 each wave writes its 64 B per group into a wave-private LDS ring of CH groups and
// writes the ring out with ordinary 64-lane global stores when it is full and at the end of the kernel (CH = 8, 32, 64, and
// "never full": one flush per wave), st=3 the direct store as a non-temporal store.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
typedef double v2f64 __attribute__((ext_vector_type(2)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int GV = 32;   // 16-byte loads per lane and group: 64 lanes * 16 B * 32 = 32 KB

// wave w is resident iff floor((w + 1) nres / W) > floor(w nres / W): nres waves, evenly spaced
__device__ __forceinline__ bool is_resident(int64_t w, int64_t nres, int64_t W) { return ((w + 1) * nres) / W > (w * nres) / W; }

template <int ST>   // 0: no store, 1: direct store, 2: LDS ring of `ch` groups per wave, 3: direct non-temporal store
__global__ __launch_bounds__(256) void k_mix(const v2f64 *__restrict__ x, int64_t ngroups, int nres, double *__restrict__ tcol, double *out, int ch)
{
    extern __shared__ double ring_all[];   // ST == 2: [4][ch][8]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t W = (int64_t)gridDim.x * 4, w = (int64_t)blockIdx.x * 4 + wv;
    double acc = 0.0;
    double *ring = ring_all + (ST == 2 ? __builtin_amdgcn_readfirstlane(wv) * ch * 8 : 0);
    int fill = 0;
    int64_t done = 0;
    auto flush = [&] {   // lane l: slot s + l / 8, row l % 8 of the group the wave read in iteration done + slot
        const int nf = __builtin_amdgcn_readfirstlane(fill);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int s = 0; s < nf; s += 8) {
            const int slot = s + lane / 8;
            if (slot < nf) tcol[(w + (done + slot) * W) * 8 + lane % 8] = ring[s * 8 + lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        done += nf;
        fill = 0;
    };
    auto body = [&](auto nt) {
        constexpr bool NT = decltype(nt)::value;
        v2f64 a[GV], b[GV];
        auto fetch = [&](v2f64 (&v)[GV], int64_t g) {
            const v2f64 *p = x + (size_t)g * (GV * 64) + lane;
#pragma unroll
            for (int u = 0; u < GV; ++u) v[u] = NT ? __builtin_nontemporal_load(p + 64 * u) : p[64 * u];
        };
        auto use = [&](v2f64 (&v)[GV], int64_t g) {
#pragma unroll
            for (int u = 0; u < GV; ++u) acc += v[u].x + v[u].y;
            if (ST == 1 && lane < 8) tcol[g * 8 + lane] = acc;
            if (ST == 3 && lane < 8) __builtin_nontemporal_store(acc, tcol + g * 8 + lane);
            if (ST == 2) {
                if (lane < 8) ring[fill * 8 + lane] = acc;
                if (__builtin_amdgcn_readfirstlane(++fill) == ch) flush();
            }
        };
        int64_t g = w;
        if (g < ngroups) fetch(a, g);
        while (g < ngroups) {
            if (g + W < ngroups) fetch(b, g + W);
            use(a, g);
            g += W;
            if (g < ngroups) {
                if (g + W < ngroups) fetch(a, g + W);
                use(b, g);
                g += W;
            }
        }
    };
    if (is_resident(w, nres, W)) body(std::false_type{});   // wave-uniform, fixed for the launch
    else body(std::true_type{});
    if (ST == 2) flush();
    if (acc == 123.456) out[0] = acc;
}

struct Stat { float first, mean, mn, mx; };

static Stat run(const v2f64 *x, size_t bytes, int blocks, int nres, int st, double *tcol, double *out, void *flush, size_t flush_bytes, int ch = 0)
{
    static hipEvent_t ev[26];
    static bool init = false;
    if (!init) { for (auto &e : ev) CK(hipEventCreate(&e)); init = true; }
    const int64_t ngroups = (int64_t)(bytes / (GV * 64 * 16));
    CK(hipMemsetAsync(flush, 1, flush_bytes, 0));
    CK(hipEventRecord(ev[0], 0));
    for (int l = 0; l < 25; ++l) {
        const size_t lds = st == 2 ? sizeof(double) * 4 * ch * 8 : 0;   // (at most 4 x 158 groups x 64 B = 40 KB here)
        if (st == 1) hipLaunchKernelGGL(k_mix<1>, dim3(blocks), dim3(256), 0, 0, x, ngroups, nres, tcol, out, 0);
        else if (st == 2) hipLaunchKernelGGL(k_mix<2>, dim3(blocks), dim3(256), lds, 0, x, ngroups, nres, tcol, out, ch);
        else if (st == 3) hipLaunchKernelGGL(k_mix<3>, dim3(blocks), dim3(256), 0, 0, x, ngroups, nres, tcol, out, 0);
        else hipLaunchKernelGGL(k_mix<0>, dim3(blocks), dim3(256), 0, 0, x, ngroups, nres, tcol, out, 0);
        CK(hipEventRecord(ev[l + 1], 0));
    }
    CK(hipEventSynchronize(ev[25]));
    CK(hipGetLastError());
    Stat s{0, 0, 1e30f, 0};
    for (int l = 0; l < 25; ++l) {
        float ms; CK(hipEventElapsedTime(&ms, ev[l], ev[l + 1]));
        if (l == 0) { s.first = ms; continue; }
        s.mean += ms / 24; s.mn = std::min(s.mn, ms); s.mx = std::max(s.mx, ms);
    }
    return s;
}

int main(int argc, char **argv)
{
    const bool tstage = argc > 1 && !strcmp(argv[1], "tstage");
    const size_t maxbytes = 4ull << 30, flush_bytes = 512ull << 20;
    v2f64 *x; double *out, *tcol; void *flush;
    CK(hipMalloc(&x, maxbytes)); CK(hipMalloc(&out, 8)); CK(hipMalloc(&flush, flush_bytes));
    CK(hipMalloc(&tcol, (maxbytes / (GV * 64 * 16)) * 8 * sizeof(double)));
    CK(hipMemset(x, 1, maxbytes));
    if (tstage) {
        const size_t bytes = maxbytes;
        const int blocks = 208;
        const int64_t ngroups = (int64_t)(bytes / (GV * 64 * 16)), W = (int64_t)blocks * 4;
        const int never = (int)((ngroups + W - 1) / W);   // every group of the wave with the most of them: one flush, at the end
        if ((size_t)never * 4 * 8 * sizeof(double) > 64 * 1024) { fprintf(stderr, "ring too long\n"); return 1; }
        struct Mode { int st, ch; const char *name; };
        const Mode modes[] = {{0, 0, "read-only"}, {1, 0, "direct"}, {2, 8, "ring 8"}, {2, 32, "ring 32"}, {2, 64, "ring 64"}, {2, never, "ring never full"}, {3, 0, "direct nt"}};
        printf("# size_MiB blocks S_MiB st CH rep (mode) | launch1_us | launches 2-25: mean min max us | GB/s(mean)\n");
        for (int s : {0, 128}) {
            const double per_wave = (double)ngroups / (double)W * (GV * 64 * 16);
            const int nres = (int)std::min<int64_t>(W, (int64_t)((double)s * 1048576.0 / per_wave + 0.5));
            for (int r = 0; r < 3; ++r)          // the modes interleaved, three rounds
                for (const Mode &m : modes) {
                    const Stat t = run(x, bytes, blocks, nres, m.st, tcol, out, flush, flush_bytes, m.ch);
                    printf("%5d %4d %4d %d %4d %d (%s) | %8.1f | %8.1f %8.1f %8.1f | %7.1f\n", 4096, blocks, s, m.st, m.ch, r, m.name,
                           t.first * 1e3, t.mean * 1e3, t.mn * 1e3, t.mx * 1e3, bytes / (t.mean * 1e-3) / 1e9);
                    fflush(stdout);
                }
        }
        return 0;
    }
    const int S[] = {0, 64, 128, 192, 224, 256, 320, -1};   // MiB; -1: every wave with plain loads
    printf("# size_MiB blocks st S_MiB nres/W rep | launch1_us | launches 2-25: mean min max us | GB/s(mean)\n");
    for (int pass = 0; pass < 3; ++pass) {   // pass 2: the store variant, 4 GiB only
        for (size_t mib : {4096, 1024, 512}) {
            const bool store = pass == 2;
            if (store && mib != 4096) continue;
            const size_t bytes = mib << 20;
            const int64_t ngroups = (int64_t)(bytes / (GV * 64 * 16));
            for (int blocks : {208, 256}) {
                if (pass < 2 && (pass == 0) != (blocks == 208)) continue;   // pass 0: 208 blocks, pass 1: 256 blocks
                if (store && blocks != 208) continue;
                const int64_t W = (int64_t)blocks * 4;
                for (int s : S) {
                    const double per_wave = (double)ngroups / (double)W * (GV * 64 * 16);   // bytes a wave reads per launch
                    int nres = s < 0 ? (int)W : (int)std::min<int64_t>(W, (int64_t)((double)s * 1048576.0 / per_wave + 0.5));
                    const int reps = s == 0 ? 5 : 2;
                    for (int r = 0; r < reps; ++r) {
                        const Stat t = run(x, bytes, blocks, nres, store, tcol, out, flush, flush_bytes);
                        printf("%5zu %4d %d %4d %4d/%-4lld %d | %8.1f | %8.1f %8.1f %8.1f | %7.1f\n", mib, blocks, (int)store, s, nres, (long long)W, r,
                               t.first * 1e3, t.mean * 1e3, t.mn * 1e3, t.mx * 1e3, bytes / (t.mean * 1e-3) / 1e9);
                        fflush(stdout);
                    }
                }
            }
        }
    }
    return 0;
}

// Host-side check of jch_col_median_mad and jch_stah under AddressSanitizer, without a GPU: the argument validation of both entries, and the host
// fold of jch_stah (P with ldp > p, mu_scal, s_scal in heap blocks of exactly their size, so that a read past any of them is reported) up to the
// first HIP call, which fails on a machine without a device before anything is reserved or queued.  A stand-alone program with its own main:
//
//   make -C jchemo.jl_amd/csrc asan
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address -shared-libasan -fno-gpu-sanitize -Iinclude -Ijchemo.jl_amd/csrc \
//         tools/stah_args_check.hip -o tools/stah_args_check -Ljchemo.jl_amd/lib -ljchemo_hip_asan -Wl,-rpath,$PWD/jchemo.jl_amd/lib
//   tools/stah_args_check          (prints "stah_args_check ok"; with a device present the valid calls run to the end instead)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jch_internal.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "stah_args_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main()
{
    jch_ctx ctx;   // what jch_ctx_create builds, minus the device: enough for every path in front of the first HIP call
    const int64_t n = 7, p = 5, a = 19, ldx = 9, ldp = 6;
    std::vector<double> X((size_t)ldx * p, 1.0), P((size_t)ldp * (a - 1) + p, 1.0), ms(p, 0.5), ss(p, 2.0), mu(a), s(a), d(n), med(p), mad(p);
    // ---- jch_col_median_mad
    EXPECT(jch_col_median_mad(nullptr, 0, X.data(), n, p, ldx, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, nullptr, n, p, ldx, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, X.data(), n, p, ldx, nullptr, mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, X.data(), 0, p, ldx, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, X.data(), n, 0, ldx, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, X.data(), n, p, n - 1, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 2, X.data(), n, p, ldx, med.data(), mad.data(), 0) == JCH_EINVAL);
    EXPECT(jch_col_median_mad(&ctx, 0, X.data(), n, p, ldx, med.data(), mad.data(), 2) == JCH_EINVAL);
    EXPECT(ctx.err.find("jch_col_median_mad") != std::string::npos);
    // ---- jch_stah
    EXPECT(jch_stah(nullptr, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, nullptr, n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), nullptr, a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, nullptr, s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), nullptr, d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), nullptr) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), 0, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), 0, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, n - 1, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, p - 1, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(jch_stah(&ctx, 3, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    ctx.nranks = 2;
    EXPECT(jch_stah(&ctx, 0, X.data(), n, p, ldx, ms.data(), ss.data(), P.data(), a, ldp, 1, mu.data(), s.data(), d.data()) == JCH_EINVAL);
    EXPECT(ctx.err.find("one rank only") != std::string::npos);
    ctx.nranks = 1;
    // valid arguments: the fold reads P (ldp > p, the last column ending with the block), mu_scal and s_scal; then the device is asked for
    int ndev = 0;
    const bool have_dev = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    for (int fit = 0; fit < 2; ++fit)
        for (int scal = 0; scal < 2; ++scal) {
            const int32_t st = jch_stah(&ctx, 0, X.data(), n, p, ldx, scal ? ms.data() : nullptr, scal ? ss.data() : nullptr, P.data(), a, ldp, fit, mu.data(), s.data(), d.data());
            EXPECT(have_dev ? st == JCH_OK || st == JCH_EHIP : st == JCH_EHIP);
        }
    const int32_t st = jch_col_median_mad(&ctx, 0, X.data(), n, p, ldx, med.data(), nullptr, 0);
    EXPECT(have_dev ? st == JCH_OK || st == JCH_EHIP : st == JCH_EHIP);
    printf("stah_args_check ok\n");
    return 0;
}

// abi_common.hpp -- what every translation unit of libburgers_hip.so shares at the C-ABI boundary:
// the per-thread record of the last failed launch (read back by bg_last_hip_error) and the
// cached per-device CU count (no other process-wide state exists in the library), and the launch idiom of the entry
// points: the persistent grid, the projection and the rows per thread as compile-time tags, the fast-then-repair pair of launches.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "../../include/burgers_hip.h"

namespace bg {

extern thread_local int tls_last_hip_error;     // defined in fom.hip

// Call right after a kernel launch: BG_OK, or BG_ERR_LAUNCH with the hipError_t kept for bg_last_hip_error().
inline int check_launch()
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return BG_OK;
    tls_last_hip_error = (int)e;
    return BG_ERR_LAUNCH;
}

// Compute units of the current device, queried once per device (a launch must not pay two runtime calls).
inline int device_cu_count()
{
    static std::atomic<int> cached[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
    int c = cached[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cached[dev].store(c, std::memory_order_relaxed);
    return c;
}

// Grid of a persistent kernel whose workgroups walk over `units` (samples, or groups of them), `per_cu` resident per CU.
inline int persistent_grid(int units, int per_cu)
{
    const int slots = per_cu * device_cu_count();
    return units < slots ? units : slots;
}

// The projection as a compile-time tag: kernels templated on `int PROJ` take ::value, those on `bool GAL` ::galerkin.
template <int P>
struct ProjectionTag {
    static constexpr int value = P;
    static constexpr bool galerkin = P == BG_PROJ_GALERKIN;
};

// f(tag) for a projection the entry point has already validated (anything but Galerkin is LSPG).
template <class F>
auto dispatch_projection(int projection, F&& f)
{
    if (projection == BG_PROJ_GALERKIN) return f(ProjectionTag<BG_PROJ_GALERKIN>{});
    return f(ProjectionTag<BG_PROJ_LSPG>{});
}

// Rows per thread as a compile-time constant: f(std::integral_constant<int, R>) for the first R of Rs... with
// N <= THREADS * R (THREADS threads share one sample's N rows); BG_ERR_UNSUPPORTED_N when none is large enough.
template <int THREADS, int... Rs, class F>
int dispatch_rows(int N, F&& f)
{
    int rc = BG_ERR_UNSUPPORTED_N;
    (void)(... || (N <= THREADS * Rs && ((rc = f(std::integral_constant<int, Rs>{})), true)));
    return rc;
}

// The two launches of a loop with a repair kernel: the fast kernel (guarded pivot-free elimination, `fast_per_cu`
// workgroups per CU) unless BG_OPT_FORCE_PIVOTED, then the repair kernel (one per CU; every workgroup leaves at once unless
// a sample is marked).  `launch(piv, grid)`, piv a std::bool_constant, launches the instantiation with PIV = piv.
template <class Launch>
int launch_fast_then_repair(int B, int fast_per_cu, bool force_pivoted, const Launch& launch)
{
    if (!force_pivoted) {
        launch(std::false_type{}, persistent_grid(B, fast_per_cu));
        const int rc_fast = check_launch();
        if (rc_fast != BG_OK) return rc_fast;
    }
    launch(std::true_type{}, persistent_grid(B, 1));
    return check_launch();
}

}  // namespace bg

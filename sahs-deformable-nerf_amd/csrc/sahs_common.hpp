// sahs_common.hpp -- small shared helpers for the HIP sources.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdlib>
#include "sahs_model.hpp"

// Once per (call site, device), safe from several host threads: kernel attributes and device properties belong to a DEVICE,
// and a process may drive more than one (the library keeps no other state).  The guarded action is idempotent, so two threads
// racing on the first call both perform it; nothing is cached until it has succeeded.
namespace sahs_once {
constexpr int MAX_DEVICES = 64;
struct Flags { std::atomic<int> v[MAX_DEVICES]; };
template <class F>
inline hipError_t per_device(Flags &flags, F &&action)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEVICES) return action();
    if (flags.v[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = action();
    if (e == hipSuccess) flags.v[dev].store(1, std::memory_order_release);
    return e;
}
}  // namespace sahs_once

// One launch of a persistent kernel: a workgroup per tile, at most one per CU (the kernel walks the tiles), with lds_bytes of dynamic LDS
// -- more than a kernel gets by default, so the attribute that allows it is set first, once per device and kernel (the flags are this
// instantiation's own).  Returns the HIP error of the attribute or of the launch, 0 for none.
template <auto Kernel, class... A>
inline int sahs_launch_persistent(long ntiles, int num_cu, int threads, size_t lds_bytes, hipStream_t stream, A... args)
{
    const int grid = (int)(ntiles < num_cu ? ntiles : num_cu);
    static sahs_once::Flags attr_set;
    hipError_t ae = sahs_once::per_device(attr_set, [&]() {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    });
    if (ae != hipSuccess) return (int)ae;
    Kernel<<<grid, threads, lds_bytes, stream>>>(args...);
    return (int)hipGetLastError();
}

// Timing-only switches and tuning aids are read from the environment by SAHS_DIAG builds only (tools/ablate.py); the shipped library,
// which build.py refuses to build with extra defines, takes the default of each: there this is a constant null.
#ifdef SAHS_DIAG
inline const char *sahs_diag_env(const char *name) { return getenv(name); }
#else
constexpr const char *sahs_diag_env(const char *) { return nullptr; }
#endif

namespace SAHS_NS {
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int WAVE = 64;   // gfx950 wavefront
}  // namespace SAHS_NS

// pdp_launch.h - the host-side launch layer of both translation units (pdp_model.hip, pdp_lqr.hip): how an entry point turns run-time values into a kernel
// instantiation and launches it.  Host code only, everything inlined away; no device code lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "../../include/pdp_hip.h"

namespace pdp {

// launch-error protocol: stale errors of other libraries in the process are cleared in front of a launch (clear_stale_error), the error of our own launch
// is reported on stderr and mapped to PDP_E_LAUNCH
inline void clear_stale_error() { (void)hipGetLastError(); }
inline int launched() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    fprintf(stderr, "[pdp_hip] kernel launch failed: %s\n", hipGetErrorString(e));
    return PDP_E_LAUNCH;
}

// an integer switch of the environment (atoi of the variable, `dflt` where it is unset); a call site keeps the value in a `static const int`: read once per process
inline int env_int(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }

// one launch of a sequence: the dynamic-LDS limit of the kernel is raised in front of every launch that asks for LDS (not cached); neither clears nor checks
template <class Kernel, class... Args>
inline void enqueue(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
    if (lds_bytes > 0) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
}
// the launch of an entry point, always in this order: clear stale error, LDS attribute, launch, check
template <class Kernel, class... Args>
inline int launch(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args... args) {
    clear_stale_error();
    enqueue(kernel, grid, block, lds_bytes, stream, args...);
    return launched();
}

// run-time value -> compile-time constant: f(std::integral_constant<int, V>) for the listed V that equals v, the LAST listed value for every other v (what the
// `default:` label of a switch did).  Inside f the template argument, block size, grid and LDS size of a kernel all come from that one constant: K().  Nest it
// for kernels with two parameters - f is instantiated for exactly the listed values, a nest for exactly their product.
template <int V, int... Rest, class F>
inline int with_int(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, V>{});
    else return v == V ? f(std::integral_constant<int, V>{}) : with_int<Rest...>(v, f);
}
template <class F>
inline int with_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// trajectories per workgroup of the wave-pair kernels: 4 (the two waves of a trajectory share a SIMD) once the batch fills the chip that way; a smaller batch
// spreads over the CUs with the two waves on different SIMDs.  max_tpw = 2 for the kernels that are instantiated for one / two trajectories only.
inline int traj_per_workgroup(int B, int cus, int max_tpw) { return B <= cus ? 1 : (B <= 2 * cus || max_tpw == 2 ? 2 : 4); }

// nt parameter tiles of a trajectory spread over at most `want` workgroups (grid.y): each carries `per` of them
struct TileSplit { int gy, per; };
inline TileSplit split_tiles(int nt, int64_t want) {
    const int gy = want < 1 ? 1 : (want > nt ? nt : (int)want), per = (nt + gy - 1) / gy;
    return {(nt + per - 1) / per, per};
}

}  // namespace pdp

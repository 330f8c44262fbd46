// pbn_launch.hpp -- host-side launch and dispatch helpers shared by the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pbn_params.hpp"

namespace pbn {

// Dynamic LDS above 64 KiB has to be allowed per kernel before a launch or an occupancy query.
inline hipError_t allow_lds(const void* fn, uint32_t lds) {
    if (lds <= 64u * 1024u) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// Launches fn (a kernel taking one argument struct, *args) with lds bytes of dynamic LDS.
// A null fn (no kernel for the requested shape) is hipErrorInvalidValue. Returns hipError_t as int.
inline int launch(void* fn, int grid, int block, uint32_t lds, void* stream, void* args) {
    if (!fn) return (int)hipErrorInvalidValue;
    if (hipError_t e = allow_lds(fn, lds)) return (int)e;
    void* kargs[] = {args};
    return (int)hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)block), kargs, lds, (hipStream_t)stream);
}

// Resident workgroups of fn per CU at this block size and LDS use (at least 1).
inline int occupancy(void* fn, int block, uint32_t lds, int* blocks_per_cu) {
    if (!fn) return (int)hipErrorInvalidValue;
    if (hipError_t e = allow_lds(fn, lds)) return (int)e;
    int nb = 0;
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)fn, block, lds)) return (int)e;
    *blocks_per_cu = nb < 1 ? 1 : nb;
    return 0;
}

// Run-time words per env W -> compile-time: f(std::integral_constant<int, W>{}) for W in 1..MAXW
// (f returns the kernel as void*), nullptr outside. Instantiates f for exactly 1..MAXW.
template <int MAXW, class F>
void* by_words(int W, F f) {
    if constexpr (MAXW >= 1) {
        if (W == MAXW) return f(std::integral_constant<int, MAXW>{});
        return by_words<MAXW - 1>(W, f);
    }
    return nullptr;
}

// k_env_grp<W, grp> / k_rollout_grp<W, grp> (pbn_group.hip) for pbn_env.hip's and pbn_step.hip's dispatch;
// nullptr without such a kernel (W > 4, grp not 2, 4 or 8)
void* env_grp_kernel(int W, int grp);
void* rollout_grp_kernel(int W, int grp);

#ifdef PBN_STAMPS
// measurement builds: each file zeroes its own stamp array (pbn_exp_stamps_clear calls both)
int step_stamps_clear();
int env_stamps_clear();
#endif

}  // namespace pbn

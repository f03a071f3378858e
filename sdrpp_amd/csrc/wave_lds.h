// Cross-lane LDS hand-off inside one wave (chan_dft_gemm in chan_kernels.h, fmif_kernel in
// ifnr_kernels.h): the HIP memory model does not order one lane's LDS store before another lane's
// later LDS load, so a write phase whose values other lanes of the same wave read next is closed by a
// wave-scope release fence + wave barrier + acquire fence. No workgroup barrier is needed where each
// wave touches only its own part of LDS. Costs a few cycles per phase.
#pragma once
#include <hip/hip_runtime.h>

namespace sdrgpu {

__device__ __forceinline__ void wave_lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace sdrgpu

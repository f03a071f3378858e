// The walk shared by the serial (data-dependent) loops of loop_kernels.h and symsync_kernels.h, and
// the amplitude / scaling helpers both use. Include only from a translation unit built with
// -ffp-contract=off (the headers that include this one say why).
#pragma once
#include "sdrgpu_internal.h"

namespace sdrgpu {

constexpr int LOOP_CHUNK = 1024;
constexpr int LOOP_NT = 256;

// |x| exactly as complex_t::amplitude() (types.h:79) / fabsf, no contraction
__device__ __forceinline__ float amp_of(float x) { return fabsf(x); }
// (sqrtf is correctly rounded under HIP's default -fhip-fp32-correctly-rounded-divide-sqrt;
// __fsqrt_rn is the native approximation unless OCML_BASIC_ROUNDED_OPERATIONS is defined)
__device__ __forceinline__ float amp_of(float2 x) { return sqrtf((x.x * x.x) + (x.y * x.y)); }
__device__ __forceinline__ float scale_of(float x, float g) { return x * g; }
__device__ __forceinline__ float2 scale_of(float2 x, float g) { return make_float2(x.x * g, x.y * g); }

// The walk of a serial block, by its one workgroup of LOOP_NT lanes, E LDS elements per sample: per
// chunk of n <= LOOP_CHUNK samples starting at i0, all lanes stage(i0, e) the chunk's elements e <
// n E into LDS, lane 0 runs step(i) over its samples in order, and all lanes emit(i0, e) the
// elements. The kernel owns the LDS arrays and the recurrence's state; the hooks capture them.
template <int E = 1, typename Stage, typename Step, typename Emit>
__device__ __forceinline__ void serial_chunks(int count, Stage stage, Step step, Emit emit) {
    const int t = threadIdx.x;
    for (int i0 = 0; i0 < count; i0 += LOOP_CHUNK) {
        const int n = min(LOOP_CHUNK, count - i0);
        for (int e = t; e < n * E; e += LOOP_NT) stage(i0, e);
        __syncthreads();
        if (t == 0) {
            for (int i = 0; i < n; i++) step(i);
        }
        __syncthreads();
        for (int e = t; e < n * E; e += LOOP_NT) emit(i0, e);
        __syncthreads();
    }
}

}  // namespace sdrgpu

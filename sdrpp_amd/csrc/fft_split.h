// Spectrum device code, the front end's per-block launch pair (fft_execute_split, fft.hip):
// fft_passA_vfo_kernel and fft_passB_tail_kernel. Included after fft_onepass.h: these two and
// fft_1p_tail_fold_kernel share the VFO tail's device functions, and the compiler's inlining of those
// depends on the order in which their callers are defined (profiles/r8/README.md).
#pragma once
#include "fft_passes.h"

namespace sdrgpu {

// ---- the front end's per-block launch: pass A (frame straddling two pushes read in place) + the
// VFO's first stage + its history carry + the tail copy, one launch (sdrgpu_frontend_*): the block is
// small (a reference-size block has ~5 frames and 9,600 stage-1 outputs), so the stage's segments
// are the small-call ones (32 outputs, one row batch each: 300 segments, 19 workgroups of 16).
struct VfoCall {
    FirArgs a;
    int blocks;      // stage-1 workgroups (16 segments each)
};
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void fft_passA_vfo_kernel(
    const float2* __restrict__ in, long long frameStride, int frames, const float* __restrict__ win, int nz, int N2,
    int logN, const float2* __restrict__ tw, const float2* __restrict__ tfull, float2* __restrict__ scratch,
    const float2* __restrict__ headp, int nh, SideCopy side, VfoCall v) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    const int ntiles = (N2 / 32) * frames;
    int b = blockIdx.x;
    if (b < ntiles) {
        passA_tile<256, 32>(lds, b, in, frameStride, frames, win, nz, N2, logN, tw, tfull, scratch, headp, nh);
        return;
    }
    b -= ntiles;
    if (b < v.blocks) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        fir_rows_segment<32, 5, true, false, 32, 32, true>(v.a, ((long long)b * 8 + wave) * 2 + (lane >> 5), lane);
        return;
    }
    b -= v.blocks;
    if (b == 0) {   // the stage's history carry (fir.h:80)
        fir_hist_copy<float2, true, false>(v.a);
        return;
    }
    const int w = b - 1, nw = gridDim.x - ntiles - v.blocks - 1;   // spare workgroups: the side copies
    for (int k = 0; k < side.count; k++)
        for (int i = w * blockDim.x + threadIdx.x; i < side.n[k]; i += nw * blockDim.x) side.dst[k][i] = side.src[k][i];
}

// ... and its pass-B launch: the pass-B tiles + the VFO's tail workgroups (fir_tail_block on the
// first 256 threads of a 512-thread block), one launch for both (the tail needs only the stage-1
// output the pass-A launch wrote)
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void fft_passB_tail_kernel(
    const float2* __restrict__ scratch, int frames, int N1, int logN, const float2* __restrict__ tw, float* __restrict__ out,
    TailArgs t) {
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    __shared__ TailGeom gs[TAIL_MAXS];
    const int ntiles = (N1 / 32) * frames;
    if ((int)blockIdx.x < ntiles) {
        passB_tile<256, 32, false>(lds, blockIdx.x, scratch, frames, N1, logN, tw, out, nullptr);
        return;
    }
    const int w = blockIdx.x - ntiles;
    fir_tail_block<TAIL_K, TAIL_NT>(t, w, w == t.G - 1, lds, gs);
}

}  // namespace sdrgpu

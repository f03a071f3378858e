// Bit-exact sums: include this header only from a translation unit built with -ffp-contract=off
// (sdrpp_amd/build.py does that for bank.hip; bank_kernels.h says why).
//
// Device code of the rate-changing banks of bank.hip: multirate::PolyphaseResampler<T> per stream
// (polyphase_resampler.h:69-99 over polyphase_bank.h:15-47) in the bank layout, element m of stream k at
// x[m * S + k]. filter::DecimatingFIR<D, float> (decimating_fir.h:45-68) is the same kernel with interp = 1 and
// the one phase equal to the taps.
//
// The closed form of PolyBlock / poly_kernel (chain_kernels.h): with pos0 = offset * interp + phase at the start
// of the call, output row j reads work rows off_j .. off_j + tpp - 1 of [hist (tpp - 1 rows) || in] through the
// taps of phase ph_j, (off_j, ph_j) = divmod(pos0 + j * decim, interp):
//   out[j * S + k] = sum_t work_k[off_j + t] * bank[ph_j * tpp + t]
// in ascending t, fp32, unfused, as bank_fir_kernel sums: decim = interp = 1 is that kernel's arithmetic.
// All streams share offset and phase (shared parameters, a common start), so (off_j, ph_j) belongs to the row:
// rate_row computes it from uniform values only (block index, kernel arguments, the wave's number through
// readfirstlane), i.e. once per row on the scalar side, and the taps of the row's phase are read at a uniform
// address (scalar loads). A thread's element is the uniform row base plus its stream k: no division by S and no
// 64-bit divmod per element. The loads and stores of a row are consecutive words over k.
//
// Two forms with the same sum, hence the same bits:
//   direct  one thread per output element, block = one row x 256 streams; the work rows come from global memory
//           (hist / in), each input element about tpp * interp / decim times, out of L2.
//   tiled   a workgroup owns 64 streams x R output rows (RateArgs::R, rate_tile_rows on the host). Its 8 waves
//           stage work rows off_first .. off_last + tpp - 1 of the chunk once into LDS, X[row][64 lanes]: a lane
//           reads column l only, word r * 64 + l (C64: dwords 2l, 2l + 1), conflict-free at any row as in
//           bank_kernels.h. Wave w then makes rows w, w + 8, ... of the R from LDS. Global reads per input element:
//           (span + tpp - 1) / span, span = the input rows R outputs consume. R is the largest count whose staged rows
//           fit RATE_LDS = 64 KiB (two workgroups per CU of 160 KiB), at most RATE_RMAX; below RATE_RMIN rows the
//           configuration runs the direct kernel. A call with few rows takes smaller tiles (BankRate::run): as many as
//           give RATE_WGS workgroups, RATE_TW rows (one per wave) at least. The bits do not depend on R.
// Bounds: off_j < frames for every output row (the host's count), so the last work row read, off_j + tpp - 1, is
// below frames + tpp - 1 = the rows of [hist || in]; k < S is checked before any access.
#pragma once
#include <hip/hip_runtime.h>

namespace sdrgpu {

constexpr int RATE_W = 64;              // streams per tiled workgroup (lanes of a wave)
constexpr int RATE_TW = 8;              // waves per tiled workgroup
constexpr int RATE_XS = 256;            // streams per direct block (= threads)
constexpr int RATE_LDS = 64 * 1024;     // LDS bytes of a tile at most
constexpr int RATE_RMIN = 4, RATE_RMAX = 64;   // output rows per tile
constexpr int RATE_WGS = 512;           // workgroups a call aims for before its tiles grow past a row per wave (2 per CU)

struct RateArgs {
    int S, H, tpp, interp;   // streams, history rows (tpp - 1), taps per phase, phases
    int qD, rD;              // divmod(decim, interp)
    int off0, ph0;           // divmod(pos0, interp) = the call's (offset, phase)
    int M, R, chunks;        // output rows of the call; rows per tile (tiled); stream chunks per row (group)
};

// (off_j, ph_j) of output row j; every operand is uniform over the wave. pos0 + j * decim = (off0 + j * qD) * interp
// + ph0 + j * rD: the division is of ph0 + j * rD, 32-bit unless the call is very long, and none where interp
// divides decim (a decimating FIR).
__device__ __forceinline__ void rate_row(const RateArgs& a, int j, int& off, int& ph) {
    if (a.rD == 0) {
        off = a.off0 + j * a.qD;
        ph = a.ph0;
        return;
    }
    const unsigned long long t = (unsigned)a.ph0 + (unsigned long long)(unsigned)j * (unsigned)a.rD;
    unsigned q, r;
    if ((t >> 32) == 0) {
        q = (unsigned)t / (unsigned)a.interp;
        r = (unsigned)t % (unsigned)a.interp;
    } else {
        q = (unsigned)(t / (unsigned)a.interp);
        r = (unsigned)(t % (unsigned)a.interp);
    }
    off = a.off0 + j * a.qD + (int)q;
    ph = (int)r;
}

template <typename DT>
__device__ __forceinline__ void rate_mac(DT& acc, DT x, float t) {
    if constexpr (sizeof(DT) == 4) {
        acc += x * t;
    } else {
        acc.x += x.x * t;
        acc.y += x.y * t;
    }
}

// work row w of column k
template <typename DT>
__device__ __forceinline__ DT rate_work(const DT* __restrict__ hist, const DT* __restrict__ in, int w, int H, int S, int k) {
    return w < H ? hist[(size_t)w * S + k] : in[(size_t)(w - H) * S + k];
}

// direct: block b is the 256-stream chunk b % chunks of output row b / chunks
template <typename DT>
__global__ __launch_bounds__(RATE_XS) void bank_rate_direct_kernel(const DT* __restrict__ hist, const DT* __restrict__ in,
                                                                   const float* __restrict__ bank, DT* __restrict__ out, RateArgs a) {
    const int j = blockIdx.x / a.chunks;
    const int k = (blockIdx.x - j * a.chunks) * RATE_XS + threadIdx.x;
    if (k >= a.S) return;
    int off, ph;
    rate_row(a, j, off, ph);
    const float* hb = bank + (size_t)ph * a.tpp;
    DT acc{};
#pragma unroll 4
    for (int t = 0; t < a.tpp; t++) rate_mac(acc, rate_work(hist, in, off + t, a.H, a.S, k), hb[t]);
    out[(size_t)j * a.S + k] = acc;
}

// tiled: block b is the 64-stream chunk b % chunks of the R-row group b / chunks.
// Dynamic LDS: (off_last - off_first + tpp) * 64 elements, at most RATE_LDS bytes (rate_tile_rows).
template <typename DT>
__global__ __launch_bounds__(RATE_TW* RATE_W) void bank_rate_tiled_kernel(const DT* __restrict__ hist, const DT* __restrict__ in,
                                                                          const float* __restrict__ bank, DT* __restrict__ out,
                                                                          RateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bank_rate_lds[];
    DT* X = reinterpret_cast<DT*>(bank_rate_lds);
    const int g = blockIdx.x / a.chunks;
    const int l = threadIdx.x & (RATE_W - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / RATE_W));
    const int k = (blockIdx.x - g * a.chunks) * RATE_W + l;
    const int j0 = g * a.R, n = min(a.R, a.M - j0);
    int offA, offB, ph;
    rate_row(a, j0, offA, ph);
    rate_row(a, j0 + n - 1, offB, ph);
    const int nr = offB - offA + a.tpp;   // staged rows
    if (k < a.S) {
#pragma unroll 4
        for (int r = wv; r < nr; r += RATE_TW) X[r * RATE_W + l] = rate_work(hist, in, offA + r, a.H, a.S, k);
    }
    __syncthreads();
    if (k >= a.S) return;
    for (int r = wv; r < n; r += RATE_TW) {
        int off;
        rate_row(a, j0 + r, off, ph);
        const float* hb = bank + (size_t)ph * a.tpp;
        const DT* x = X + (off - offA) * RATE_W + l;
        DT acc{};
#pragma unroll 8
        for (int t = 0; t < a.tpp; t++) rate_mac(acc, x[t * RATE_W], hb[t]);
        out[(size_t)(j0 + r) * a.S + k] = acc;
    }
}

}  // namespace sdrgpu

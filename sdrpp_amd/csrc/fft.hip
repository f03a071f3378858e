// Spectrum hot path, host side: window * FFT(N) * 10*log10(|X|^2), replacing
// IQFrontEnd::handler (signal_path/iq_frontend.cpp:230-249): K1 volk window
// multiply, K2 fftwf_execute (forward, unnormalised), K3 power spectrum.
// The kernels are in fft_passes.h, fft_onepass.h and fft_split.h (fp64 interior: fft64.hip); this file holds the
// plan (FftPlan), one host function per launch family and the C entry points.
//
// Launch families (DESIGN.md "Spectrum kernels"), and who takes which:
//  1. single pass, N <= 4096 (dispatch_single): S frames per workgroup entirely in LDS.
//  2. two passes, N > 4096 as N1 x N2 (dispatch_passA / _passA2 + dispatch_passB): pass A = N2
//     column FFTs of length N1 (window + zero-pad fused into the load, W_N^(n2 k1) fused into the
//     store), pass B = N1 row FFTs of length N2 with |X|^2 -> dB (and the N / 32 zoom row) fused into
//     a transposing store. The intermediate is streamed in frame chunks sized to stay resident in
//     the 256 MB Infinity Cache. On the 64k plan's default tiles (tiles_64k) a call of several chunks
//     merges pass B of chunk c with pass A of chunk c + 1 (launch_merged over chunk_walk). 64k calls
//     below k1pMinFrames frames, the front end's plans and every other two-pass size run these.
//  3. the persistent 1M passes (dispatch_1m): N1 = N2 = 1024 with 16-B aligned input.
//  4. the one-pass 64k kernel (launch_1p), alone or with the zoom partials and a VFO's first stage:
//     64k calls of >= k1pMinFrames frames (sdrgpu_fft_set_kernel); its zoom fold is a launch of its
//     own or rides in the VFO's tail launch (launch_tail_fold), on the tail stream where one is set.
//  5. two-pass launches that carry a VFO: fft_vfo_kernel over the chunk walk (vfo_twopass: short
//     sdrgpu_fft_execute_(zoom_)vfo_dev calls), and the front end's per-block pair
//     fft_passA_vfo_kernel + fft_passB_tail_kernel (fft_execute_split).
// The fp64 plan (sdrgpu_fft_set_precision) runs fft64.hip's launches in place of 1-4 and fuses nothing.
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <utility>
#include "sdrgpu_internal.h"
#include "fft_passes.h"
#include "fft_onepass.h"
#include "fft_split.h"   // (after fft_onepass.h: see there)
#include "blocks.h"

namespace sdrgpu {

struct FftPlan {
    int device = 0, N = 0, logN = 0, nz = 0;
    int N1 = 0, N2 = 0;               // two-pass split (N1 * N2 = N); N1 = 0 -> single pass
    DevBuf win, tw1, tw2, tfull, scratch, scratch2;
    int chunkFrames = 1;
    int sa = 16;                      // pass-A columns per workgroup (32, with 32 pass-B rows, on the 64k plan)
    float2* cur = nullptr;            // scratch buffer of the chunk being launched
    int sa2 = 0;                      // paired pass-A columns per workgroup (0: paired kernel off)
    int gridA = 0, gridB = 0;         // the persistent 1M passes' grids (resident workgroups)
    DevBuf wt;                        // fp64 W_N^(256 j), W_N^j (j < 256) for the 1M pass A
    hipStream_t own = nullptr;
    PinnedBuf pin_in, pin_out;
    DevBuf dev_in, dev_out;
    // merged pass-B(c) + pass-A(c+1) launches (64k split): one launch boundary per chunk
    // instead of two; 1.87 -> 1.73 ms per 2^28 samples (A/B on one box). SDRGPU_FFT_MERGE=0 off.
    int merge = 1;
    StreamOrder order;                // scratch is per plan: calls on different streams are serialised
    sdrgpu_zoom* zoom = nullptr;      // execute_zoom's unfused zoom (sizes other than N / 32)
    int zoomSize = 0;
    Fft64Plan* f64 = nullptr;         // sdrgpu_fft_set_precision(h, 1): the fp64-interior kernels (fft64.hip)
    // sdrgpu_fft_set_timing: HIP events around each call's spectrum launch group (the fused VFO
    // stage included, the VFO's later stages not), a ring of kTimed calls read by sdrgpu_fft_group_times
    static constexpr int kTimed = 256;
    bool timing = false;
    hipEvent_t tev[kTimed][2] = {};
    long long tcalls = 0;
    int vfoFuse = 1;                  // the VFO's first stage inside the spectrum launches
    int onepass = 0;                  // the 64k plan's one-pass kernel (fft_1p_kernel): 0 never, 1 always, 2 calls of
                                      // >= k1pMinFrames frames (SDRGPU_FFT_1P, tuning)
    int grid1p = -1;                  // fft_1p_kernel's item workgroups: -1 the co-resident ones (persistent walk), 0 one
                                      // per item, n that many (SDRGPU_FFT_1P_GRID, tuning)
    int res1p[4] = {};                // co-resident workgroups of each fft_1p_kernel instantiation (launch_1p)
    DevBuf tab1p, tab1p64, zpart;
    // sdrgpu_fft_set_tail_stream: the fused VFO's later stages and the zoom fold of
    // sdrgpu_fft_execute_(zoom_)vfo_dev run on this stream, overlapping the next call's spectrum launch.
    // Their inputs (the VFO's stage-1 outputs, the zoom partials) are double-buffered per call parity;
    // call k + 2's spectrum launch waits for call k's tail (tdone) before rewriting its buffers.
    hipStream_t tailStream = nullptr;
    DevBuf s1T[2], zpartT[2];
    hipEvent_t gdone[2] = {}, tdone[2] = {};
    bool tdoneRec[2] = {};
    long long tcallsT = 0;
};
static int time_mark(FftPlan& p, int which, hipStream_t s) {
    if (!p.timing) return SDRGPU_OK;
    SDRGPU_HIP(hipEventRecord(p.tev[p.tcalls % FftPlan::kTimed][which], s));
    if (which == 1) p.tcalls++;
    return SDRGPU_OK;
}

// the 64k plan's default tiles: 256 x 256, 32 pass-A columns / 32 pass-B rows per workgroup, one-column
// pass A -- the shape of the merged, zoom-fused, VFO-carrying and split launches
static bool tiles_64k(const FftPlan& p) { return p.N1 == 256 && p.N2 == 256 && p.sa == 32 && p.sa2 == 0; }
constexpr size_t kLds64k = sizeof(float2) * (32 * Lds<256>::LS + 256 + 256);   // a 512-thread workgroup of either 64k pass
static bool zoom_fusable(const FftPlan& p, int zoomSize) { return tiles_64k(p) && zoomSize * 32 == p.N; }
static bool pipe1m_ok(const FftPlan& p, bool paired) { return paired && p.N1 == 1024 && p.N2 == 1024 && (p.nz % 2) == 0; }
// Below k1pMinFrames frames a call runs the two-pass launches: with two workgroups per frame, each two
// 16k transforms long, a reference-size block (4.7 frames) took 33 us against 27 us for the two-pass
// launches (per-call trace r6c vs r4); the one-pass kernel fills the device from ~128 frames.
constexpr int k1pMinFrames = 64;
static bool onepass_ok(const FftPlan& p, int frames) {
    return p.N == 65536 && p.tab1p.p && !p.f64 && (p.onepass == 1 || (p.onepass == 2 && frames >= k1pMinFrames));
}

// ---------------------------------------------------------------- twiddle tables (plan creation)
template <typename T>
static int upload(DevBuf& b, const std::vector<T>& v) {
    SDRGPU_CHECK(b.ensure(sizeof(T) * v.size()));
    if (hipMemcpy(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("fft: twiddle upload failed");
        return SDRGPU_EHIP;
    }
    return SDRGPU_OK;
}
static double2 wexp(long long m, int N) {   // W_N^m in fp64, exact argument mod N
    const double a = -2.0 * M_PI * (double)(m % N) / (double)N;
    return make_double2(std::cos(a), std::sin(a));
}
static float2 wexpf(long long m, int N) {
    const double2 w = wexp(m, N);
    return make_float2((float)w.x, (float)w.y);
}
// t[m] = W_L^m for m < L: a transform's stage twiddles
static int make_twiddles(DevBuf& b, int L) {
    std::vector<float2> t(L);
    for (int m = 0; m < L; m++) t[m] = wexpf(m, L);
    return upload(b, t);
}
// fft_1p_kernel's exact twiddles (op1::TAB, op1::TAB64), N = 65536
static int make_tab1p(FftPlan& p) {
    std::vector<float2> t(op1::TAB);
    for (int q1 = 0; q1 < 32; q1++)
        for (int t0 = 0; t0 < 16; t0++) t[16 * q1 + t0] = wexpf(128LL * t0 * q1, p.N);
    for (int r = 0; r < 4; r++)
        for (int i = 0; i < 32; i++) t[512 + 32 * r + i] = wexpf(512LL * r * i, p.N);
    std::vector<double2> t64(op1::TAB64);   // fp64: W_N^m, m < 2048 (the stage-1 twiddle recurrence); W_128^(r i)
    for (int m = 0; m < 2048; m++) t64[m] = wexp(m, p.N);
    for (int r = 0; r < 4; r++)
        for (int i = 0; i < 32; i++) t64[2048 + 32 * r + i] = wexp(512LL * r * i, p.N);
    SDRGPU_CHECK(upload(p.tab1p, t));
    return upload(p.tab1p64, t64);
}
// fp64 W_N^(256 j), W_N^j (j < 256) for the 1M pass A
static int make_wt(FftPlan& p) {
    std::vector<double2> t(512);
    for (int j = 0; j < 256; j++) {
        t[j] = wexp(256LL * j, p.N);
        t[256 + j] = wexp(j, p.N);
    }
    return upload(p.wt, t);
}
// Tfull[k1][n2] = W_N^(n2 k1), exact argument mod N (both pass-A kernels)
static int make_tfull(FftPlan& p) {
    std::vector<float2> t((size_t)p.N);
    for (int k1 = 0; k1 < p.N1; k1++)
        for (int n2 = 0; n2 < p.N2; n2++) t[(size_t)k1 * p.N2 + n2] = wexpf((long long)n2 * k1, p.N);
    return upload(p.tfull, t);
}

// ---------------------------------------------------------------- launch helpers
// one launch with `lds` bytes of dynamic LDS: the kernel's LDS attribute, the launch, its error
template <typename K, typename... A>
static int launch(K k, int grid, int threads, size_t lds, hipStream_t s, A&&... a) {
    SDRGPU_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, s, std::forward<A>(a)...);
    SDRGPU_HIP(hipGetLastError());
    return SDRGPU_OK;
}

// the co-resident workgroups of a persistent kernel, queried once (grid: the cached value, 0 = not yet)
template <typename K>
static int resident_grid(const FftPlan& p, K k, int threads, size_t lds, int& grid) {
    if (!grid) {
        int per = 0, cus = 0;
        // (the occupancy query counts against the kernel's LDS attribute: set before it, as launch() will)
        SDRGPU_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        SDRGPU_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)k, threads, lds));
        SDRGPU_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p.device));
        grid = std::max(1, per) * std::max(1, cus);
    }
    return SDRGPU_OK;
}

// spare workgroups a launch adds for the caller's side copies: ~4 elements per thread, 1..64
static int side_spare(const SideCopy& side, int threads) {
    if (side.count <= 0) return 0;
    int mx = 0;
    for (int i = 0; i < side.count; i++) mx = std::max(mx, side.n[i]);
    return std::max(1, std::min(64, (mx + threads * 4 - 1) / (threads * 4)));
}

// ---------------------------------------------------------------- 1. single pass
template <int L, int S>
static int launch_single(const FftPlan& p, const float2* in, long long stride, int frames, float* out, hipStream_t s) {
    return launch(fft_single_kernel<L, S>, (frames + S - 1) / S, S * L / 16, sizeof(float2) * S * Lds<L>::LS, s, in, stride,
                  frames, p.win.as<float>(), p.nz, p.tw1.as<float2>(), out);
}

static int dispatch_single(const FftPlan& p, const float2* in, long long stride, int frames, float* out, hipStream_t s) {
    switch (p.N) {
    case 64: return launch_single<64, 16>(p, in, stride, frames, out, s);
    case 128: return launch_single<128, 16>(p, in, stride, frames, out, s);
    case 256: return launch_single<256, 16>(p, in, stride, frames, out, s);
    case 512: return launch_single<512, 8>(p, in, stride, frames, out, s);
    case 1024: return launch_single<1024, 4>(p, in, stride, frames, out, s);
    case 2048: return launch_single<2048, 2>(p, in, stride, frames, out, s);
    case 4096: return launch_single<4096, 1>(p, in, stride, frames, out, s);
    }
    set_error("fft: unsupported size %d", p.N);
    return SDRGPU_EARG;
}

// ---------------------------------------------------------------- 2. two passes
template <int L, int S>
static int launch_passA(const FftPlan& p, const float2* in, long long stride, int frames, hipStream_t s,
                        const float2* headp = nullptr, int nh = 0, const SideCopy* side = nullptr) {
    const size_t lds = sizeof(float2) * (S * Lds<L>::LS + (L == 256 ? L + 256 : 0));   // + stage twiddles (256-point columns)
    const SideCopy sc = side && side->count > 0 ? *side : SideCopy{};
    const int g = (p.N2 / S) * frames + side_spare(sc, S * L / 16);
    return launch(fft_passA_kernel<L, S>, g, S * L / 16, lds, s, in, stride, frames, p.win.as<float>(), p.nz, p.N2, p.logN,
                  p.tw1.as<float2>(), p.tfull.as<float2>(), p.cur, headp, nh, sc);
}

template <int L, int S>
static int launch_passA2(const FftPlan& p, const float2* in, long long stride, int frames, hipStream_t s) {
    if (p.N2 % S) { set_error("fft: N2 %d not a multiple of %d columns", p.N2, S); return SDRGPU_ESTATE; }
    return launch(fft_passA2_kernel<L, S>, (p.N2 / S) * frames, S / 2 * L / 16, sizeof(float2) * (S * Lds<L>::LS + L), s, in,
                  stride, frames, p.win.as<float>(), p.nz, p.N2, p.logN, p.tw1.as<float2>(), p.tfull.as<float2>(), p.cur);
}

template <int L, int S, bool ZM = false>
static int launch_passB(const FftPlan& p, int frames, float* out, hipStream_t s, float* zoom = nullptr) {
    const size_t lds = sizeof(float2) * (S * Lds<L>::LS + (L >= 256 ? 256 : 0));   // + passB_tile's tw16
    return launch(fft_passB_kernel<L, S, ZM>, (p.N1 / S) * frames, S * L / 16, lds, s, p.cur, frames, p.N1, p.logN,
                  p.tw2.as<float2>(), out, zoom);
}

// merged pass B (chunk c) + pass A (chunk c+1) launch of the 64k split (tiles_64k; fft_merged_kernel)
template <bool ZM>
static int launch_merged(const FftPlan& p, const float2* scratchB, int framesB, float* outB, const float2* in,
                         long long stride, int framesA, float2* scratchA, hipStream_t s, float* zoomB = nullptr) {
    const int nB = 8 * framesB, nA = 8 * framesA;
    return launch(fft_merged_kernel<ZM>, nB + nA, 512, kLds64k, s, nB, scratchB, framesB, outB, zoomB, in, stride, framesA,
                  p.win.as<float>(), p.nz, p.logN, p.tw1.as<float2>(), p.tw2.as<float2>(), p.tfull.as<float2>(), scratchA);
}

// pass-A column FFT length N1 with SA columns per workgroup (8*SA-byte row segments)
static int dispatch_passA(const FftPlan& p, const float2* in, long long stride, int frames, hipStream_t s) {
    switch (p.N1) {
    case 64: return launch_passA<64, 16>(p, in, stride, frames, s);
    case 128: return launch_passA<128, 16>(p, in, stride, frames, s);
    case 256:
        if (p.sa == 32) return launch_passA<256, 32>(p, in, stride, frames, s);
        return launch_passA<256, 16>(p, in, stride, frames, s);
    case 512: return launch_passA<512, 8>(p, in, stride, frames, s);
    case 1024: return launch_passA<1024, 16>(p, in, stride, frames, s);
    }
    set_error("fft: unsupported N1 %d", p.N1);
    return SDRGPU_EARG;
}

// paired-column pass A (16-B accesses; +13% on the 1M transform, slower than the one-column kernel
// at N1 = 256): N1 >= 512, when the input allows 16-B loads
static int dispatch_passA2(const FftPlan& p, const float2* in, long long stride, int frames, hipStream_t s) {
    switch (p.N1) {
    case 512: return launch_passA2<512, 16>(p, in, stride, frames, s);
    case 1024: return launch_passA2<1024, 16>(p, in, stride, frames, s);
    }
    set_error("fft: unsupported paired N1 %d", p.N1);
    return SDRGPU_EARG;
}

static int dispatch_passB(const FftPlan& p, int frames, float* out, hipStream_t s, float* zoom = nullptr) {
    if (zoom) return launch_passB<256, 32, true>(p, frames, out, s, zoom);   // (zoom_fusable checked the plan)
    switch (p.N2) {
    case 64: return launch_passB<64, 32>(p, frames, out, s);
    case 128: return launch_passB<128, 32>(p, frames, out, s);
    case 256: return launch_passB<256, 32>(p, frames, out, s);
    case 512: return launch_passB<512, 16>(p, frames, out, s);
    case 1024: return launch_passB<1024, 16>(p, frames, out, s);
    }
    set_error("fft: unsupported N2 %d", p.N2);
    return SDRGPU_EARG;
}

// The chunk walk of the launches that pair pass B of one chunk with pass A of the next, over two
// ping-pong scratch buffers: A(0); [B(c-1) + A(c)] for c = 1..; B(last). step(scB, fB, nfB, scA, fA, nfA)
// launches pass B of the nfB frames from frame fB out of scB and pass A of the nfA frames from frame fA
// into scA; the first step has no B half (nfB = 0, scB = nullptr), the last no A half.
template <class Step>
static int chunk_walk(FftPlan& p, int frames, Step&& step) {
    const int cf = p.chunkFrames, nchunks = (frames + cf - 1) / cf;
    // the intermediate grows with the largest chunk seen (a single-frame drop-in plan holds 0.5 MB)
    SDRGPU_CHECK(p.scratch.ensure((size_t)std::min(cf, frames) * p.N * sizeof(float2)));
    SDRGPU_CHECK(p.scratch2.ensure(p.scratch.bytes));
    float2* sc[2] = {p.scratch.as<float2>(), p.scratch2.as<float2>()};
    for (int c = 0; c <= nchunks; c++) {
        const int fB = (c - 1) * cf, nfB = c > 0 ? std::min(cf, frames - fB) : 0;
        const int fA = c * cf, nfA = c < nchunks ? std::min(cf, frames - fA) : 0;
        SDRGPU_CHECK(step(nfB ? sc[(c - 1) & 1] : nullptr, fB, nfB, nfA ? sc[c & 1] : nullptr, fA, nfA));
    }
    return SDRGPU_OK;
}

// ---------------------------------------------------------------- 3. the persistent 1M passes
// one chunk (pass B reads pass A's tile-major intermediate)
static int dispatch_1m(FftPlan& p, const float2* xc, long long stride, int nf, float* o, hipStream_t s) {
    const size_t ldsA = sizeof(float2) * (16 * Lds<1024>::LS + 1024 + 256);
    const size_t ldsB = sizeof(float2) * (8 * kPassB1mLS + 1024 + 256);   // 80,000 B: two workgroups per CU
    SDRGPU_CHECK(resident_grid(p, fft_passA_1m_kernel, 512, ldsA, p.gridA));
    SDRGPU_CHECK(resident_grid(p, fft_passB_1m_kernel, 512, ldsB, p.gridB));
    SDRGPU_CHECK(launch(fft_passA_1m_kernel, std::min(p.gridA, (p.N2 / 16) * nf), 512, ldsA, s, xc, stride, nf, p.win.as<float>(),
                        p.nz, p.N2, p.logN, p.tw1.as<float2>(), p.wt.as<double2>(), p.cur));
    return launch(fft_passB_1m_kernel, std::min(p.gridB, (p.N1 / 8) * nf), 512, ldsB, s, p.cur, nf, p.N1, p.logN,
                  p.tw2.as<float2>(), o);
}

// ---------------------------------------------------------------- 4. the one-pass 64k kernel
// The one-pass launch (+ the zoom fold of the partials in zp, unless the caller folds): 2 items per frame
// (quarter pairs), XCD-grouped in blocks of 8 frames, walked by the co-resident workgroups
// (SDRGPU_FFT_1P_GRID), + the VFO stage's history workgroup
template <bool ZM, bool VFO>
static int launch_1p(FftPlan& p, const float2* in, long long stride, int frames, float* out, float* zoom, VfoWork v,
                     hipStream_t s, bool fold, DevBuf& zp) {
    // LDS-DMA rows need whole frames, an even frame stride and a 16-B aligned base (16-B pieces);
    // anything else streams through the range-checked register ring
    const bool pad = p.nz < 65536 || (stride & 1) || ((uintptr_t)in & 15);
    if (ZM) SDRGPU_CHECK(zp.ensure(sizeof(float) * 2 * 2048 * (size_t)frames));   // the two workgroups' partial rows
    auto k = pad ? fft_1p_kernel<ZM, VFO, true> : fft_1p_kernel<ZM, VFO, false>;
    // item workgroups: the co-resident ones walk the items (tables staged once, the next item's first row sets
    // prefetched; fft_1p_kernel), a multiple of 16 so a workgroup keeps its quarter pair and its XCD group
    const int items = 16 * ((frames + 7) / 8);
    int G = items;
    if (p.grid1p != 0 && !pad) {   // (the range-checked instantiations: one item per workgroup, fft_1p_kernel)
        int n = p.grid1p;
        if (n < 0) {
            SDRGPU_CHECK(resident_grid(p, k, 512, op1::LDS_BYTES, p.res1p[2 * ZM + VFO]));
            n = p.res1p[2 * ZM + VFO];
        }
        G = std::min(items, std::max(16, n / 16 * 16));
    }
    SDRGPU_CHECK(launch(k, G + (VFO && v.hist ? 1 : 0), 512, op1::LDS_BYTES, s,
                        Args1p{in, stride, frames, p.win.as<float>(), p.nz, p.tab1p.as<float2>(), p.tab1p64.as<double2>(), out,
                               ZM ? zp.as<float>() : nullptr, v}));
    if (ZM && fold) {
        const long long n = (long long)frames * 2048 / 4;
        hipLaunchKernelGGL(fft_1p_zoom_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, zp.as<float>(),
                           frames, zoom);
        SDRGPU_HIP(hipGetLastError());
    }
    return SDRGPU_OK;
}

// a one-pass call's zoom fold inside the launch of the VFO's later stages (fft_1p_tail_fold_kernel)
static int launch_tail_fold(const TailArgs& t, size_t ldsTail, const DevBuf& zp, int frames, float* zoom, hipStream_t s) {
    const int nzb = (int)(((long long)frames * 2048 / 4 + 255) / 256);
    return launch(fft_1p_tail_fold_kernel, t.G + nzb, TAIL_NT_BIG, ldsTail, s, t, zp.as<float>(), frames, zoom);
}

// ---------------------------------------------------------------- 5. two-pass launches that carry a VFO
// fft_vfo_kernel: pass B of framesB frames + pass A and the VFO's stage-1 quarters of framesA frames
template <bool ZM>
static int launch_vfo(FftPlan& p, const float2* scratchB, int framesB, float* outB, float* zoomB, const float2* in,
                      int framesA, float2* scratchA, VfoWork v, hipStream_t s) {
    const int nB = 8 * framesB;
    const int g = nB + 96 * ((framesA + 7) / 8) + (v.hist ? 1 : 0);
    return launch(fft_vfo_kernel<ZM>, g, 512, kLds64k, s, nB, scratchB, framesB, outB, zoomB, in, (long long)p.N, framesA,
                  p.win.as<float>(), p.nz, p.logN, p.tw1.as<float2>(), p.tw2.as<float2>(), p.tfull.as<float2>(), scratchA, v);
}

}  // namespace sdrgpu

using namespace sdrgpu;

struct sdrgpu_fft {
    FftPlan p;
};

// ================================================================== plan
static int fft_upload_window(sdrgpu_fft* h, const float* window, int nz) {
    if (nz <= 0 || nz > h->p.N) { set_error("fft: nz %d out of range (N %d)", nz, h->p.N); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(h->p.device);
    SDRGPU_CHECK(h->p.win.ensure(sizeof(float) * nz));
    SDRGPU_HIP(hipMemcpy(h->p.win.p, window, sizeof(float) * nz, hipMemcpyHostToDevice));
    h->p.nz = nz;
    return SDRGPU_OK;
}

// choose split, chunk, tile shape and kernel form; build the tables this plan needs
static int fft_plan_init(FftPlan& p) {
    if (p.N <= 4096) return make_twiddles(p.tw1, p.N);
    p.N1 = 1 << ((p.logN + 1) / 2);   // N1 >= N2, both <= 1024
    p.N2 = p.N / p.N1;
    const bool is1m = p.N1 == 1024 && p.N2 == 1024;
    // chunk so the pass-A -> pass-B intermediate (+ the input it came from) stays
    // resident in the Infinity Cache: 128 MB of intermediate per chunk (64 and 192-256 MB
    // measured 2-5% slower for 64k with merged launches; 1M: 2.32 vs 2.39 ms at 64 MB)
    long long chunkMB = 128;
    // the 1M plan (N1 = N2 = 1024): 64 MB = 8 frames, two persistent pass-A tiles per workgroup:
    // C2 1.770 -> 1.724 ms (r4u), 64 / 96 / 128 / 256 MB 1.742 / 1.802 / 1.77 / 2.10 (r4v, r4u; 3
    // and 2 interleaved runs); tile counts that are not a multiple of the grid (4 / 6 frames) are slower
    if (is1m) chunkMB = 64;
    if (const char* e = tuning_env("SDRGPU_FFT_CHUNK_MB")) chunkMB = std::max(1, atoi(e));
    p.chunkFrames = std::max(1, (int)((chunkMB << 20) / ((long long)p.N * 8)));
    // 64k (256 x 256): 32 columns / 32 rows per workgroup (256-B pass-A row segments, 128-B
    // pass-B dB segments, 512 threads, 2 workgroups per CU): the merged spectrum launches
    // take 1.44 vs 1.58 ms per 2^28 samples with 16 / 16 (A/B on one box)
    if (p.N1 == 256 && p.N2 == 256) p.sa = 32;
    if (const char* e = tuning_env("SDRGPU_FFT_MERGE")) p.merge = atoi(e);
    // paired-column pass A: +13% on the 1M transform (N1 = 1024), but slower than the
    // one-column kernel at N1 = 256 (64k: 2.05-2.10 vs 1.86 ms per 2^28 samples, A/B on
    // one box), so it is the default only for N1 >= 512
    p.sa2 = p.N1 >= 512 ? 16 : 0;
    // 64k: the one-pass transform (fft_1p_kernel) is the default since r5 (C5 group 1.45 vs 1.63 ms
    // per 2^28 samples for the two-pass launches, A/B on one box); SDRGPU_FFT_1P=0 keeps the latter
    p.onepass = p.N == 65536 ? 2 : 0;
    if (const char* e = tuning_env("SDRGPU_FFT_1P")) p.onepass = atoi(e);
    if (const char* e = tuning_env("SDRGPU_FFT_1P_GRID")) p.grid1p = std::max(0, atoi(e));
    SDRGPU_CHECK(make_twiddles(p.tw1, p.N1));
    SDRGPU_CHECK(make_twiddles(p.tw2, p.N2));
    if (p.N == 65536) SDRGPU_CHECK(make_tab1p(p));
    if (is1m) SDRGPU_CHECK(make_wt(p));
    return make_tfull(p);
}

extern "C" int sdrgpu_fft_create(sdrgpu_fft** out, int device, int fftSize, int nz, int windowType) {
    if (!out) { set_error("fft_create: null handle"); return SDRGPU_EARG; }
    *out = nullptr;
    int logN = 0;
    while ((1 << logN) < fftSize) logN++;
    if (fftSize < 64 || fftSize > (1 << 20) || (1 << logN) != fftSize) {
        set_error("fft_create: size %d must be a power of two in [64, 2^20]", fftSize);
        return SDRGPU_EARG;
    }
    SDRGPU_SET_DEVICE(device);
    sdrgpu_fft* h = new sdrgpu_fft();
    FftPlan& p = h->p;
    p.device = device; p.N = fftSize; p.logN = logN;
    int rc = fft_plan_init(p);
    if (rc >= 0 && hipStreamCreateWithFlags(&p.own, hipStreamNonBlocking) != hipSuccess) {
        set_error("fft_create: hipStreamCreate failed");
        rc = SDRGPU_EHIP;
    }
    if (rc >= 0) rc = sdrgpu_fft_set_window_type(h, windowType, nz);
    if (rc < 0) { sdrgpu_fft_destroy(h); return rc; }
    *out = h;
    return SDRGPU_OK;
}

extern "C" int sdrgpu_fft_set_window(sdrgpu_fft* h, const float* window, int nz) {
    if (!h || !window) { set_error("fft_set_window: null argument"); return SDRGPU_EARG; }
    return fft_upload_window(h, window, nz);
}

extern "C" int sdrgpu_fft_set_window_type(sdrgpu_fft* h, int windowType, int nz) {
    if (!h) { set_error("fft_set_window_type: null handle"); return SDRGPU_EARG; }
    if (nz <= 0 || nz > h->p.N) { set_error("fft: nz %d out of range (N %d)", nz, h->p.N); return SDRGPU_EARG; }
    std::vector<float> w(nz);
    SDRGPU_CHECK(create_window(windowType, w.data(), nz, 1));   // IQFrontEnd::updateFFTSize: centred
    return fft_upload_window(h, w.data(), nz);
}

extern "C" int sdrgpu_fft_size(sdrgpu_fft* h) { return h ? h->p.N : SDRGPU_EARG; }

// Spectrum arithmetic: 0 = fp32 kernels (default), 1 = fp64 interior (fft64.hip: the fp32 window
// product as the reference forms it, then fp64 butterflies, twiddles, |X|^2 and dB, rounded once)
extern "C" int sdrgpu_fft_set_precision(sdrgpu_fft* h, int mode) {
    if (!h || mode < 0 || mode > 1) { set_error("fft_set_precision: bad argument"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    SDRGPU_HIP(hipDeviceSynchronize());   // no call of the plan in flight while its kernels change
    if (mode == 0 && p.f64) {
        fft64_destroy(p.f64);
        p.f64 = nullptr;
    } else if (mode == 1 && !p.f64) {
        SDRGPU_CHECK(fft64_create(&p.f64, p.N));
    }
    return SDRGPU_OK;
}
extern "C" int sdrgpu_fft_get_precision(sdrgpu_fft* h) { return h ? (h->p.f64 ? 1 : 0) : SDRGPU_EARG; }

// The 64k plan's transform: 1 = the one-pass kernel, 0 = the two-pass launches, 2 = per call size (the
// default). Returns the previous mode (2 for every other size, where the call changes nothing).
extern "C" int sdrgpu_fft_set_kernel(sdrgpu_fft* h, int mode) {
    if (!h || mode < 0 || mode > 2) { set_error("fft_set_kernel: bad argument"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    const int prev = p.N == 65536 ? p.onepass : 2;
    if (p.N == 65536) p.onepass = mode;   // (read at call time: calls in flight keep their form)
    return prev;
}

// ================================================================== rows (and zoom rows)
// frames -> dB rows (and, with zoom != nullptr on a zoom_fusable plan, the full-span zoom rows): the launches
static int fft_launch_rows(FftPlan& p, const float2* x, long long frameStride, int frames, float* out, float* zoom,
                           hipStream_t s) {
    if (p.f64) return fft64_execute(p.f64, x, frameStride, frames, p.win.as<float>(), p.nz, out, s);   // (zoom: unfused)
    if (p.N1 == 0) return dispatch_single(p, x, frameStride, frames, out, s);
    if (onepass_ok(p, frames))
        return zoom ? launch_1p<true, false>(p, x, frameStride, frames, out, zoom, VfoWork{}, s, true, p.zpart)
                    : launch_1p<false, false>(p, x, frameStride, frames, out, nullptr, VfoWork{}, s, true, p.zpart);
    const long long zw = p.N / 32;   // zoom row width when fused
    auto zoomAt = [&](long long f0) { return zoom ? zoom + f0 * zw : nullptr; };
    const int nchunks = (frames + p.chunkFrames - 1) / p.chunkFrames;
    if (p.merge && nchunks > 1 && tiles_64k(p))
        return chunk_walk(p, frames, [&](float2* scB, int fB, int nfB, float2* scA, int fA, int nfA) {
            float* ob = out + (long long)fB * p.N;
            const float2* xa = x + (long long)fA * frameStride;
            p.cur = nfB ? scB : scA;   // (the first and the last launch: plain pass A, plain pass B)
            if (!nfB) return dispatch_passA(p, xa, frameStride, nfA, s);
            if (!nfA) return dispatch_passB(p, nfB, ob, s, zoomAt(fB));
            return zoom ? launch_merged<true>(p, scB, nfB, ob, xa, frameStride, nfA, scA, s, zoomAt(fB))
                        : launch_merged<false>(p, scB, nfB, ob, xa, frameStride, nfA, scA, s);
        });
    // 16-B loads need an even frame stride and a 16-B aligned base
    const bool paired = p.sa2 > 0 && (frameStride % 2) == 0 && ((uintptr_t)x & 15) == 0;
    // the intermediate grows with the largest chunk seen (a single-frame drop-in plan holds 0.5 MB)
    SDRGPU_CHECK(p.scratch.ensure((size_t)std::min(p.chunkFrames, frames) * p.N * sizeof(float2)));
    p.cur = p.scratch.as<float2>();
    for (int c = 0; c < nchunks; c++) {
        const int f0 = c * p.chunkFrames;
        const int nf = std::min(p.chunkFrames, frames - f0);
        const float2* xc = x + (long long)f0 * frameStride;
        if (pipe1m_ok(p, paired)) {
            SDRGPU_CHECK(dispatch_1m(p, xc, frameStride, nf, out + (long long)f0 * p.N, s));
            continue;
        }
        if (paired) SDRGPU_CHECK(dispatch_passA2(p, xc, frameStride, nf, s));
        else SDRGPU_CHECK(dispatch_passA(p, xc, frameStride, nf, s));
        SDRGPU_CHECK(dispatch_passB(p, nf, out + (long long)f0 * p.N, s, zoomAt(f0)));
    }
    return SDRGPU_OK;
}
// ... inside the call's timing bracket; returns frames
static int fft_execute(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out, float* zoom,
                       hipStream_t s) {
    SDRGPU_CHECK(time_mark(h->p, 0, s));
    SDRGPU_CHECK(fft_launch_rows(h->p, (const float2*)in, frameStride, frames, out, zoom, s));
    SDRGPU_CHECK(time_mark(h->p, 1, s));
    return frames;
}

// Rows + the waterfall's zoom rows of any width: fft_scaler(0, bw, bw, N, zoomSize).doZoom of every
// row (gui/widgets/fft_scaler.h:27-64: max over the bins [round(f0), round(f0 + N / zoomSize))).
// On the 64k plan with zoomSize = N / 32 the zoom is fused into the last pass's dB store (the rows are
// not read again); any other size, and the fp64 plan, runs the zoom kernel over the rows afterwards.
static int fft_execute_zoom(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out, float* zoomOut,
                            int zoomSize, hipStream_t s) {
    FftPlan& p = h->p;
    if (zoom_fusable(p, zoomSize) && !p.f64) return fft_execute(h, in, frameStride, frames, out, zoomOut, s);
    SDRGPU_CHECK(fft_execute(h, in, frameStride, frames, out, nullptr, s));
    if (!p.zoom || p.zoomSize != zoomSize) {
        if (p.zoom) sdrgpu_zoom_destroy(p.zoom);
        p.zoom = nullptr;
        SDRGPU_CHECK(sdrgpu_zoom_create(&p.zoom, p.device, 0.0, 1.0, 1.0, p.N, zoomSize));
        p.zoomSize = zoomSize;
    }
    SDRGPU_CHECK(sdrgpu_zoom_execute_dev(p.zoom, out, frames, zoomOut, s));
    return frames;
}

extern "C" int sdrgpu_fft_execute_dev(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out,
                                      void* stream) {
    if (!h || !in || !out || frames < 0 || frameStride < 0) { set_error("fft_execute: bad argument"); return SDRGPU_EARG; }
    if (frames == 0) return 0;
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    hipStream_t s = stream ? (hipStream_t)stream : p.own;
    SDRGPU_CHECK(p.order.follow(s));
    OrderScope od(p.order, s);
    return fft_execute(h, in, frameStride, frames, out, nullptr, s);
}

int sdrgpu::fft_execute_owned(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out, hipStream_t s) {
    if (!h || !in || !out || frames < 0 || frameStride < 0) { set_error("fft_execute: bad argument"); return SDRGPU_EARG; }
    if (frames == 0) return 0;
    return fft_execute(h, in, frameStride, frames, out, nullptr, s);
}

extern "C" int sdrgpu_fft_execute_zoom_dev(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out,
                                           float* zoomOut, int zoomSize, void* stream) {
    if (!h || !in || !out || !zoomOut || frames < 0 || frameStride < 0 || zoomSize <= 0 || zoomSize > h->p.N) {
        set_error("fft_execute_zoom: bad argument");
        return SDRGPU_EARG;
    }
    if (frames == 0) return 0;
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    hipStream_t s = stream ? (hipStream_t)stream : p.own;
    SDRGPU_CHECK(p.order.follow(s));
    OrderScope od(p.order, s);
    return fft_execute_zoom(h, in, frameStride, frames, out, zoomOut, zoomSize, s);
}

// ================================================================== the front end's per-block call
int sdrgpu::fft_execute_split(sdrgpu_fft* h, const float2* head, int nh, const float2* body, long long stride, int frames,
                              float* out, const SideCopy& side, hipStream_t s, const VfoStage1* vfo, sdrgpu_block* vfoBlock,
                              void* vfoOut, int* vfoN) {
    if (!h || !body || frames <= 0 || nh < 0 || (nh > 0 && !head)) return SDRGPU_ESTATE;
    FftPlan& p = h->p;
    if (p.f64 || !tiles_64k(p) || frames > p.chunkFrames || nh >= p.nz) return SDRGPU_ESTATE;   // (one chunk)
    SDRGPU_CHECK(p.scratch.ensure((size_t)frames * p.N * sizeof(float2)));
    p.cur = p.scratch.as<float2>();
    SDRGPU_CHECK(time_mark(p, 0, s));
    if (!vfo) {
        SDRGPU_CHECK((launch_passA<256, 32>(p, body, stride, frames, s, head, nh, &side)));
        SDRGPU_CHECK(dispatch_passB(p, frames, out, s));
        SDRGPU_CHECK(time_mark(p, 1, s));
        return frames;
    }
    // pass A + the VFO's stage 1 + its history carry + the tail copy
    const VfoCall v{vfo->a, (int)((((long long)vfo->M + 31) / 32 + 15) / 16)};
    SDRGPU_CHECK(launch(fft_passA_vfo_kernel, 8 * frames + v.blocks + 1 + side_spare(side, 512), 512, kLds64k, s, body, stride,
                        frames, p.win.as<float>(), p.nz, p.N2, p.logN, p.tw1.as<float2>(), p.tfull.as<float2>(), p.cur, head, nh,
                        side, v));
    // pass B + the VFO's later stages (one tail launch's workgroups) where the chain has that form
    TailArgs t;
    size_t ldsTail = 0;
    int tail = vfo_tail_prepare(vfoBlock, *vfo, vfoOut, &t, &ldsTail);
    if (tail < 0) return tail;
    if (tail && (t.NT != TAIL_NT || t.K != TAIL_K)) tail = 0;   // (a big call's workgroups: the later stages run after pass B)
    if (tail) {
        SDRGPU_CHECK(launch(fft_passB_tail_kernel, 8 * frames + t.G, 512, std::max(kLds64k, ldsTail), s, p.cur, frames, p.N1,
                            p.logN, p.tw2.as<float2>(), out, t));
        *vfoN = vfo_tail_commit(vfoBlock, *vfo, t);
        SDRGPU_CHECK(time_mark(p, 1, s));
        return frames;
    }
    SDRGPU_CHECK(dispatch_passB(p, frames, out, s));
    SDRGPU_CHECK(time_mark(p, 1, s));
    const int n = vfo_stage1_finish(vfoBlock, *vfo, vfoOut, s);
    if (n < 0) return n;
    *vfoN = n;
    return frames;
}

// ================================================================== spectrum + one VFO over the same batch
static bool vfo_fusable(const FftPlan& p, float* zoom, int zoomSize) {
    return p.vfoFuse && !p.f64 && tiles_64k(p) && p.nz == p.N && (zoom == nullptr || zoom_fusable(p, zoomSize));
}

// The one-pass group: fft_1p_kernel with the VFO's stage-1 halves, then the VFO's later stages on the
// call's stream (vfo_stage1_finish). With zoom rows and a big-call tail the zoom fold rides in the tail's
// launch instead (launch_tail_fold) -- and in tail-stream mode (sdrgpu_fft_set_tail_stream) that launch runs
// on the tail stream, from this call parity's stage-1 and zoom-partial buffers. *onTail is set when it did.
static int vfo_onepass(FftPlan& p, const float2* x, int frames, float* out, float* zoom, const VfoStage1& st0,
                       sdrgpu_block* vfo, void* vfoOut, hipStream_t s, bool* onTail) {
    VfoStage1 st = st0;
    const bool tmode = p.tailStream && zoom;
    const int b = (int)(p.tcallsT & 1);
    if (tmode) {   // stage 1 writes this call parity's buffer, free once call k - 2's tail is done
        if (p.tdoneRec[b]) SDRGPU_HIP(hipStreamWaitEvent(s, p.tdone[b], 0));
        SDRGPU_CHECK(p.s1T[b].ensure(sizeof(float2) * (size_t)std::max(st.M, 1)));
        st.out = p.s1T[b].p;
        st.a.out = p.s1T[b].p;
    }
    TailArgs t;
    size_t ldsTail = 0;
    int tail = zoom ? vfo_tail_prepare(vfo, st, vfoOut, &t, &ldsTail) : 0;
    if (tail < 0) return tail;
    if (tail && (t.NT != TAIL_NT_BIG || t.K != TAIL_K_BIG)) tail = 0;
    // Here the call takes the tail stream or stays on `s`. ADVICE.md's open race (a tail-stream call followed
    // by a call whose VFO stages run on `s`) starts from this decision; it is unchanged here.
    const bool onT = tmode && tail;
    if (!onT) st = st0;   // (no big-call tail: the VFO's own scratch, everything on `s`)
    DevBuf& zp = onT ? p.zpartT[b] : p.zpart;
    const VfoWork v{st.a, 0, 1};
    SDRGPU_CHECK(time_mark(p, 0, s));
    SDRGPU_CHECK(zoom ? (launch_1p<true, true>(p, x, p.N, frames, out, zoom, v, s, !tail, zp))
                      : (launch_1p<false, true>(p, x, p.N, frames, out, nullptr, v, s, true, zp)));
    SDRGPU_CHECK(time_mark(p, 1, s));
    if (!tail) return vfo_stage1_finish(vfo, st, vfoOut, s);
    const hipStream_t ts = onT ? p.tailStream : s;
    if (onT) {
        SDRGPU_HIP(hipEventRecord(p.gdone[b], s));
        SDRGPU_HIP(hipStreamWaitEvent(ts, p.gdone[b], 0));
    }
    SDRGPU_CHECK(launch_tail_fold(t, ldsTail, zp, frames, zoom, ts));
    if (onT) {
        SDRGPU_HIP(hipEventRecord(p.tdone[b], ts));
        p.tdoneRec[b] = true;
        p.tcallsT++;
        *onTail = true;
    }
    return vfo_tail_commit(vfo, st, t);
}

// The two-pass group (fft_vfo_kernel over the chunk walk): A(0)+V(0); [B(c-1) + A(c)+V(c)] for c = 1..;
// B(last) + the stage's history workgroup. The VFO's later stages (vfo_stage1_finish) need only the stage-1
// outputs, complete once the last pass-A launch is done; they run after the group on the call's stream (on a
// side stream beside the last launch they measured slower: 1.725 vs 1.705 ms, r4i).
static int vfo_twopass(FftPlan& p, const float2* x, int frames, float* out, float* zoom, const VfoStage1& st,
                       sdrgpu_block* vfo, void* vfoOut, hipStream_t s) {
    const long long zw = p.N / 32;
    VfoWork v{st.a, 0, 0};
    SDRGPU_CHECK(time_mark(p, 0, s));
    SDRGPU_CHECK(chunk_walk(p, frames, [&](float2* scB, int fB, int nfB, float2* scA, int fA, int nfA) {
        if (nfA) v.frame0 = fA;
        v.hist = !nfA;
        float* ob = nfB ? out + (long long)fB * p.N : nullptr;
        float* zb = nfB && zoom ? zoom + fB * zw : nullptr;
        const float2* xa = nfA ? x + (long long)fA * p.N : nullptr;
        return zoom ? launch_vfo<true>(p, scB, nfB, ob, zb, xa, nfA, scA, v, s)
                    : launch_vfo<false>(p, scB, nfB, ob, zb, xa, nfA, scA, v, s);
    }));
    SDRGPU_CHECK(time_mark(p, 1, s));
    return vfo_stage1_finish(vfo, st, vfoOut, s);
}

// Spectrum (+ the waterfall's zoom rows) + one RxVFO over the same device batch of back-to-back
// frames (fftRate = fs / N: the IQFrontEnd's reshaper keeps every sample, iq_frontend.h:56-60), the
// VFO reading the batch in place like every consumer of the front end's splitter
// (iq_frontend.cpp:15-52). On the 64k plan with the VFO's D = 32 first stage (the RxVFO's plan_256
// at 61.44 MS/s) the batch is read from HBM once: the stage runs inside the spectrum launches
// (vfo_onepass / vfo_twopass) and only the VFO's later stages run after them. Otherwise: the spectrum
// launch group, then the VFO. Returns the VFO's output count (vfoOut).
extern "C" int sdrgpu_fft_execute_zoom_vfo_dev(sdrgpu_fft* h, const void* in, int frames, float* out, float* zoomOut,
                                               int zoomSize, sdrgpu_block* vfo, void* vfoOut, void* stream) {
    if (!h || !in || !out || !vfo || !vfoOut || frames < 0 || (zoomOut && (zoomSize <= 0 || zoomSize > h->p.N))) {
        set_error("fft_execute_vfo: bad argument");
        return SDRGPU_EARG;
    }
    FftPlan& p = h->p;
    const long long count = (long long)frames * p.N;
    if (count > 0x7fffffffLL) { set_error("fft_execute_vfo: %lld samples per call (max 2^31 - 1)", count); return SDRGPU_EARG; }
    // back-to-back frames: the spectrum must cover every sample the VFO consumes, on one device
    if (p.nz != p.N) { set_error("fft_execute_vfo: plan nz %d != N %d (frames must be back to back)", p.nz, p.N); return SDRGPU_EARG; }
    if (!vfo->impl) { set_error("fft_execute_vfo: null VFO block handle"); return SDRGPU_EARG; }
    if (vfo->impl->device != p.device) {
        set_error("fft_execute_vfo: VFO on device %d, spectrum plan on device %d", vfo->impl->device, p.device);
        return SDRGPU_EARG;
    }
    if (frames == 0) return 0;
    SDRGPU_SET_DEVICE(p.device);
    hipStream_t s = stream ? (hipStream_t)stream : p.own;
    SDRGPU_CHECK(p.order.follow(s));
    OrderScope od(p.order, s);
    // tail-stream mode: the VFO's work of a call ends on the tail stream; its next call on `s` needs
    // only what `s` itself ordered (stage 1's history), so a VFO last used by this plan's tail is
    // not waited for here (that wait would serialise the overlap)
    const bool tmode = p.tailStream && zoomOut && p.tailStream != s;
    if (!(tmode && vfo->impl->order.last == p.tailStream)) SDRGPU_CHECK(vfo->impl->order.follow(s));
    OrderScope ov(vfo->impl->order, tmode ? p.tailStream : s);
    VfoStage1 st;
    const int fuse = vfo_fusable(p, zoomOut, zoomSize) ? vfo_stage1_prepare(vfo, in, (int)count, &st) : 0;
    if (fuse < 0) return fuse;
    bool onTail = false;
    int n;
    if (fuse) {
        n = onepass_ok(p, frames) ? vfo_onepass(p, (const float2*)in, frames, out, zoomOut, st, vfo, vfoOut, s, &onTail)
                                  : vfo_twopass(p, (const float2*)in, frames, out, zoomOut, st, vfo, vfoOut, s);
    } else {
        n = zoomOut ? fft_execute_zoom(h, in, p.N, frames, out, zoomOut, zoomSize, s)
                    : fft_execute(h, in, p.N, frames, out, nullptr, s);
        if (n >= 0) n = block_run_owned(vfo, in, (int)count, vfoOut, s);
    }
    if (n >= 0 && tmode && !onTail) {
        // (this call ran everything on `s`: the tail stream's consumers wait for it)
        SDRGPU_HIP(hipEventRecord(p.gdone[0], s));
        SDRGPU_HIP(hipStreamWaitEvent(p.tailStream, p.gdone[0], 0));
    }
    return n;
}

extern "C" int sdrgpu_fft_execute_vfo_dev(sdrgpu_fft* h, const void* in, int frames, float* out, sdrgpu_block* vfo,
                                          void* vfoOut, void* stream) {
    return sdrgpu_fft_execute_zoom_vfo_dev(h, in, frames, out, nullptr, 0, vfo, vfoOut, stream);
}

extern "C" int sdrgpu_fft_set_tail_stream(sdrgpu_fft* h, void* stream) {
    if (!h) { set_error("fft_set_tail_stream: null handle"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    if (p.tailStream && p.tailStream != (hipStream_t)stream)   // tails in flight keep their buffers until done
        for (int b = 0; b < 2; b++)
            if (p.tdoneRec[b]) SDRGPU_HIP(hipEventSynchronize(p.tdone[b]));
    if (stream && !p.gdone[0])
        for (int b = 0; b < 2; b++) {
            SDRGPU_HIP(hipEventCreateWithFlags(&p.gdone[b], hipEventDisableTiming));
            SDRGPU_HIP(hipEventCreateWithFlags(&p.tdone[b], hipEventDisableTiming));
        }
    if ((hipStream_t)stream != p.tailStream) {
        p.tdoneRec[0] = p.tdoneRec[1] = false;
        p.tcallsT = 0;
    }
    p.tailStream = (hipStream_t)stream;
    return SDRGPU_OK;
}

// ================================================================== timing, host-pointer call, teardown
// Timing of the spectrum launch group (HIP events on the call's stream; off by default)
extern "C" int sdrgpu_fft_set_timing(sdrgpu_fft* h, int on) {
    if (!h) { set_error("fft_set_timing: null handle"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    if (on && !p.tev[0][0])
        for (auto& e : p.tev) {
            SDRGPU_HIP(hipEventCreate(&e[0]));
            SDRGPU_HIP(hipEventCreate(&e[1]));
        }
    p.timing = on != 0;
    p.tcalls = 0;
    return SDRGPU_OK;
}
// the group times (ms) of the last min(n, calls, 256) timed calls, oldest first; waits for them
extern "C" int sdrgpu_fft_group_times(sdrgpu_fft* h, float* ms, int n) {
    if (!h || !ms || n < 0) { set_error("fft_group_times: bad argument"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    const long long k = std::min<long long>({(long long)n, p.tcalls, (long long)FftPlan::kTimed});
    for (long long i = 0; i < k; i++) {
        auto& e = p.tev[(p.tcalls - k + i) % FftPlan::kTimed];
        SDRGPU_HIP(hipEventSynchronize(e[1]));
        SDRGPU_HIP(hipEventElapsedTime(&ms[i], e[0], e[1]));
    }
    return (int)k;
}

extern "C" int sdrgpu_fft_logmag(sdrgpu_fft* h, const void* in, float* out) {
    if (!h || !in) { set_error("fft_logmag: null argument"); return SDRGPU_EARG; }
    FftPlan& p = h->p;
    SDRGPU_SET_DEVICE(p.device);
    size_t inB = sizeof(float2) * p.nz, outB = sizeof(float) * p.N;
    SDRGPU_CHECK(p.pin_in.ensure(inB));
    SDRGPU_CHECK(p.dev_in.ensure(inB));
    SDRGPU_CHECK(p.dev_out.ensure(outB));
    // registered host buffers (sdrgpu_host_register) are DMA'd directly, others staged
    const void* src = in;
    if (!host_pinned(in, inB)) {
        std::memcpy(p.pin_in.p, in, inB);
        src = p.pin_in.p;
    }
    SDRGPU_HIP(hipMemcpyAsync(p.dev_in.p, src, inB, hipMemcpyHostToDevice, p.own));
    SDRGPU_CHECK(sdrgpu_fft_execute_dev(h, p.dev_in.p, p.nz, 1, p.dev_out.as<float>(), p.own));
    if (out && host_pinned(out, outB)) {
        SDRGPU_HIP(hipMemcpyAsync(out, p.dev_out.p, outB, hipMemcpyDeviceToHost, p.own));
        SDRGPU_HIP(hipStreamSynchronize(p.own));
    } else if (out) {
        SDRGPU_CHECK(p.pin_out.ensure(outB));
        SDRGPU_HIP(hipMemcpyAsync(p.pin_out.p, p.dev_out.p, outB, hipMemcpyDeviceToHost, p.own));
        SDRGPU_HIP(hipStreamSynchronize(p.own));
        std::memcpy(out, p.pin_out.p, outB);
    } else {
        SDRGPU_HIP(hipStreamSynchronize(p.own));
    }
    return p.N;
}

extern "C" int sdrgpu_fft_destroy(sdrgpu_fft* h) {
    if (!h) return SDRGPU_OK;
    (void)hipSetDevice(h->p.device);
    for (int b = 0; b < 2; b++) {
        if (h->p.tdoneRec[b]) (void)hipEventSynchronize(h->p.tdone[b]);
        if (h->p.gdone[b]) (void)hipEventDestroy(h->p.gdone[b]);
        if (h->p.tdone[b]) (void)hipEventDestroy(h->p.tdone[b]);
    }
    if (h->p.own) (void)hipStreamDestroy(h->p.own);
    if (h->p.zoom) sdrgpu_zoom_destroy(h->p.zoom);
    if (h->p.f64) fft64_destroy(h->p.f64);
    for (auto& e : h->p.tev)
        for (auto& ev : e)
            if (ev) (void)hipEventDestroy(ev);
    delete h;
    return SDRGPU_OK;
}

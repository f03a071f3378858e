// Spectrum device code, one-pass side: the 64k one-pass kernel (fft_1p_kernel), its zoom fold and the
// launch that folds beside the VFO's later stages (fft_1p_tail_fold_kernel). Host side: fft.hip.
#pragma once
#include "fft_passes.h"

namespace sdrgpu {

// ---- one-pass 64k spectrum: no intermediate leaves the CU ----------------------------------------
// N = 65536 as four 16,384-point transforms (one radix-4 decimation-in-frequency step). Item (f, r)
// computes the bins 4 m + r of frame f:
//   X[4 m + r] = sum_{n < M} W_M^(n m) y_r[n],   y_r[n] = W_N^(n r) sum_{j < 4} W_4^(j r) w[n + M j] x[n + M j],
// M = 16384. The 16k transform is M = 32 x 32 x 16 on one CU (512 threads, one workgroup per CU):
//   stage 1 (registers): thread t holds y_r[t + 512 i], i < 32, straight from its loads (the four
//     quarters combined as they arrive); a radix-32 DFT over i and the twiddle W_M^(t k2) W_N^(t r)
//     = W_N^(t (4 k2 + r)) give A[t][k2];
//   stage 2 (LDS): per (k2, t0), a radix-32 DFT over t1 of A[t0 + 16 t1][k2], twiddle W_512^(t0 q1);
//   stage 3 (LDS): per (k2, q1), a radix-16 DFT over t0 -> Y[k2 + 32 q1 + 1024 q2], dB, store.
// A frame's two workgroups (quarters 0-1 and 2-3, the pair's bins 4 m + r0, 4 m + r0 + 1 adjacent so
// the dB rows leave as 8-byte pairs) sit on one XCD (blocks of 8 frames under round-robin dispatch, for
// speed only), so the frame is fetched from HBM once per reader and its second read is mostly served by
// that XCD's L2. The rows stream into LDS by LDS-DMA through a wave-private ring of row sets (below: every wave
// fetches what its own threads read, so the row loop has no barrier; round 15, profiles/r15/README.md). The default
// since round 5 (C5 group 1.51 ms, 20.9 B/sample of fabric traffic, against 1.63 ms and 30.4 B for the
// two-pass launches). Rejected forms: one item per
// workgroup (1.89 ms), a persistent software-pipelined quarter-per-workgroup walk (2.06 ms, spills), the
// VFO half inside the row loop (1.60-1.91 ms).
// Since round 7 the launch is persistent: the co-resident workgroups (one per CU, a multiple of 16) walk the
// items with a stride of the grid, stage the twiddle tables once, and issue each next item's first ring row
// sets under the current item's last dft16, dB and store burst; nothing is carried between items in
// registers and an item's arithmetic is unchanged, so the bits are those of one item per workgroup
// (SDRGPU_FFT_1P_GRID=0; profiles/r7/README.md).
// LDS image: 32 rows k2 of 544 used float2 (stage 1: column pad16(t); stage 2: column 17 q1 +
// (t0 ^ ((k2 >> 1) & 15))), row stride 560 (= 16 mod 32): every stage-2/3 access of a half-wave hits
// 32 distinct 8-byte bank pairs.
namespace op1 {
constexpr int M = 16384;
constexpr int RS = 560;                 // LDS row stride (float2)
constexpr int TW512 = 32 * RS;          // W_512^(t0 q1) at [q1][t0]
constexpr int W128 = TW512 + 512;       // W_128^(r i), i < 32
constexpr int W128D = (W128 + 64) * 8;   // (bytes) fp64 W_128^(r i), r = r0, r0 + 1, i < 32
constexpr int PHI = W128D + 64 * 16;    // (bytes) the walk's coarse NCO phasors of the fused VFO, 512 float2
constexpr int LDS_BYTES = PHI + 512 * 8;
constexpr int TAB = 512 + 128;          // device table: [q1][t0] W_512^(t0 q1), [r][i] W_128^(r i)
constexpr int TAB64 = 2048 + 128;       // fp64 table: W_N^m (m < 2048), [r][i] W_128^(r i)
}

// x w, rounded on its own: never contracted into the radix-4 adds that follow (left to the compiler,
// whether it fused x w + u into one fma differed between kernel instantiations, so the one-pass rows
// with and without the fused VFO differed in the last bit)
__device__ __forceinline__ float2 wmul(float2 x, float w) {
#pragma clang fp contract(off)
    return make_float2(x.x * w, x.y * w);
}

// 32-point DFT as 2 x 16 (even / odd halves), natural order in and out
__device__ __forceinline__ void dft32(float2* v) {
    constexpr float C[16] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
                             0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f,
                             0.19509032201612826785f, 0.0f, -0.19509032201612826785f, -0.38268343236508977173f,
                             -0.55557023301960222474f, -0.70710678118654752440f, -0.83146961230254523708f,
                             -0.92387953251128675613f, -0.98078528040323044913f};
    float2 e[16], o[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        e[i] = v[2 * i];
        o[i] = v[2 * i + 1];
    }
    dft16(e);
    dft16(o);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        float2 t = o[k];
        if (k == 8) t = mul_negi(t);
        else if (k) t = cmul(t, make_float2(C[k], -C[(k + 8) & 15] * (k < 8 ? -1.0f : 1.0f)));   // W_32^k
        v[k] = cadd(e[k], t);
        v[k + 16] = csub(e[k], t);
    }
}

// Stage-1 twiddles W_N^(t (4 k2 + r)) by an fp64 recurrence W_N^(t r) (W_N^(4 t))^k2 from two values of
// an fp64 table, rounded once (against one exact table value each, 128 KB per item from L2: 1.942 ->
// 1.893 ms, r41pb).
constexpr int k1pSlots = 5;   // LDS-DMA ring slots (24 KiB row sets) in the image region
constexpr int k1pPB = 2;   // (PAD) sample rows per load batch: 4 PB loads of x and of w, two batches in flight
#ifndef SDRGPU_1P_ABL
#define SDRGPU_1P_ABL 0   // (ablation builds, wrong results, timing only) 1: no loads, 2: no transforms, 4: no VFO,
                          // 8: fp32 stage-1 twiddles, 16: no dB / stores (32, round 15 only: the shared row ring without
                          // its 32 barriers, group 1.449 -> 1.383 ms, the ceiling of the wave-private ring; profiles/r15),
                          // 64: the VFO half's round 0 reads the same rows of a fixed frame of the call (hot in L2: the
                          // ceiling of warming round 0's lines), 128: the VFO segments' coarse phasor a constant (the
                          // ceiling of forming it outside the walk); profiles/r20
#endif
// Decided A/Bs, kept forms only: the ring's first k1pSlots - 1 row sets are issued before the VFO half, so they
// land while it computes (C5 group 1.518 -> 1.499 ms, same bits, r6g); quarter r0 + 1's W_128 products run
// during quarter r0's stage-3 reads (C5 group 1.4748 / 1.4833 vs 1.4782 / 1.4880 ms, r7t, r7u, same bits); every
// wave DMAs the bytes its own threads read, so the ring loop has no barrier, and holds its lanes' offsets over the
// loop (C5 group 1.451 -> 1.419 ms, same bits; recomputed per row set 1.427-1.439 ms; r15c, r15d). Measured and not
// kept (profiles/r15): stage 2 without the barrier between its reads and writes, which orders nothing across waves
// (1.435 vs 1.448 and 1.435 vs 1.421 ms alone, 1.409 vs 1.419 ms beside the ring: inside the run-to-run spread).
// Round 20 (profiles/r20): the VFO segments' coarse NCO phasors come from an LDS table formed once per launch
// (C5 group 1.418 -> 1.397 and 1.398 -> 1.366 ms, same bits, r20f, r20g). Measured and not kept: the next item's VFO
// round-0 lines touched from the prefetch (1.472 ms at a 128-B lane stride, 1.485 ms at 64 B, vs 1.447 ms, r20c).
#ifdef SDRGPU_1P_TIMING   // (measurement builds) per-item phase stamps of wave 0: slots 0-7 and 9 (the first
                          // ring wait) s_memtime; slot 8 the CU's identity, XCC_ID << 32 | HW_ID
constexpr int k1pStamps = 10;
__device__ unsigned long long g_1p_t[16384 * k1pStamps];
#define T1P_AT(item, k)                                                                               \
    do {                                                                                              \
        if (threadIdx.x == 0 && (item) < 16384) g_1p_t[(item) * k1pStamps + (k)] = clock64();         \
    } while (0)
#define T1P_CU(item)                                                                                  \
    do {                                                                                              \
        if (threadIdx.x == 0 && (item) < 16384) {                                                     \
            unsigned hw, xcc;                                                                         \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" \
                         : "=s"(hw), "=s"(xcc));                                                      \
            g_1p_t[(item) * k1pStamps + 8] = (unsigned long long)xcc << 32 | hw;                       \
        }                                                                                             \
    } while (0)
#else
#define T1P_AT(item, k) do {} while (0)
#define T1P_CU(item) do {} while (0)
#endif
#define T1P(k) T1P_AT(b, k)
struct NcoPhiConst {   // (ablation 128)
    __device__ __forceinline__ float2 operator()(const FirArgs&, long long) const { return make_float2(0.6f, 0.8f); }
};
// The VFO half's geometry as the walk needs it: item (frame g, quarter pair p) runs the segments
// 64 (frame0 + g) + 32 p .. + 31 (vfo_half_block), segment s starts at input index offset0 - H + 32 * 32 s
// (fir_rows_segment: RS = 32 outputs of the D = 32 decimator) and forms its phasor at its first 32 samples.
namespace op1 {
constexpr int VSEG = 32 * 32;   // a segment's step in input samples
// coarse indices (nco_value.h: input index >> NCO_LO_BITS, an arithmetic shift: the floor, inside the history
// too) an item's 32 segment starts can take: the starts span 31 VSEG + 32 samples
constexpr int PHI_E = ((31 * VSEG + 31) >> NCO_LO_BITS) + 2;
constexpr int PHI_ITEMS = 512 / PHI_E;   // items of a walk the table holds (one entry per thread of the prologue)
// coarse index of an item's first entry
__device__ __forceinline__ long long vfo_item_j0(const FirArgs& a, int frame0, int g, int p) {
    return ((long long)a.offset0 - a.H + ((long long)(frame0 + g) * 64 + p * 32) * VSEG) >> NCO_LO_BITS;
}
}
// The coarse phasors of an item from the workgroup's LDS table (fft_1p_kernel's prologue), or formed in place for
// the items of a walk beyond the table (workgroup-uniform)
struct NcoPhiLds {
    unsigned base;   // LDS byte address of the item's entry of coarse index 0 (entries of 8 bytes; modulo 2^32)
    bool tab;
    __device__ __forceinline__ float2 operator()(const FirArgs& a, long long j) const {
        if (tab) {
            const auto* e = (const __attribute__((address_space(3))) float*)(size_t)(base + 8u * (unsigned)j);
            return make_float2(e[0], e[1]);
        }
        return nco_phi(a.ncoTheta0, a.ncoW, j);
    }
};
// (the quarter pair of a workgroup: its VFO share, 32 segments of the frame's 64)
template <class PHI = NcoPhiInline>
__device__ __forceinline__ void vfo_half_block(const VfoWork& v, int g, int p, const PHI& coarse = PHI{}) {
    int u = threadIdx.x;
    asm volatile("" : "+v"(u));   // (laundered: nothing of a segment's addressing is hoisted out of the item walk)
    const int lane = u & 63, wave = u >> 6;
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const long long seg = (long long)(v.frame0 + g) * 64 + p * 32 + k * 16 + wave * 2 + (lane >> 5);
#if SDRGPU_1P_ABL & 64
        // round 0 from frame 1 of the call, which every workgroup reads: the same offsets in the frame (frame 0
        // would put the first segment's halo in front of the buffer)
        FirArgs a = v.a;
        if (k == 0 && v.frame0 + g > 1) a.in = reinterpret_cast<const float2*>(a.in) - (long long)(v.frame0 + g - 1) * 65536;
#else
        const FirArgs& a = v.a;
#endif
        if constexpr (SDRGPU_1P_ABL & 128) fir_rows_segment<32, 5, true, false, 32, 32, true>(a, seg, lane, NcoPhiConst{});
        else fir_rows_segment<32, 5, true, false, 32, 32, true>(a, seg, lane, coarse);
    }
}
// (one struct, at offset 0 of the kernel's argument segment: every item of the walk reads what it needs of it
// through a laundered pointer to that segment, as scalar loads. Plain arguments are loaded once in front of the
// walk and stay live through all of it, ~40 SGPRs with the VFO's, and the kernel spills)
struct Args1p {
    const float2* in;
    long long frameStride;
    int frames;
    const float* win;
    int nz;
    const float2* tab;
    const double2* tab64;
    float* out;
    float* zpart;
    VfoWork v;
};
template <bool ZM, bool VFO, bool PAD>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1))) void fft_1p_kernel(Args1p ka) {
    using op1::M;
    using op1::RS;
    using op1::TW512;
    using op1::W128;
    extern __shared__ __attribute__((aligned(16))) float2 lds[];
    if constexpr (VFO) {
        if (ka.v.hist && blockIdx.x == gridDim.x - 1) {   // the stage's history carry (fir.h:80)
            (void)fir_hist_block<float2, true, false>(ka.v.a);
            return;
        }
    }
    // The workgroup walks the items b = blockIdx.x + n G (G item workgroups, a multiple of 16; launch_1p), item
    // b = quarters r0, r0 + 1 of frame f = 8 (b >> 4) + (b & 7), r0 = 2 ((b >> 3) & 1): along the walk r0 and
    // b & 7 (the XCD group the workgroup shares with its partner b +- 8) stay, and f only grows. What does not
    // depend on the frame is set up once, here: the twiddle tables in LDS (the image and the ring slots end
    // below them), the window's buffer resource and the wave's DMA pieces.
    const int frames = ka.frames, G = (int)gridDim.x - (VFO && ka.v.hist ? 1 : 0), items = 16 * ((frames + 7) >> 3);
    int p = (blockIdx.x >> 3) & 1;
    constexpr bool kDma = !PAD && !(SDRGPU_1P_ABL & 1);   // whole frames: the LDS-DMA row ring below
    constexpr bool kVfo = VFO && !(SDRGPU_1P_ABL & 4);
    constexpr bool kTab = kVfo && kDma && !(SDRGPU_1P_ABL & 128);   // the coarse-phasor table (below)
    // Index arithmetic is recomputed from a laundered thread index where it is used: left alone, the
    // compiler hoists the loop-invariant load / LDS / store addresses and spills them.
    auto tid = [] {
        int u = threadIdx.x;
        asm volatile("" : "+v"(u));
        return u;
    };
    {
        const int t = threadIdx.x;
        lds[TW512 + t] = ka.tab[t];
        if (t < 64) reinterpret_cast<double2*>(reinterpret_cast<char*>(lds) + op1::W128D)[t] = ka.tab64[2048 + 32 * (2 * p + (t >> 5)) + (t & 31)];
        // The VFO segments' coarse NCO phasors (nco_phi: an fp64 division, rint and sincos) depend on the call and
        // the item's frame only, and an item's 32 segments take at most PHI_E of them: thread t forms entry t % PHI_E
        // of item t / PHI_E of this workgroup's walk, once per launch, instead of every wave forming its own twice
        // per item (the same expression, so the same bits; round 20, profiles/r20/README.md).
        if constexpr (kTab) {
            const int n = t / op1::PHI_E, bn = (int)blockIdx.x + n * G;
            if (n < op1::PHI_ITEMS && bn < items)
                reinterpret_cast<float2*>(reinterpret_cast<char*>(lds) + op1::PHI)[t] =
                    nco_phi(ka.v.a.ncoTheta0, ka.v.a.ncoW,
                            op1::vfo_item_j0(ka.v.a, ka.v.frame0, 8 * (bn >> 4) + (bn & 7), p) + (t - n * op1::PHI_E));
        }
    }
    __syncthreads();   // (the tables staged: an item's W_128 products read them in front of its first barrier)
    const unsigned lim = PAD ? (unsigned)ka.nz : 65536u;     // (PAD: range-checked loads, 0 past nz)
    const __amdgpu_buffer_rsrc_t rw = brsrc(ka.win, lim * 4u);
    // Whole frames: the rows stream into LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave
    // instruction, 16 B per lane, no VGPRs) through a ring of k1pSlots row sets in the (still
    // unused) image region. A row set = row i of the four quarters: x 4 x 4 KiB, w 4 x 2 KiB = 24
    // wave instructions, 3 per wave. 8- and 4-byte register loads reached ~25 GB/s per CU here
    // (the r5 phase stamps: the load phase was 60% of a workgroup's life); 16-B accesses are the
    // L2 path's full rate. The ring is wave-private: a DMA's LDS destination is wave-uniform but its
    // source address is per lane, so wave v fetches exactly the samples 64 v .. 64 v + 63 of row i that
    // its own threads read, into its own 3-KiB region of the slot: x of quarter j at 512 j (two
    // instructions: lanes 0-31 quarter 2 e, lanes 32-63 quarter 2 e + 1, 16 B = 2 samples per lane), w of
    // quarter j at 2048 + 256 j (one instruction: lanes 16 j .. 16 j + 15, 16 B = 4 values per lane).
    // Nothing a wave reads was fetched by another wave, so the loop has no barrier (it had one per row
    // set, where all eight waves waited for the slowest of 24 DMAs): the wave waits for its own pieces
    // of row set i (counted vmcnt: the younger row sets stay in flight), issues row set i + k1pSlots - 1
    // into its region of slot i - 1, then every thread reads its sample of the four quarters (ds_read_b64
    // at 8 lane, _b32 at 4 lane of a region: consecutive addresses, conflict-free) and combines.
    constexpr int S = k1pSlots, SLOT = 24576, WREG = SLOT / 8;
    typedef __attribute__((address_space(3))) char lchar;
    lchar* const lds3 = (lchar*)lds;
    unsigned ldsBase = (unsigned)(size_t)lds3;
    int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // gb: the wave's 3 row pointers of an item (x of quarters 0-1, of quarters 2-3, w), at its 64 samples of row 0
    // (the geometry is scalar arithmetic on the laundered wave index where it is used)
    const char* gb[3];
    auto set_rows = [&](const float2* xf, const float* w) {   // (the frame base is all of the ring that depends on the item)
        gb[0] = reinterpret_cast<const char*>(xf + 64 * wave);
        gb[1] = reinterpret_cast<const char*>(xf + 2 * M + 64 * wave);
        gb[2] = reinterpret_cast<const char*>(w + 64 * wave);
    };
    // a lane's byte offsets in a piece: x, two 512-B runs a quarter apart; w, four 256-B runs a quarter apart
    auto lane_offs = [&](unsigned& xo, unsigned& wo) {
        const unsigned lane = (unsigned)(tid() & 63);
        xo = (lane >> 5) * (unsigned)(M * 8) + (lane & 31u) * 16u;
        wo = (lane >> 4) * (unsigned)(M * 4) + (lane & 15u) * 16u;
    };
    // LDS-DMA in inline asm: the compiler neither counts it (the waits below are explicit) nor
    // drains it with a vmcnt(0) before every LDS read it cannot prove disjoint (it did with the
    // builtin: no row set stayed in flight); M0 set and restored in the same statement
    // (the row pointers advance by one row step per row set, laundered: left alone, the compiler
    // precomputes all 96 pointers and spills them to VGPR lanes)
    auto dma_at = [&](auto ic, unsigned xo, unsigned wo) {
        constexpr int i = decltype(ic)::value;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const char* src = gb[e] + (e < 2 ? xo : wo);
            gb[e] += e < 2 ? 512 * 8 : 512 * 4;
            asm volatile("" : "+s"(gb[e]));
            const unsigned dst = __builtin_amdgcn_readfirstlane(ldsBase + (unsigned)((i % S) * SLOT + 1024 * e) + (unsigned)(WREG * wave));
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
        }
    };
    auto dma = [&](auto ic) {   // (outside the ring loop: the lane's offsets from the laundered thread index, where they are used)
        unsigned xo, wo;
        lane_offs(xo, wo);
        dma_at(ic, xo, wo);
    };
    // Cross-item prefetch: once an item's last image reads are done (stage 3 of quarter r0 + 1, behind a
    // barrier of their own), the next item's first S - 1 row sets are issued into the ring, so they fly
    // under this item's last dft16, dB and store burst instead of behind the next item's first instruction.
    bool pre = false;   // (workgroup-uniform) this item's first S - 1 row sets were issued by the previous item
    int nItem = 0;      // the item's place in the walk: its entries of the coarse-phasor table
#pragma unroll 1
    for (int b = blockIdx.x; b < items; b += G, nItem++) {
        // (per-item index math from laundered values, the workgroup's constants included: left alone, the compiler
        // hoists what the items share out of the walk -- the ring's 96 slot addresses, the VFO segments' and the
        // image's addressing -- and spills it)
        asm volatile("" : "+s"(b), "+s"(p));
        if constexpr (kDma) {
            asm volatile("" : "+s"(ldsBase), "+s"(wave));
        }
        typedef const __attribute__((address_space(4))) char kchar;
        kchar* kp = (kchar*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const Args1p& ia = *reinterpret_cast<const Args1p*>((const char*)kp);   // (the arguments, read per item)
        const float2* __restrict__ in = ia.in;
        const long long frameStride = ia.frameStride;
        const float* __restrict__ win = ia.win;
        const double2* __restrict__ tab64 = ia.tab64;
        float* __restrict__ out = ia.out;
        float* __restrict__ zpart = ia.zpart;
        const VfoWork& v = ia.v;
        const int f = 8 * (b >> 4) + (b & 7), r0 = 2 * p;
        lchar* l3 = lds3;
        asm volatile("" : "+s"(l3));
        float2* const lds = reinterpret_cast<float2*>((char*)l3);   // (the image and the tables, per item as well)
        // stage 1: y_r for r = r0 (even) and r0 + 1 (odd) from the four quarters: y_r = A_r + W_4^r q_r with
        // A_r = u0 + s_r u2, q_r = u1 + s_r u3, s_r = (-1)^r; W_4^r in {1, -i, -1, i} as (fx, fy), one of
        // them 0, the other +-1 (exact products). The pair's bins 4 m + r0, 4 m + r0 + 1 are adjacent: the
        // dB rows leave as 8-byte pairs.
        // (the signs from the laundered p, per item: kept across the walk they are VGPRs, and spilled)
        const float fxa = p ? -1.0f : 1.0f, fyb = p ? 1.0f : -1.0f;   // W_4^r0 = (fxa, 0), W_4^(r0+1) = (0, fyb)
        auto combine2 = [&](const float2 (&u)[4], float2& ya, float2& yb) {
            const float2 aa = cadd(u[0], u[2]), qa = cadd(u[1], u[3]), ab = csub(u[0], u[2]), qb = csub(u[1], u[3]);
            ya = make_float2(fmaf(fxa, qa.x, aa.x), fmaf(fxa, qa.y, aa.y));     // aa + W_4^r0 qa (exact products)
            yb = make_float2(fmaf(-fyb, qb.y, ab.x), fmaf(fyb, qb.x, ab.y));    // ab + W_4^(r0+1) qb
        };
        if (f >= frames) {   // (padding of the last group of 8 frames; f is workgroup-uniform and only grows)
            if constexpr (PAD) break;
            continue;
        }
        T1P(0);
        T1P_CU(b);
        // the frame's first reader (HBM): half of the VFO's stage 1. (Measured and rejected, r5: the VFO
        // inside the row loop -- from the LDS ring, 1.91 ms; as two batches of segments right after the
        // ring fetched their lines, 1.60 ms; after the loop / between the transforms, spilled)
        if constexpr (kVfo && !kDma) vfo_half_block(v, f, p);
        T1P(1);
        const __amdgpu_buffer_rsrc_t rx = brsrc(in + (long long)f * frameStride, lim * 8u);
        constexpr int PB = k1pPB, NB = 32 / PB;
        float2 za[32], zb[32];
        float2 xv[2][PB][4];   // the load ring: two batches of PB sample rows x 4 quarters
        float wv[2][PB][4];
        auto issue = [&](auto bbc) {
            constexpr int bb = decltype(bbc)::value;
            const int t = tid();
#pragma unroll
            for (int ii = 0; ii < PB; ii++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int n0 = 512 * (PB * bb + ii) + M * j;
                    if constexpr (PAD) {   // the offset in the per-lane part: the range check ignores soffset
                        xv[bb & 1][ii][j] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rx, (t + n0) * 8, 0, 0));
                        wv[bb & 1][ii][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, (t + n0) * 4, 0, 0));
                    } else {               // the row offset rides in soffset
                        xv[bb & 1][ii][j] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rx, t * 8, n0 * 8, 0));
                        wv[bb & 1][ii][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, t * 4, n0 * 4, 0));
                    }
                }
        };
        // combine batch bb into za / zb, then reuse its ring slot for batch bb + 2
        auto step = [&](auto bbc) {
            constexpr int bb = decltype(bbc)::value;
#pragma unroll
            for (int ii = 0; ii < PB; ii++) {
                float2 u[4];
#pragma unroll
                for (int j = 0; j < 4; j++) u[j] = wmul(xv[bb & 1][ii][j], wv[bb & 1][ii][j]);
                combine2(u, za[PB * bb + ii], zb[PB * bb + ii]);

            }
            if constexpr (bb + 2 < NB) issue(std::integral_constant<int, bb + 2>{});
            __builtin_amdgcn_sched_barrier(0);
        };
        if constexpr (SDRGPU_1P_ABL & 1) {
#pragma unroll
            for (int i = 0; i < 32; i++) {
                za[i] = make_float2((float)(tid() + i), (float)i);
                zb[i] = make_float2((float)i, (float)(tid() - i));
            }
        } else if constexpr (PAD) {   // zero-padded or unaligned frames: range-checked register loads through the ring
            issue(std::integral_constant<int, 0>{});
            issue(std::integral_constant<int, 1>{});
            static_for<0, NB>(step);
        } else {
            if (!pre) {   // (the walk's first item; before the VFO half)
                set_rows(in + (long long)f * frameStride, win);
                static_for<0, S - 1>(dma);
            }
            // (the VFO half: its loads wait behind the ring's)
            if constexpr (kTab) {   // the segments' coarse phasors from the prologue's table; past its items, in place
                const NcoPhiLds coarse{(unsigned)(size_t)l3 + (unsigned)op1::PHI +
                                           8u * ((unsigned)(nItem * op1::PHI_E) - (unsigned)op1::vfo_item_j0(v.a, v.frame0, f, p)),
                                       nItem < op1::PHI_ITEMS};
                vfo_half_block(v, f, p, coarse);
            } else if constexpr (kVfo) {
                vfo_half_block(v, f, p);
            }
            // The loop's counted waits take this wave's vmcnt to hold nothing but the row sets younger than the
            // one waited for. Behind a prefetch it also holds the previous item's dB and zoom stores, issued after
            // the prefetched row sets, and loads and stores do not retire in order relative to each other: a count
            // of 3 x younger could then be met by retired stores while a piece of row set i is still in flight.
            // So everything is drained once here: the prefetched row sets were issued a dft16, the dB and the
            // store burst ago (and the VFO half's own waits have already drained them), so nothing is left to
            // wait for; from here on only row sets S - 1 .. are in flight, in issue order, as the counts assume.
            if (pre) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // The lane's DMA offsets and its read offsets in a slot stay in four VGPRs over the loop (from the
            // laundered thread index, per item; recomputed per row set they cost 13 VALU of a 72-instruction step)
            unsigned xo, wo;
            lane_offs(xo, wo);
            const unsigned tl = (unsigned)tid();
            const unsigned rdx = WREG * (tl >> 6) + 8 * (tl & 63), rdw = WREG * (tl >> 6) + 2048 + 4 * (tl & 63);
            static_for<0, 32>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                constexpr int younger = (S - 2 < 31 - i) ? S - 2 : 31 - i;   // row sets issued after i, in flight
                // This wave's pieces of row set i have landed: only its own vmcnt orders its reads behind its DMAs,
                // and no other wave reads them, so there is no barrier. Its region of slot i - 1 is free for row set
                // i + S - 1: its reads of it returned before the previous step's combine2 used them, which ran in
                // front of that step's sched_barrier, in front of this DMA (the lgkmcnt(0) states it, and costs
                // nothing: the count is already zero).
                asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(3 * younger) : "memory");
                if constexpr (i == 0) T1P(9);
                if constexpr (i + S - 1 < 32) dma_at(std::integral_constant<int, i + S - 1>{}, xo, wo);
                const char* slot = reinterpret_cast<const char*>(lds) + (i % S) * SLOT;
                float2 u[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float2 xx = *reinterpret_cast<const float2*>(slot + rdx + 512 * j);
                    const float ww = *reinterpret_cast<const float*>(slot + rdw + 256 * j);
                    u[j] = wmul(xx, ww);
                }
                combine2(u, za[i], zb[i]);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        T1P(2);
        float* zf = ZM ? zpart + ((long long)f << 12) : nullptr;   // [f][workgroup][2048]
        const __amdgpu_buffer_rsrc_t ro = brsrc(out + ((long long)f << 16), 65536u * 4u);
        // the 16k transform of quarter r = r0 + h from its stage-1 registers z. Quarter r0's dB values wait in
        // registers (dA) for quarter r0 + 1's, and the two leave as one 8-byte store per bin pair.
        float dA[2][16];
        auto w128mul = [&](float2 (&z)[32], int hh) {
            const double2* w128 = reinterpret_cast<const double2*>(reinterpret_cast<const char*>(lds) + op1::W128D) + 32 * hh;
#pragma unroll
            for (int i = 1; i < 32; i++) {
                const double2 q = zmul(make_double2(z[i].x, z[i].y), w128[i]);
                z[i] = make_float2((float)q.x, (float)q.y);
            }
        };
        auto prefetch = [&] {
            int bn = b + G;
            asm volatile("" : "+s"(bn));
            const int fn = 8 * (bn >> 4) + (bn & 7);
            pre = bn < items && fn < frames;   // (workgroup-uniform; a padding item ends the walk: f only grows)
            if (pre) {
                // this wave's image reads have returned; behind the barrier, every wave's: the slots are free
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                set_rows(in + (long long)fn * frameStride, win);
                static_for<0, S - 1>(dma);
                // (Measured and not kept, round 20: every wave touching the lines of the next item's VFO round 0 here,
                // as 4-byte LDS-DMAs one line per lane into a region nobody reads: C5 group +1.7 % at a 128-B lane
                // stride, +2.6 % at 64 B; the round-0 loads from a frame hot in L2 were worth 0.1-0.4 % at most)
            }
        };
        auto transform = [&](auto hc, float2 (&z)[32]) {
            constexpr int h = decltype(hc)::value;
            const int r = r0 + h;
            {   // stage-1 finish: W_128^(r i), radix 32, W_N^(t (4 k2 + r)), into the LDS image
                const int t = tid();
                // W_128^(r i) = W_N^(512 r i) as an fp64 product of the fp64 twiddle, rounded once. As an fp32
                // product with an fp32 table (two roundings) the near-peak bins of tonal frames were 1-2 ulp
                // off more often than pocketfft's (AES17: 7 of 22 bins beyond 1 ulp vs pocketfft's 4; 2 in
                // this form), +2.7% kernel time (r5x-r5z; applied at the combine instead: +5%)
                // (also for quarter 0, where W = 1 and the product is exact: a branch around it spilled)
                if constexpr (!(VFO && h == 1)) w128mul(z, h);
                dft32(z);
                // W_N^(t r) (W_N^(4 t))^k2 as two independent fp64 chains over even / odd k2 (a serial chain of
                // 31 fp64 complex products was the stage's critical path)
                const double2 st = tab64[4 * t];
                double2 ce = tab64[t * r], co = zmul(ce, st);
                const double2 st2 = zmul(st, st);
                float2* row = lds + pad16(t);
                // In front of the first image write: every wave's reads of its ring regions (h = 0; they lie under the
                // image) or of quarter r0's image (h = 1, stage 3) are done. The W_128 products and the radix 32
                // above touch registers and the tables only, so a wave that is early runs them meanwhile.
                __syncthreads();
                if constexpr (SDRGPU_1P_ABL & 8) {
                    const float2 cf = make_float2((float)ce.x, (float)ce.y), sf = make_float2((float)st.x, (float)st.y);
#pragma unroll
                    for (int k2 = 0; k2 < 32; k2++) row[k2 * RS] = cmul(z[k2], k2 & 1 ? sf : cf);
                } else
#pragma unroll
                for (int k2 = 0; k2 < 32; k2 += 2) {
                    row[k2 * RS] = cmul(z[k2], make_float2((float)ce.x, (float)ce.y));
                    row[(k2 + 1) * RS] = cmul(z[k2 + 1], make_float2((float)co.x, (float)co.y));
                    if (k2 < 30) {
                        ce = zmul(ce, st2);
                        co = zmul(co, st2);
                    }
                }
            }
            __syncthreads();
            if constexpr (h == 0) T1P(5);
            {   // stage 2: (k2, t0) = (t >> 4, t & 15)
                const int t = tid();
                const int k2 = t >> 4, t0 = t & 15;
                float2 a[32];
                const float2* src = lds + k2 * RS + t0;
#pragma unroll
                for (int t1 = 0; t1 < 32; t1++) a[t1] = src[17 * t1];
                dft32(a);
#pragma unroll
                for (int q1 = 1; q1 < 32; q1++) a[q1] = cmul(a[q1], lds[TW512 + 16 * q1 + t0]);
                __syncthreads();
                float2* dst = lds + k2 * RS + (t0 ^ ((k2 >> 1) & 15));
#pragma unroll
                for (int q1 = 0; q1 < 32; q1++) dst[17 * q1] = a[q1];
            }
            __syncthreads();
            T1P(6 + h);
            // stage 3: (k2, q1) = (e & 31, e >> 5), e = t, t + 512. The thread holds the same (k2, q1) bins
            // of both quarters, so quarter r0 + 1 stores (dA, dB) at float 4 (k2 + 32 q1 + 1024 q2) + r0
            // (8-byte aligned: r0 even) through a buffer resource, the q2 step in soffset
            static_for<0, 2>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                const int t = tid();
                const int pe = t + 512 * e, k2 = pe & 31, q1 = pe >> 5, sw = (k2 >> 1) & 15;
                float2 c3[16];
                const float2* src = lds + k2 * RS + 17 * q1;
#pragma unroll
                for (int t0 = 0; t0 < 16; t0++) c3[t0] = src[t0 ^ sw];
                // quarter r0 + 1's W_128 products (registers only) while these reads are in flight (the VFO
                // instantiations only: the others spill two registers with it)
                if constexpr (VFO && h == 0 && e == 0) w128mul(zb, 1);
                // the item's last image reads: the next item's first row sets go in flight (above)
                if constexpr (kDma && h == 1 && e == 1) prefetch();
                dft16(c3);
                if constexpr (SDRGPU_1P_ABL & 16) {
                    if constexpr (h == 1) {
                        float acc = 0.0f;
#pragma unroll
                        for (int q2 = 0; q2 < 16; q2++) acc += c3[q2].x + c3[q2].y;
                        out[(f << 16) + pe] = acc;
                    }
                } else if constexpr (h == 0) {
#pragma unroll
                    for (int q2 = 0; q2 < 16; q2++) dA[e][q2] = db_of(c3[q2]);
                } else {
                    float dv[16];
                    const unsigned vo = (unsigned)(4 * (k2 + 32 * q1) + r0) * 4u;
#pragma unroll
                    for (int q2 = 0; q2 < 16; q2++) {
                        dv[q2] = db_of(c3[q2]);
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(bu2, make_float2(dA[e][q2], dv[q2])), ro, vo,
                                                              q2 * 4096 * 4, 0);
                    }
                    if constexpr (ZM) {   // max over both quarters and the 8 lanes k2 & 7: zoom column (k2 >> 3) + 4 q1 + 128 q2
#pragma unroll
                        for (int q2 = 0; q2 < 16; q2++) dv[q2] = fmaxf(dA[e][q2], dv[q2]);
                        const int lane = t & 63;
                        tr_step<1, 8>(dv, lane);
                        tr_step<2, 4>(dv, lane);
                        tr_step<4, 2>(dv, lane);
                        // lane bits (b0 b1 b2) now select q2 = 8 b0 + 4 b1 + 2 b2 + i in dv[i], i < 2
                        const int q2 = ((lane & 1) << 3) | ((lane & 2) << 1) | (lane & 4) >> 1;
                        float* zp = zf + ((long long)p << 11) + (k2 >> 3) + 4 * q1 + 128 * q2;
                        zp[0] = dv[0];
                        zp[128] = dv[1];
                    }
                }
            });
        };
        if constexpr (SDRGPU_1P_ABL & 2) {
            float2 acc = make_float2(0.0f, 0.0f);
#pragma unroll
            for (int i = 0; i < 32; i++) acc = cadd(acc, cadd(za[i], zb[i]));
            out[(f << 16) + tid()] = acc.x + acc.y;
            continue;
        }
        transform(std::integral_constant<int, 0>{}, za);
        T1P(3);
        transform(std::integral_constant<int, 1>{}, zb);
        T1P(4);
        // (PAD: one item per workgroup, launch_1p: inside a walk the compiler keeps the VFO half's fp64 polynomial
        // constants in ~19 VGPRs from in front of the walk to its end, and the register ring then spills 8 VGPRs)
        if constexpr (PAD) break;
    }   // (the walk)
}

#ifdef SDRGPU_1P_TIMING
extern "C" int sdrgpu_debug_1p_times(unsigned long long* host, int n) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_1p_t), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif

// zoom[f][o] = max over the two workgroups' partial maxima (fft_1p_kernel's ZM): 4 columns per thread
// as 16-B loads / stores (one element per thread took 20.8 us per 2^28-sample step); 256 threads per
// workgroup (both launches below)
static_assert(TAIL_NT_BIG == 256, "zoom_fold_block's indexing and the fold's block count assume 256 threads");
__device__ __forceinline__ void zoom_fold_block(const float* __restrict__ zpart, int frames, float* __restrict__ zoom, int blk) {
    const long long i = ((long long)blk * 256 + threadIdx.x) * 4;
    if (i >= (long long)frames * 2048) return;
    const long long f = i >> 11, o = i & 2047;
    const float4 a = *reinterpret_cast<const float4*>(zpart + (f << 12) + o);
    const float4 b = *reinterpret_cast<const float4*>(zpart + (f << 12) + 2048 + o);
    const float4 m = make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
    if (((uintptr_t)zoom & 15) == 0) {   // (wave-uniform)
        *reinterpret_cast<float4*>(zoom + i) = m;
    } else {
        zoom[i] = m.x; zoom[i + 1] = m.y; zoom[i + 2] = m.z; zoom[i + 3] = m.w;
    }
}
__global__ __launch_bounds__(256) void fft_1p_zoom_kernel(const float* __restrict__ zpart, int frames, float* __restrict__ zoom) {
    zoom_fold_block(zpart, frames, zoom, blockIdx.x);
}
// The VFO's later stages (fir_tail_kernel's workgroups, first) and the zoom fold (the rest) in one launch:
// the tail is latency-bound (dependent fmaf chains, barriers between stages), the fold moves 96 MB per C5
// step, so the fold's workgroups fill the CUs the tail leaves idle (both need only the one-pass
// launch's outputs). Same code, same bits as the two launches.
__global__ __launch_bounds__(TAIL_NT_BIG) void fft_1p_tail_fold_kernel(TailArgs t, const float* __restrict__ zpart, int frames,
                                                                         float* __restrict__ zoom) {
    extern __shared__ __attribute__((aligned(16))) float2 XS[];
    __shared__ TailGeom gs[TAIL_MAXS];
    const int w = blockIdx.x;
    if (w < t.G) fir_tail_block<TAIL_K_BIG, TAIL_NT_BIG>(t, w, w == t.G - 1, XS, gs);
    else zoom_fold_block(zpart, frames, zoom, w - t.G);
}

}  // namespace sdrgpu

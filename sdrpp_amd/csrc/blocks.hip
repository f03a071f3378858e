// Channel-chain blocks, host side: frequency xlator, FIR / decimating FIR (optionally with the
// xlator fused into its load and the FM quadrature demodulator fused into its store), power-of-two
// decimator, polyphase and rational resamplers, RxVFO, FM / broadcast-FM (mono) demodulators, ingest
// converters. Reference semantics are cited per block; DESIGN.md has the layout. The kernels are in
// fir_tile.h, fir_mfma.h, fir_rows.h, fir_tail.h and chain_kernels.h; what other translation units
// call is declared in blocks.h. Top to bottom:
//   1. buffers, stream ordering and the Block base (declared in sdrgpu_internal.h);
//   2. Nco: the host side of the NCO tables; carry_history; the one FIR launch helper;
//   3. FirBlock: configuration and state, tuning knobs, kernel selection, argument fill, one function
//      per kernel family (rows, MFMA, MFMA phase-split, tile), run / advance / reset / out_count;
//   4. XlatorBlock, QuadBlock, PolyBlock;
//   5. ChainBlock with the FIR cascade tail (tail_plan / launch_tail), the block constructors
//      (make_fir, make_xlator, make_quad_block, new_chain), PowerDecimator / RationalResampler
//      composition, VfoBlock, WfmBlock;
//   6. the hooks of a VFO carried by the spectrum launches (vfo_stage1_* / vfo_tail_*);
//   7. enter_block and publish_block, then the C ABI: create functions (one publish_block() each), setters,
//      process / reset / destroy, converters.
// Only section 7 selects the device, creates a stream (publish_block: one per handle) or waits for the
// device; the block structs and the hooks above assume the handle's device is current (blocks.h).
#include <cmath>
#include <cstring>
#include <algorithm>
#include <array>
#include <memory>
#include <numeric>
#include <type_traits>
#include "sdrgpu_internal.h"
#include "fir_rows.h"
#include "fir_tail.h"
#include "fir_tile.h"
#include "fir_mfma.h"
#include "chain_kernels.h"
#include "blocks.h"

namespace sdrgpu {

// ================================================================ host blocks
int DevBuf::ensure(size_t want) {
    if (want <= bytes) return SDRGPU_OK;
    release();
    size_t sz = std::max<size_t>(want, 256);
    if (hipMalloc(&p, sz) != hipSuccess) {
        p = nullptr;
        set_error("hipMalloc(%zu) failed", sz);
        return SDRGPU_ENOMEM;
    }
    bytes = sz;
    return SDRGPU_OK;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}
int PinnedBuf::ensure(size_t want) {
    if (want <= bytes) return SDRGPU_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    size_t sz = std::max<size_t>(want, 256);
    if (hipHostMalloc(&p, sz, hipHostMallocDefault) != hipSuccess) {
        p = nullptr;
        set_error("hipHostMalloc(%zu) failed", sz);
        return SDRGPU_ENOMEM;
    }
    bytes = sz;
    return SDRGPU_OK;
}
PinnedBuf::~PinnedBuf() {
    if (p) (void)hipHostFree(p);
}

int StreamOrder::follow(hipStream_t s) {
    if (last == nullptr || last == s) return SDRGPU_OK;
    if (multi) {
        SDRGPU_HIP(hipStreamWaitEvent(s, ev, 0));
        return SDRGPU_OK;
    }
    SDRGPU_HIP(hipDeviceSynchronize());   // first stream change: the previous stream may be gone
    if (!ev) SDRGPU_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    multi = true;
    return SDRGPU_OK;
}
int StreamOrder::done(hipStream_t s) {
    if (multi) SDRGPU_HIP(hipEventRecord(ev, s));
    last = s;
    return SDRGPU_OK;
}
StreamOrder::~StreamOrder() {
    if (ev) (void)hipEventDestroy(ev);
}

Block::~Block() {
    if (own) (void)hipStreamDestroy(own);
}

// host side of the NCO tables
constexpr int NCO_PF = 64;   // >= the FIR kernel's load slots per thread
struct Nco {
    double w = 0.0;
    PhaseAcc phase;     // phase of the next input sample
    DevBuf plo, phi;
    DevBuf step;        // [3][NCO_PF]: e^{i w u NT}, NT = 64, 128, 256 (fp64 -> float)
    DevBuf rstep;       // [2][ROWS_STEP]: e^{i w D u}, D = 8, 32 (fir_rows_kernel's row step)
    const float2* rstep_for(int D) const { return rstep.as<float2>() + (D == 8 ? 0 : ROWS_STEP); }
    const float2* step_for(int NT) const { return step.as<float2>() + (NT == 64 ? 0 : NT == 128 ? 1 : 2) * NCO_PF; }
    // appends e^{i w stride u}, u < n (fp64 -> float)
    void phasors(std::vector<float2>& t, int n, double stride) const {
        for (int u = 0; u < n; u++) {
            const double a = std::fmod(w * (double)u * stride, 2.0 * M_PI);
            t.push_back(make_float2((float)std::cos(a), (float)std::sin(a)));
        }
    }
    static int upload(DevBuf& b, const std::vector<float2>& t) {
        SDRGPU_CHECK(b.ensure(sizeof(float2) * t.size()));
        SDRGPU_HIP(hipMemcpy(b.p, t.data(), sizeof(float2) * t.size(), hipMemcpyHostToDevice));
        return SDRGPU_OK;
    }
    int set_w(double w_) {
        w = w_;
        std::vector<float2> st, rs, lo;
        for (double nt : {64.0, 128.0, 256.0}) phasors(st, NCO_PF, nt);
        for (double d : {8.0, 32.0}) phasors(rs, ROWS_STEP, d);
        phasors(lo, NCO_LO, 1.0);
        SDRGPU_CHECK(upload(step, st));
        SDRGPU_CHECK(upload(rstep, rs));
        return upload(plo, lo);
    }
    // coarse table for a call of `count` samples starting at the current phase
    int prepare(int count, hipStream_t s) {
        const int nhi = (count >> NCO_LO_BITS) + 2;
        SDRGPU_CHECK(phi.ensure(sizeof(float2) * nhi));
        hipLaunchKernelGGL(nco_hi_kernel, dim3((nhi + 255) / 256), dim3(256), 0, s, phi.as<float2>(), nhi,
                           phase.value(), w);
        SDRGPU_HIP(hipGetLastError());
        return SDRGPU_OK;
    }
};

// the same Nco for bank.hip's translator (blocks.h)
Nco* nco_new() { return new Nco(); }
void nco_delete(Nco* n) { delete n; }
int nco_set_w(Nco* n, double w) { return n->set_w(w); }
int nco_prepare(Nco* n, int count, hipStream_t s, const float2** phi, const float2** plo) {
    SDRGPU_CHECK(n->prepare(count, s));
    *phi = n->phi.as<float2>();
    *plo = n->plo.as<float2>();
    return SDRGPU_OK;
}
void nco_advance(Nco* n, long long count) { n->phase.advance(n->w, count); }
void nco_reset(Nco* n) { n->phase.reset(); }

// The history carry on its own launch (blocks.h): FirBlock's zero-output call, PolyBlock, BroadcastFM's
// delay line (loops.hip) and the channelizer (channelizer.hip).
int carry_history(int dtype, const Nco* nco, const DevBuf& hist, const void* in, DevBuf& next, int H, int count,
                         hipStream_t s) {
    const dim3 g((H + 255) / 256), b(256);
    if (dtype == SDRGPU_F32) {
        hipLaunchKernelGGL((fir_hist_kernel<float, false>), g, b, 0, s, hist.as<float>(), (const float*)in, next.as<float>(),
                           H, count, nullptr, nullptr);
    } else if (nco) {
        hipLaunchKernelGGL((fir_hist_kernel<float2, true>), g, b, 0, s, hist.as<float2>(), (const float2*)in,
                           next.as<float2>(), H, count, nco->phi.as<float2>(), nco->plo.as<float2>());
    } else {
        hipLaunchKernelGGL((fir_hist_kernel<float2, false>), g, b, 0, s, hist.as<float2>(), (const float2*)in,
                           next.as<float2>(), H, count, nullptr, nullptr);
    }
    SDRGPU_HIP(hipGetLastError());
    return SDRGPU_OK;
}

// One FIR launch: the kernel's dynamic-LDS attribute (where it takes any), `tiles` workgroups plus the
// history workgroup where the call carries a history (fir_hist_block), the launch's error.
using FirKernel = void (*)(FirArgs);
static int launch(FirKernel k, int tiles, int threads, size_t lds, const FirArgs& a, hipStream_t s) {
    if (lds > 0) SDRGPU_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(tiles + (a.histNext ? 1 : 0)), dim3(threads), lds, s, a);
    SDRGPU_HIP(hipGetLastError());
    return SDRGPU_OK;
}

// ------------------------------------------------------------------ FIR block
struct FirBlock : Block {
    // ---- configuration, tap tables, state
    int ttype = SDRGPU_F32, ntaps = 0, D = 1;
    bool xl = false, quad = false, stereo = false;
    Nco nco;                // XL: fused frequency xlator
    float invDev = 1.0f;    // QUAD
    std::vector<float> host_taps;
    DevBuf taps;            // [p][q] = h[q*D + p], Q per phase, zero past ntaps (phase-major like the LDS span)
    int Q = 1;              // padded taps per phase: a multiple of the kernels' chunk QC = 8
    DevBuf gzTaps;          // MFMA kernels: gz[p][t] = h[(t - 15) D + p], gzs entries per phase
    int gzs = MF_GZ;
    DevBuf hist[2], din[2]; // ping-pong: the last ntaps - 1 inputs (stored translated); QUAD: y[-1]
    int cur = 0;            // ping-pong index
    int offset = 0;         // decimation phase: the next call's first output starts at input `offset`

    // ---- tuning knobs (SDRGPU_TUNING=1), read when the block is created
    int mfNW = 4;           // SDRGPU_FIR_MFMA_NW: waves (x 256 outputs) per workgroup, 4 or 2 (2: 4 WG/CU, measured 13% slower on C3)
    // fir_mfma_kernel HALF: half the phases' span in LDS at a time, 4 workgroups per CU (105 VGPRs, no
    // spill); C3 kernel 0.842 -> 0.787 ms (3 interleaved runs, r4d). SDRGPU_FIR_MFMA_HALF=0 off
    int mfHalf = 1;
    int mfDc = 1;           // SDRGPU_FIR_MFMA_DC=0: D = 8 as a run-time value (fir_mfma_kernel DC)
    int usePS = 1;          // SDRGPU_FIR_MFMA_PS: 0 off, 1 auto (D >= 4 where fir_mfma_kernel is not used), 2 force
    int useRows = 1;        // SDRGPU_FIR_ROWS: 0 off, 1 auto (D = 32), 2 also D = 8
    void read_knobs() {
        if (const char* e = tuning_env("SDRGPU_FIR_MFMA_NW")) mfNW = atoi(e);
        if (const char* e = tuning_env("SDRGPU_FIR_MFMA_HALF")) mfHalf = atoi(e);
        if (const char* e = tuning_env("SDRGPU_FIR_MFMA_DC")) mfDc = atoi(e);
        if (const char* e = tuning_env("SDRGPU_FIR_MFMA_PS")) usePS = atoi(e);
        if (const char* e = tuning_env("SDRGPU_FIR_ROWS")) useRows = atoi(e);
    }

    static int decim_ok(int d) {
        if (d < 1) { set_error("fir: decimation %d < 1", d); return SDRGPU_EARG; }
        return SDRGPU_OK;
    }
    int setup(int dev, int dtype_, int ttype_, const float* t, int n, int decim) {
        device = dev;
        in_dtype = dtype_;
        out_dtype = quad ? SDRGPU_F32 : (stereo ? SDRGPU_C64 : dtype_);
        ttype = ttype_;
        SDRGPU_CHECK(decim_ok(decim));
        D = decim;
        read_knobs();
        return set_taps(t, n);
    }
    // FIR::setTaps (fir.h:31-52): history kept aligned to the newest sample;
    // DecimatingFIR::setTaps resets the decimation phase (decimating_fir.h:19-26)
    int set_taps(const float* t, int n) {
        if (!t || n < 1 || n > 64001) { set_error("fir: tap count %d out of range [1, 64001]", n); return SDRGPU_EARG; }
        const size_t es = esize(in_dtype);
        const int oldH = ntaps > 0 ? ntaps - 1 : 0, newH = n - 1;
        std::vector<unsigned char> oldHist((size_t)oldH * es), newHist((size_t)std::max(newH, 1) * es, 0);
        if (oldH > 0) SDRGPU_HIP(hipMemcpy(oldHist.data(), hist[cur].p, oldHist.size(), hipMemcpyDeviceToHost));
        const int keep = std::min(oldH, newH);
        if (keep > 0) std::memcpy(newHist.data() + (size_t)(newH - keep) * es, oldHist.data() + (size_t)(oldH - keep) * es, keep * es);
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(newHist.size()));
        SDRGPU_HIP(hipMemcpy(hist[cur].p, newHist.data(), newHist.size(), hipMemcpyHostToDevice));
        host_taps.assign(t, t + (size_t)n * (ttype == SDRGPU_C64 ? 2 : 1));
        ntaps = n;
        offset = 0;
        SDRGPU_CHECK(upload_taps());
        for (int k = 0; quad && k < 2; k++) SDRGPU_CHECK(din[k].ensure(sizeof(float2)));
        return SDRGPU_OK;
    }
    int set_decimation(int d) {
        SDRGPU_CHECK(decim_ok(d));
        D = d;
        offset = 0;
        return upload_taps();
    }
    // the device tap tables for the current taps / decimation, and the kernel that takes them
    int upload_taps() {
        Q = (qr() + 7) / 8 * 8;      // kernel chunk QC = 8 (zero taps past ntaps)
        const int e = ttype == SDRGPU_C64 ? 2 : 1;
        std::vector<float> pq((size_t)D * Q * e, 0.0f);
        for (int p = 0; p < D; p++)
            for (int q = 0; q < Q; q++) {
                const int j = q * D + p;
                if (j < ntaps)
                    for (int k = 0; k < e; k++) pq[((size_t)p * Q + q) * e + k] = host_taps[(size_t)j * e + k];
            }
        SDRGPU_CHECK(taps.ensure(sizeof(float) * pq.size()));
        SDRGPU_HIP(hipMemcpy(taps.p, pq.data(), sizeof(float) * pq.size(), hipMemcpyHostToDevice));
        select_kernel();
        if (mf || mfps) {
            // gz[p][t] = h[(t - 15) D + p], gzs entries per phase (t < 15 + 4 ks suffice)
            const int Qr = qr();
            gzs = mf ? MF_GZ : 16 + 4 * ((15 + Qr + 3) / 4);
            std::vector<float> g((size_t)D * gzs, 0.0f);
            for (int p = 0; p < D; p++)
                for (int t = 15; t < gzs; t++) {
                    const int j = (t - 15) * D + p;
                    if (t - 15 < Qr && j < ntaps) g[(size_t)p * gzs + t] = host_taps[j];
                }
            SDRGPU_CHECK(gzTaps.ensure(sizeof(float) * g.size()));
            SDRGPU_HIP(hipMemcpy(gzTaps.p, g.data(), sizeof(float) * g.size(), hipMemcpyHostToDevice));
        }
        return SDRGPU_OK;
    }

    // ---- kernel selection for the current taps / decimation: rowsk, else mf, else mfps, else the tile kernel
    bool mf = false;        // fir_mfma_kernel
    bool mfps = false;      // fir_mfma_ps_kernel
    bool rowsk = false;     // fir_rows_kernel
    int qr() const { return (ntaps + D - 1) / D; }   // taps per phase, unpadded
    // taps per phase of the rows kernel: D = 32 exact (2..8), D = 8 padded to 16, 24 or 32
    static int rows_qp(int D, int Qr) {
        if (D == 32) return (Qr >= 2 && Qr <= 8) ? Qr : 0;
        if (D == 8) return Qr < 2 ? 0 : Qr <= 16 ? 16 : Qr <= 24 ? 24 : Qr <= 32 ? 32 : 0;
        return 0;
    }
    void select_kernel() {
        const int Qr = qr();
        const bool cr = in_dtype == SDRGPU_C64 && ttype == SDRGPU_F32 && !stereo;   // complex data, real taps
        // matrix-core path (fir_mfma_kernel): 16..32 taps per phase, D a power of two <= 8 (with 128
        // threads, a load slot advances by whole 16-row pad groups)
        const bool cplx = cr && (D & (D - 1)) == 0 && Qr <= 32;
        mf = cplx && D <= 8 && Qr >= 16;
        // phase-split tiles for the larger decimations (and on request for the others)
        mfps = cplx && !mf && D >= 4 && D <= 32 && (usePS != 0);
        if (usePS == 2 && cplx && D >= 4 && D <= 32) { mfps = true; mf = false; }
        // row-streaming kernel for D = 32 with <= 8 taps per phase (VFO stage 1), ahead of the MFMA tiles
        rowsk = cr && rows_qp(D, Qr) > 0 && !(quad && D == 32) && (useRows == 2 || (useRows == 1 && D == 32));
    }
    // tile kernel, outputs per thread: register blocking pays when a row feeds several taps per phase
    // (unpadded Q large)
    int choose_k() const {
        const int Qr = qr();
        if (Qr >= 16) return 4;
        if (Qr >= 6) return 2;
        return 1;
    }
    // The tile kernel's shape. LDS budget: span (TM + Q + K rows) * D elements (+ taps); prefer a tile
    // that leaves room for two workgroups per CU, else whatever fits; shrink K, then the tile's thread
    // count (256, 128, 64), until it does (large decimations: plan_8192 stage 0). lds > kLdsMax: none fits.
    static constexpr size_t kLdsTwoPerCu = 76 * 1024, kLdsMax = 150 * 1024;
    struct TileShape { int K, NT, RSK, RSP; size_t lds; };
    TileShape tile_shape() const {
        TileShape t{};
        for (size_t cap : {kLdsTwoPerCu, kLdsMax}) {
            t.K = choose_k();
            t.NT = 256;
            for (;;) {
                const int rows = t.NT * t.K + Q + 2 * t.K;
                t.RSK = (rows + t.K - 1) / t.K;
                t.RSP = t.K * t.RSK + 1;
                t.lds = esize(in_dtype) * (size_t)D * t.RSP;
                if (t.lds <= cap) return t;
                if (t.K > 1) t.K /= 2;
                else if (t.NT > 64) t.NT /= 2;
                else break;
            }
        }
        return t;
    }

    // ---- argument fill: what every family's launch takes (state as it stands: nothing changes here);
    // histNext: where this call's launch writes the next history (null: it carries none)
    FirArgs base_args(const void* in, int count, void* out, int M, void* histNext) const {
        FirArgs a{};
        a.histNext = histNext;
        a.hist = hist[cur].p; a.in = in; a.out = out;
        a.din = din[cur].as<float2>(); a.dinNext = din[cur ^ 1].as<float2>();
        a.phi = nco.phi.as<float2>(); a.plo = nco.plo.as<float2>(); a.ncoTheta0 = nco.phase.value(); a.ncoW = nco.w;
        a.ntaps = ntaps; a.H = ntaps - 1; a.count = count; a.D = D; a.offset0 = offset; a.M = M;
        a.invDev = invDev;
        return a;
    }

    // ---- fir_rows_kernel
    template <int D_, int QP, bool QD, int RS = rows_rs<D_>()>
    FirKernel rows_kernel_rs(int& rs) const {
        rs = RS;
        return xl ? fir_rows_kernel<D_, QP, true, QD, RS> : fir_rows_kernel<D_, QP, false, QD, RS>;
    }
    // D = 32: 32-output segments (one row batch each) at every call size, the segments the spectrum
    // launches cut for a fused first stage (fft.hip vfo_quarter_block: same segments, same bits); a
    // reference-size block (9,600 stage-1 outputs) is 300 segments, where 128-output ones were 75
    // segments in 10 workgroups (62 us)
    template <int D_, int QP, bool QD>
    FirKernel rows_kernel(int& rs) const {
        if constexpr (D_ == 32 && !QD) return rows_kernel_rs<D_, QP, QD, 32>(rs);
        // (reached by D = 8 only, but compiled for D = 32 as well: its 128-output kernels stay in the
        // library, never launched, as long as no round is to change the set of kernels)
        return rows_kernel_rs<D_, QP, QD>(rs);
    }
    FirKernel rows_kernel(int& rs) const {
        const int qp = rows_qp(D, qr());
        if (D == 32 && !quad) {
            switch (qp) {
            case 2: return rows_kernel<32, 2, false>(rs);
            case 3: return rows_kernel<32, 3, false>(rs);
            case 4: return rows_kernel<32, 4, false>(rs);
            case 5: return rows_kernel<32, 5, false>(rs);
            case 6: return rows_kernel<32, 6, false>(rs);
            case 7: return rows_kernel<32, 7, false>(rs);
            case 8: return rows_kernel<32, 8, false>(rs);
            }
        } else if (D == 8) {
            switch (qp) {
            case 16: return quad ? rows_kernel<8, 16, true>(rs) : rows_kernel<8, 16, false>(rs);
            case 24: return quad ? rows_kernel<8, 24, true>(rs) : rows_kernel<8, 24, false>(rs);
            case 32: return quad ? rows_kernel<8, 32, true>(rs) : rows_kernel<8, 32, false>(rs);
            }
        }
        return nullptr;
    }
    FirArgs rows_args(const void* in, int count, void* out, int M, void* histNext) const {
        FirArgs a = base_args(in, count, out, M, histNext);
        a.taps = taps.p;
        a.Q = Q;
        a.nstep = xl ? nco.rstep_for(D) : nullptr;
        return a;
    }
    int run_rows(const void* in, int count, void* out, int M, void* histNext, hipStream_t s) {
        int rs = 0;
        const FirKernel k = rows_kernel(rs);
        if (!k) { set_error("fir: rows kernel does not take (D %d, ntaps %d)", D, ntaps); return SDRGPU_EARG; }
        const int q = quad ? 1 : 0;   // (with the quadrature a segment starts one output early)
        const long long segs = ((long long)M + q + (rs - q) - 1) / (rs - q);
        const int blocks = (int)((segs + 4 * (64 / D) - 1) / (4 * (64 / D)));   // 4 waves x 64/D groups
        return launch(k, blocks, 256, 0, rows_args(in, count, out, M, histNext), s);
    }
    // A call whose row-kernel segments another launch runs (fft.hip's spectrum launches, VfoStage1):
    // D = 32 with the fused xlator, 5 taps per phase (the RxVFO's plan_256 stage 1), a history to
    // carry. Those launches use 128-output segments at any call size: a segment's length does not
    // change any output's bits (each output's partial runs over its own QP rows, in row order).
    // The caller launches with rows_args and then calls advance().
    bool rows_external(int count) {
        return rowsk && xl && !quad && D == 32 && rows_qp(D, qr()) == 5 && ntaps > 1 && out_count(count) > 0;
    }

    // ---- fir_mfma_kernel
    template <int NW, bool XL, bool QD>
    FirKernel mfma_kernel(bool half) const {
        const bool dc = D == 8 && mfDc;
        return half ? (dc ? fir_mfma_kernel<NW, XL, QD, true, 8> : fir_mfma_kernel<NW, XL, QD, true>)
                    : (dc ? fir_mfma_kernel<NW, XL, QD, false, 8> : fir_mfma_kernel<NW, XL, QD, false>);
    }
    template <int NW>
    int run_mfma_nw(const void* in, int count, void* out, int M, void* histNext, hipStream_t s) {
        constexpr int MF_TM = 256 * NW, MF_ROWS = mf_rows(NW);
        FirArgs a = base_args(in, count, out, M, histNext);
        a.taps = gzTaps.p;
        a.TMS = quad ? MF_TM - 1 : MF_TM;
        a.RSP = MF_ROWS + MF_ROWS / 16 + 1;
        a.dshift = __builtin_ctz((unsigned)D);
        a.nstep = xl ? nco.step_for(64 * NW) : nullptr;
        // HALF needs two phase halves (D >= 2) and the PF load slots covering the span (D <= 8)
        const bool half = mfHalf && D >= 2 && D <= 8;
        const size_t xb = std::max(sizeof(float2) * (size_t)(half ? D / 2 : D) * a.RSP, sizeof(float2) * (size_t)MF_TM);
        a.tapsLdsOff = (int)((xb + 15) / 16 * 16);
        const size_t lds = a.tapsLdsOff + sizeof(float) * D * MF_GZ;
        a.ntiles = (M + a.TMS - 1) / a.TMS;
        const FirKernel k = xl ? (quad ? mfma_kernel<NW, true, true>(half) : mfma_kernel<NW, true, false>(half))
                               : (quad ? mfma_kernel<NW, false, true>(half) : mfma_kernel<NW, false, false>(half));
        return launch(k, a.ntiles, 64 * NW, lds, a, s);
    }
    int run_mfma(const void* in, int count, void* out, int M, void* histNext, hipStream_t s) {
        return mfNW == 4 ? run_mfma_nw<4>(in, count, out, M, histNext, s) : run_mfma_nw<2>(in, count, out, M, histNext, s);
    }

    // ---- fir_mfma_ps_kernel
    int run_mfma_ps(const void* in, int count, void* out, int M, void* histNext, hipStream_t s) {
        FirArgs a = base_args(in, count, out, M, histNext);
        a.taps = gzTaps.p;
        a.Q = (15 + qr() + 3) / 4;                      // k steps
        const int rows = 256 + 4 * a.Q;
        a.RSP = (rows + rows / 16) | 1;                 // odd: the D phases of one load slot in distinct banks
        a.TMS = quad ? 255 : 256;
        a.dshift = __builtin_ctz((unsigned)D);
        a.nstep = xl ? nco.step_for(256) : nullptr;
        const size_t xb = std::max(sizeof(float2) * (size_t)D * a.RSP, sizeof(float2) * 4 * 256);   // span / partials
        a.tapsLdsOff = (int)((xb + 15) / 16 * 16);
        a.gzs = gzs;
        const size_t lds = a.tapsLdsOff + sizeof(float) * D * gzs;   // D = 32, Qp = 5: 79.6 KB, 2 per CU
        if (lds > kLdsMax) { set_error("fir: MFMA tile does not fit (D %d)", D); return SDRGPU_EARG; }
        a.ntiles = (M + a.TMS - 1) / a.TMS;
        const FirKernel k = xl ? (quad ? fir_mfma_ps_kernel<true, true> : fir_mfma_ps_kernel<true, false>)
                               : (quad ? fir_mfma_ps_kernel<false, true> : fir_mfma_ps_kernel<false, false>);
        return launch(k, a.ntiles, 256, lds, a, s);
    }

    // ---- fir_kernel (the tile kernel: every other shape)
    template <typename DT, typename TT, bool XL, bool QD, bool ST>
    static FirKernel tile_kernel(int K, bool tl) {
        switch (K) {
        case 8: return tl ? fir_kernel<DT, TT, 8, XL, QD, ST, true> : fir_kernel<DT, TT, 8, XL, QD, ST, false>;
        case 4: return tl ? fir_kernel<DT, TT, 4, XL, QD, ST, true> : fir_kernel<DT, TT, 4, XL, QD, ST, false>;
        case 2: return tl ? fir_kernel<DT, TT, 2, XL, QD, ST, true> : fir_kernel<DT, TT, 2, XL, QD, ST, false>;
        default: return tl ? fir_kernel<DT, TT, 1, XL, QD, ST, true> : fir_kernel<DT, TT, 1, XL, QD, ST, false>;
        }
    }
    FirKernel tile_kernel(int K, bool tl) const {
        if (in_dtype == SDRGPU_F32) return stereo ? tile_kernel<float, float, false, false, true>(K, tl)
                                                  : tile_kernel<float, float, false, false, false>(K, tl);
        if (ttype == SDRGPU_C64) return tile_kernel<float2, float2, false, false, false>(K, tl);
        if (xl) return quad ? tile_kernel<float2, float, true, true, false>(K, tl) : tile_kernel<float2, float, true, false, false>(K, tl);
        return quad ? tile_kernel<float2, float, false, true, false>(K, tl) : tile_kernel<float2, float, false, false, false>(K, tl);
    }
    int run_tile(const void* in, int count, void* out, int M, void* histNext, hipStream_t s) {
        const TileShape t = tile_shape();
        if (t.lds > kLdsMax) {
            set_error("fir: tile does not fit LDS (ntaps %d, decim %d)", ntaps, D);
            return SDRGPU_EARG;
        }
        const int TM = t.NT * t.K;
        FirArgs a = base_args(in, count, out, M, histNext);
        a.taps = taps.p;
        a.Q = Q;
        a.TMS = quad ? TM - 1 : TM; a.RSK = t.RSK; a.RSP = t.RSP;
        a.dshift = (D & (D - 1)) ? -1 : __builtin_ctz((unsigned)D);
        // taps behind the span in LDS when they fit (<= 16 KB)
        const size_t tb = (size_t)D * Q * esize(ttype);
        const bool tl = tb <= 16 * 1024 && t.lds + tb <= 160 * 1024;
        a.tapsLdsOff = (int)((t.lds + 15) / 16 * 16);
        a.ntiles = (M + a.TMS - 1) / a.TMS;
        a.simple = (t.NT % D == 0) && ((t.NT / D) % t.K == 0);
        a.nstep = xl ? nco.step_for(t.NT) : nullptr;
        // one tile per workgroup: a co-resident persistent grid with a register prefetch of the
        // next tile was measured 1.5x SLOWER on C3 (the hardware's own workgroup turnover
        // staggers the load/compute phases of the workgroups sharing a CU better)
        return launch(tile_kernel(t.K, tl), a.ntiles, t.NT, tl ? a.tapsLdsOff + tb : t.lds, a, s);
    }

    // ---- one call
    int out_count(int count) override { return count > offset ? (count - offset + D - 1) / D : 0; }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, (size_t)std::max(ntaps - 1, 1) * esize(in_dtype)));
        if (quad) SDRGPU_HIP(hipMemset(din[cur].p, 0, sizeof(float2)));
        offset = 0;
        nco.phase.reset();
        return SDRGPU_OK;
    }
    // the state update after a call of `count` inputs and M outputs, whichever launch computed it
    void advance(int count, int M) {
        cur ^= 1;
        offset = offset + M * D - count;
        if (xl) nco.phase.advance(nco.w, count);
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count < 0) { set_error("fir: negative count"); return SDRGPU_EARG; }
        const int M = out_count(count);
        const int H = ntaps - 1;
        // the row kernel forms its coarse phasors itself (nco_inline); the tile kernels and the
        // separate history kernel of a call without outputs read the per-call table
        if (xl && count > 0 && (M == 0 || !rowsk)) SDRGPU_CHECK(nco.prepare(count, s));
        if (M > 0) {
            // with outputs to compute, the FIR launch itself carries the history (fir_hist_block)
            void* histNext = H > 0 ? hist[cur ^ 1].p : nullptr;
            SDRGPU_CHECK(rowsk  ? run_rows(in, count, out, M, histNext, s)
                         : mf   ? run_mfma(in, count, out, M, histNext, s)
                         : mfps ? run_mfma_ps(in, count, out, M, histNext, s)
                                : run_tile(in, count, out, M, histNext, s));
        } else {
            if (quad) SDRGPU_HIP(hipMemcpyAsync(din[cur ^ 1].p, din[cur].p, sizeof(float2), hipMemcpyDeviceToDevice, s));
            if (H > 0) SDRGPU_CHECK(carry_history(in_dtype, xl ? &nco : nullptr, hist[cur], in, hist[cur ^ 1], H, count, s));
        }
        advance(count, M);
        return M;
    }

    // ---- as a stage of the FIR cascade tail (fir_tail.h): plain complex data x real taps at a
    // power-of-two decimation, no fused xlator / quadrature
    bool tail_ok() const {
        return in_dtype == SDRGPU_C64 && ttype == SDRGPU_F32 && !xl && !quad && !stereo && offset <= ntaps - 1 && Q % 8 == 0 &&
               !(D & (D - 1)) && D <= TAIL_NT / 8;
    }
    TailStage tail_stage(int n) {
        TailStage st;
        st.hist = hist[cur].as<float2>();
        st.histNext = hist[cur ^ 1].as<float2>();
        st.taps = taps.as<float>();
        st.H = ntaps - 1;
        st.n = n;
        st.D = D;
        st.dsh = __builtin_ctz((unsigned)D);
        st.Q = Q;
        st.off = offset;
        st.M = out_count(n);
        return st;
    }
};

// --------------------------------------------------------------- xlator block
struct XlatorBlock : Block {
    Nco nco;
    int out_count(int count) override { return count; }
    int reset() override { nco.phase.reset(); return SDRGPU_OK; }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count > 0) {
            SDRGPU_CHECK(nco.prepare(count, s));
            hipLaunchKernelGGL(xlator_kernel, dim3((count + 255) / 256), dim3(256), 0, s, (const float2*)in, (float2*)out,
                               (long long)count, nco.phi.as<float2>(), nco.plo.as<float2>());
            SDRGPU_HIP(hipGetLastError());
        }
        nco.phase.advance(nco.w, count);
        return count;
    }
};

// ------------------------------------------------------------ quadrature block
struct QuadBlock : Block {
    float invDev = 1.0f;
    DevBuf din[2];
    int cur = 0;
    int out_count(int count) override { return count; }
    int reset() override {
        SDRGPU_HIP(hipMemset(din[cur].p, 0, sizeof(float2)));
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (count <= 0) return 0;
        hipLaunchKernelGGL(quad_kernel, dim3((count + 255) / 256), dim3(256), 0, s, (const float2*)in, (float*)out, count,
                           din[cur].as<float2>(), din[cur ^ 1].as<float2>(), invDev);
        SDRGPU_HIP(hipGetLastError());
        cur ^= 1;
        return count;
    }
};

// ------------------------------------------------------------- polyphase block
struct PolyBlock : Block {
    int interp = 1, decim = 1, tpp = 1, phase = 0, offset = 0;
    DevBuf bank, hist[2];
    int cur = 0;
    static int args_ok(int ip, int dc, const float* taps, int n) {
        if (ip < 1 || dc < 1 || !taps || n < 1) { set_error("polyphase: bad ratio/taps"); return SDRGPU_EARG; }
        return SDRGPU_OK;
    }
    int setup(int dev, int dtype, int ip, int dc, const float* taps, int n) {
        device = dev;
        in_dtype = out_dtype = dtype;
        SDRGPU_CHECK(args_ok(ip, dc, taps, n));
        interp = ip; decim = dc;
        // multirate/polyphase_bank.h:15-47: phases[P-1-(i%P)][i/P] = taps[i]
        tpp = (n + interp - 1) / interp;
        std::vector<float> b((size_t)interp * tpp, 0.0f);
        for (int i = 0; i < interp * tpp; i++)
            b[(size_t)((interp - 1) - (i % interp)) * tpp + i / interp] = (i < n) ? taps[i] : 0.0f;
        SDRGPU_CHECK(bank.ensure(sizeof(float) * b.size()));
        SDRGPU_HIP(hipMemcpy(bank.p, b.data(), sizeof(float) * b.size(), hipMemcpyHostToDevice));
        for (int k = 0; k < 2; k++) SDRGPU_CHECK(hist[k].ensure(esize(dtype) * std::max(tpp - 1, 1)));
        return reset();
    }
    int out_count(int count) override {
        // while (offset < count) { out; phase += decim; offset += phase / interp; phase %= interp; }
        long long pos = (long long)offset * interp + phase;
        long long lim = (long long)count * interp;
        if (pos >= lim) return 0;
        return (int)((lim - 1 - pos) / decim + 1);
    }
    int reset() override {
        SDRGPU_HIP(hipMemset(hist[cur].p, 0, esize(in_dtype) * std::max(tpp - 1, 1)));
        phase = 0; offset = 0;
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        const int M = out_count(count);
        const int H = tpp - 1;
        const long long pos0 = (long long)offset * interp + phase;
        if (M > 0) {
            if (in_dtype == SDRGPU_F32)
                hipLaunchKernelGGL((poly_kernel<float>), dim3((M + 255) / 256), dim3(256), 0, s, hist[cur].as<float>(),
                                   (const float*)in, bank.as<float>(), (float*)out, H, tpp, interp, decim, pos0, M);
            else
                hipLaunchKernelGGL((poly_kernel<float2>), dim3((M + 255) / 256), dim3(256), 0, s, hist[cur].as<float2>(),
                                   (const float2*)in, bank.as<float>(), (float2*)out, H, tpp, interp, decim, pos0, M);
            SDRGPU_HIP(hipGetLastError());
        }
        if (H > 0) {
            SDRGPU_CHECK(carry_history(in_dtype, nullptr, hist[cur], in, hist[cur ^ 1], H, count, s));
            cur ^= 1;
        }
        long long pos = pos0 + (long long)M * decim;
        offset = (int)(pos / interp) - count;
        phase = (int)(pos % interp);
        return M;
    }
};

// ---------------------------------------------------------- chains of blocks
// Runs children back to back on one stream through device scratch buffers.
struct ChainBlock : Block {
    std::vector<std::unique_ptr<Block>> kids;
    DevBuf scratch[2];
    size_t keepOnReset = 0;   // the last kids that reset() leaves as they are (AM's low-pass, am.h:104-112)
    int out_count(int count) override {
        for (auto& k : kids) count = k->out_count(count);   // (does not mutate state)
        return count;
    }
    int reset() override {
        for (size_t i = 0; i + keepOnReset < kids.size(); i++) SDRGPU_CHECK(kids[i]->reset());
        return SDRGPU_OK;
    }
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (kids.empty()) {
            SDRGPU_HIP(hipMemcpyAsync(out, in, (size_t)count * esize(in_dtype), hipMemcpyDeviceToDevice, s));
            return count;
        }
        int nt = 0;
        const int tr = run_tail(in, count, out, s, &nt);
        if (tr < 0) return tr;
        if (tr > 0) return nt;
        return run_from(0, in, count, out, s);
    }
    // kids[i0..] on n samples at src (kid i0's input), the last one writing `out`
    int run_from(size_t i0, const void* src, int n, void* out, hipStream_t s) {
        if (i0 >= kids.size()) {
            if (src != out) SDRGPU_HIP(hipMemcpyAsync(out, src, (size_t)n * esize(out_dtype), hipMemcpyDeviceToDevice, s));
            return n;
        }
        // upper bound of intermediate sizes: each child's output never exceeds its input here
        for (size_t i = i0; i < kids.size(); i++) {
            void* dst;
            if (i + 1 == kids.size()) {
                dst = out;
            } else {
                const int m = kids[i]->out_count(n);
                SDRGPU_CHECK(scratch[i & 1].ensure((size_t)std::max(m, 1) * esize(kids[i]->out_dtype)));
                dst = scratch[i & 1].p;
            }
            n = kids[i]->run(src, n, dst, s);
            if (n < 0) return n;
            src = dst;
        }
        return n;
    }
    // Short calls: the first kid as usual, then every later kid -- when all are plain FIR blocks
    // (FirBlock::tail_ok) -- in one fir_tail_kernel launch.
    static constexpr int kTailMaxIn = 1 << 15;   // first kid's outputs (a reference block: 9,600)
    // SDRGPU_VFO_TAIL (tuning): 0 off; 1 calls up to kTailMaxIn; 2 (default) every size (big calls:
    // thousands of tail workgroups, each ~TAIL_PF * TAIL_NT stage-0 samples: the C5 step's three
    // later-stage launches become one, 1.760 -> 1.747 ms, 3 interleaved runs, r4j; 512 last-stage
    // outputs per workgroup to start from measured best of 32 / 64 / 128 / 512, r4l)
    int tailMode = -1;
    int tailBigOut = 512;   // big calls: last-stage outputs per workgroup to start from
    // big calls: the workgroup count and image size depend only on (n0, the stages' offsets), which
    // repeat call after call; the per-workgroup geometry scan is kept for the last key: n0, the stage
    // count, and every stage's offset, history, padded taps per phase and decimation (the geometry
    // depends on exactly these)
    using TailKey = std::array<int, 2 + 4 * TAIL_MAXS>;
    TailKey tailKey{{-1}};
    int tailG = 0, tailMaxEl = 0;
    // The tail launch's arguments for kids[1..] on n0 samples of kid 0's output: 1 (t and lds
    // filled; no state changed), 0 (not applicable: the per-kid path runs).
    int tail_plan(int n0, TailArgs& t, size_t& lds) {
        if (tailMode < 0) {
            const char* e = tuning_env("SDRGPU_VFO_TAIL");
            tailMode = e ? atoi(e) : 2;
            if (const char* b = tuning_env("SDRGPU_TAIL_BIGOUT")) tailBigOut = std::max(32, atoi(b));
        }
        const int S = (int)kids.size() - 1;
        if (!tailMode || S < 2 || S > TAIL_MAXS) return 0;
        const bool big = n0 > kTailMaxIn;
        if (big && tailMode < 2) return 0;
        t = TailArgs{};
        t.S = S;
        t.K = big ? TAIL_K_BIG : TAIL_K;
        t.NT = big ? TAIL_NT_BIG : TAIL_NT;
        int n = n0;
        TailKey key{{n0, S}};
        for (int i = 0; i < S; i++) {
            auto* f = dynamic_cast<FirBlock*>(kids[i + 1].get());
            if (!f || !f->tail_ok()) return 0;
            const TailStage& st = t.st[i] = f->tail_stage(n);
            n = st.M;
            key[2 + 4 * i] = st.off; key[3 + 4 * i] = st.H; key[4 + 4 * i] = st.Q; key[5 + 4 * i] = st.D;
        }
        // ~128 last-stage outputs per workgroup, more workgroups while stage 0's image exceeds one
        // load batch (TAIL_PF per thread); big calls start from ~512 per workgroup
        int maxEl = 0;
        TailGeom g[TAIL_MAXS];
        if (big && key == tailKey) {
            t.G = tailG;
            maxEl = tailMaxEl;
        } else {
            for (t.G = big ? std::max((n + tailBigOut - 1) / tailBigOut, 1) : std::min(std::max((n + 127) / 128, 1), 32);; t.G *= 2) {
                int nel0 = 0;
                maxEl = 0;
                for (int w = 0; w < t.G; w++) {
                    maxEl = std::max(maxEl, tail_geometry(t, w, g));
                    nel0 = std::max(nel0, g[0].nel);
                }
                if (nel0 <= TAIL_PF * t.NT) break;
                if ((!big && t.G >= 64) || t.G >= std::max(n, 1) || t.G >= (1 << 20)) return 0;
            }
            if (big) {
                tailKey = key;
                tailG = t.G;
                tailMaxEl = maxEl;
            }
        }
        t.ldsEl = maxEl;
        int tapF = 0;
        for (int i = 0; i < S; i++) {
            t.tapOff[i] = tapF;
            tapF += t.st[i].D * t.st[i].Q;
            if (i > 0 && t.st[i].H > TAIL_NT) return 0;   // one history load per thread
        }
        t.tapTotal = tapF;
        if (tapF > 2 * TAIL_NT) return 0;                 // two tap loads per thread
        lds = sizeof(float2) * (size_t)maxEl + sizeof(float) * (size_t)tapF;
        if (lds > TAIL_LDSMAX) return 0;
        return 1;
    }
    // the state update of kids[1..] (FIR blocks: tail_plan) after a launch that ran the tail t; returns
    // the last stage's output count
    int advance_tail(const TailArgs& t) {
        for (int i = 0; i < t.S; i++) static_cast<FirBlock*>(kids[i + 1].get())->advance(t.st[i].n, t.st[i].M);
        return t.st[t.S - 1].M;
    }
    // the tail launch over kid 0's output s1 into out, and the kids' state update
    int launch_tail(TailArgs& t, size_t lds, const void* s1, void* out, hipStream_t s) {
        t.in = reinterpret_cast<const float2*>(s1);
        t.out = reinterpret_cast<float2*>(out);
        if (t.K == TAIL_K_BIG && t.NT == TAIL_NT_BIG) hipLaunchKernelGGL((fir_tail_kernel<TAIL_K_BIG, TAIL_NT_BIG>), dim3(t.G), dim3(TAIL_NT_BIG), lds, s, t);
        else hipLaunchKernelGGL((fir_tail_kernel<TAIL_K, TAIL_NT>), dim3(t.G), dim3(TAIL_NT), lds, s, t);
        SDRGPU_HIP(hipGetLastError());
        return advance_tail(t);
    }
    // Returns 1 (done, *nout = outputs), 0 (not applicable: the per-kid path runs) or an error.
    int run_tail(const void* in, int count, void* out, hipStream_t s, int* nout) {
        TailArgs t;
        size_t lds = 0;
        const int n0 = kids.empty() ? 0 : kids[0]->out_count(count);
        const int ok = tail_plan(n0, t, lds);
        if (ok <= 0) return ok;
        SDRGPU_CHECK(scratch[0].ensure(sizeof(float2) * (size_t)std::max(n0, 1)));
        const int m0 = kids[0]->run(in, count, scratch[0].p, s);
        if (m0 < 0) return m0;
        if (m0 != n0) { set_error("chain: first stage produced %d samples, expected %d", m0, n0); return SDRGPU_ESTATE; }
        const int n = launch_tail(t, lds, scratch[0].p, out, s);
        if (n < 0) return n;
        *nout = n;
        return 1;
    }
    // kids[1..] on kid 0's output that another launch produced (vfo_stage1_finish): the tail launch
    // where it applies, else kid by kid
    int run_rest(const void* s1, int n0, void* out, hipStream_t s) {
        TailArgs t;
        size_t lds = 0;
        const int ok = tail_plan(n0, t, lds);
        if (ok < 0) return ok;
        if (ok) return launch_tail(t, lds, s1, out, s);
        return run_from(1, s1, n0, out, s);
    }
};

// ------------------------------------------------------- block constructors
// (each returns its block even where *rc < 0: the caller deletes it, or publish_block() does)
static std::unique_ptr<FirBlock> make_fir(int dev, int dtype, int ttype, const float* taps, int n, int decim, int* rc,
                                          bool xl = false, double w = 0.0, bool quad = false, float invDev = 1.0f,
                                          bool stereo = false) {
    auto f = std::make_unique<FirBlock>();
    f->xl = xl; f->quad = quad; f->invDev = invDev; f->stereo = stereo;
    *rc = f->setup(dev, dtype, ttype, taps, n, decim);
    if (*rc >= 0 && xl) *rc = f->nco.set_w(w);
    if (*rc >= 0) *rc = f->reset();
    return f;
}
// w: the NCO's step as it is (xlator_effective_omega already applied where the reference applies it;
// applying it twice need not give the same double)
static std::unique_ptr<XlatorBlock> make_xlator(int dev, double w, int* rc) {
    auto x = std::make_unique<XlatorBlock>();
    x->device = dev;
    *rc = x->nco.set_w(w);
    return x;
}
template <typename C = ChainBlock>
static C* new_chain(int dev, int in_dtype, int out_dtype) {
    auto* c = new C();
    c->device = dev; c->in_dtype = in_dtype; c->out_dtype = out_dtype;
    return c;
}

// composition helpers for other translation units (blocks.h)
Block* chain_new(int dev, int in_dtype, int out_dtype) { return new_chain(dev, in_dtype, out_dtype); }
int chain_append(Block* chain, Block* kid) {
    auto* c = dynamic_cast<ChainBlock*>(chain);
    if (!c || !kid) { delete kid; set_error("chain_append: bad argument"); return SDRGPU_EARG; }
    c->kids.emplace_back(kid);
    return SDRGPU_OK;
}
int chain_keep_on_reset(Block* chain, int lastKids) {
    auto* c = dynamic_cast<ChainBlock*>(chain);
    if (!c || lastKids < 0 || (size_t)lastKids > c->kids.size()) { set_error("chain_keep_on_reset: bad argument"); return SDRGPU_EARG; }
    c->keepOnReset = (size_t)lastKids;
    return SDRGPU_OK;
}
int chain_size(Block* chain) {
    auto* c = dynamic_cast<ChainBlock*>(chain);
    return c ? (int)c->kids.size() : -1;
}
Block* chain_kid(Block* chain, int i) {
    auto* c = dynamic_cast<ChainBlock*>(chain);
    return (c && i >= 0 && i < (int)c->kids.size()) ? c->kids[i].get() : nullptr;
}
Block* make_fir_block(int dev, int dtype, int ttype, const float* taps, int n, int decim, bool stereo, int* rc) {
    return make_fir(dev, dtype, ttype, taps, n, decim, rc, false, 0.0, false, 1.0f, stereo).release();
}
Block* make_quad_block(int dev, double deviationRad, int* rc) {
    auto* q = new QuadBlock();
    q->device = dev; q->in_dtype = SDRGPU_C64; q->out_dtype = SDRGPU_F32;
    q->invDev = (float)(1.0 / deviationRad);
    *rc = SDRGPU_OK;
    for (int k = 0; k < 2 && *rc >= 0; k++) *rc = q->din[k].ensure(sizeof(float2));
    if (*rc >= 0) *rc = q->reset();
    return q;
}
Block* make_xlator_block(int dev, double offsetRad, int* rc) {
    return make_xlator(dev, xlator_effective_omega(offsetRad), rc).release();
}
int xlator_block_set_offset(Block* xlator, double offsetRad) {
    auto* x = dynamic_cast<XlatorBlock*>(xlator);
    if (!x) { set_error("not an xlator"); return SDRGPU_ESTATE; }
    return x->nco.set_w(xlator_effective_omega(offsetRad));
}

// PowerDecimator<T> (multirate/power_decimator.h): cascade of plan stages. With
// `xlFirst` the RxVFO's xlator is fused into the first (full-rate) stage.
static int build_power_decim(ChainBlock* c, int dev, int dtype, int ratio, bool xlFirst, double w) {
    if (ratio == 1) return SDRGPU_OK;
    int d[8], n[8];
    const float* t[8];
    int ns = decim_plan(ratio, d, n, t);
    if (ns < 0) return ns;
    for (int i = 0; i < ns; i++) {
        int rc;
        auto f = make_fir(dev, dtype, SDRGPU_F32, t[i], n[i], d[i], &rc, xlFirst && i == 0, w);
        if (rc < 0) return rc;
        c->kids.push_back(std::move(f));
    }
    return SDRGPU_OK;
}

// RationalResampler<T>::reconfigure (multirate/rational_resampler.h:121-167); RationalPlan: blocks.h
int plan_rational(double inSr, double outSr, RationalPlan& rp) {
    if (!(inSr > 0) || !(outSr > 0)) { set_error("rational resampler: bad samplerates"); return SDRGPU_EARG; }
    const int maxRatio = 8192;
    int predecPower = std::min<int>((int)std::floor(std::log2(inSr / outSr)), maxRatio);
    int predecRatio = std::min<int>(predecPower >= 0 && predecPower < 31 ? (1 << predecPower) : maxRatio, maxRatio);
    double intSr = inSr;
    bool useDecim = (inSr > outSr && predecPower > 0);
    if (useDecim) intSr = inSr / (double)predecRatio;
    rp.predec = useDecim ? predecRatio : 1;
    int IntSR = (int)std::round(intSr), OutSR = (int)std::round(outSr);
    int g = std::gcd(IntSR, OutSR);
    rp.interp = OutSR / g;
    rp.decim = IntSR / g;
    if (rp.interp == rp.decim) { rp.mode = useDecim ? 1 : 3; return SDRGPU_OK; }
    double tapSr = intSr * (double)rp.interp;
    double tapBw = std::min<double>(inSr, outSr) / 2.0;
    SDRGPU_CHECK(design_taps(rp.taps, taps_low_pass, tapBw, tapBw * 0.1, tapSr, 0));
    for (auto& v : rp.taps) v *= (float)rp.interp;
    rp.mode = useDecim ? 0 : 2;
    return SDRGPU_OK;
}

static int build_rational(ChainBlock* c, int dev, int dtype, double inSr, double outSr, bool xlFirst, double w) {
    RationalPlan rp;
    SDRGPU_CHECK(plan_rational(inSr, outSr, rp));
    bool xlDone = false;
    if (rp.mode == 0 || rp.mode == 1) {
        SDRGPU_CHECK(build_power_decim(c, dev, dtype, rp.predec, xlFirst, w));
        xlDone = true;
    }
    if (xlFirst && !xlDone) {
        int rc;
        auto x = make_xlator(dev, w, &rc);
        SDRGPU_CHECK(rc);
        c->kids.insert(c->kids.begin(), std::move(x));
    }
    if (rp.mode == 0 || rp.mode == 2) {
        auto p = std::make_unique<PolyBlock>();
        SDRGPU_CHECK(p->setup(dev, dtype, rp.interp, rp.decim, rp.taps.data(), (int)rp.taps.size()));
        c->kids.push_back(std::move(p));
    }
    return SDRGPU_OK;
}
Block* make_xlate_resample_block(int dev, double inSr, double outSr, double w, int* rc) {
    auto* c = new_chain(dev, SDRGPU_C64, SDRGPU_C64);
    *rc = build_rational(c, dev, SDRGPU_C64, inSr, outSr, true, w);
    return c;
}

// RxVFO (channel/rx_vfo.h:24-121)
struct VfoBlock : ChainBlock {
    double inSr = 0, outSr = 0, bw = 0, offset = 0;
    int build() {
        kids.clear();
        const double w = xlator_effective_omega(hz_to_rads(-offset, inSr));
        SDRGPU_CHECK(build_rational(this, device, SDRGPU_C64, inSr, outSr, true, w));
        if (bw != outSr) {
            double fw = bw / 2.0;
            std::vector<float> t;
            SDRGPU_CHECK(design_taps(t, taps_low_pass, fw, fw * 0.1, outSr, 0));
            int rc;
            auto f = make_fir(device, SDRGPU_C64, SDRGPU_F32, t.data(), (int)t.size(), 1, &rc);
            if (rc < 0) return rc;
            kids.push_back(std::move(f));
        }
        return SDRGPU_OK;
    }
    // setOffset keeps the running NCO phase (frequency_xlator.h:25-29)
    int set_offset(double off) {
        offset = off;
        const double w = xlator_effective_omega(hz_to_rads(-offset, inSr));
        for (auto& k : kids) {
            if (auto* f = dynamic_cast<FirBlock*>(k.get()); f && f->xl) return f->nco.set_w(w);
            if (auto* x = dynamic_cast<XlatorBlock*>(k.get())) return x->nco.set_w(w);
        }
        return SDRGPU_OK;
    }
};

// [quadrature, stereo FIR at D = 1] in one launch: wfm_short_kernel for calls up to kShortMax
// samples, wfm_big_kernel above
struct WfmBlock : ChainBlock {
    static constexpr int kShortMax = 1 << 15;
    int run(const void* in, int count, void* out, hipStream_t s) override {
        if (kids.size() != 2) return ChainBlock::run(in, count, out, s);
        auto* qb = static_cast<QuadBlock*>(kids[0].get());
        auto* fb = static_cast<FirBlock*>(kids[1].get());
        if (count <= 0 || fb->D != 1 || fb->Q % WFM_BK != 0 || fb->Q > 256) return ChainBlock::run(in, count, out, s);
        const bool big = count > kShortMax;
        const auto k = big ? wfm_big_kernel : wfm_short_kernel;
        const int per = big ? WFM_BCH : WFM_TM, threads = big ? WFM_BNT : WFM_TM;   // outputs, threads per workgroup
        const int blocks = (int)(((long long)count + per - 1) / per);
        const size_t lds = sizeof(float) * (big ? (size_t)WFM_BK * (WFM_BNT + fb->Q / WFM_BK + 2) + fb->Q : (size_t)(WFM_TM + fb->Q));
        // (+ 1: the last workgroup writes the next call's FIR history and y[-1])
        hipLaunchKernelGGL(k, dim3(blocks + 1), dim3(threads), lds, s, (const float2*)in, count, qb->din[qb->cur].as<float2>(),
                           qb->din[qb->cur ^ 1].as<float2>(), fb->hist[fb->cur].as<float>(), fb->hist[fb->cur ^ 1].as<float>(),
                           fb->taps.as<float>(), fb->Q, fb->ntaps - 1, qb->invDev, (float2*)out);
        SDRGPU_HIP(hipGetLastError());
        qb->cur ^= 1;
        fb->cur ^= 1;
        return count;
    }
};

// ---- a VFO inside the spectrum launches (blocks.h) ----------------------------------------------
// the chain behind a VFO handle and its first stage (null: not such a chain)
static ChainBlock* vfo_chain(sdrgpu_block* vfo) { return vfo && vfo->impl ? dynamic_cast<ChainBlock*>(vfo->impl) : nullptr; }
static FirBlock* vfo_stage1(ChainBlock* c) { return c && !c->kids.empty() ? dynamic_cast<FirBlock*>(c->kids[0].get()) : nullptr; }

int vfo_stage1_prepare(sdrgpu_block* vfo, const void* in, int count, VfoStage1* st) {
    auto* c = vfo_chain(vfo);
    auto* f = vfo_stage1(c);
    if (!f || count <= 0 || !f->rows_external(count)) return 0;
    const int M = f->out_count(count);
    SDRGPU_CHECK(c->scratch[0].ensure(sizeof(float2) * (size_t)M));
    st->a = f->rows_args(in, count, c->scratch[0].p, M, f->hist[f->cur ^ 1].p);
    st->M = M;
    st->count = count;
    st->out = c->scratch[0].p;
    return 1;
}
int vfo_tail_prepare(sdrgpu_block* vfo, const VfoStage1& st, void* out, TailArgs* t, size_t* lds) {
    const int ok = vfo_chain(vfo)->tail_plan(st.M, *t, *lds);
    if (ok <= 0) return ok;
    t->in = reinterpret_cast<const float2*>(st.out);
    t->out = reinterpret_cast<float2*>(out);
    return 1;
}
// called once the launches that carry stage 1 and the tail are in: only then does any stage's state
// move on (a failed launch leaves the VFO as it was, as the header promises)
int vfo_tail_commit(sdrgpu_block* vfo, const VfoStage1& st, const TailArgs& t) {
    auto* c = vfo_chain(vfo);
    vfo_stage1(c)->advance(st.count, st.M);
    return c->advance_tail(t);
}
int vfo_stage1_finish(sdrgpu_block* vfo, const VfoStage1& st, void* out, hipStream_t s) {
    auto* c = vfo_chain(vfo);
    vfo_stage1(c)->advance(st.count, st.M);
    return c->run_rest(st.out, st.M, out, s);
}

// The gate of an entry point that takes a block handle (blocks.h states the entry rule).
int enter_block(::sdrgpu_block* h, bool wait) {
    if (!h || !h->impl) { set_error("null block handle"); return SDRGPU_EARG; }
    SDRGPU_SET_DEVICE(h->impl->device);
    if (wait) SDRGPU_HIP(hipDeviceSynchronize());
    return SDRGPU_OK;
}

// The one way a create function hands a new block to its caller (blocks.h states the entry and ordering rules).
int publish_block(::sdrgpu_block** h, Block* b, int rc) {
    std::unique_ptr<Block> own(b);
    if (rc < 0) return rc;
    SDRGPU_SET_DEVICE(b->device);
    SDRGPU_HIP(hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking));   // the handle's one stream
    // The state written at creation (reset(): memsets / copies on the null stream) must be complete
    // before the first call, which runs on a non-blocking stream the null stream does not order:
    // a handle whose buffer recycled non-zero memory otherwise may start from it (seen once per
    // process on a fresh Quadrature: y[-1] != 0).
    if (hipDeviceSynchronize() != hipSuccess) { set_error("hipDeviceSynchronize failed at create"); return SDRGPU_EHIP; }
    *h = new ::sdrgpu_block{own.release()};
    return SDRGPU_OK;
}

}  // namespace sdrgpu

using namespace sdrgpu;

// ================================================================== C ABI
#define NEED_HANDLE(h) do { if (!(h) || !(h)->impl) { set_error("null block handle"); return SDRGPU_EARG; } } while (0)
#define NEED_OUT(h) do { if (!(h)) { set_error("null out-handle"); return SDRGPU_EARG; } } while (0)

extern "C" int sdrgpu_xlator_create(sdrgpu_block** h, int device, double offsetRad) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    int rc;
    Block* x = make_xlator_block(device, offsetRad, &rc);
    return publish_block(h, x, rc);
}
extern "C" int sdrgpu_xlator_set_offset(sdrgpu_block* h, double offsetRad) {
    SDRGPU_CHECK(enter_block(h, true));   // (a queued call still reads the fine table that set_w rewrites)
    return xlator_block_set_offset(h->impl, offsetRad);
}

extern "C" int sdrgpu_fir_create(sdrgpu_block** h, int device, int dtype, int ttype, const float* taps, int ntaps, int decim) {
    NEED_OUT(h);
    if ((dtype != SDRGPU_F32 && dtype != SDRGPU_C64) || (ttype != SDRGPU_F32 && ttype != SDRGPU_C64) ||
        (dtype == SDRGPU_F32 && ttype == SDRGPU_C64)) {
        set_error("fir_create: unsupported (dtype %d, ttype %d)", dtype, ttype);
        return SDRGPU_EARG;
    }
    SDRGPU_CHECK(FirBlock::decim_ok(decim));
    SDRGPU_SET_DEVICE(device);
    int rc;
    auto f = make_fir(device, dtype, ttype, taps, ntaps, decim, &rc);
    return publish_block(h, f.release(), rc);
}
// the FIR setters read the history back and rewrite it and the tap tables, which a queued call still uses: they wait
extern "C" int sdrgpu_fir_set_taps(sdrgpu_block* h, const float* taps, int ntaps) {
    SDRGPU_CHECK(enter_block(h, true));
    auto* f = dynamic_cast<FirBlock*>(h->impl);
    if (!f) f = find_kid<FirBlock>(h, true);   // the AM chain's low-pass (am.h:51-60)
    if (!f) { set_error("not a FIR"); return SDRGPU_ESTATE; }
    return f->set_taps(taps, ntaps);
}
extern "C" int sdrgpu_fir_set_decimation(sdrgpu_block* h, int decim) {
    SDRGPU_CHECK(enter_block(h, true));
    auto* f = dynamic_cast<FirBlock*>(h->impl);
    if (!f) { set_error("not a FIR"); return SDRGPU_ESTATE; }
    return f->set_decimation(decim);
}

extern "C" int sdrgpu_quadrature_create(sdrgpu_block** h, int device, double deviationRad) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    int rc;
    Block* q = make_quad_block(device, deviationRad, &rc);
    return publish_block(h, q, rc);
}
extern "C" int sdrgpu_quadrature_set_deviation(sdrgpu_block* h, double deviationRad) {
    NEED_HANDLE(h);
    if (auto* q = dynamic_cast<QuadBlock*>(h->impl)) { q->invDev = (float)(1.0 / deviationRad); return SDRGPU_OK; }
    if (auto* f = dynamic_cast<FirBlock*>(h->impl); f && f->quad) { f->invDev = (float)(1.0 / deviationRad); return SDRGPU_OK; }
    set_error("not a quadrature demodulator");
    return SDRGPU_ESTATE;
}

extern "C" int sdrgpu_power_decimator_create(sdrgpu_block** h, int device, int dtype, int ratio) {
    NEED_OUT(h);
    if (ratio < 1 || (ratio & (ratio - 1)) || ratio > (8192)) {
        set_error("power_decimator: ratio %d must be a power of two <= 8192", ratio);   // checkRatio
        return SDRGPU_EARG;
    }
    SDRGPU_SET_DEVICE(device);
    auto* c = new_chain(device, dtype, dtype);
    return publish_block(h, c, build_power_decim(c, device, dtype, ratio, false, 0.0));
}

extern "C" int sdrgpu_polyphase_resampler_create(sdrgpu_block** h, int device, int dtype, int interp, int decim,
                                                 const float* taps, int ntaps) {
    NEED_OUT(h);
    SDRGPU_CHECK(PolyBlock::args_ok(interp, decim, taps, ntaps));
    SDRGPU_SET_DEVICE(device);
    auto* p = new PolyBlock();
    return publish_block(h, p, p->setup(device, dtype, interp, decim, taps, ntaps));
}

extern "C" int sdrgpu_rational_resampler_create(sdrgpu_block** h, int device, int dtype, double inSr, double outSr) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    auto* c = new_chain(device, dtype, dtype);
    return publish_block(h, c, build_rational(c, device, dtype, inSr, outSr, false, 0.0));
}

extern "C" int sdrgpu_rxvfo_create(sdrgpu_block** h, int device, double inSr, double outSr, double bw, double offset) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    auto* v = new_chain<VfoBlock>(device, SDRGPU_C64, SDRGPU_C64);
    v->inSr = inSr; v->outSr = outSr; v->bw = bw; v->offset = offset;
    return publish_block(h, v, v->build());
}
extern "C" int sdrgpu_rxvfo_set_offset(sdrgpu_block* h, double offset) {
    SDRGPU_CHECK(enter_block(h, true));   // (a queued call still reads the NCO tables that set_w rewrites)
    auto* v = dynamic_cast<VfoBlock*>(h->impl);
    if (!v) { set_error("not an RxVFO"); return SDRGPU_ESTATE; }
    return v->set_offset(offset);
}

extern "C" int sdrgpu_ddc_fm_create(sdrgpu_block** h, int device, double offsetRad, const float* taps, int ntaps, int decim,
                                    double deviationRad) {
    NEED_OUT(h);
    SDRGPU_CHECK(FirBlock::decim_ok(decim));
    SDRGPU_SET_DEVICE(device);
    int rc;
    auto f = make_fir(device, SDRGPU_C64, SDRGPU_F32, taps, ntaps, decim, &rc, true, xlator_effective_omega(offsetRad),
                      true, (float)(1.0 / deviationRad));
    return publish_block(h, f.release(), rc);
}

// Fused DDC without the demodulator: FrequencyXlator(offsetRad) -> DecimatingFIR<complex_t,float>
// (frequency_xlator.h:43-50, decimating_fir.h:45-68), complex_t out. The same kernels as the fused
// DDC+FM block with the quadrature epilogue off (RxVFO's first stage has this shape too).
extern "C" int sdrgpu_ddc_create(sdrgpu_block** h, int device, double offsetRad, const float* taps, int ntaps, int decim) {
    NEED_OUT(h);
    SDRGPU_CHECK(FirBlock::decim_ok(decim));
    SDRGPU_SET_DEVICE(device);
    int rc;
    auto f = make_fir(device, SDRGPU_C64, SDRGPU_F32, taps, ntaps, decim, &rc, true, xlator_effective_omega(offsetRad));
    return publish_block(h, f.release(), rc);
}

// FM<float> (demod/fm.h:25-133): quadrature(bw/2) -> optional LPF/HPF/BPF
extern "C" int sdrgpu_fm_create(sdrgpu_block** h, int device, double samplerate, double bandwidth, int lowPass, int highPass) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    int rc;
    auto* c = new_chain(device, SDRGPU_C64, SDRGPU_F32);
    c->kids.emplace_back(make_quad_block(device, hz_to_rads(bandwidth / 2.0, samplerate), &rc));
    if (rc >= 0 && (lowPass || highPass)) {
        std::vector<float> t;
        rc = (lowPass && highPass) ? design_taps(t, taps_band_pass_f, 300.0, bandwidth / 2.0, 100.0, samplerate, 0)
             : highPass            ? design_taps(t, taps_high_pass, 300.0, 100.0, samplerate, 0)
                                   : design_taps(t, taps_low_pass, bandwidth / 2.0, (bandwidth / 2.0) * 0.1, samplerate, 0);
        if (rc >= 0) {
            auto f = make_fir(device, SDRGPU_F32, SDRGPU_F32, t.data(), (int)t.size(), 1, &rc);
            if (rc >= 0) c->kids.push_back(std::move(f));
        }
    }
    return publish_block(h, c, rc);
}

// BroadcastFM, stereo == false (demod/broadcast_fm.h:144-215): quadrature(dev) ->
// 228-tap (at 240 kS/s) audio LPF lowPass(15 kHz, 4 kHz) -> LRToStereo(l = r)
extern "C" int sdrgpu_wfm_create(sdrgpu_block** h, int device, double deviation, double samplerate, int lowPass) {
    NEED_OUT(h);
    SDRGPU_SET_DEVICE(device);
    int rc;
    auto* c = new_chain<WfmBlock>(device, SDRGPU_C64, SDRGPU_C64);
    c->kids.emplace_back(make_quad_block(device, hz_to_rads(deviation, samplerate), &rc));
    if (rc >= 0) {
        std::vector<float> t;
        // unfiltered MPX (or no low-pass at this rate): identity tap, same stereo interleave
        if (!lowPass || design_taps(t, taps_low_pass, 15000.0, 4000.0, samplerate, 0) < 0) t.assign(1, 1.0f);
        auto f = make_fir(device, SDRGPU_F32, SDRGPU_F32, t.data(), (int)t.size(), 1, &rc, false, 0.0, false, 1.0f, true);
        if (rc >= 0) c->kids.push_back(std::move(f));
    }
    return publish_block(h, c, rc);
}

extern "C" int sdrgpu_block_out_count(sdrgpu_block* h, int count) {
    NEED_HANDLE(h);
    return h->impl->out_count(count);
}

extern "C" int sdrgpu_block_process_dev(sdrgpu_block* h, const void* in, int count, void* out, void* stream) {
    SDRGPU_CHECK(enter_block(h));
    if (count < 0 || (count > 0 && (!in || !out))) { set_error("process: bad buffers"); return SDRGPU_EARG; }
    Block* b = h->impl;
    const hipStream_t s = stream ? (hipStream_t)stream : b->own;
    SDRGPU_CHECK(b->order.follow(s));
    OrderScope od(b->order, s);
    return b->run(in, count, out, s);
}

// (the owner's entry point has selected the device)
int sdrgpu::block_run_owned(sdrgpu_block* h, const void* in, int count, void* out, hipStream_t s) {
    NEED_HANDLE(h);
    if (count < 0 || (count > 0 && (!in || !out))) { set_error("process: bad buffers"); return SDRGPU_EARG; }
    return h->impl->run(in, count, out, s);
}

extern "C" int sdrgpu_block_process(sdrgpu_block* h, const void* in, int count, void* out) {
    SDRGPU_CHECK(enter_block(h));
    if (count < 0 || (count > 0 && (!in || !out))) { set_error("process: bad buffers"); return SDRGPU_EARG; }
    Block* b = h->impl;
    const size_t inB = (size_t)std::max(count, 1) * esize(b->in_dtype);
    const int mExp = b->out_count(count);
    const size_t outB = (size_t)std::max(mExp, 1) * esize(b->out_dtype);
    SDRGPU_CHECK(b->pin_in.ensure(inB));
    SDRGPU_CHECK(b->pin_out.ensure(outB));
    SDRGPU_CHECK(b->dev_in.ensure(inB));
    SDRGPU_CHECK(b->dev_out.ensure(outB));
    // buffers registered with sdrgpu_host_register are DMA'd directly; others go through the
    // handle's pinned staging buffers
    const bool inPinned = host_pinned(in, (size_t)count * esize(b->in_dtype));
    const bool outPinned = host_pinned(out, (size_t)mExp * esize(b->out_dtype));
    if (count > 0 && !inPinned) std::memcpy(b->pin_in.p, in, (size_t)count * esize(b->in_dtype));
    SDRGPU_CHECK(b->order.follow(b->own));
    OrderScope od(b->order, b->own);
    if (count > 0)
        SDRGPU_HIP(hipMemcpyAsync(b->dev_in.p, inPinned ? in : b->pin_in.p, (size_t)count * esize(b->in_dtype),
                                  hipMemcpyHostToDevice, b->own));
    int m = b->run(b->dev_in.p, count, b->dev_out.p, b->own);
    if (m < 0) return m;
    void* dst = (outPinned && m <= mExp) ? out : b->pin_out.p;
    if (m > 0) SDRGPU_HIP(hipMemcpyAsync(dst, b->dev_out.p, (size_t)m * esize(b->out_dtype), hipMemcpyDeviceToHost, b->own));
    SDRGPU_HIP(hipStreamSynchronize(b->own));
    if (m > 0 && dst != out) std::memcpy(out, b->pin_out.p, (size_t)m * esize(b->out_dtype));
    return m;
}

extern "C" int sdrgpu_block_reset(sdrgpu_block* h) {
    SDRGPU_CHECK(enter_block(h, true));   // queued calls still read and write the state that reset() rewrites
    int rc = h->impl->reset();
    if (rc >= 0) SDRGPU_HIP(hipDeviceSynchronize());
    return rc;
}

extern "C" int sdrgpu_block_destroy(sdrgpu_block* h) {
    if (!h) return SDRGPU_OK;
    if (h->impl) {
        (void)hipSetDevice(h->impl->device);
        (void)hipDeviceSynchronize();
        delete h->impl;
    }
    delete h;
    return SDRGPU_OK;
}

// ---- ingest converters: mono = one-channel input, I = Q = the converted sample (complex out)
static int convert_dev(bool mono, int device, int kind, const void* in, long long n, void* out, void* stream) {
    if (kind < SDRGPU_CONV_U8 || kind > SDRGPU_CONV_F32 || n < 0 || (n > 0 && (!in || !out))) {
        set_error("%s: bad argument", mono ? "convert_mono" : "convert");
        return SDRGPU_EARG;
    }
    SDRGPU_SET_DEVICE(device);
    if (n == 0) return 0;
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    if (mono) hipLaunchKernelGGL(convert_mono_kernel, g, b, 0, (hipStream_t)stream, kind, in, n, (float2*)out);
    else hipLaunchKernelGGL(convert_kernel, g, b, 0, (hipStream_t)stream, kind, in, n, (float*)out);
    SDRGPU_HIP(hipGetLastError());
    return (int)std::min<long long>(n, 0x7fffffff);
}
// host buffers: to the device, convert_dev, back
static int convert_host(bool mono, int device, int kind, const void* in, long long n, void* out) {
    static const int isz[] = {1, 2, 3, 4, 8, 1, 4};
    if (kind < SDRGPU_CONV_U8 || kind > SDRGPU_CONV_F32 || n < 0) {
        set_error("%s: bad argument", mono ? "convert_mono" : "convert");
        return SDRGPU_EARG;
    }
    if (n == 0) return 0;
    SDRGPU_SET_DEVICE(device);
    const size_t inB = (size_t)n * isz[kind], outB = (size_t)n * (mono ? sizeof(float2) : sizeof(float));
    DevBuf din, dout;
    SDRGPU_CHECK(din.ensure(inB));
    SDRGPU_CHECK(dout.ensure(outB));
    SDRGPU_HIP(hipMemcpy(din.p, in, inB, hipMemcpyHostToDevice));
    SDRGPU_CHECK(convert_dev(mono, device, kind, din.p, n, dout.p, nullptr));
    SDRGPU_HIP(hipMemcpy(out, dout.p, outB, hipMemcpyDeviceToHost));
    return (int)std::min<long long>(n, 0x7fffffff);
}
extern "C" int sdrgpu_convert_dev(int device, int kind, const void* in, long long n, float* out, void* stream) {
    return convert_dev(false, device, kind, in, n, out, stream);
}
extern "C" int sdrgpu_convert_mono_dev(int device, int kind, const void* in, long long n, void* out, void* stream) {
    return convert_dev(true, device, kind, in, n, out, stream);
}
extern "C" int sdrgpu_convert(int device, int kind, const void* in, long long n, float* out) {
    return convert_host(false, device, kind, in, n, out);
}
extern "C" int sdrgpu_convert_mono(int device, int kind, const void* in, long long n, void* out) {
    return convert_host(true, device, kind, in, n, out);
}

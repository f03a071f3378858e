// What the other translation units call in blocks.hip (host side only): chains of blocks and the
// block constructors (loops.hip, symsync.hip), the gate and the publication of a handle (with the rules of who
// selects the device, owns a stream and waits) and the history carry (loops.hip, channelizer.hip, ifnr.hip,
// symsync.hip), the xlator's NCO and the rational resampler's plan (bank.hip), and the hooks through which a spectrum launch carries an RxVFO's stages (fft.hip, frontend.hip).
#pragma once
#include "sdrgpu_internal.h"

namespace sdrgpu {

// ---- composition: a chain of blocks run back to back on one stream ------------------------------
Block* chain_new(int dev, int in_dtype, int out_dtype);
int chain_append(Block* chain, Block* kid);   // takes the kid (deleted on error)
// a freshly built block (its construction's status in rc) joins the chain, or is deleted
inline int append_owned(Block* chain, Block* b, int rc) {
    if (rc < 0) { delete b; return rc; }
    return chain_append(chain, b);
}
// the chain's reset() leaves its last `lastKids` kids as they are
int chain_keep_on_reset(Block* chain, int lastKids);
int chain_size(Block* chain);
Block* chain_kid(Block* chain, int i);
// the first (or last) kid of type T of the chain behind h; null where h is no chain or has none
template <typename T>
T* find_kid(Block* chain, bool last) {
    T* found = nullptr;
    for (int i = 0, n = chain ? chain_size(chain) : 0; i < n; i++) {
        if (auto* k = dynamic_cast<T*>(chain_kid(chain, i))) {
            found = k;
            if (!last) break;
        }
    }
    return found;
}
template <typename T>
T* find_kid(sdrgpu_block* h, bool last) {
    return h ? find_kid<T>(h->impl, last) : nullptr;
}
// Constructors: the block is returned even where *rc < 0 (the caller deletes it).
Block* make_fir_block(int dev, int dtype, int ttype, const float* taps, int n, int decim, bool stereo, int* rc);
Block* make_xlator_block(int dev, double offsetRad, int* rc);
Block* make_quad_block(int dev, double deviationRad, int* rc);
// FrequencyXlator(w) -> RationalResampler<complex_t>(inSr -> outSr) with the xlator fused into the
// first decimation stage (BroadcastFM's RDS branch, broadcast_fm.h:164-171)
Block* make_xlate_resample_block(int dev, double inSr, double outSr, double w, int* rc);

// The taps of one of host_design.cpp's designers (taps_low_pass, taps_high_pass, taps_band_pass_f: with
// out = nullptr they return the count) into t. A negative count is passed through; none: SDRGPU_EARG.
template <typename Fn, typename... A>
int design_taps(std::vector<float>& t, Fn design, A... args) {
    const int n = design(args..., nullptr);
    if (n < 1) return n < 0 ? n : SDRGPU_EARG;
    t.resize(n);
    design(args..., t.data());
    return SDRGPU_OK;
}

// ---- entry points: device, stream, ordering ------------------------------------------------------
// The entry rule, stated once: for a block handle, only the C entry points (and enter_block / publish_block,
// which they call for this purpose) select the device, create the handle's stream and wait for the device.
// Block members (run, reset, setters, the setup of a kid) assume the handle's device is current and touch no
// stream but the one they are given: a chain's kids, inner chains and BroadcastFM's RDS branch have none.
// enter_block is the gate of an extern "C" function that takes a sdrgpu_block* and touches the device: a null
// handle is SDRGPU_EARG, else the handle's device is selected and, with `wait`, idle on return. A create
// function selects the device once its own argument checks are done and ends in publish_block: rc < 0 deletes
// b and passes rc on; else b gets the handle's one stream, the device is synchronised and *h is the new handle.
// The ordering rule, stated once: a block's calls run on non-blocking streams, which the null stream does not
// order. An entry point that rewrites device state which a queued call may still read or write (a reset, an
// NCO or tap table, a latched gain; a query that reads state back) waits first: enter_block(h, true). One that
// wrote device state on the null stream (a memset or a copy in setup(), reset() or a setter) ends with
// hipDeviceSynchronize(): publish_block for a create, sdrgpu_block_reset for a reset, and the setter itself
// otherwise (sdrgpu_fmif_set_bins; sdrgpu_broadcast_fm_set_rds when it builds the RDS chain). Block::reset()
// implementations do not synchronise: a chain's reset pays for one, not one per kid. (A setter whose only device
// write is a blocking hipMemcpy from host memory, AgcBlock::set_gain, has nothing pending when it returns; one
// that only latches host-side parameters, the next call's kernel arguments, needs neither wait.)
int enter_block(::sdrgpu_block* h, bool wait = false);
int publish_block(::sdrgpu_block** h, Block* b, int rc);

// The history carry on its own launch (fir_hist_kernel): next = the last H elements (of dtype) of
// [hist || in] after `count` inputs. nco (non-null, C64): the fused xlator applied to the `in` samples,
// from its per-call table.
struct Nco;
int carry_history(int dtype, const Nco* nco, const DevBuf& hist, const void* in, DevBuf& next, int H, int count,
                  hipStream_t s);

// ---- the xlator's NCO for a translator outside blocks.hip (bank.hip) ----------------------------
// The host Nco of XlatorBlock, as that block drives it: nco_set_w(w = xlator_effective_omega(offsetRad))
// keeps the running phase; per call of `count` samples nco_prepare (the per-call coarse table on s; *phi
// and *plo are the tables nco_tab reads), the launch, then nco_advance(count). The device is selected
// by the caller.
Nco* nco_new();
void nco_delete(Nco* n);
int nco_set_w(Nco* n, double w);
int nco_prepare(Nco* n, int count, hipStream_t s, const float2** phi, const float2** plo);
void nco_advance(Nco* n, long long count);
void nco_reset(Nco* n);
// FrequencyXlator::setOffset (frequency_xlator.h:25-29) of an xlator block (make_xlator_block): the phase is kept;
// SDRGPU_ESTATE on another block. The caller has waited for the device: a queued call still reads the table.
int xlator_block_set_offset(Block* xlator, double offsetRad);

// ---- the rational resampler's plan for a resampler outside blocks.hip (bank.hip) -----------------
// RationalResampler<T>::reconfigure (multirate/rational_resampler.h:121-167), host only: mode 0 = PowerDecimator
// (predec) then PolyphaseResampler(interp, decim, taps), 1 = the decimator alone, 2 = the resampler alone, 3 = a
// copy; taps = lowPass(min(in, out) / 2, 10 %, intSr * interp) * interp. Sample rates not > 0: SDRGPU_EARG.
struct RationalPlan {
    int mode = 3, predec = 1, interp = 1, decim = 1;
    std::vector<float> taps;
};
int plan_rational(double inSr, double outSr, RationalPlan& rp);

// ---- an RxVFO inside the spectrum launches ------------------------------------------------------
struct VfoStage1;   // fir_rows.h
struct TailArgs;    // fir_tail.h
// A VFO's first stage (row kernel) run by the spectrum launches over the same device batch
// (fft.hip, sdrgpu_fft_execute_vfo_dev / _zoom_vfo_dev): vfo_stage1_prepare fills the launch
// arguments for a call of `count` samples at `in` without touching the VFO's state (1: fusable,
// 0: not -- the caller then runs the VFO on its own; < 0: error); the caller launches all M / (16 *
// RS) segment workgroups (16 segments of 128 outputs each) and the history workgroup; then
// vfo_stage1_finish commits the stage's state and runs the VFO's remaining stages into `out`.
// These hooks are block members in effect: the caller's entry point has selected the device.
int vfo_stage1_prepare(::sdrgpu_block* vfo, const void* in, int count, VfoStage1* st);
int vfo_stage1_finish(::sdrgpu_block* vfo, const VfoStage1& st, void* out, hipStream_t s);
// the tail of a VFO whose first stage ran in the front end's pass-A launch, as the pass-B launch
// carries it: 1 = t / lds filled, no state changed -- the caller launches the t.G tail
// workgroups, then calls vfo_tail_commit (stage 1 and the tail stages move on together); 0 = not
// applicable (nothing changed: the caller then calls vfo_stage1_finish)
int vfo_tail_prepare(::sdrgpu_block* vfo, const VfoStage1& st, void* out, TailArgs* t, size_t* lds);
int vfo_tail_commit(::sdrgpu_block* vfo, const VfoStage1& st, const TailArgs& t);

}  // namespace sdrgpu

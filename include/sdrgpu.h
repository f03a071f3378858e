/*
 * sdrgpu.h -- C ABI of the MI355X (gfx950) streaming-DSP hot path of SDR++.
 *
 * Plain pointers and sizes only; no C++ or torch types. Two calling styles:
 *   *_process(...)      drop-in for the reference's host-buffer process(count, in, out)
 *                       (synchronous, host pointers; staged through pinned memory)
 *   *_process_dev(...)  device-resident batches on a caller stream (hipStream_t as void*,
 *                       NULL = the handle's own stream); asynchronous, host-side state
 *                       (decimation offsets, output counts) is updated at call time.
 * Every call returns >= 0 on success (an output count where meaningful) or a
 * negative SDRGPU_E* code; sdrgpu_last_error() gives the thread's last message.
 * A handle is used by one thread at a time (the reference's one-worker-per-block
 * model, core/src/dsp/block.h:70-76).
 *
 * Reference interfaces replaced (paths in qrp73/SDRPP, core/src/...):
 *   spectrum  : IQFrontEnd::handler + updateFFTSize, signal_path/iq_frontend.cpp:230-249,272-296
 *   windows   : dsp::window::createWindow, dsp/window/window.h:38-64
 *   taps      : dsp::taps::{lowPass,highPass,bandPass,windowedSinc}, dsp/taps/
 *   FIR       : dsp::filter::FIR::process, dsp/filter/fir.h:62-83
 *   decim FIR : dsp::filter::DecimatingFIR::process, dsp/filter/decimating_fir.h:45-68
 *   xlator    : dsp::channel::FrequencyXlator::process, dsp/channel/frequency_xlator.h:43-50
 *   power dec : dsp::multirate::PowerDecimator::process, dsp/multirate/power_decimator.h:51-70
 *   polyphase : dsp::multirate::PolyphaseResampler::process, dsp/multirate/polyphase_resampler.h:69-99
 *   rational  : dsp::multirate::RationalResampler, dsp/multirate/rational_resampler.h:83-167
 *   VFO       : dsp::channel::RxVFO::process, dsp/channel/rx_vfo.h:89-100
 *   quadrature: dsp::demod::Quadrature::process, dsp/demod/quadrature.h:41-56
 *   FM        : dsp::demod::FM<float>::process, dsp/demod/fm.h:86-103
 *   WFM       : dsp::demod::BroadcastFM::process (mono), dsp/demod/broadcast_fm.h:144-215
 *   ingest    : file_source converters, source_modules/file_source/src/main.cpp:361-542
 *   symbols   : loop::FastAGC, loop::Costas, clock_recovery::MM, digital::BinarySlicer,
 *               digital::DifferentialDecoder, demod::PSK, demod::GFSK (dsp/loop/fast_agc.h, dsp/loop/costas.h,
 *               dsp/clock_recovery/mm.h, dsp/digital/, dsp/demod/psk.h, dsp/demod/gfsk.h)
 */
#ifndef SDRGPU_H
#define SDRGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDRGPU_VERSION 100

enum {
    SDRGPU_OK = 0,
    SDRGPU_EARG = -1,     /* invalid argument (reference: assert / std::runtime_error) */
    SDRGPU_EHIP = -2,     /* HIP runtime error (name in sdrgpu_last_error) */
    SDRGPU_ENOMEM = -3,
    SDRGPU_ESTATE = -4,   /* wrong handle kind / not initialised */
    SDRGPU_ENODEV = -5,
    SDRGPU_ETIMEOUT = -6  /* a peer rank did not answer within the deadline (gather: communicator aborted) */
};

/* element types (dsp::complex_t is {float re, im}, dsp/types.h:6; stereo_t {float l, r}) */
/* SDRGPU_U8: uint8_t symbols / bits (digital/binary_slicer.h, digital/differential_decoder.h) */
enum { SDRGPU_F32 = 0, SDRGPU_C64 = 1, SDRGPU_U8 = 2 };

/* window ids = dsp::window::windowType (dsp/window/window.h:27-35) */
enum { SDRGPU_WIN_RECTANGULAR = 0, SDRGPU_WIN_HAMMING, SDRGPU_WIN_HANN, SDRGPU_WIN_BLACKMAN,
       SDRGPU_WIN_NUTTALL, SDRGPU_WIN_BLACKMAN_HARRIS4, SDRGPU_WIN_BLACKMAN_HARRIS7 };

/* ----------------------------------------------------------- runtime ---- */
int         sdrgpu_version(void);
const char* sdrgpu_last_error(void);
int         sdrgpu_device_count(void);
int         sdrgpu_malloc(int device, void** dptr, size_t bytes);
int         sdrgpu_free(void* dptr);
int         sdrgpu_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int         sdrgpu_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int         sdrgpu_stream_create(int device, void** stream);
int         sdrgpu_stream_destroy(void* stream);
int         sdrgpu_stream_synchronize(void* stream);
int         sdrgpu_host_register(void* ptr, size_t bytes);   /* pin a dsp::stream buffer */
int         sdrgpu_host_unregister(void* ptr);
int         sdrgpu_host_alloc(void** ptr, size_t bytes);   /* pinned + registered (DMA'd directly) */
int         sdrgpu_host_free(void* ptr);

/* ------------------------------------------- host-side design (exact) ---- */
/* Bit-exact restatements evaluated on the host, as the reference does. */
int  sdrgpu_create_window(int type, float* buffer, int size, int centered);          /* window.h:38 */
void sdrgpu_gen_reshape_params(double sampleRate, int size, double rate, int* skip, int* nz); /* iq_frontend.h:56 */
int  sdrgpu_taps_estimate_count(double transWidth, double sampleRate);               /* estimate_tap_count.h:4 */
int  sdrgpu_taps_windowed_sinc(int count, double omega, double norm, float* out);   /* windowed_sinc.h:9 (window::nuttall) */
int  sdrgpu_taps_low_pass(double cutoff, double transWidth, double sampleRate, int odd, float* out); /* low_pass.h:7; out NULL -> count */
int  sdrgpu_taps_high_pass(double cutoff, double transWidth, double sampleRate, int odd, float* out); /* high_pass.h:7 */
int  sdrgpu_taps_band_pass_f(double start, double stop, double transWidth, double sampleRate, int odd, float* out); /* band_pass.h:11 */
int  sdrgpu_taps_band_pass_c(double start, double stop, double transWidth, double sampleRate, int odd, float* out);
int  sdrgpu_decim_plan(int ratio, int* decims, int* ntaps, const float** taps);      /* decim/plans.h */
/* taps::rootRaisedCosine<float>(count, beta, Ts) (taps/root_raised_cosine.h:8-29), Ts = samplerate /
 * symbolrate; fp64, rounded once; out NULL -> count */
int  sdrgpu_taps_root_raised_cosine(int count, double beta, double Ts, float* out);
/* host only: clock_recovery::MM's interpolator bank (clock_recovery/mm.h:173-178): phases x tapsPerPhase
 * floats, row p = interpBank.phases[p] (multirate/polyphase_bank.h:32-34); returns phases * tapsPerPhase
 * (out NULL too); phases in [1, SDRGPU_MM_MAX_PHASES], tapsPerPhase in [1, SDRGPU_MM_MAX_TAPS] */
#define SDRGPU_MM_MAX_PHASES 1024
#define SDRGPU_MM_MAX_TAPS 64
int  sdrgpu_mm_interp_bank(int phases, int tapsPerPhase, float* out);

/* --------------------------------------------------------- spectrum ---- */
/* Window * FFT(N, forward, unnormalised) * 10*log10(|X|^2) of nz <= N samples,
 * zero-padded to N (iq_frontend.cpp:230-249 + :295). N = 2^k, 64 <= N <= 2^20. */
typedef struct sdrgpu_fft sdrgpu_fft;
typedef struct sdrgpu_block sdrgpu_block;   /* stream blocks (below) */
int sdrgpu_fft_create(sdrgpu_fft** h, int device, int fftSize, int nz, int windowType);
int sdrgpu_fft_set_window(sdrgpu_fft* h, const float* window, int nz);   /* exact host floats */
int sdrgpu_fft_set_window_type(sdrgpu_fft* h, int windowType, int nz);
/* device batch: frame f starts at in + f*frameStride complex samples; out: frames x N floats */
int sdrgpu_fft_execute_dev(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out, void* stream);
/* rows + the waterfall's full-span zoom rows (fft_scaler(0, bw, bw, N, zoomSize).doZoom of each
 * row, gui/widgets/fft_scaler.h:27-64) into zoomOut (frames x zoomSize floats). With N = 65536 and
 * zoomSize = 2048 the zoom is fused into the transform's last pass. */
int sdrgpu_fft_execute_zoom_dev(sdrgpu_fft* h, const void* in, long long frameStride, int frames, float* out,
                                float* zoomOut, int zoomSize, void* stream);
/* spectrum + one RxVFO over the same device batch of `frames` back-to-back frames (frame stride
 * N, nz = N: fftRate = fs / N), the VFO reading the batch in place as the front end's splitter
 * feeds both (iq_frontend.cpp:15-52, splitter.h:46-60), on one stream. Returns the VFO's output
 * count (vfoOut). On the 64k plan with an RxVFO whose first stage is the D = 32 row decimator
 * (61.44 MS/s -> 240 kHz) that stage runs inside the spectrum launches, so the batch is read from
 * HBM once; otherwise the spectrum and the VFO run as two launch groups. */
int sdrgpu_fft_execute_vfo_dev(sdrgpu_fft* h, const void* in, int frames, float* out, sdrgpu_block* vfo,
                               void* vfoOut, void* stream);
/* the same + the waterfall's full-span zoom rows (as sdrgpu_fft_execute_zoom_dev; zoomOut may be NULL) */
int sdrgpu_fft_execute_zoom_vfo_dev(sdrgpu_fft* h, const void* in, int frames, float* out, float* zoomOut,
                                    int zoomSize, sdrgpu_block* vfo, void* vfoOut, void* stream);
/* (not in the reference; its IQFrontEnd hands the spectrum and each VFO to blocks on their own
 * threads, iq_frontend.cpp:15-52) A second stream for sdrgpu_fft_execute_zoom_vfo_dev calls with zoom
 * rows: the VFO's later stages and the zoom fold run on `tailStream`, so they overlap the next call's
 * spectrum launch on the call's stream instead of following it. Then `out` (the dB rows) is complete
 * on the call's stream, while `vfoOut` and `zoomOut` are complete on `tailStream`: their consumers
 * (a demodulator, a gather) must run on, or wait for, `tailStream`. Results are bit-identical to the
 * one-stream calls. NULL turns it off (waiting for tails in flight). */
int sdrgpu_fft_set_tail_stream(sdrgpu_fft* h, void* tailStream);
/* (measurement, not in the reference) HIP events around each call's spectrum launch group -- the
 * fused VFO stage included, the VFO's later stages not; group_times returns the last
 * min(n, calls, 256) group times in ms, oldest first, waiting for them */
int sdrgpu_fft_set_timing(sdrgpu_fft* h, int on);
int sdrgpu_fft_group_times(sdrgpu_fft* h, float* ms, int n);
/* drop-in for IQFrontEnd::handler: in = host complex_t[nz]; out = host float[N] or NULL
 * (acquireFFTBuffer may return NULL; the spectrum is then computed but not written). */
int sdrgpu_fft_logmag(sdrgpu_fft* h, const void* in, float* out);
int sdrgpu_fft_size(sdrgpu_fft* h);
/* spectrum arithmetic (not in the reference: the north_star's <= 1 ulp parity mode):
 * 0 = fp32 kernels (default; FFTW-class accuracy), 1 = fp64 interior: the reference's fp32 window
 * product (volk_32fc_32f_multiply_32fc), then fp64 butterflies, twiddles, |X|^2 and 10 log10,
 * rounded once to fp32 -- the correctly rounded dB of the exact DFT up to ~1e-15. Waits for the
 * device; the zoom rows of sdrgpu_fft_execute_zoom_dev are then computed unfused. */
int sdrgpu_fft_set_precision(sdrgpu_fft* h, int mode);
int sdrgpu_fft_get_precision(sdrgpu_fft* h);
/* 64k transform form (not in the reference; FFTW picks its plan per size the same way). The 64k
 * plan has two fp32 kernels that round differently: the one-pass transform (one radix-4 DIF step
 * into four 16k sub-transforms, fft_1p_kernel) and the two-pass 256 x 256 four-step launches. Both
 * meet the spectrum parity bar against the exact DFT, but they are not bit-identical to each other:
 * rows of the same frame differ by at most 0.05 dB anywhere and 1e-3 dB within 40 dB of the frame's
 * peak (further down, each form's fp32 error is a growing fraction of the bin: 60 dB below a noise
 * frame's peak two rows were measured 5.4e-3 dB apart) (tests/test_gpu_parity.py::
 * test_spectrum_64k_rows_vs_call_size, test_spectrum_onepass_rows_and_zoom). mode 2 (the default) picks
 * per call: one-pass for calls of >= 64 frames, two-pass below (a reference-size block of 4.7
 * frames runs faster there), so a stream's 64k rows then depend on how it is batched into calls.
 * mode 1 (always one-pass) or 0 (always two-pass) pins the form per plan: rows then depend only on
 * the frame. Other sizes have one form and ignore the mode. The device front end
 * (sdrgpu_frontend_*) pins its plans to 0. Returns the previous mode. */
int sdrgpu_fft_set_kernel(sdrgpu_fft* h, int mode);
int sdrgpu_fft_destroy(sdrgpu_fft* h);

/* ---------------------------------------------------- stream blocks ---- */
/* FrequencyXlator (offset in rad/sample, like init(in, offset)) */
int sdrgpu_xlator_create(sdrgpu_block** h, int device, double offsetRad);
int sdrgpu_xlator_set_offset(sdrgpu_block* h, double offsetRad);
/* FIR<D,T> (decim = 1) and DecimatingFIR<D,T>: dtype/ttype SDRGPU_F32 or SDRGPU_C64 */
int sdrgpu_fir_create(sdrgpu_block** h, int device, int dtype, int ttype, const float* taps, int ntaps, int decim);
int sdrgpu_fir_set_taps(sdrgpu_block* h, const float* taps, int ntaps);   /* (also on an AM handle: its low-pass, am.h:51-60) */
int sdrgpu_fir_set_decimation(sdrgpu_block* h, int decim);
/* Quadrature (deviation in rad/sample) */
int sdrgpu_quadrature_create(sdrgpu_block** h, int device, double deviationRad);
int sdrgpu_quadrature_set_deviation(sdrgpu_block* h, double deviationRad);
/* PowerDecimator<T> (ratio = 1 or 2^k <= 8192), PolyphaseResampler<T>, RationalResampler<T> */
int sdrgpu_power_decimator_create(sdrgpu_block** h, int device, int dtype, int ratio);
int sdrgpu_polyphase_resampler_create(sdrgpu_block** h, int device, int dtype, int interp, int decim, const float* taps, int ntaps);
int sdrgpu_rational_resampler_create(sdrgpu_block** h, int device, int dtype, double inSamplerate, double outSamplerate);
/* RxVFO: xlator(-offset) -> rational resampler -> LPF(bw/2) if bw != outSr */
int sdrgpu_rxvfo_create(sdrgpu_block** h, int device, double inSamplerate, double outSamplerate, double bandwidth, double offset);
int sdrgpu_rxvfo_set_offset(sdrgpu_block* h, double offset);
/* Fused DDC: xlator(offsetRad) -> DecimatingFIR<complex_t,float>(taps, decim); complex_t out
 * (frequency_xlator.h:43-50 + decimating_fir.h:45-68 in one kernel) */
int sdrgpu_ddc_create(sdrgpu_block** h, int device, double offsetRad, const float* taps, int ntaps, int decim);
/* Fused DDC: xlator(offsetRad) -> DecimatingFIR<complex_t,float>(taps, decim) -> Quadrature(deviationRad); float out */
int sdrgpu_ddc_fm_create(sdrgpu_block** h, int device, double offsetRad, const float* taps, int ntaps, int decim, double deviationRad);
/* FM<float> (demod/fm.h) and BroadcastFM mono (stereo_t out, broadcast_fm.h) */
int sdrgpu_fm_create(sdrgpu_block** h, int device, double samplerate, double bandwidth, int lowPass, int highPass);
int sdrgpu_wfm_create(sdrgpu_block** h, int device, double deviation, double samplerate, int lowPass);
/* Serial loops (one workgroup per stream; bit-identical to the reference arithmetic) */
/* loop::AGC<T> (loop/agc.h:13-147); dtype F32 or C64; setGain latched at the next process() */
int sdrgpu_agc_create(sdrgpu_block** h, int device, int dtype, double setPoint, double attack, double decay,
                      double maxGain, double maxOutputAmp, double initGain);
int sdrgpu_agc_set_params(sdrgpu_block* h, double setPoint, double attack, double decay, double maxGain,
                          double maxOutputAmp, double initGain);   /* agc.h:44-79 setters (state kept) */
int sdrgpu_agc_set_enabled(sdrgpu_block* h, int enabled);      /* agc.h:38 */
int sdrgpu_agc_set_gain(sdrgpu_block* h, float gain);          /* agc.h:31 */
int sdrgpu_agc_get_gain(sdrgpu_block* h, float* gain);         /* agc.h:28 (synchronises) */
/* correction::DCBlocker<T> (correction/dc_blocker.h:17-60); rate = rate_hz / samplerate */
int sdrgpu_dc_blocker_create(sdrgpu_block** h, int device, int dtype, double rate);
int sdrgpu_dc_blocker_set_rate(sdrgpu_block* h, double rate);   /* dc_blocker.h:30 (also on an AM handle) */
/* demod::AM<T> (demod/am.h:27-142): agcMode 0 OFF, 1 CARRIER, 2 AUDIO; stereo != 0 -> stereo_t out.
 * sdrgpu_block_reset is AM::reset() (am.h:104-112): the AGCs and the DC blocker; the low-pass keeps its history. */
int sdrgpu_am_create(sdrgpu_block** h, int device, int agcMode, double bandwidth, double agcAttack, double agcDecay,
                     double dcBlockRate, double samplerate, int stereo);
/* demod::SSB<T> (demod/ssb.h:20-105): mode 0 USB, 1 LSB, 2 DSB; stereo != 0 -> stereo_t out */
int sdrgpu_ssb_create(sdrgpu_block** h, int device, int mode, double bandwidth, double samplerate, int agcEnabled,
                      double agcAttack, double agcDecay, int stereo);
/* demod::CW<T> (demod/cw.h:15-28, 72-85): xlate by hzToRads(tone, samplerate) -> Re -> AGC(1, attack, decay,
 * 10e6, 1.0, 1.0), enabled iff agcEnabled [-> MonoToStereo]; arguments in CW::init's order; stereo != 0 ->
 * stereo_t out. sdrgpu_block_reset resets the phase and the AGC. */
int sdrgpu_cw_create(sdrgpu_block** h, int device, double tone, int agcEnabled, double agcAttack, double agcDecay,
                     double samplerate, int stereo);
int sdrgpu_cw_set_tone(sdrgpu_block* h, double tone);   /* cw.h:30-35: phase kept; SDRGPU_ESTATE on another handle */
/* AGC inside an AM / SSB / CW handle: which 0 = first AGC (AM carrier AGC, SSB AGC, CW AGC), 1 = last (AM
 * audio AGC); am.h:63-97 setAGCGain/getAGCGain/setAGCAttack/setAGCDecay, ssb.h:62-84, cw.h:37-63 */
int sdrgpu_demod_agc_set_gain(sdrgpu_block* h, int which, float gain);
int sdrgpu_demod_agc_get_gain(sdrgpu_block* h, int which, float* gain);
int sdrgpu_demod_agc_set_enabled(sdrgpu_block* h, int which, int enabled);
int sdrgpu_demod_agc_set_attack_decay(sdrgpu_block* h, double attack, double decay);
/* demod::BroadcastFM with the stereo decoder (broadcast_fm.h:34-60, 144-215): quadrature ->
 * pilot band-pass (complex taps) -> PLL (loop/pll.h) -> L+R / L-R matrix -> audio low-pass;
 * stereo_t out. stereo = 0 gives the mono path (= sdrgpu_wfm_create). */
int sdrgpu_broadcast_fm_create(sdrgpu_block** h, int device, double deviation, double samplerate, int stereo, int lowPass);
/* RDS branch (broadcast_fm.h:121-127, 164-171, 193-203): when on, every process call
 * also produces complex_t RDS baseband = RationalResampler(fs -> 5 kHz)(FrequencyXlator(-57 kHz)(MPX)),
 * read with rds_dev (device pointer + count of the last call) or read_rds (host copy).
 * sdrgpu_broadcast_fm_set_rds switches the branch and keeps all state. The reference's setRDSOut also calls
 * reset(): setRDSOut is sdrgpu_broadcast_fm_set_rds followed by sdrgpu_block_reset.
 * sdrgpu_block_reset is BroadcastFM::reset() (broadcast_fm.h:130-142): the demodulator, the pilot filter and PLL,
 * the delays and the audio filters. The RDS branch's xlator phase and resampler history survive it. */
int sdrgpu_broadcast_fm_set_rds(sdrgpu_block* h, int enabled);
int sdrgpu_broadcast_fm_rds_dev(sdrgpu_block* h, const void** out, int* n);
int sdrgpu_broadcast_fm_read_rds(sdrgpu_block* h, void* out, int max);
/* filter::Deemphasis<T> (filter/deephasis.h:57-93): dtype F32 (float) or C64 (stereo_t);
 * serial recurrence, bit-identical to the reference arithmetic */
int sdrgpu_deemphasis_create(sdrgpu_block** h, int device, int dtype, double tau, double samplerate);
int sdrgpu_deemphasis_set(sdrgpu_block* h, double tau, double samplerate);   /* setTau / setSamplerate */
/* M-channel critically sampled polyphase channelizer (BASELINE C4): channel k of output frame
 * m is FrequencyXlator(-k fs/M) -> DecimatingFIR<complex_t,float>(taps, M) (frequency_xlator.h:43,
 * decimating_fir.h:45) with an exact NCO; taps <= 16 M (bank layout polyphase_bank.h:32).
 * Output: frames x M complex, out[m*M + k]; out_count = frames * M. M in {256, 512, 1024}. */
int sdrgpu_channelizer_create(sdrgpu_block** h, int device, int channels, const float* taps, int ntaps);
/* The channelizer's per-frame M-point DFT (same definition as above): mode 0 = LDS FFT (default),
 * 1 = the polyphase filterbank "cast as batched MFMA GEMM" (BASELINE C4): 1024 = 32 x 32, two
 * complex 32x32 products per frame on v_mfma_f32_16x16x4_f32. M = 1024 only. */
int sdrgpu_channelizer_set_dft(sdrgpu_block* h, int mode);
/* IF noise reduction: the three optional blocks of the radio module between the VFO and the
 * demodulator (decoder_modules/radio/src/radio_module.h:73-79). All C64 -> C64, out_count == count;
 * in and out must not overlap. */
/* noise_reduction::FMIF (noise_reduction/fm_if.h:20-77): per sample, the nuttall-windowed DFT of the
 * last `bins` samples, the bin of largest magnitude (lowest on a tie) kept, sample bins/2 of the
 * unnormalised back transform out. bins in [3, 32] (radio_module.h:30-35 offers 9, 15, 31, 32),
 * checked before the device is selected. History (bins - 1 samples, zero at creation / reset /
 * set_bins) stays on the device; results do not depend on how the stream is cut into calls. */
#define SDRGPU_FMIF_MIN_BINS 3
#define SDRGPU_FMIF_MAX_BINS 32
int sdrgpu_fmif_create(sdrgpu_block** h, int device, int bins);
int sdrgpu_fmif_set_bins(sdrgpu_block* h, int bins);          /* setBins (fm_if.h:26-34): new window, history cleared */
int sdrgpu_fmif_window(int bins, float* out);                 /* host only: the `bins` window floats (fm_if.h:112) */
/* noise_reduction::NoiseBlanker (noise_reduction/noise_blanker.h:12-57): serial recurrence on the
 * running amplitude, bit-identical to the reference arithmetic; amp survives set, reset -> 1.0f */
int sdrgpu_noise_blanker_create(sdrgpu_block** h, int device, double rate, double level);
int sdrgpu_noise_blanker_set(sdrgpu_block* h, double rate, double level);   /* setRate / setLevel (noise_blanker.h:19-30) */
/* noise_reduction::Squelch (noise_reduction/squelch.h:19-63): per call, level = 20 log10f(mean |x|)
 * against `level` dB with the 1 dB hysteresis and the 10-call unmute count; decision and gated copy
 * run on the caller's stream without a host synchronise. The count is per handle (the reference's is
 * a function-local static shared by every squelch of the process). */
int sdrgpu_squelch_create(sdrgpu_block** h, int device, double level);
int sdrgpu_squelch_set_level(sdrgpu_block* h, double level);  /* setLevel (squelch.h:27-31): from the next call */
int sdrgpu_squelch_get_muted(sdrgpu_block* h, int* muted);    /* state after the last call (synchronises) */

/* ------------------------------------------------ symbol recovery ---- */
/* The blocks behind WFM's "Decode RDS" (decoder_modules/radio/src/demodulators/wfm.h:56-69) and the
 * digital demodulators made of them. The loops are serial recurrences run by one workgroup per stream,
 * every step in the reference's operation order without contraction; state stays on the device between
 * calls, so results do not depend on how a stream is cut into calls. A setter also takes the handle of
 * a chain that holds its block (sdrgpu_fast_agc_set / sdrgpu_costas_set_* on a PSK handle: the first
 * such block; sdrgpu_mm_set_* on a PSK, GFSK or RDS handle: its last block). */
/* loop::FastAGC<T> (loop/fast_agc.h:13-79); dtype F32 or C64; bit-identical to the reference
 * arithmetic. _set = setSetPoint / setMaxGain / setRate / setInitGain (:24-46, the gain is kept);
 * set_gain (:48) is latched and applied at the next call; reset -> initGain (:54) */
int sdrgpu_fast_agc_create(sdrgpu_block** h, int device, int dtype, double setPoint, double maxGain, double rate, double initGain);
int sdrgpu_fast_agc_set(sdrgpu_block* h, double setPoint, double maxGain, double rate, double initGain);
int sdrgpu_fast_agc_set_gain(sdrgpu_block* h, double gain);
int sdrgpu_fast_agc_get_gain(sdrgpu_block* h, float* gain);    /* (synchronises) */
/* loop::Costas<ORDER> (loop/costas.h:17-45 over loop/pll.h:15-62, loop/phase_control_loop.h:58-85);
 * order 2, 4 or 8; C64 -> C64. Arguments in PLL::init's order (pll.h:15); alpha / beta =
 * criticallyDamped(bandwidth) in float (pll.h:20-22). The phasor is the device libm's cosf / sinf, so
 * outputs follow the reference within the loop's own sensitivity to the last bit of the phasor
 * (DESIGN.md 3.3), not bit for bit. reset -> initPhase, initFreq (pll.h:55-62). SDRGPU_EARG: an order
 * other than 2 / 4 / 8, minFreq >= maxFreq (the reference asserts), a phase or frequency that is not
 * finite or beyond 1024 rad (the phase wrap is a subtraction loop). */
int sdrgpu_costas_create(sdrgpu_block** h, int device, int order, double bandwidth, double initPhase, double initFreq,
                         double minFreq, double maxFreq);
int sdrgpu_costas_set_bandwidth(sdrgpu_block* h, double bandwidth);                  /* pll.h:27 */
int sdrgpu_costas_set_freq_limits(sdrgpu_block* h, double minFreq, double maxFreq);   /* pll.h:49: clamps freq at the next call */
/* loop::PLL (loop/pll.h:15-25, 64-70) and loop::CarrierTrackingPLL (loop/carrier_tracking_pll.h:14-20); C64 -> C64.
 * Per sample, PLL emits phasor(phase) taken before the advance and CarrierTrackingPLL the input derotated by
 * it; both advance by normalizePhase(atan2f(in.im, in.re) - phase) of the INPUT sample. Arguments in
 * PLL::init's order (pll.h:15) -- the constructors of PLL, CarrierTrackingPLL and MeteorCostas pass
 * (initFreq, initPhase) swapped to it (pll.h:13, carrier_tracking_pll.h:10-12, meteor_costas.h:11): a port of
 * code that constructs them swaps the two. The coefficients, reset and the refusals of sdrgpu_costas_create
 * (but for its order); atan2f, cosf and sinf are the device libm's, so outputs follow the reference within
 * the loop's own sensitivity. sdrgpu_costas_set_bandwidth and sdrgpu_costas_set_freq_limits are
 * the setBandwidth (pll.h:27) and setFrequencyLimits (pll.h:49) of these two loops and of MeteorCostas as well. */
int sdrgpu_pll_create(sdrgpu_block** h, int device, double bandwidth, double initPhase, double initFreq, double minFreq,
                      double maxFreq);
int sdrgpu_carrier_pll_create(sdrgpu_block** h, int device, double bandwidth, double initPhase, double initFreq, double minFreq,
                              double maxFreq);
/* loop::MeteorCostas (decoder_modules/meteor_demodulator/src/meteor_costas.h:13-16, 24-56); C64 -> C64; arguments in
 * its init's order (:13). With brokenModulation 0 the error is Costas<4>'s (:53) and the block is bit-identical
 * to sdrgpu_costas_create(order 4); else the error is the distance of the derotated sample's atan2f phase to the
 * nearest of PHASE1..4 (:36-49), times its amplitude, clamped to [-1, 1]. set_broken_modulation (:18-22) applies
 * from the next call and keeps the loop state; it also takes a Meteor handle. */
int sdrgpu_meteor_costas_create(sdrgpu_block** h, int device, double bandwidth, int brokenModulation, double initPhase,
                                double initFreq, double minFreq, double maxFreq);
int sdrgpu_meteor_costas_set_broken_modulation(sdrgpu_block* h, int enabled);
/* clock_recovery::MM<T> (clock_recovery/mm.h:24-156); dtype F32 or C64. Output count and every
 * output are bit-identical to the reference arithmetic with these definitions / deviations:
 *  - the interpolator dot product (volk_32f_x2_dot_prod_32f / volk_32fc_32f_dot_prod_32fc, whose SIMD
 *    variants are unpinned) is VOLK's generic kernel: ascending tap order, fp32, unfused;
 *  - the T - 1 history samples start as zeros (the reference leaves them uninitialised); reset
 *    (mm.h:87-98) keeps them, as the reference does;
 *  - create and the setters refuse (SDRGPU_EARG) parameters with omega * (1 - omegaRelLimit) - muGain
 *    < 1: with that every output consumes at least one input sample, a call of `count` samples makes
 *    at most `count` outputs, and sdrgpu_block_out_count(count) returns that CAPACITY (= count), not
 *    the exact count, for this block and for every chain that ends in it (PSK, GFSK, RDS);
 *  - the exact count is the call's return value: the kernel writes it to device memory and
 *    process_dev WAITS for the stream to read it, once, at the end of the call.
 * set_omega (mm.h:40-50) also zeroes offset and phase; set_gains / set_omega_rel_limit (:52-71) keep
 * the state. Setters apply at the next call. */
int sdrgpu_mm_create(sdrgpu_block** h, int device, int dtype, double omega, double omegaGain, double muGain,
                     double omegaRelLimit, int interpPhases, int interpTaps);
int sdrgpu_mm_set_omega(sdrgpu_block* h, double omega);
int sdrgpu_mm_set_gains(sdrgpu_block* h, double omegaGain, double muGain);
int sdrgpu_mm_set_omega_rel_limit(sdrgpu_block* h, double omegaRelLimit);
/* digital::BinarySlicer (digital/binary_slicer.h:12-18): F32 -> U8, out = in > 0.0f */
int sdrgpu_binary_slicer_create(sdrgpu_block** h, int device);
/* digital::DifferentialDecoder (digital/differential_decoder.h:14-47): U8 -> U8,
 * out[i] = (in[i] - in[i-1] + modulus) % modulus; the previous call's last symbol is carried */
int sdrgpu_differential_decoder_create(sdrgpu_block** h, int device, int modulus, int initSym);
/* demod::PSK<ORDER> (demod/psk.h:25-43, 138-143): FIR(rootRaisedCosine) -> FastAGC(1, 10e6, agcRate)
 * -> Costas<order>(costasBandwidth) -> MM<complex_t>(samplerate / symbolrate, ...); C64 -> C64 symbols */
int sdrgpu_psk_create(sdrgpu_block** h, int device, int order, double symbolrate, double samplerate, int rrcTapCount,
                      double rrcBeta, double agcRate, double costasBandwidth, double omegaGain, double muGain,
                      double omegaRelLimit);
/* demod::Meteor, the LRPT demodulator (decoder_modules/meteor_demodulator/src/meteor_demod.h:24-43, 150-167;
 * main.cpp:66 creates it as init(in, 72000, 150000, 33, 0.6, 0.1, 0.005, broken, oqpsk, 1e-6, 0.01)):
 * FIR(rootRaisedCosine) -> FastAGC(1, 10e6, agcRate) -> MeteorCostas(costasBandwidth, brokenModulation) -> with
 * oqpsk, the one-sample I/Q stagger of :155-164 -> MM<complex_t>(samplerate / symbolrate, ...); C64 -> C64
 * symbols. Arguments in init's order (:24). The RRC FIR sums as the stream banks' FIR does (ascending tap order, fp32,
 * no contraction: VOLK's generic kernel), not as sdrgpu_fir_create: the chain then differs from the reference by the
 * loop's libm alone, and a column of sdrgpu_bank_meteor_create is this chain bit for bit. The stagger runs in the loop's kernel; its carry lastI (:188) lives on
 * the device, starts at 0, is carried across calls (empty ones too), is updated only while oqpsk is on, keeps
 * its value while it is off, and reset (:139-148: the four blocks) does not touch it. The refusals of
 * sdrgpu_psk_create, all before the device is selected; count and capacity as sdrgpu_mm_create (the return
 * value is the exact count; the call waits once). set_broken_modulation (:127) and set_oqpsk (:133) apply from
 * the next call. sdrgpu_mm_set_*, sdrgpu_fast_agc_set and sdrgpu_costas_set_bandwidth reach its blocks. */
int sdrgpu_meteor_create(sdrgpu_block** h, int device, double symbolrate, double samplerate, int rrcTapCount, double rrcBeta,
                         double agcRate, double costasBandwidth, int brokenModulation, int oqpsk, double omegaGain,
                         double muGain, double omegaRelLimit);
int sdrgpu_meteor_set_broken_modulation(sdrgpu_block* h, int enabled);
int sdrgpu_meteor_set_oqpsk(sdrgpu_block* h, int enabled);
/* demod::GFSK (demod/gfsk.h:24-41, 131-135): Quadrature(deviation) -> FIR(rootRaisedCosine) ->
 * MM<float>; C64 -> F32 soft symbols */
int sdrgpu_gfsk_create(sdrgpu_block** h, int device, double symbolrate, double samplerate, double deviation, int rrcTapCount,
                       double rrcBeta, double omegaGain, double muGain, double omegaRelLimit);
/* WFM's RDS symbol chain with wfm.h:57-68's constants: C64 RDS baseband at 5 kS/s (it may be the device
 * pointer of sdrgpu_broadcast_fm_rds_dev) -> FastAGC(1, 1e6, 0.1) -> Costas<2>(0.005) -> FIR(bandPass
 * <complex_t>(0, 2375, 100, 5000)) -> Costas<2>(0.01, 0, w, 0.9 w, 1.1 w), w = hzToRads(2375 / 2, 5000)
 * -> ComplexToReal -> MM<float>(5000 / 1187.5, 1e-6, 0.01, 0.01) -> BinarySlicer ->
 * DifferentialDecoder(2); U8 bits out (what rds::RDSDecoder takes). The slicer and the decoder run in
 * the MM kernel's epilogue; rds_symbols_dev gives the last call's soft symbols (what wfm.h:71-73 feeds
 * the symbol diagram): device pointer and count, valid until the next call. */
int sdrgpu_rds_create(sdrgpu_block** h, int device);
int sdrgpu_rds_symbols_dev(sdrgpu_block* h, const float** out, int* n);

int sdrgpu_block_process(sdrgpu_block* h, const void* in, int count, void* out);      /* host buffers */
int sdrgpu_block_process_dev(sdrgpu_block* h, const void* in, int count, void* out, void* stream);
int sdrgpu_block_out_count(sdrgpu_block* h, int count);   /* exact output count of the next call (MM and chains ending in it: the capacity) */
int sdrgpu_block_reset(sdrgpu_block* h);
int sdrgpu_block_destroy(sdrgpu_block* h);

/* ---------------------------------------------------- stream banks ---- */
/* A bank is S independent streams that share one set of parameters, each with its own state: element
 * m of stream k is x[m * S + k], the layout sdrgpu_channelizer writes (out[m * M + k], S = M), so a
 * channelizer's device output feeds a bank as it is. Outputs have the same layout. A call processes
 * `frames` rows; state and history stay on the device, and results do not depend on how the rows are
 * cut into calls. The loops (FastAGC, Costas, MM) run one lane per stream, 64 streams per wave, on the
 * per-sample steps of the single-stream kernels: every column is bit-identical to the single-stream
 * block fed that column. Parameters are fixed at creation (sdrgpu_bank_agc_set_gain and
 * sdrgpu_bank_xlator_set_offset excepted).
 * Every create function takes (handle, device, streams, the arguments of the single-stream create
 * function in its order) and applies that function's checks; streams < 1 is SDRGPU_EARG. All checks run
 * before the device is selected. frames * streams beyond INT_MAX (the kernels' index type) is
 * SDRGPU_EARG at the call, streams beyond INT_MAX / 64 (state words and history rows) at create. */
typedef struct sdrgpu_bank sdrgpu_bank;
/* demod::Quadrature per stream (demod/quadrature.h:41-56); C64 -> F32; every stream's previous sample is
 * 0 after create / reset */
int sdrgpu_bank_quadrature_create(sdrgpu_bank** h, int device, int streams, double deviationRad);
/* filter::FIR<D, float> per stream (filter/fir.h:60-80): real taps shared by all streams, dtype F32 or
 * C64, no decimation (sdrgpu_bank_decimating_fir_create has it); out[m*S + k] = sum_j buf_k[m + j] * taps[j] over [ntaps - 1 history rows || new],
 * taps not reversed, summed in ascending tap order in fp32 without contraction (not bit-identical to
 * sdrgpu_fir_create, whose kernel and summation order depend on the shape); history zero at create / reset */
int sdrgpu_bank_fir_create(sdrgpu_bank** h, int device, int streams, int dtype, const float* taps, int ntaps);
/* loop::FastAGC<T> per stream (loop/fast_agc.h:13-79); reset -> initGain */
int sdrgpu_bank_fast_agc_create(sdrgpu_bank** h, int device, int streams, int dtype, double setPoint, double maxGain, double rate,
                                double initGain);
/* loop::Costas<ORDER> per stream (loop/costas.h:17-45 over loop/pll.h:15-62, loop/phase_control_loop.h:58-85);
 * the refusals of sdrgpu_costas_create; bit-identical to it on the same device */
int sdrgpu_bank_costas_create(sdrgpu_bank** h, int device, int streams, int order, double bandwidth, double initPhase,
                              double initFreq, double minFreq, double maxFreq);
/* clock_recovery::MM<T> per stream (clock_recovery/mm.h:24-156) with the definitions, deviations and
 * refusals of sdrgpu_mm_create. The output counts depend on the data and differ per stream: output j of
 * stream k is out[j*S + k] for j < counts[k]; the elements of a row past a stream's count are left as
 * they were. sdrgpu_bank_out_rows(frames) = frames is the capacity; the call WAITS for its stream once,
 * at the end, and returns the largest per-stream count (the rows that hold anything). reset keeps the
 * (T - 1) x S history (mm.h:87-98). */
int sdrgpu_bank_mm_create(sdrgpu_bank** h, int device, int streams, int dtype, double omega, double omegaGain, double muGain,
                          double omegaRelLimit, int interpPhases, int interpTaps);
/* demod::PSK<ORDER> per stream (demod/psk.h:25-43, 138-143): bank FIR(rootRaisedCosine) -> bank
 * FastAGC(1, 10e6, agcRate) -> bank Costas<order> -> bank MM<complex_t>, the constants of
 * sdrgpu_psk_create; bit-identical to those banks run one after another; counts as the MM bank */
int sdrgpu_bank_psk_create(sdrgpu_bank** h, int device, int streams, int order, double symbolrate, double samplerate,
                           int rrcTapCount, double rrcBeta, double agcRate, double costasBandwidth, double omegaGain,
                           double muGain, double omegaRelLimit);
/* loop::PLL, loop::CarrierTrackingPLL and loop::MeteorCostas per stream (loop/pll.h:64-70,
 * loop/carrier_tracking_pll.h:14-20, decoder_modules/meteor_demodulator/src/meteor_costas.h:24-56); the arguments and
 * refusals of the single-stream create functions; every column bit-identical to them on the same device */
int sdrgpu_bank_pll_create(sdrgpu_bank** h, int device, int streams, double bandwidth, double initPhase, double initFreq,
                           double minFreq, double maxFreq);
int sdrgpu_bank_carrier_pll_create(sdrgpu_bank** h, int device, int streams, double bandwidth, double initPhase, double initFreq,
                                   double minFreq, double maxFreq);
int sdrgpu_bank_meteor_costas_create(sdrgpu_bank** h, int device, int streams, double bandwidth, int brokenModulation,
                                     double initPhase, double initFreq, double minFreq, double maxFreq);
/* demod::Meteor per stream (meteor_demod.h:24-43, 150-167): bank FIR(rootRaisedCosine) -> bank FastAGC(1, 10e6,
 * agcRate) -> bank MeteorCostas with the per-stream stagger (lastI[S], kept by reset) -> bank MM<complex_t>, the
 * constants of sdrgpu_meteor_create; bit-identical to those banks run one after another; counts as the MM bank */
int sdrgpu_bank_meteor_create(sdrgpu_bank** h, int device, int streams, double symbolrate, double samplerate, int rrcTapCount,
                              double rrcBeta, double agcRate, double costasBandwidth, int brokenModulation, int oqpsk,
                              double omegaGain, double muGain, double omegaRelLimit);
/* demod::GFSK per stream (demod/gfsk.h:24-41, 131-135): bank Quadrature(deviation) -> bank
 * FIR(rootRaisedCosine) -> bank MM<float>; C64 -> F32 soft symbols */
int sdrgpu_bank_gfsk_create(sdrgpu_bank** h, int device, int streams, double symbolrate, double samplerate, double deviation,
                            int rrcTapCount, double rrcBeta, double omegaGain, double muGain, double omegaRelLimit);

/* -- analogue receiver banks: a channelizer's rows to squelched AM / NFM audio per channel.
 * The AGC, the DC blocker and the de-emphasis run one lane per stream on the per-sample steps of the
 * single-stream kernels: every column is bit-identical to the single-stream block fed that column in
 * the same calls. Every call is asynchronous on its stream; a call of 0 frames changes nothing. */
/* loop::AGC<T> per stream (loop/agc.h:13-147), dtype F32 or C64; `enabled` 0 is the fixed-gain limiter
 * (agc.h:127-141, the branch AM's OFF mode runs). The clip look-ahead (agc.h:109-118) is the maximum of |x|
 * from the sample to the end of the CALL for that stream, as in the reference: results depend on where
 * calls end, exactly as sdrgpu_agc_create's do. reset -> amp = setPoint / initGain, gain = min(maxGain, initGain) */
int sdrgpu_bank_agc_create(sdrgpu_bank** h, int device, int streams, int dtype, double setPoint, double attack, double decay,
                           double maxGain, double maxOutputAmp, double initGain, int enabled);
/* AGC::setGain (agc.h:31-35) for all streams, latched at the next call with rows; also on a
 * sdrgpu_bank_am_create / _ssb_create / _cw_create handle (the last AGC of the chain: AM's audio AGC);
 * SDRGPU_ESTATE without an AGC */
int sdrgpu_bank_agc_set_gain(sdrgpu_bank* h, float gain);
/* correction::DCBlocker<T> per stream (correction/dc_blocker.h:54-60), dtype F32 or C64; offset 0 at create / reset */
int sdrgpu_bank_dc_blocker_create(sdrgpu_bank** h, int device, int streams, int dtype, double rate);
/* filter::Deemphasis<float> per stream (filter/deephasis.h:58-65, 91-94); F32; alpha as sdrgpu_deemphasis_create */
int sdrgpu_bank_deemphasis_create(sdrgpu_bank** h, int device, int streams, double tau, double samplerate);
/* noise_reduction::Squelch per stream (noise_reduction/squelch.h:33-63); C64 -> C64. Per call and stream:
 * 20 log10f(mean |x| over the call's rows), the mute state machine (10 calls above the level before
 * unmute, 1 dB hysteresis) with a count per stream, and the row copied or zeroed. A stream's rows are
 * summed in an order that depends on `frames` alone (32-row tiles in ascending rows, then the tiles in
 * ascending order): not the order of sdrgpu_squelch_create, so a level within rounding of a threshold may
 * decide differently. */
int sdrgpu_bank_squelch_create(sdrgpu_bank** h, int device, int streams, double level);
int sdrgpu_bank_squelch_muted(sdrgpu_bank* h, int* muted);   /* muted[S] after the last call (synchronises) */
/* demod::FM<float> per stream (demod/fm.h:25-44, 86-93, 117-145): bank Quadrature(bandwidth / 2 at
 * samplerate) -> bank FIR of the taps of sdrgpu_fm_create (low, high or band pass; none with both flags
 * off); C64 -> F32 mono; bit-identical to those banks run one after another */
int sdrgpu_bank_fm_create(sdrgpu_bank** h, int device, int streams, double samplerate, double bandwidth, int lowPass, int highPass);
/* demod::AM<float> per stream (demod/am.h:28-49, 114-131): agcMode 0 OFF, 1 CARRIER, 2 AUDIO;
 * [CARRIER: bank AGC<C64>(1, attack, decay, 10e6, 10, inf)] -> |x| (volk_32fc_magnitude_32f) -> bank
 * DCBlocker -> [not CARRIER: bank AGC<F32>, enabled iff AUDIO] -> bank FIR(lowPass(bandwidth / 2,
 * 0.1 bandwidth / 2, samplerate)); C64 -> F32 mono; bit-identical to those banks run one after another */
int sdrgpu_bank_am_create(sdrgpu_bank** h, int device, int streams, int agcMode, double bandwidth, double agcAttack,
                          double agcDecay, double dcBlockRate, double samplerate);

/* -- SSB and CW receiver banks */
/* channel::FrequencyXlator per stream (channel/frequency_xlator.h:15-50): one offset and one running phase
 * shared by all streams (they start together): out[m*S + k] = in[m*S + k] * nco(row m), the NCO of
 * sdrgpu_xlator_create; column k is bit-identical to such a handle fed column k in the same calls. C64 -> C64;
 * reset zeroes the phase (frequency_xlator.h:35-41) */
int sdrgpu_bank_xlator_create(sdrgpu_bank** h, int device, int streams, double offsetRad);
/* the same followed by convert::ComplexToReal (ssb.h:92-93, cw.h:73-75) in one launch: C64 -> F32, bit-identical
 * to the real part of the xlator bank's output; the first stage of the SSB and CW banks on its own */
int sdrgpu_bank_xlator_real_create(sdrgpu_bank** h, int device, int streams, double offsetRad);
/* setOffset (frequency_xlator.h:25-29): keeps the running phase, applies from the next call; also on a
 * sdrgpu_bank_ssb_create / sdrgpu_bank_cw_create handle (its xlator); SDRGPU_ESTATE without one */
int sdrgpu_bank_xlator_set_offset(sdrgpu_bank* h, double offsetRad);
/* demod::SSB<float> per stream (demod/ssb.h:21-35, 90-105, 119-126): mode 0 USB, 1 LSB, 2 DSB; xlate by
 * hzToRads(+bandwidth/2 | -bandwidth/2 | 0, samplerate) -> Re -> bank AGC<F32>(1, attack, decay, 10e6, 10, inf),
 * enabled iff agcEnabled; C64 -> F32 mono; bit-identical to the xlator bank, the real part and the AGC bank
 * run one after another (the first two are one launch) */
int sdrgpu_bank_ssb_create(sdrgpu_bank** h, int device, int streams, int mode, double bandwidth, double samplerate,
                           int agcEnabled, double agcAttack, double agcDecay);
/* demod::CW<float> per stream (demod/cw.h:15-28, 72-85): xlate by hzToRads(tone, samplerate) -> Re -> bank
 * AGC<F32>(1, attack, decay, 10e6, 1.0, 1.0); arguments in CW::init's order; C64 -> F32 mono */
int sdrgpu_bank_cw_create(sdrgpu_bank** h, int device, int streams, double tone, int agcEnabled, double agcAttack,
                          double agcDecay, double samplerate);

/* -- rate-changing banks: a bank that writes another number of rows than it reads. All streams
 * share the ratio and start together, so they share one decimation phase and one row count: counts[k] is the
 * rows returned for every k, and sdrgpu_bank_out_rows(frames) is exact. dtype F32 or C64 (stereo_t is C64); real
 * taps shared by all streams; sums in ascending tap order in fp32 without contraction, as sdrgpu_bank_fir_create;
 * history zero at create / reset, which also zeroes phase and offset. Every call is asynchronous on its
 * stream; a call of 0 frames, or one that yields no row, changes only the carried phase and history. At a call,
 * rows in or rows out (of any stage) times streams beyond INT_MAX is SDRGPU_EARG. */
/* filter::DecimatingFIR<D, float> per stream (filter/decimating_fir.h:45-68): out[j*S + k] = sum_t buf_k[offset +
 * j*decim + t] * taps[t] over [ntaps - 1 history rows || new], taps not reversed, offset carried as the
 * reference does (offset -= count); bit-identical to rows [offset :: decim] of sdrgpu_bank_fir_create's output.
 * decim < 1, or (ntaps - 1) * streams beyond INT_MAX: SDRGPU_EARG */
int sdrgpu_bank_decimating_fir_create(sdrgpu_bank** h, int device, int streams, int dtype, const float* taps, int ntaps, int decim);
/* multirate::PolyphaseResampler<T> per stream (multirate/polyphase_resampler.h:69-99) over the bank of
 * multirate/polyphase_bank.h:15-47 (phases[P-1-(i%P)][i/P] = taps[i], zero-padded to ceil(ntaps / interp) per
 * phase); interp = 1 is bit-identical to the decimating FIR bank. interp or decim < 1, history rows * streams or
 * interp * taps-per-phase beyond INT_MAX: SDRGPU_EARG */
int sdrgpu_bank_polyphase_resampler_create(sdrgpu_bank** h, int device, int streams, int dtype, int interp, int decim,
                                           const float* taps, int ntaps);
/* multirate::PowerDecimator<T> per stream (multirate/power_decimator.h:51-108): the stages of
 * sdrgpu_decim_plan(ratio) as decimating FIR banks one after another, bit-identical to them; ratio 1 copies;
 * a ratio the plan refuses: SDRGPU_EARG */
int sdrgpu_bank_power_decimator_create(sdrgpu_bank** h, int device, int streams, int dtype, int ratio);
/* multirate::RationalResampler<T> per stream (multirate/rational_resampler.h:121-167) with the plan and taps of
 * sdrgpu_rational_resampler_create: power decimator bank and / or polyphase resampler bank, or a copy;
 * bit-identical to those banks run one after another. An interpolating plan writes more rows than it reads:
 * size `out` by sdrgpu_bank_out_rows. */
int sdrgpu_bank_rational_resampler_create(sdrgpu_bank** h, int device, int streams, int dtype, double inSamplerate,
                                          double outSamplerate);

/* -- broadcast FM banks: stereo_t is C64 with (l, r) = (re, im); rows out = rows in; every call is
 * asynchronous on its stream; a call of 0 frames changes nothing. No RDS branch, no setters. */
/* filter::FIR<complex_t, complex_t> per stream (filter/fir.h:75, volk_32fc_x2_dot_prod_32fc): `taps` is ntaps (re, im)
 * pairs shared by all streams, not reversed; out[m*S + k] = sum_t buf_k[m + t] * taps[t] over [ntaps - 1 history
 * rows || new], per tap re += (x.re*t.re) - (x.im*t.im), im += (x.re*t.im) + (x.im*t.re), in ascending tap order in
 * fp32 without contraction, so the result does not depend on how the rows are cut into calls. Output C64. in_dtype
 * C64: the block itself; F32: convert::RealToComplex first (demod/broadcast_fm.h:149-152) in the same launch,
 * bit-identical to C64 input with zero imaginary parts (finite taps). History zero at create / reset. in_dtype not
 * F32 / C64, null taps, ntaps < 1, or (ntaps - 1) * streams beyond INT_MAX: SDRGPU_EARG */
int sdrgpu_bank_fir_complex_create(sdrgpu_bank** h, int device, int streams, int in_dtype, const float* taps, int ntaps);
/* The stereo decoder of demod::BroadcastFM per stream (demod/broadcast_fm.h:147-162, 173-190; loop/pll.h:64-70), F32 MPX
 * -> C64 (l, r), with the constants of sdrgpu_broadcast_fm_create: pilot filter = the complex-tap FIR bank with
 * bandPass<complex_t>(18750, 19250, 3000, samplerate, odd) on the real MPX, PLL(25000 / samplerate, 0, 19 kHz, 18.75 kHz,
 * 19.25 kHz) one lane per stream on the single-stream block's step, delay ((np - 1) / 2) + 1 rows, then its matrix
 * expression. reset: the filter and delay histories to zero, (phase, freq) to (0, 19 kHz) (:129-141). Not bit-identical to
 * the single-stream block, whose pilot filter sums in another order. samplerate not > 0, or pilot taps * streams beyond
 * INT_MAX: SDRGPU_EARG */
int sdrgpu_bank_stereo_decoder_create(sdrgpu_bank** h, int device, int streams, double samplerate);
/* demod::BroadcastFM per stream (demod/broadcast_fm.h:34-60, 144-215), C64 -> C64 (l, r); arguments in the order of
 * sdrgpu_broadcast_fm_create. stereo: bank quadrature(hzToRads(deviation, samplerate)) -> stereo decoder bank ->
 * [lowPass: sdrgpu_bank_fir_create(C64, lowPass(15000, 4000, samplerate))]; mono: bank quadrature -> [lowPass: the same
 * taps, F32] -> (l, r) = (x, x) (:211). Bit-identical to those banks run one after another. samplerate or deviation not
 * > 0, or a samplerate at which the audio low-pass has no taps (as sdrgpu_broadcast_fm_create, with lowPass or
 * without): SDRGPU_EARG */
int sdrgpu_bank_broadcast_fm_create(sdrgpu_bank** h, int device, int streams, double deviation, double samplerate, int stereo,
                                    int lowPass);
/* filter::Deemphasis<stereo_t> per stream (filter/deephasis.h:66-76, 91-94): C64 rows of (l, r), each channel
 * bit-identical to sdrgpu_deemphasis_create(SDRGPU_C64 as stereo_t) fed that column; samplerate not > 0: SDRGPU_EARG */
int sdrgpu_bank_deemphasis_stereo_create(sdrgpu_bank** h, int device, int streams, double tau, double samplerate);

/* device buffers of frames * S (in) and sdrgpu_bank_out_rows(frames) * S (out) elements, on `stream` (0:
 * the handle's own); asynchronous except for a bank that ends in MM (above). Returns the rows written. */
int sdrgpu_bank_process_dev(sdrgpu_bank* h, const void* in, int frames, void* out, void* stream);
int sdrgpu_bank_process(sdrgpu_bank* h, const void* in, int frames, void* out);   /* host buffers (synchronous) */
/* the rows the next call of `frames` rows writes, from the handle's current phase and offset (which it does not
 * advance): exact for every bank but one that ends in MM, where it is the capacity (frames) */
int sdrgpu_bank_out_rows(sdrgpu_bank* h, int frames);
int sdrgpu_bank_out_counts(sdrgpu_bank* h, int* counts);  /* counts[S]: per-stream outputs of the last call (synchronises) */
int sdrgpu_bank_streams(sdrgpu_bank* h);
int sdrgpu_bank_reset(sdrgpu_bank* h);
int sdrgpu_bank_destroy(sdrgpu_bank* h);

/* ------------------------------------------------- device IQ front end ---- */
/* IQFrontEnd's data path on the device (signal_path/iq_frontend.cpp:15-52, 115-249; SURVEY
 * 8f rank 1): ingest conversion -> [PowerDecimator] -> [DCBlocker] -> [Conjugate] -> VFOs
 * (RxVFO, read in place) + spectrum frames (Reshaper keep = nz / skip from genReshapeParams,
 * window * FFT * log-power). Replaces the SampleFrameBuffer -> Splitter -> Reshaper memcpy
 * fan-out: one H2D per sample, every consumer reads the block from HBM.
 * kind: -1 complex float, else SDRGPU_CONV_* (interleaved IQ of that sample format). */
typedef struct sdrgpu_frontend sdrgpu_frontend;
int sdrgpu_frontend_create(sdrgpu_frontend** f, int device, double sampleRate, int decimRatio, int dcBlocking,
                           int fftSize, double fftRate, int windowType);                    /* IQFrontEnd::init */
int sdrgpu_frontend_destroy(sdrgpu_frontend* f);
int sdrgpu_frontend_configure(sdrgpu_frontend* f, double sampleRate, int decimRatio, int dcBlocking); /* setSampleRate/setDecimation/setDCBlocking */
int sdrgpu_frontend_set_invert_iq(sdrgpu_frontend* f, int enabled);                       /* setInvertIQ */
int sdrgpu_frontend_set_fft(sdrgpu_frontend* f, int fftSize, double fftRate, int windowType);  /* setFFTSize/Rate/Window */
int sdrgpu_frontend_framing(sdrgpu_frontend* f, int* nz, int* skip, double* effectiveSampleRate);
int sdrgpu_frontend_add_vfo(sdrgpu_frontend* f, int* id, double outSampleRate, double bandwidth, double offset); /* addVFO */
int sdrgpu_frontend_remove_vfo(sdrgpu_frontend* f, int id);                                /* removeVFO */
int sdrgpu_frontend_set_vfo_offset(sdrgpu_frontend* f, int id, double offset);
/* push a block; returns the number of spectrum rows completed by it */
int sdrgpu_frontend_push(sdrgpu_frontend* f, const void* in, int count, int kind);          /* host block (synchronous) */
int sdrgpu_frontend_push_dev(sdrgpu_frontend* f, const void* in, int count, int kind, void* stream); /* device block (async) */
int sdrgpu_frontend_spectra_dev(sdrgpu_frontend* f, const float** rows, int* nrows);       /* returns N */
int sdrgpu_frontend_read_spectra(sdrgpu_frontend* f, float* out, int maxRows);
int sdrgpu_frontend_vfo_dev(sdrgpu_frontend* f, int id, const void** out, int* n);
int sdrgpu_frontend_read_vfo(sdrgpu_frontend* f, int id, void* out, int max);
/* host copy of the last push's preprocessed IQ (what bound IQ streams receive, iq_frontend.cpp:114-120) */
int sdrgpu_frontend_read_iq(sdrgpu_frontend* f, void* out, int max);
/* Pipelined host call style (the IQFrontEnd drop-in's worker, round 3): submit enqueues a host
 * block's H2D on the front end's copy stream, its processing and the read-back of its rows, VFO
 * outputs and (flags & SDRGPU_FE_IQ) preprocessed IQ into pinned result slots, and returns a
 * ticket without waiting; block k + 1's H2D overlaps block k's kernels and read-back. collect
 * waits for a ticket and returns its row count with pinned host pointers to its results (valid
 * until release). At most two tickets are in flight: release(k) before submitting block k + 2.
 * A registered (sdrgpu_host_register / sdrgpu_host_alloc) `in` is DMA'd directly and must stay
 * untouched until its ticket is collected; any other `in` is staged and may be reused at once. */
#define SDRGPU_FE_IQ 1
int sdrgpu_frontend_submit(sdrgpu_frontend* f, const void* in, int count, int kind, int flags);
int sdrgpu_frontend_collect(sdrgpu_frontend* f, int ticket, const float** rows, const void** iq, int* niq);
int sdrgpu_frontend_collected_vfo(sdrgpu_frontend* f, int ticket, int id, const void** out, int* n);
int sdrgpu_frontend_release(sdrgpu_frontend* f, int ticket);

/* ------------------------------------------ spectra gather (multi-GPU) ---- */
/* Independent IQ streams run one per GPU; the only collective is a gather of their
 * spectrum rows to rank 0 (the display) over RCCL / xGMI. Rank 0 makes a communicator id, the
 * host hands it to every rank out of band, each rank creates its handle on its own GPU.
 * gather_rows: `count` device floats of this rank -> rank 0's out[r * count + i] (out: world x
 * count device floats, rank 0 only), asynchronous on `stream` (RCCL send/recv in one group).
 * RCCL is loaded at first use; without it these calls fail with SDRGPU_ESTATE. */
#define SDRGPU_GATHER_ID_BYTES 128
typedef struct sdrgpu_gather sdrgpu_gather;
int sdrgpu_gather_get_id(void* id /* SDRGPU_GATHER_ID_BYTES */);
/* Every wait on the peers has a deadline (SDRGPU_GATHER_TIMEOUT_S, default 120 s; set_timeout per
 * handle): create and rows poll the non-blocking communicator, wait polls `stream`; on expiry the
 * communicator is aborted and the call returns SDRGPU_ETIMEOUT naming the rank (the reference never
 * blocks forever on a stopped peer either: utils/threading.h:53-62, dsp/stream.h:94-116). After a
 * failure the handle accepts only destroy. create's device < 0: the thread's current device. */
int sdrgpu_gather_create(sdrgpu_gather** g, int device, int rank, int world, const void* id);
int sdrgpu_gather_set_timeout(sdrgpu_gather* g, double seconds);
int sdrgpu_gather_rows(sdrgpu_gather* g, const float* rows, long long count, float* out, void* stream);
int sdrgpu_gather_wait(sdrgpu_gather* g, void* stream, double timeoutS /* <= 0: the handle's */);
int sdrgpu_gather_destroy(sdrgpu_gather* g);

/* ---------------------------------------------- spectrum/IQ consumers ---- */
/* waterfall zoom, fft_scaler(viewOffset, viewBandwidth, wholeBandwidth, fftSize, outSize).doZoom
 * (gui/widgets/fft_scaler.h:27-64) on device dB rows: out[r][o] = max over the reference's bins */
typedef struct sdrgpu_zoom sdrgpu_zoom;
int sdrgpu_zoom_create(sdrgpu_zoom** z, int device, double viewOffset, double viewBandwidth, double wholeBandwidth,
                       int fftSize, int outSize);
int sdrgpu_zoom_execute_dev(sdrgpu_zoom* z, const float* rows, int nrows, float* out, void* stream);
int sdrgpu_zoom_destroy(sdrgpu_zoom* z);
/* SampleStreamCompressor::process (compression/sample_stream_compressor.h:26-60) of a device block:
 * pcmType 0 I8, 1 I16, 2 F32; `scratch` = 4 device bytes (I8/I16); returns bytes written */
int sdrgpu_compress_dev(int device, int pcmType, const float* in, int count, unsigned char* out, unsigned* scratch, void* stream);
/* SampleStreamDecompressor::process (sample_stream_decompressor.h:13-33): hdr = host copy of the
 * 8-byte header, payload = device bytes after it; returns complex samples written */
int sdrgpu_decompress_dev(int device, const unsigned char* hdr, const unsigned char* payload, int nbytes, float* out, void* stream);

/* WaterFall::pushFFT consumers (gui/widgets/waterfall.cpp), device buffers, bit-exact:
 *  colormap: zoomed dB -> waterfall pixels, pallet[(int)(((clamp(v) - min) / (max - min)) * (res - 1))] (:903-910);
 *  fft_smooth_hold: per column over nrows rows in order, smoothing (smooth = row*alpha + smooth*beta,
 *    row <- smooth; :918-925) then hold (hold[i] = max(row[i], hold[i] - speed), i >= 1; :952-957);
 *  vfo_signal_info: calculateVFOSignalInfo per raw row -> strength (in-band max) and snr (max minus
 *    side-band mean) (:563-601) */
int sdrgpu_colormap_dev(int device, const float* in, long long n, float wfMin, float wfMax, const unsigned* pallet, int res,
                        unsigned* out, void* stream);
int sdrgpu_fft_smooth_hold_dev(int device, float* rows, int nrows, int width, int smoothing, float alpha, float beta,
                               float* smooth, int holdOn, float holdSpeed, float* hold, void* stream);
int sdrgpu_vfo_signal_info_dev(int device, const float* rows, int nrows, int fftSize, double wholeBandwidth,
                               double centerOffset, double bandwidth, float* strength, float* snr, void* stream);

/* recorder WAV encoders (utils/wav.cpp:296-336) of n device floats: kind 0 u8, 1 i16, 2 i24
 * (packed LE), 3 i32, 4 f32; returns bytes written */
int sdrgpu_wav_encode_dev(int device, int kind, const float* in, long long n, unsigned char* out, void* stream);

/* ------------------------------------------------------------ ingest ---- */

/* file_source / rtl_sdr / hackrf sample converters (elementwise, n scalars):
 * kind 0 u8 (b-128+0.5f)/127.5f, 1 i16 (s+0.5f)/32767.5f, 2 i24 packed LE,
 * 3 i32 ((v+0.5)/(2^31-0.5) in double), 4 f64 -> f32, 5 i8 x*(1/128) */
enum { SDRGPU_CONV_U8 = 0, SDRGPU_CONV_I16, SDRGPU_CONV_I24, SDRGPU_CONV_I32, SDRGPU_CONV_F64, SDRGPU_CONV_I8,
       SDRGPU_CONV_F32 /* 32-bit IEEE float copied as it is (WAV IEEE_FLOAT 32) */ };
int sdrgpu_convert_dev(int device, int kind, const void* in, long long n, float* out, void* stream);
int sdrgpu_convert(int device, int kind, const void* in, long long n, float* out);      /* host buffers */
/* one-channel file_source WAV (main.cpp:294-430): n samples -> n complex_t with I = Q = the
 * converted sample (any SDRGPU_CONV_* kind) */
int sdrgpu_convert_mono_dev(int device, int kind, const void* in, long long n, void* out, void* stream);
int sdrgpu_convert_mono(int device, int kind, const void* in, long long n, void* out);   /* host buffers */

/* file_source WavReader (source_modules/file_source/src/wavreader.h:34-226): RIFF / RF64 WAVE,
 * fmt PCM / IEEE_FLOAT / EXTENSIBLE (by SubFormat), samples = [data offset, end of file) */
typedef struct sdrgpu_wav sdrgpu_wav;
int sdrgpu_wav_open(sdrgpu_wav** h, const char* path);
int sdrgpu_wav_info(sdrgpu_wav* h, int* format, int* channels, int* bits, double* sampleRate, long long* sampleCount);
/* converter kind (SDRGPU_CONV_*) for the file's (format, bits) as worker_1ch / worker_2ch pick it
 * (main.cpp:316-560); < 0 = unsupported (error) */
int sdrgpu_wav_kind(sdrgpu_wav* h);
int sdrgpu_wav_block_size(sdrgpu_wav* h);                      /* min(fs / 200, 1e6) frames */
int sdrgpu_wav_read(sdrgpu_wav* h, void* out, int maxFrames);   /* raw frames; 0 at the end */
int sdrgpu_wav_seek(sdrgpu_wav* h, long long frame);
int sdrgpu_wav_close(sdrgpu_wav* h);

#ifdef __cplusplus
}
#endif
#endif

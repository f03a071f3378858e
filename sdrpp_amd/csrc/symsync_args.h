// The argument checks and parameter conversions of the symbol-recovery loops, stated once for the
// single-stream blocks (symsync.hip) and the stream banks (bank.hip). Host code only; include after
// symsync_kernels.h (the parameter structs).
#pragma once
#include <cmath>
#include <initializer_list>
#include "symsync_kernels.h"

namespace sdrgpu {

inline bool finite_all(std::initializer_list<double> v) {
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

inline bool real_or_complex(int dtype) { return dtype == SDRGPU_F32 || dtype == SDRGPU_C64; }

// loop::FastAGC members are float (fast_agc.h:93-97)
inline void fast_agc_params(FastAgcParams& p, double setPoint, double maxGain, double rate) {
    p.setPoint = (float)setPoint;
    p.maxGain = (float)maxGain;
    p.rate = (float)rate;
}

// Frequencies and phases are rad/sample: a bound far above any meaningful value keeps the phase wrap
// (a subtraction loop, phase_control_loop.h:82-85) to a few hundred steps per sample
constexpr double COSTAS_MAX_RAD = 1024.0;

inline bool costas_limits_ok(double minFreq, double maxFreq) {   // PhaseControlLoop: assert(maxFreq > minFreq)
    return finite_all({minFreq, maxFreq}) && maxFreq > minFreq && std::fabs(minFreq) <= COSTAS_MAX_RAD &&
           std::fabs(maxFreq) <= COSTAS_MAX_RAD;
}
inline bool costas_args_ok(int order, double bandwidth, double initPhase, double initFreq, double minFreq, double maxFreq) {
    if (!(order == 2 || order == 4 || order == 8) || !finite_all({bandwidth, initPhase, initFreq}) ||
        std::fabs(initPhase) > COSTAS_MAX_RAD || std::fabs(initFreq) > COSTAS_MAX_RAD || !costas_limits_ok(minFreq, maxFreq)) {
        set_error("costas: order %d not 2 / 4 / 8, or a phase / frequency not finite, beyond %g rad, or minFreq >= maxFreq", order,
                  COSTAS_MAX_RAD);
        return false;
    }
    return true;
}

// pcl.init(alpha, beta, initPhase, -FL_M_PI, FL_M_PI, initFreq, minFreq, maxFreq) (pll.h:22) as pll_step takes it
inline PllParams pll_params(const PclParams& pcl) {
    PllParams pp{};
    pp.alpha = pcl.alpha;
    pp.beta = pcl.beta;
    pp.minPhase = -3.1415926535f;
    pp.maxPhase = 3.1415926535f;
    pp.phaseDelta = pp.maxPhase - pp.minPhase;   // phase_control_loop.h:28
    pp.minFreq = pcl.minFreq;
    pp.maxFreq = pcl.maxFreq;
    return pp;
}

// Every MM output must consume at least one input sample: phase >= 0 before advance, freq >= minFreq and
// alpha * error >= -alpha, so floorf(phase) >= 1 when minFreq - alpha >= 1 (also in the floats the
// kernel computes with).
inline bool mm_params_ok(double omega, double omegaGain, double muGain, double rel) {
    if (!finite_all({omega, omegaGain, muGain, rel}) || !(omega > 0.0) || !(rel > 0.0) || muGain < 0.0) return false;
    if (omega * (1.0 - rel) - muGain < 1.0) return false;
    return (float)(omega * (1.0 - rel)) - (float)muGain >= 1.0f && omega * (1.0 + rel) < 1e6;
}
inline bool mm_args_ok(double omega, double omegaGain, double muGain, double rel, int P, int T) {
    if (P < 1 || P > SDRGPU_MM_MAX_PHASES || T < 1 || T > SDRGPU_MM_MAX_TAPS) {
        set_error("mm: interpolator bank %d x %d outside [1, %d] x [1, %d]", P, T, SDRGPU_MM_MAX_PHASES, SDRGPU_MM_MAX_TAPS);
        return false;
    }
    if (!mm_params_ok(omega, omegaGain, muGain, rel)) {
        set_error("mm: omega * (1 - omegaRelLimit) - muGain must be >= 1 (an output per input sample at most)");
        return false;
    }
    return true;
}
// pcl.init / setCoefficients / setFreqLimits arguments (mm.h:32, 48, 56, 70): doubles to float
inline void mm_pcl_params(MmParams& p, double omega, double omegaGain, double muGain, double rel) {
    p.pcl.alpha = (float)muGain;
    p.pcl.beta = (float)omegaGain;
    p.pcl.minFreq = (float)(omega * (1.0 - rel));
    p.pcl.maxFreq = (float)(omega * (1.0 + rel));
    p.omega = (float)omega;
}

}  // namespace sdrgpu

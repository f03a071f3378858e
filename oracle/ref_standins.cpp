// Stand-ins that let the reference's own block headers link and run without VOLK, FFTW or the
// reference's host runtime (test infrastructure; linked only into oracle/_ref/ref_blocks*). Our own
// code, written from the libraries' published semantics:
//
// * the VOLK functions the included headers call, as scalar loops in ascending index order, fp32,
//   unfused (the build passes -ffp-contract=off). With -DREF_SUM4 the dot products and the
//   accumulator keep four interleaved partial sums (element i goes to sum i % 4) combined at the end
//   as (s0 + s1) + (s2 + s3): the order a 4-lane SIMD kernel has. That build exists only to measure
//   how sensitive the reference itself is to summation order;
// * fftwf_*: a direct O(n^2) DFT evaluated in fp64, unnormalised in both directions as FFTW is, each
//   output rounded once to fp32. noise_reduction/fm_if.h with at most 32 bins is its only user;
// * the five host symbols block.h's thread wrapper refers to, as no-ops (the probe never starts a
//   thread), and flog::logImpl, which drops the message (RationalResampler logs its plan).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include <volk/volk.h>
#include <fftw3.h>
#include <utils/threading.h>
#include <utils/flog.h>

// ---------------------------------------------------------------- VOLK
size_t volk_get_alignment(void) { return 64; }

void* volk_malloc(size_t size, size_t alignment) {
    // Zero-filled: MM's work buffer is allocated and never cleared (clock_recovery/mm.h:34), so its
    // first T - 1 history samples are whatever the allocator returns. Zeros make the probe
    // deterministic and are what the restatement and the device start from.
    void* p = nullptr;
    if (posix_memalign(&p, alignment, size ? size : alignment)) { return nullptr; }
    memset(p, 0, size);
    return p;
}

void volk_free(void* p) { free(p); }

#ifdef REF_SUM4
static const int LANES = 4;
#else
static const int LANES = 1;
#endif

static inline float combine(const float* s) { return LANES == 4 ? (s[0] + s[1]) + (s[2] + s[3]) : s[0]; }

void volk_32f_x2_dot_prod_32f(float* result, const float* input, const float* taps, unsigned int num_points) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned int i = 0; i < num_points; i++) { s[i % LANES] += input[i] * taps[i]; }
    *result = combine(s);
}

void volk_32fc_32f_dot_prod_32fc(lv_32fc_t* result, const lv_32fc_t* input, const float* taps, unsigned int num_points) {
    const float* in = (const float*)input;
    float re[4] = {0.0f, 0.0f, 0.0f, 0.0f}, im[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned int i = 0; i < num_points; i++) {
        re[i % LANES] += in[2 * i] * taps[i];
        im[i % LANES] += in[2 * i + 1] * taps[i];
    }
    *result = lv_cmake(combine(re), combine(im));
}

void volk_32fc_x2_dot_prod_32fc(lv_32fc_t* result, const lv_32fc_t* input, const lv_32fc_t* taps, unsigned int num_points) {
    const float* a = (const float*)input;
    const float* b = (const float*)taps;
    float re[4] = {0.0f, 0.0f, 0.0f, 0.0f}, im[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned int i = 0; i < num_points; i++) {
        float pr = (a[2 * i] * b[2 * i]) - (a[2 * i + 1] * b[2 * i + 1]);
        float pi = (a[2 * i] * b[2 * i + 1]) + (a[2 * i + 1] * b[2 * i]);
        re[i % LANES] += pr;
        im[i % LANES] += pi;
    }
    *result = lv_cmake(combine(re), combine(im));
}

void volk_32f_accumulator_s32f(float* result, const float* inputBuffer, unsigned int num_points) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned int i = 0; i < num_points; i++) { s[i % LANES] += inputBuffer[i]; }
    *result = combine(s);
}

void volk_32fc_magnitude_32f(float* magnitudeVector, const lv_32fc_t* complexVector, unsigned int num_points) {
    const float* in = (const float*)complexVector;
    for (unsigned int i = 0; i < num_points; i++) {
        magnitudeVector[i] = sqrtf((in[2 * i] * in[2 * i]) + (in[2 * i + 1] * in[2 * i + 1]));
    }
}

void volk_32fc_32f_multiply_32fc(lv_32fc_t* cVector, const lv_32fc_t* aVector, const float* bVector, unsigned int num_points) {
    const float* a = (const float*)aVector;
    float* c = (float*)cVector;
    for (unsigned int i = 0; i < num_points; i++) {
        c[2 * i] = a[2 * i] * bVector[i];
        c[2 * i + 1] = a[2 * i + 1] * bVector[i];
    }
}

void volk_32f_index_max_32u(uint32_t* target, const float* src0, uint32_t num_points) {
    // the first maximum: a later equal value does not replace it
    if (!num_points) { return; }
    uint32_t idx = 0;
    float best = src0[0];
    for (uint32_t i = 1; i < num_points; i++) {
        if (src0[i] > best) { best = src0[i]; idx = i; }
    }
    *target = idx;
}

void volk_32fc_deinterleave_real_32f(float* iBuffer, const lv_32fc_t* complexVector, unsigned int num_points) {
    const float* in = (const float*)complexVector;
    for (unsigned int i = 0; i < num_points; i++) { iBuffer[i] = in[2 * i]; }
}

// The elementwise kernels of the analogue demodulators (demod/broadcast_fm.h, convert/*.h, math/*.h): one plain loop
// each, one rounding per operation; none of them sums.
void volk_32f_s32f_multiply_32f(float* cVector, const float* aVector, const float scalar, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { cVector[i] = aVector[i] * scalar; }
}

void volk_32fc_conjugate_32fc(lv_32fc_t* cVector, const lv_32fc_t* aVector, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { cVector[i] = lv_cmake(aVector[i].real(), -aVector[i].imag()); }
}

void volk_32fc_x2_multiply_32fc(lv_32fc_t* cVector, const lv_32fc_t* aVector, const lv_32fc_t* bVector, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) {
        const float ar = aVector[i].real(), ai = aVector[i].imag(), br = bVector[i].real(), bi = bVector[i].imag();
        cVector[i] = lv_cmake((ar * br) - (ai * bi), (ar * bi) + (ai * br));
    }
}

void volk_32f_x2_multiply_32f(float* cVector, const float* aVector, const float* bVector, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { cVector[i] = aVector[i] * bVector[i]; }
}

void volk_32f_x2_add_32f(float* cVector, const float* aVector, const float* bVector, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { cVector[i] = aVector[i] + bVector[i]; }
}

void volk_32f_x2_subtract_32f(float* cVector, const float* aVector, const float* bVector, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { cVector[i] = aVector[i] - bVector[i]; }
}

void volk_32f_x2_interleave_32fc(lv_32fc_t* complexVector, const float* iBuffer, const float* qBuffer, unsigned int num_points) {
    for (unsigned int i = 0; i < num_points; i++) { complexVector[i] = lv_cmake(iBuffer[i], qBuffer[i]); }
}

// VOLK's generic rotator as published (volk_32fc_s32fc_x2_rotator_32fc_generic): out = in * phase, phase
// *= phase_inc in fp32, phase renormalised after every 512 samples and once more at the end of a call
// that leaves a remainder. With -DREF_ROT64 the phase is carried in fp64 beside the block's fp32 copy
// (found again by its address; a copy the block has rewritten, as reset() does, is taken over) and each
// output is the fp64 product rounded once: that build exists only to measure how far the reference's
// own fp32 phase recurrence drifts from the phase it stands for.
static const unsigned ROTATOR_RELOAD = 512;

#ifdef REF_ROT64
#include <map>
void volk_32fc_s32fc_x2_rotator_32fc(lv_32fc_t* outVector, const lv_32fc_t* inVector, const lv_32fc_t phase_inc, lv_32fc_t* phase,
                                     unsigned int num_points) {
    static std::map<const lv_32fc_t*, std::complex<double>> carried;
    auto it = carried.find(phase);
    if (it == carried.end() || lv_32fc_t((float)it->second.real(), (float)it->second.imag()) != *phase) {
        it = carried.insert_or_assign(phase, std::complex<double>(phase->real(), phase->imag())).first;
    }
    double pr = it->second.real(), pi = it->second.imag();
    const double dr = phase_inc.real(), di = phase_inc.imag();
    for (unsigned int i = 0; i < num_points; i++) {
        const double ar = inVector[i].real(), ai = inVector[i].imag();
        outVector[i] = lv_cmake((float)(ar * pr - ai * pi), (float)(ar * pi + ai * pr));
        const double nr = pr * dr - pi * di, ni = pr * di + pi * dr;
        pr = nr;
        pi = ni;
        if ((i + 1) % ROTATOR_RELOAD == 0 || i + 1 == num_points) {
            const double h = hypot(pr, pi);
            pr /= h;
            pi /= h;
        }
    }
    it->second = std::complex<double>(pr, pi);
    *phase = lv_cmake((float)pr, (float)pi);
}
#else
void volk_32fc_s32fc_x2_rotator_32fc(lv_32fc_t* outVector, const lv_32fc_t* inVector, const lv_32fc_t phase_inc, lv_32fc_t* phase,
                                     unsigned int num_points) {
    float pr = phase->real(), pi = phase->imag();
    const float dr = phase_inc.real(), di = phase_inc.imag();
    for (unsigned int i = 0; i < num_points; i++) {
        const float ar = inVector[i].real(), ai = inVector[i].imag();
        outVector[i] = lv_cmake((ar * pr) - (ai * pi), (ar * pi) + (ai * pr));
        const float nr = (pr * dr) - (pi * di), ni = (pr * di) + (pi * dr);
        pr = nr;
        pi = ni;
        if ((i + 1) % ROTATOR_RELOAD == 0 || i + 1 == num_points) {
            const float h = hypotf(pr, pi);
            pr /= h;
            pi /= h;
        }
    }
    *phase = lv_cmake(pr, pi);
}
#endif

// ---------------------------------------------------------------- FFTW (single precision)
struct fftwf_plan_s {
    int n, sign;
    fftwf_complex* in;
    fftwf_complex* out;
    std::vector<double> c, s;   // cos / sin of 2 pi k / n, k < n
};

void* fftwf_malloc(size_t n) { return volk_malloc(n, 64); }

void fftwf_free(void* p) { free(p); }

fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex* in, fftwf_complex* out, int sign, unsigned) {
    fftwf_plan p = new fftwf_plan_s{n, sign, in, out, {}, {}};
    p->c.resize(n);
    p->s.resize(n);
    for (int k = 0; k < n; k++) {
        p->c[k] = cos(2.0 * M_PI * (double)k / (double)n);
        p->s[k] = sin(2.0 * M_PI * (double)k / (double)n);
    }
    return p;
}

void fftwf_execute(const fftwf_plan p) {
    // out[k] = sum_j in[j] e^{sign 2 pi i j k / n}, no 1/n in either direction
    const int n = p->n;
    std::vector<double> re(n), im(n);
    for (int k = 0; k < n; k++) {
        double ar = 0.0, ai = 0.0;
        for (int j = 0; j < n; j++) {
            int m = (int)(((long long)j * k) % n);
            double c = p->c[m], s = p->sign < 0 ? -p->s[m] : p->s[m];
            double xr = p->in[j][0], xi = p->in[j][1];
            ar += xr * c - xi * s;
            ai += xr * s + xi * c;
        }
        re[k] = ar;
        im[k] = ai;
    }
    for (int k = 0; k < n; k++) {
        p->out[k][0] = (float)re[k];
        p->out[k][1] = (float)im[k];
    }
}

void fftwf_destroy_plan(fftwf_plan p) { delete p; }

// ---------------------------------------------------------------- host runtime
namespace flog {
    void exception(const std::exception&) {}
    void exception() {}
    void logImpl(flog::Type, std::string, const std::chrono::time_point<std::chrono::steady_clock>,
                 const std::shared_ptr<const stack_trace>) {}
}

namespace threading {
    void thread::onStarting(const std::string&) {}
    void thread::onStarted(const std::string&) {}
    void thread::onFinished(const std::string&) {}
}

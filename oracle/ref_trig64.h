// Forced in (-include) ahead of the reference's headers for oracle/_ref/ref_blocks_trig64 only: cosf, sinf and
// atan2f, as the translation unit that includes the reference's block headers spells them, are evaluated in fp64
// and rounded once to fp32. The standard headers are included first, so only the code after them sees the
// macros. That build measures how far the reference's outputs move with one more libm; nothing else uses it.
#pragma once
#include <math.h>
#include <cmath>
#include <complex>
#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
static inline float ref_trig64_cosf(float x) { return (float)cos((double)x); }
static inline float ref_trig64_sinf(float x) { return (float)sin((double)x); }
static inline float ref_trig64_atan2f(float y, float x) { return (float)atan2((double)y, (double)x); }
#define cosf(x) ref_trig64_cosf(x)
#define sinf(x) ref_trig64_sinf(x)
#define atan2f(y, x) ref_trig64_atan2f(y, x)

// darknet's activations (DN/activations.h) for the kernels that apply any of them to one value: k_activate / k_shortcut (ew_ops.hip), the
// [rnn] epilogues (rnn_ops.hip).  Compile with -ffp-contract=off.
#pragma once
#include "device_common.h"
#include <math.h>

// One value through activation `act`.  The slope family is the conv epilogues' max(v, v * slope) (act_slope: a float product where the
// reference's .1 * x is a double one).  Every other formula is evaluated as DN/activations.h writes it, operation for operation and in the
// reference's types -- its constants and its exp are double, so the arithmetic here is double and the result is rounded to float once, as the
// C compiler rounds the reference's return value.  (A float expf would leave loggy and tanh a few units of 2^-24 off near 0, where the
// result is the small difference of numbers close to 1.)  None of this is on a network's hot path.
__device__ __forceinline__ float act_apply(float x, int act)
{
    switch (act) {
    case ACT_LINEAR: return x;
    case ACT_LEAKY: case ACT_RELU: case ACT_RELIE: return fmaxf(x, x * act_slope(act));
    case ACT_LOGISTIC: return (float)(1. / (1. + exp((double)-x)));
    case ACT_LOGGY: return (float)(2. / (1. + exp((double)-x)) - 1);
    case ACT_ELU: return (float)((double)((float)(x >= 0) * x) + (double)(x < 0) * (exp((double)x) - 1));
    case ACT_RAMP: return (float)((double)(x * (float)(x > 0)) + .1 * (double)x);
    case ACT_TANH: { const double e = exp((double)(2 * x)); return (float)((e - 1) / (e + 1)); }
    case ACT_PLSE:
        if (x < -4) return (float)(.01 * (double)(x + 4));
        if (x > 4) return (float)(.01 * (double)(x - 4) + 1);
        return (float)(.125 * (double)x + .5);
    case ACT_STAIR: {
        const int n = (int)floor((double)x);
        if (n % 2 == 0) return (float)floor((double)x / 2.);
        return (float)((double)(x - (float)n) + floor((double)x / 2.));
    }
    case ACT_HARDTAN: return x < -1 ? -1.f : x > 1 ? 1.f : x;
    case ACT_LHTAN:
        if (x < 0) return (float)(.001 * (double)x);
        if (x > 1) return (float)(.001 * (double)(x - 1) + 1);
        return x;
    }
    return x;
}

// AdamW's per-element update, shared by adamw_kernel (ops.hip) and adamw8_kernel (adam8.hip) so that both compile the same function.
#pragma once
#include "common.h"

// One element's update, every fused multiply-add written out.  Left to the compiler, m = b1 * m + (1 - b1) * g, v = b2 * v + (1 - b2) * g * g
// and p = p * decay - step * m / denom were contracted one way in the 4-wide body (the three fmaf below) and not at all in the scalar
// tail, and which way it went followed the shape of the code around the expression: the last elements of a tensor whose size is no multiple
// of 4 got an m, v and master one ulp away from what the same element gets in the body.  With the forms spelled out there is nothing left
// to contract, so the body and the tail share the function and round alike (the body compiles to the instructions it had before).
DEVINL void adamw_update(float& pp, float& mm, float& vv, float gg, float decay, float step, float b1, float b2, float rs2, float eps) {
    mm = fmaf(1.f - b1, gg, b1 * mm);
    vv = fmaf(b2, vv, ((1.f - b2) * gg) * gg);
    pp = fmaf(decay, pp, -(step * mm / fmaf(sqrtf(vv), rs2, eps)));
}

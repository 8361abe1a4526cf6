// What the stages that reproject through a G-buffer share (bmfr.hip, reprojection.hip): the octahedral normal, the tap position of a
// screen position and the bilinear weights of a kept set of taps.
#pragma once
#include "common.h"

namespace tr {

TR_DEV f3 octahedral_unpack(f2 o) {      // math.glsl:487-496
    f3 n = F3(o.x, o.y, 1.0f - fabsf(o.x) - fabsf(o.y));
    const float t = clampf(n.z, -1.0f, 0.0f);
    n.x = n.x + t * ((n.x >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
    n.y = n.y + t * ((n.y >= 0.0f ? 1.0f : 0.0f) * 2.0f - 1.0f);
    return normalize(n);
}

// The top-left tap of the reprojected position and its fractions.  Three operations per axis, in this order (tests/bmfr_model.py and
// tests/reprojection_model.py do the same three in float32): y -> 1 - y, * size, - 0.5.  The clamp only moves positions whose four taps are outside anyway.
TR_DEV void tap_position(f2 motion /* uv, y up */, int w, int h, int& tx, int& ty, float& qx, float& qy) {
    float fx = motion.x * (float)w - 0.5f;
    float fy = (1.0f - motion.y) * (float)h - 0.5f;
    fx = fmin2(fmax2(-2.0f, fx), (float)w + 1.0f);
    fy = fmin2(fmax2(-2.0f, fy), (float)h + 1.0f);
    const float flx = floorf(fx), fly = floorf(fy);
    tx = (int)flx; ty = (int)fly;
    qx = fx - flx; qy = fy - fly;
}

// Bilinear weights of the kept taps, renormalised; returns their sum before that.
TR_DEV float tap_weights(float qx, float qy, uint bits, float cw[4]) {
    const float sx[2] = {1.0f - qx, qx}, sy[2] = {1.0f - qy, qy};
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { cw[k] = (bits & (1u << k)) ? sx[k & 1] * sy[k >> 1] : 0.0f; sum = sum + cw[k]; }
    if (sum > 1e-5f) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cw[k] = cw[k] / sum;
    }
    return sum;
}

}  // namespace tr

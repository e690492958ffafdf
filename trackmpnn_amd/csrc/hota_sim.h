// The box similarity of the evaluation kernels (csrc/hota.hip, csrc/evalprep.hip): one definition, so that the preprocessing
// and the scoring agree on every bit.  Host: trackmpnn_amd.hota.hota_sim_host.  Contraction is switched off inside the bodies,
// so that they mean the same in whatever translation unit includes them.
#pragma once
#include <hip/hip_runtime.h>

namespace tmpnn {

// np.maximum / np.minimum: the first operand where it is larger (smaller) or NaN
__device__ __forceinline__ double hota_fmax(double a, double b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ double hota_fmin(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ bool hota_finite(double x) { return __builtin_fabs(x) < __builtin_huge_val(); }

// IoU of two x1 y1 x2 y2 boxes (host: hota.hota_sim_host -- the operations of mot_dist up to inter / union, in its order),
// 0 where union > 0 is false or the quotient is not finite
__device__ __forceinline__ double hota_sim(float4 o, float4 h) {
#pragma clang fp contract(off)
    const float wo = o.z - o.x, ho = o.w - o.y, wh = h.z - h.x, hh = h.w - h.y;      // float32
    const double otx = o.x, oty = o.y, htx = h.x, hty = h.y;
    const double obx = otx + (double)wo, oby = oty + (double)ho, hbx = htx + (double)wh, hby = hty + (double)hh;
    const double iw = hota_fmax(hota_fmin(obx, hbx) - hota_fmax(otx, htx), 0.0);
    const double ih = hota_fmax(hota_fmin(oby, hby) - hota_fmax(oty, hty), 0.0);
    const double inter = iw * ih;
    const double uni = ((double)wo * (double)ho + (double)wh * (double)hh) - inter;
    const double q = inter / uni;
    return (uni > 0.0 && hota_finite(q)) ? q : 0.0;
}

}  // namespace tmpnn

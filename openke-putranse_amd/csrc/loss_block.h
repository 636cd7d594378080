// The block between the two passes of a weighted external-batch step (k_step_adv, k_step_distmult): one lane group
// holds its positive's K negative entries in LDS and forms, lane-parallel over them, the self-adversarial weights,
// the loss partial and dL/d(entry k), which overwrites entry k.
//   SigmoidLoss.py:19-26:  L = -1/2 [mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik)],  w = softmax_k(T n) | 1/K
//   MarginLoss.py:24-31:   L = mean_i sum_k w_ik max(p_i - n_ik, -m) + m,                    w = softmax_k(-T n) | 1/K
// with the weights detached (constants of the backward pass) and torch's maximum tie -> half.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

template <int G>
__device__ __forceinline__ float gmax(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// overflow-safe log(sigmoid(x)) and sigmoid(x)
__device__ __forceinline__ float logsig(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigm(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// sc[0 .. neg): the group's entries e_k (LDS); the score handed to the loss is n_k = gamma - e_k under L.mflag, else
// e_k (sg = dn / de: -1 or 1); ps = the positive's score. On return sc[k] = dL / de_k, *dldp = dL / d(ps), and the
// value is the group's loss partial (pt::loss_affine maps the sum of the partials to the step's loss).
// The caller puts a wave barrier before and after (LDS order inside a wave is program order).
template <int G>
__device__ __forceinline__ float loss_block(const LossParams &L, float margin, int64_t bs, int neg, float *sc,
                                            int lane, float ps, float sg, float *dldp) {
    const float invB = 1.0f / (float)bs;
    float zt = 0.f, ext = 0.f, winv = 1.0f / (float)neg;
    if (L.adv) {
        zt = L.kind == 1 ? L.temp : -L.temp;
        float mx = -INFINITY;
        for (int k = lane; k < neg; k += G) {
            const float n = L.mflag ? L.gamma - sc[k] : sc[k];
            mx = fmaxf(mx, zt > 0.f ? n : -n);
        }
        mx = gmax<G>(mx);
        ext = zt > 0.f ? mx : -mx;   // the score of the largest weight: every exponent below is <= 0
        float se = 0.f;
        for (int k = lane; k < neg; k += G) {
            const float n = L.mflag ? L.gamma - sc[k] : sc[k];
            se += expf(zt * (n - ext));
        }
        winv = 1.0f / gsum<G>(se);
    }
    float lp = 0.f, cs = 0.f;
    for (int k = lane; k < neg; k += G) {
        const float n = L.mflag ? L.gamma - sc[k] : sc[k];
        const float w = L.adv ? expf(zt * (n - ext)) * winv : winv;
        float c;   // dL / dn_k
        if (L.kind == 1) {
            lp += w * logsig(-n);
            c = w * sigm(n) * (0.5f * invB);
        } else {
            const float a = ps - n, m = margin;
            lp += w * (a > -m ? a : -m);
            const float hc = a > -m ? 1.0f : (a == -m ? 0.5f : 0.f);
            cs += w * hc;
            c = -(w * hc) * invB;
        }
        sc[k] = c * sg;
    }
    lp = gsum<G>(lp);
    if (L.kind == 1) {
        lp += logsig(ps);
        *dldp = -sigm(-ps) * (0.5f * invB);
    } else {
        *dldp = gsum<G>(cs) * invB;
    }
    return lp;
}

}  // namespace dev
}  // namespace pt

// HIP kernel of the weighted external-batch step for gfx950: TransE under SigmoidLoss (with or without the
// self-adversarial weights), MarginLoss with the self-adversarial weights, and plain MarginLoss on a model that
// carries its own margin (score = gamma - d).
//
// Semantics: d = ||h^ + r^ - t^||_p (TransE.py:46-60, rows normalised under norm_flag), score s = gamma - d with the
// model's margin (TransE.py:62-67) else d; a batch of B positives with K negatives each in the reference layout
// (NegativeSampling.py:13-21: negative k of positive i at (k + 1) * B + i);
//   SigmoidLoss.py:19-26:  L = -1/2 [mean_i logsig(p_i) + mean_i sum_k w_ik logsig(-n_ik)],  w = softmax_k(T n) | 1/K
//   MarginLoss.py:24-31:   L = mean_i sum_k w_ik max(p_i - n_ik, -m) + m,                    w = softmax_k(-T n) | 1/K
// with the weights detached (constants of the backward pass) and torch's maximum tie -> half.
//
// Mapping: the lane-group row layout of device.h; ONE lane group owns a positive and all its negatives (the softmax
// couples them) and walks them twice. Pass 1 forms v_k and stores d_k in LDS (K floats per group); the group then
// finds the extreme score, the softmax and the loss partial lane-parallel over those K floats and overwrites d_k by
// dL/dd_k; pass 2 re-forms v_k (same instructions: the same bits) and emits gradients: entity and relation
// gradients in normalised space (the apply pass multiplies by the normalise Jacobian), the positive's relation and
// uncorrupted side summed in registers (chunk partials first), every other row through float atomics into the
// trainer's gradient rows plus touched flags (row_atomic below). A negative that shares the positive's relation and
// one entity (every cross-sampled negative, and every normal-mode entity corruption) costs one row load per pass:
// h^ + r^ and t^ stay in registers. Rows of NCH negatives are in flight together. Pass 2 re-reads the rows it needs
// (K x dim x 4 bytes per positive: L2-sized); a pass 2 that read them from rows staged in LDS by pass 1 was measured
// slower.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"
#include "loss_block.h"

namespace pt {
namespace dev {

struct AdvSink {   // (row_atomic: device.h)
    float *gent, *grel;
    int *fent, *frel;
    template <int G, int VEC, int KCH>
    __device__ __forceinline__ void ent(int64_t row, const V<G, VEC, KCH> &g, float *tb, int D, int lane) const {
        row_atomic(g, gent + row * D, tb, D, lane);
        if (lane == 0) fent[row] = 1;
    }
    template <int G, int VEC, int KCH>
    __device__ __forceinline__ void rel(int64_t row, const V<G, VEC, KCH> &g, float *tb, int D, int lane) const {
        row_atomic(g, grel + row * D, tb, D, lane);
        if (lane == 0) frel[row] = 1;
    }
};

template <int G, int VEC, int KCH, int NCH>
__global__ __launch_bounds__(256) void k_step_adv(StepParams P, LossParams L, const int64_t *__restrict__ bh,
                                                  const int64_t *__restrict__ bt, const int64_t *__restrict__ br,
                                                  AdvSink sink, float *__restrict__ lpart) {
    using Vec = V<G, VEC, KCH>;
    constexpr int RW = VEC == 4 ? KCH * G * VEC : 0;   // floats of a group's transpose row (row_atomic)
    // [groups per block][RW] transpose rows, then [groups per block][neg] scores
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    const int gpb = (int)blockDim.x / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t bs = P.batch_size;
    const int neg = (int)P.neg;
    const int64_t b = (int64_t)blockIdx.x * gpb + grp;
    if (b >= bs) return;   // (no block-wide barrier below: a group is inside one wave)
    float *tb = s_lds + (size_t)grp * RW;
    float *sc = s_lds + (size_t)gpb * RW + (size_t)grp * neg;
    const int D = (int)P.dim;
    const int p = P.p_norm;
    const bool nf = P.norm_flag != 0;
    // ---- positive
    const int64_t hp = bh[b], tp = bt[b], rp = br[b];
    Vec hh, th, rh, base, vpos;
    {
        Vec H, T, R;
        vload(H, P.ent + hp * D, D, lane);
        vload(T, P.ent + tp * D, D, lane);
        vload(R, P.rel + rp * D, D, lane);
        if (nf) {
            vnormalize(H, hh);
            vnormalize(R, rh);
            vnormalize(T, th);
        } else {
            hh = H; rh = R; th = T;
        }
    }
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        base.x[i] = hh.x[i] + rh.x[i];
        vpos.x[i] = base.x[i] - th.x[i];
    }
    const float dp = vpnorm(vpos, p);
    const float sg = L.mflag ? -1.f : 1.f;   // ds / dd
    const float ps = L.mflag ? L.gamma - dp : dp;
    float dldp = 0.f;                        // dL / d(positive score)
    // on-chip sums over the negatives that share the positive's rows: aH = sum of dL/dv_k over those that keep its
    // head (dL/dh^), aT = minus the sum over those that keep its tail (dL/dt^); dL/dr^ = aH - aT. Each chunk sums
    // into accumulators of its own first (a K-term sequential float32 sum into one accumulator was measured
    // 3e-7 off at K = 256; chunk partials bring it to 5e-8)
    Vec aH, aT;
    vzero(aH); vzero(aT);

    for (int pass = 0; pass < 2; ++pass) {
        for (int c0 = 0; c0 < neg; c0 += NCH) {
            int64_t hk[NCH], tk[NCH], rk[NCH];
            int kind[NCH];   // 0: shares (h, r): row t_k; 1: shares (r, t): row h_k; 2: any other slot; -1: nothing to do
            Vec E[NCH], cH, cT;
            vzero(cH); vzero(cT);
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                kind[u] = -1;
                if (c0 + u >= neg) continue;
                if (pass == 1 && sc[c0 + u] == 0.f) continue;   // no gradient through this negative
                const int64_t o = (int64_t)(c0 + u + 1) * bs + b;
                hk[u] = bh[o]; tk[u] = bt[o]; rk[u] = br[o];
                kind[u] = rk[u] != rp ? 2 : (hk[u] == hp ? 0 : (tk[u] == tp ? 1 : 2));
                if (kind[u] < 2) vload(E[u], P.ent + (kind[u] == 0 ? tk[u] : hk[u]) * D, D, lane);
            }
#pragma unroll
            for (int u = 0; u < NCH; ++u) {
                if (kind[u] < 0) continue;
                Vec vk;
                if (kind[u] < 2) {
                    Vec eh;
                    if (nf) vnormalize(E[u], eh); else eh = E[u];
                    if (kind[u] == 0) {
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) vk.x[i] = base.x[i] - eh.x[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) vk.x[i] = (eh.x[i] + rh.x[i]) - th.x[i];
                    }
                } else {
                    Vec A, B, C, a, bb, c;
                    vload(A, P.ent + hk[u] * D, D, lane);
                    vload(B, P.rel + rk[u] * D, D, lane);
                    vload(C, P.ent + tk[u] * D, D, lane);
                    if (nf) {
                        vnormalize(A, a);
                        vnormalize(B, bb);
                        vnormalize(C, c);
                    } else {
                        a = A; bb = B; c = C;
                    }
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) vk.x[i] = (a.x[i] + bb.x[i]) - c.x[i];
                }
                if (pass == 0) {
                    const float d = vpnorm(vk, p);
                    if (lane == 0) sc[c0 + u] = d;
                    continue;
                }
                const float cd = sc[c0 + u];   // dL / dd_k
                const float nd = p == 2 ? vpnorm(vk, 2) : 0.f;
                Vec g, gn;   // dL/dv_k and its negation
                vpnorm_bwd(vk, nd, p, cd, g);
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) gn.x[i] = -g.x[i];
                if (kind[u] == 0) {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) cH.x[i] += g.x[i];
                    sink.ent(tk[u], gn, tb, D, lane);
                } else if (kind[u] == 1) {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) cT.x[i] -= g.x[i];
                    sink.ent(hk[u], g, tb, D, lane);
                } else {
                    sink.ent(hk[u], g, tb, D, lane);
                    sink.rel(rk[u], g, tb, D, lane);
                    sink.ent(tk[u], gn, tb, D, lane);
                }
            }
            if (pass == 1) {
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) {
                    aH.x[i] += cH.x[i];
                    aT.x[i] += cT.x[i];
                }
            }
        }
        if (pass == 1) break;
        // ---- between the passes: weights, loss partial and dL/dd_k, lane-parallel over the group's scores
        __builtin_amdgcn_wave_barrier();   // LDS order inside a wave is program order
        const float lp = loss_block<G>(L, P.margin, bs, neg, sc, lane, ps, sg, &dldp);   // (loss_block.h)
        if (lane == 0 && lpart) lpart[b] = lp;
        __builtin_amdgcn_wave_barrier();
    }
    // ---- positive backward and the on-chip sums
    Vec aR;
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) aR.x[i] = aH.x[i] - aT.x[i];
    if (dldp != 0.f) {
        Vec g;
        vpnorm_bwd(vpos, dp, p, dldp * sg, g);
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) {
            aH.x[i] += g.x[i];
            aR.x[i] += g.x[i];
            aT.x[i] -= g.x[i];
        }
    }
    if (vnonzero(aR)) sink.rel(rp, aR, tb, D, lane);
    if (vnonzero(aH)) sink.ent(hp, aH, tb, D, lane);
    if (vnonzero(aT)) sink.ent(tp, aT, tb, D, lane);
}

}  // namespace dev

// a group's K scores and its transpose row sit in LDS: at most 64 KB of it (the launch default) for one group
static constexpr int64_t kAdvLdsFloats = 64 * 1024 / 4;
static int64_t adv_row_floats(const Shape &s) { return s.VEC == 4 ? (int64_t)s.KCH * s.G * s.VEC : 0; }
int64_t step_adv_max_neg(int64_t dim) { return kAdvLdsFloats - adv_row_floats(pick_shape(dim)); }
// rows of negatives in flight per chunk (NCH): 4 where a lane holds up to 8 floats of a row; 2 at 12 and 16 floats
// (KCH 3 and 4, dims 516..1,024), where 4 rows in flight leave one wave per SIMD (256 VGPRs) - as k_step_transd
// drops to 2 at 8 floats per lane. The rule rests on dim 768 (KCH 3), where 4 rows measured 17 % slower than 2
// (487.8 against 415.1 us); at dim 1,024 the depths 1, 2 and 4 tie within 1 %
constexpr int adv_nch(int vec, int kch) { return vec * kch > 8 ? 2 : 4; }

hipError_t launch_step_adv(const StepParams &P, const LossParams &L, const int64_t *bh, const int64_t *bt,
                           const int64_t *br, const StepWorkspace &W, hipStream_t st) {
    if (P.batch_size <= 0) return hipSuccess;
    if (P.model != 0 || P.neg < 1 || P.neg > step_adv_max_neg(P.dim)) return hipErrorInvalidValue;   // (cap >= 1 below)
    const Shape s = pick_shape(P.dim);
    // lane groups per block: 256 threads' worth, fewer when their score rows would not fit 64 KB of LDS (the block
    // is then gpb * G threads, not always a multiple of 64: harmless, a group never straddles a wave and the kernel
    // has no block-wide barrier)
    int64_t gpb = 256 / s.G;
    const int64_t rw = adv_row_floats(s);
    const int64_t cap = kAdvLdsFloats / (P.neg + rw);
    if (gpb > cap) gpb = cap;
    dev::AdvSink sink{W.gent, W.grel, W.fent, W.frel};
    const dim3 grid((unsigned)((P.batch_size + gpb - 1) / gpb)), block((unsigned)(gpb * s.G));
    const size_t lds = sizeof(float) * (size_t)(gpb * (P.neg + rw));
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_step_adv<T::G, T::VEC, T::KCH, adv_nch(T::VEC, T::KCH)>), grid, block, lds, st, P, L,
                           bh, bt, br, sink, W.lpart);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

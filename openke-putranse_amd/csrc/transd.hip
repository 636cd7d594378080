// HIP kernels of TransD for gfx950: the external-batch training step under plain MarginLoss and the scores behind
// pt_score / pt_score_queries / pt_score_rows.
//
// Semantics (TransD.py:94-129 with dim_e == dim_r, where _resize is the identity): tables ent, rel, ent_transfer,
// rel_transfer; N(x) = x / max(||x||, 1e-12);
//   u_e = e + (e . e_p) r_p,  e_perp = N(u_e)  (always), under norm_flag e_perp <- N(e_perp) and r <- N(r);
//   d = ||(h_perp + r) - t_perp||_p  (head_batch: h_perp + (r - t_perp));
//   MarginLoss.py:24-31 through NegativeSampling.py:13-31: L = mean_{i,k} max(p_i - n_ik, -m) + m, maximum tie -> half.
// Backward of one projected side with upstream gradient g_u at u: de = g_u + (g_u . r_p) e_p, de_p = (g_u . r_p) e,
// dr_p += (e . e_p) g_u; g_u comes from the gradient at the scored vector through the normalise Jacobian(s).
//
// Mapping of k_step_transd (the one k_step_adv arrived at): the lane-group row layout of device.h; ONE lane group
// owns a positive and walks its K negatives, the rows of NCH negatives in flight together. The positive's six rows
// are loaded once; h_perp, t_perp, r^ and the projection scalars stay in registers. A negative that shares the
// positive's relation and one entity (every entity corruption, every cross-sampled slot) loads two rows (e, e_p);
// any other slot loads its six. The gradients at the positive's scored vectors are summed over the negatives in
// registers (chunk partials first) and pushed through the normalise Jacobians and the transfer chain ONCE per
// positive: those depend on the positive's rows only, so the chain is linear in the upstream gradient. Per negative
// only the corrupted side's chain runs; its two rows (ent, ent_transfer) are added with float atomics through the
// group's LDS transpose row (row_atomic, device.h) plus touched flags. Entity and transfer gradients leave the
// kernel finished (the apply pass applies no Jacobian to them); the relation row's gradient stays in normalised
// space under norm_flag and the apply pass multiplies by the Jacobian of the pre-step row, as for TransE.
// lpart[b] = sum_k max(p_b - n_bk, -m); the apply pass reduces the partials in a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

// one projected entity: its two rows, u = e + (e . e_p) r_p, the scored vector f and the scalars of the chain
template <int G, int VEC, int KCH>
struct DSide {
    V<G, VEC, KCH> E, Ep, u, f;
    float s, nu, n2;   // e . e_p, ||u||, ||N(u)|| (the second normalise's input norm; unused without norm_flag)
};

template <int G, int VEC, int KCH>
__device__ __forceinline__ void d_load(DSide<G, VEC, KCH> &S, const StepParams &P, int64_t e, int D, int lane) {
    vload(S.E, P.ent + e * D, D, lane);
    vload(S.Ep, P.ent_t + e * D, D, lane);
}

template <int G, int VEC, int KCH>
__device__ __forceinline__ void d_project(DSide<G, VEC, KCH> &S, const V<G, VEC, KCH> &Rp, bool nf) {
    using Vec = V<G, VEC, KCH>;
    S.s = vdot(S.E, S.Ep);
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) S.u.x[i] = S.E.x[i] + S.s * Rp.x[i];
    if (nf) {
        Vec h1;
        S.nu = vnormalize(S.u, h1);
        S.n2 = vnormalize(h1, S.f);
    } else {
        S.nu = vnormalize(S.u, S.f);
        S.n2 = 1.f;
    }
}

// gs = gradient at the scored vector f: dE, dEp = the gradients of the side's two rows; aRp += (e . e_p) g_u
template <int G, int VEC, int KCH>
__device__ __forceinline__ void d_project_bwd(const DSide<G, VEC, KCH> &S, const V<G, VEC, KCH> &Rp, bool nf,
                                              const V<G, VEC, KCH> &gs, V<G, VEC, KCH> &dE, V<G, VEC, KCH> &dEp,
                                              V<G, VEC, KCH> &aRp) {
    using Vec = V<G, VEC, KCH>;
    Vec g1, gu;
    if (nf) {
        Vec h1;   // N(u), re-formed by the forward's instructions
        const float inv = 1.0f / (S.nu > kEps ? S.nu : kEps);
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) h1.x[i] = S.u.x[i] * inv;
        vnormalize_bwd(h1, S.n2, gs, g1);
    } else {
        g1 = gs;
    }
    vnormalize_bwd(S.u, S.nu, g1, gu);
    const float c = vdot(gu, Rp);
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        dE.x[i] = gu.x[i] + c * S.Ep.x[i];
        dEp.x[i] = c * S.E.x[i];
        aRp.x[i] += S.s * gu.x[i];
    }
}

struct TransDSink {
    float *gent, *grel, *gentt, *grelt;
    int *fent, *frel, *fentt, *frelt;
    template <int G, int VEC, int KCH>
    __device__ __forceinline__ void ent(int64_t row, const V<G, VEC, KCH> &g, const V<G, VEC, KCH> &gp, float *tb,
                                        int D, int lane) const {
        row_atomic(g, gent + row * D, tb, D, lane);
        row_atomic(gp, gentt + row * D, tb, D, lane);
        if (lane == 0) {
            fent[row] = 1;
            fentt[row] = 1;
        }
    }
    template <int G, int VEC, int KCH>
    __device__ __forceinline__ void rel(int64_t row, const V<G, VEC, KCH> &g, const V<G, VEC, KCH> &gp, float *tb,
                                        int D, int lane) const {
        row_atomic(g, grel + row * D, tb, D, lane);
        row_atomic(gp, grelt + row * D, tb, D, lane);
        if (lane == 0) {
            frel[row] = 1;
            frelt[row] = 1;
        }
    }
};

template <int G, int VEC, int KCH, int NCH>
__global__ __launch_bounds__(256) void k_step_transd(StepParams P, const int64_t *__restrict__ bh,
                                                     const int64_t *__restrict__ bt, const int64_t *__restrict__ br,
                                                     TransDSink sink, float *__restrict__ lpart) {
    using Vec = V<G, VEC, KCH>;
    using Side = DSide<G, VEC, KCH>;
    constexpr int RW = VEC == 4 ? KCH * G * VEC : 0;   // floats of a group's transpose row (row_atomic)
    extern __shared__ __attribute__((aligned(16))) float s_lds[];   // [groups per block][RW]
    const int gpb = (int)blockDim.x / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t bs = P.batch_size;
    const int neg = (int)P.neg;
    const int64_t b = (int64_t)blockIdx.x * gpb + grp;
    if (b >= bs) return;   // (no block-wide barrier below: a group is inside one wave)
    float *tb = s_lds + (size_t)grp * RW;
    const int D = (int)P.dim;
    const int p = P.p_norm;
    const bool nf = P.norm_flag != 0;
    const float m = P.margin, inv = P.inv_count;
    // ---- positive
    const int64_t hp = bh[b], tp = bt[b], rp = br[b];
    Side Hs, Ts;
    Vec rh, Rp, base, vpos;
    {
        Vec R;
        d_load(Hs, P, hp, D, lane);
        d_load(Ts, P, tp, D, lane);
        vload(R, P.rel + rp * D, D, lane);
        vload(Rp, P.rel_t + rp * D, D, lane);
        d_project(Hs, Rp, nf);
        d_project(Ts, Rp, nf);
        if (nf) vnormalize(R, rh); else rh = R;
    }
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        base.x[i] = Hs.f.x[i] + rh.x[i];
        vpos.x[i] = base.x[i] - Ts.f.x[i];
    }
    const float dp = vpnorm(vpos, p);
    // on-chip sums over the negatives that share the positive's rows: aH = dL/dh_perp, aT = dL/dt_perp (their sum of
    // dL/dv_k, signed), aP = dL/dr_p of the corrupted sides; each chunk sums into accumulators of its own first
    Vec aH, aT, aP;
    vzero(aH); vzero(aT); vzero(aP);
    float csum = 0.f, lsum = 0.f;

    for (int c0 = 0; c0 < neg; c0 += NCH) {
        int64_t hk[NCH], tk[NCH], rk[NCH];
        int kind[NCH];   // 0: shares (h, r): rows of t_k; 1: shares (r, t): rows of h_k; 2: any other slot; -1: none
        Side S[NCH];
        Vec cH, cT, cP;
        vzero(cH); vzero(cT); vzero(cP);
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            kind[u] = -1;
            if (c0 + u >= neg) continue;
            const int64_t o = (int64_t)(c0 + u + 1) * bs + b;
            hk[u] = bh[o]; tk[u] = bt[o]; rk[u] = br[o];
            kind[u] = rk[u] != rp ? 2 : (hk[u] == hp ? 0 : (tk[u] == tp ? 1 : 2));
            if (kind[u] < 2) d_load(S[u], P, kind[u] == 0 ? tk[u] : hk[u], D, lane);
        }
#pragma unroll
        for (int u = 0; u < NCH; ++u) {
            if (kind[u] < 0) continue;
            Vec vk, g, dE, dEp;
            if (kind[u] < 2) {
                d_project(S[u], Rp, nf);
                if (kind[u] == 0) {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) vk.x[i] = base.x[i] - S[u].f.x[i];
                } else {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) vk.x[i] = (S[u].f.x[i] + rh.x[i]) - Ts.f.x[i];
                }
                const float ns = vpnorm(vk, p);
                const float a = dp - ns;
                lsum += a > -m ? a : -m;
                const float c = a > -m ? inv : (a == -m ? inv * 0.5f : 0.f);
                if (c == 0.f) continue;   // no gradient through this negative
                csum += c;
                vpnorm_bwd(vk, ns, p, -c, g);   // dL/dv_k
                Vec gs;
                if (kind[u] == 0) {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) {
                        cH.x[i] += g.x[i];
                        gs.x[i] = -g.x[i];
                    }
                    d_project_bwd(S[u], Rp, nf, gs, dE, dEp, cP);
                    sink.ent(tk[u], dE, dEp, tb, D, lane);
                } else {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) cT.x[i] -= g.x[i];
                    d_project_bwd(S[u], Rp, nf, g, dE, dEp, cP);
                    sink.ent(hk[u], dE, dEp, tb, D, lane);
                }
            } else {
                Side A, C;
                Vec Rk, rkh, Rpk, gn, gpk;
                d_load(A, P, hk[u], D, lane);
                d_load(C, P, tk[u], D, lane);
                vload(Rk, P.rel + rk[u] * D, D, lane);
                vload(Rpk, P.rel_t + rk[u] * D, D, lane);
                d_project(A, Rpk, nf);
                d_project(C, Rpk, nf);
                if (nf) vnormalize(Rk, rkh); else rkh = Rk;
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) vk.x[i] = (A.f.x[i] + rkh.x[i]) - C.f.x[i];
                const float ns = vpnorm(vk, p);
                const float a = dp - ns;
                lsum += a > -m ? a : -m;
                const float c = a > -m ? inv : (a == -m ? inv * 0.5f : 0.f);
                if (c == 0.f) continue;
                csum += c;
                vpnorm_bwd(vk, ns, p, -c, g);
                vzero(gpk);
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) gn.x[i] = -g.x[i];
                d_project_bwd(A, Rpk, nf, g, dE, dEp, gpk);
                sink.ent(hk[u], dE, dEp, tb, D, lane);
                d_project_bwd(C, Rpk, nf, gn, dE, dEp, gpk);
                sink.ent(tk[u], dE, dEp, tb, D, lane);
                sink.rel(rk[u], g, gpk, tb, D, lane);
            }
        }
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) {
            aH.x[i] += cH.x[i];
            aT.x[i] += cT.x[i];
            aP.x[i] += cP.x[i];
        }
    }
    if (lane == 0 && lpart) lpart[b] = lsum;
    // ---- positive backward and the on-chip sums: the positive's chains run once
    Vec aR;
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) aR.x[i] = aH.x[i] - aT.x[i];
    if (csum != 0.f) {
        Vec g;
        vpnorm_bwd(vpos, dp, p, csum, g);
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) {
            aH.x[i] += g.x[i];
            aR.x[i] += g.x[i];
            aT.x[i] -= g.x[i];
        }
    }
    Vec dE, dEp;
    if (vnonzero(aH)) {
        d_project_bwd(Hs, Rp, nf, aH, dE, dEp, aP);
        sink.ent(hp, dE, dEp, tb, D, lane);
    }
    if (vnonzero(aT)) {
        d_project_bwd(Ts, Rp, nf, aT, dE, dEp, aP);
        sink.ent(tp, dE, dEp, tb, D, lane);   // (a self-loop positive adds twice to the same rows)
    }
    if (vnonzero(aR) || vnonzero(aP)) sink.rel(rp, aR, aP, tb, D, lane);
}

// ---------------------------------------------------------------- scoring ----------------------
// model.predict over n triples (mode 0 normal, 1 head_batch: h varies, 2 tail_batch: t varies), IEEE sqrt and
// division throughout (the scores feed ranking)
template <int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_score_transd(StepParams P, int mode, const int64_t *__restrict__ h,
                                                      const int64_t *__restrict__ t, const int64_t *__restrict__ r,
                                                      int64_t n, float *__restrict__ out) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (i >= n) return;
    const int D = (int)P.dim;
    const bool nf = P.norm_flag != 0;
    const int64_t hi = h[mode == 1 || mode == 0 ? i : 0];
    const int64_t ti = t[mode == 2 || mode == 0 ? i : 0];
    const int64_t ri = r[mode == 0 ? i : 0];
    DSide<G, VEC, KCH> H, T;
    Vec R, Rp, rh, v;
    d_load(H, P, hi, D, lane);
    d_load(T, P, ti, D, lane);
    vload(R, P.rel + ri * D, D, lane);
    vload(Rp, P.rel_t + ri * D, D, lane);
    d_project(H, Rp, nf);
    d_project(T, Rp, nf);
    if (nf) vnormalize(R, rh); else rh = R;
#pragma unroll
    for (int k = 0; k < Vec::N; ++k)
        v.x[k] = mode == 1 ? H.f.x[k] + (rh.x[k] - T.f.x[k]) : (H.f.x[k] + rh.x[k]) - T.f.x[k];
    const float s = vpnorm(v, P.p_norm);
    if (lane == 0) out[i] = s;
}

// Candidate scoring for link prediction (the layout and candidate orders of k_score_queries): per query the anchor's
// projected row and r^ are formed once; per candidate two row loads, the projection, the normalise(s), the p-norm
template <int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_score_queries_transd(StepParams P, int side, const int64_t *__restrict__ qh,
                                                              const int64_t *__restrict__ qt,
                                                              const int64_t *__restrict__ qr, int64_t nq, int64_t E,
                                                              float *__restrict__ out, int global_order) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t q = blockIdx.y;
    if (q >= nq) return;
    const int D = (int)P.dim;
    const bool nf = P.norm_flag != 0;
    const int64_t h = qh[q], t = qt[q], r = qr[q];
    const int64_t truth = side == 0 ? h : t;
    const int64_t anchor = side == 0 ? t : h;
    Vec R, Rp, rh, base;
    {
        DSide<G, VEC, KCH> A;
        d_load(A, P, anchor, D, lane);
        vload(R, P.rel + r * D, D, lane);
        vload(Rp, P.rel_t + r * D, D, lane);
        d_project(A, Rp, nf);
        if (nf) vnormalize(R, rh); else rh = R;
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) base.x[k] = side == 0 ? rh.x[k] - A.f.x[k] : A.f.x[k] + rh.x[k];
    }
    float *row = out + q * E;
    for (int64_t j = (int64_t)blockIdx.x * GPB + grp; j < E; j += (int64_t)gridDim.x * GPB) {
        const int64_t e = global_order ? j : (j == 0 ? truth : (j - 1 < truth ? j - 1 : j));
        DSide<G, VEC, KCH> X;
        Vec v;
        d_load(X, P, e, D, lane);
        d_project(X, Rp, nf);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) v.x[k] = side == 0 ? X.f.x[k] + base.x[k] : base.x[k] - X.f.x[k];
        const float s = vpnorm(v, P.p_norm);
        if (lane == 0) row[j] = s;
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
hipError_t launch_step_transd(const StepParams &P, const int64_t *bh, const int64_t *bt, const int64_t *br,
                              const StepWorkspace &W, hipStream_t st) {
    if (P.batch_size <= 0) return hipSuccess;
    if (P.model != 2 || P.neg < 1 || !P.ent_t || !P.rel_t || !W.gentt || !W.grelt || !W.fentt || !W.frelt)
        return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const int64_t rw = s.VEC == 4 ? (int64_t)s.KCH * s.G * s.VEC : 0;
    dev::TransDSink sink{W.gent, W.grel, W.gentt, W.grelt, W.fent, W.frel, W.fentt, W.frelt};
    const dim3 grid((unsigned)((P.batch_size + gpb - 1) / gpb)), block(256);
    const size_t lds = sizeof(float) * (size_t)(gpb * rw);   // <= 8 KB
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        // rows of negatives in flight per lane group: 4, or 2 where a row vector holds 8 floats per lane
        constexpr int NCH = T::VEC * T::KCH > 4 ? 2 : 4;
        hipLaunchKernelGGL((dev::k_step_transd<T::G, T::VEC, T::KCH, NCH>), grid, block, lds, st, P, bh, bt, br, sink,
                           W.lpart);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_transd(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                               int64_t n, float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!P.ent_t || !P.rel_t) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_transd<T::G, T::VEC, T::KCH>), grid, block, 0, st, P, mode, h, t, r, n, out);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_queries_transd(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                       const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                       int global_order) {
    if (nq <= 0) return hipSuccess;
    if (!P.ent_t || !P.rel_t) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    int64_t bx = (E + gpb - 1) / gpb;
    if (bx > 128) bx = 128;
    const dim3 grid((unsigned)bx, (unsigned)nq), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_queries_transd<T::G, T::VEC, T::KCH>), grid, block, 0, st, P, side, qh, qt,
                           qr, nq, E, out, global_order);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

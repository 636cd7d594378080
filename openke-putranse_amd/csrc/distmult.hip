// HIP kernels of DistMult for gfx950: the external-batch training step under SigmoidLoss (= SoftplusLoss) with or
// without the self-adversarial weights and with the batch regulariser (regul_rate) folded in, and the scores behind
// pt_score / pt_score_queries / pt_score_rows.
//
// Semantics (DistMult.py:34-72): ent [E][dim], rel [R][dim], nothing normalised; s = sum_j h_j r_j t_j is handed to
// the loss as it is (higher is better; no margin enters), predict returns -s. The loss is loss_block.h's SigmoidLoss
// (SoftplusLoss.py:22-26 is the same function up to nn.Softplus's threshold at 20: exp(-20) off, below a float32 ulp).
// regul_rate (DistMult.py:57-65, NegativeSampling.py:28-29) adds regul_rate * (mean h^2 + mean t^2 + mean r^2) / 3
// over the rows the data loader hands over: with N = B (1 + K) slots, every slot's row counts with 1 / (N dim) in
// normal mode; in head_batch / tail_batch (RegulParams::mode 1 / 2) only the varying side does, the fixed side and
// the relation are handed over once per positive and count with 1 / (B dim). As a gradient that is rho * row with
// rho = 2 regul_rate / (3 N dim) or 2 regul_rate / (3 B dim), as a loss rho / 2 * |row|^2.
//
// Mapping of k_step_distmult (k_step_adv's and k_step_rotate's): ONE lane group owns a positive and its K negatives
// and walks them twice. Pass 1 puts s_k into LDS; loss_block (shared with step_adv.hip) forms the weights, the loss
// partial and c_k = dL/ds_k lane-parallel; pass 2 emits gradients. A dot product is separable over the dims, so both
// passes walk the row in PIECES of G * VEC floats as k_step_rotate does and pass 1 adds a piece's partial score into
// the group's LDS score: register use does not depend on the dim. Per piece the structure of a product score stays
// on chip:
//   a negative that keeps (h, r):  s_k = <u, t_k> with u = h o r in registers; dL/dt_k = c_k u goes out through
//                                  row_atomic; A = sum_k c_k t_k stays on chip (the positive joins it as c_p t);
//   a negative that keeps (r, t):  the mirror case with w = r o t: dL/dh_k = c_k w, B = sum_k c_k h_k;
//   finished once per positive:    dL/dh = r o A,  dL/dt = r o B + c_p u,  dL/dr = h o A + t o B;
//   any other slot (a relation corruption, both entities replaced): its own three rows, one slot at a time.
// regul_rate (template flag REG; with REG off none of it is read or computed): rho * row is added to a gradient row
// where that row is written anyway - the corrupted entity's row per slot, the positive's three rows with rho times
// the number of slots that share them (per-positive coefficient in modes 1 / 2). The squared norms of every slot's
// rows are summed in pass 1 and join the loss partial DIVIDED BY loss_affine's scale, so that the apply pass's
// scale * sum(lpart) + cst stays the step's loss (one term, not two). A regularised step does not skip a negative
// whose weight underflowed to 0: its row still takes rho * row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"
#include "loss_block.h"

namespace pt {
namespace dev {

struct DmSink {   // (row_atomic: device.h)
    float *gent, *grel;
    int *fent, *frel;
    template <typename Vec>
    __device__ __forceinline__ void ent(int64_t e, const Vec &g, float *tb, int D, int o, int lane) const {
        row_atomic(g, gent + e * (int64_t)D + o, tb, D - o, lane);
        if (lane == 0) fent[e] = 1;
    }
    template <typename Vec>
    __device__ __forceinline__ void rel(int64_t r, const Vec &g, float *tb, int D, int o, int lane) const {
        row_atomic(g, grel + r * (int64_t)D + o, tb, D - o, lane);
        if (lane == 0) frel[r] = 1;
    }
};

// gradient coefficients rho of the regulariser: p* of the positive's slot, q* of a negative's slot (h, t, r rows);
// lscale = 1 / loss_affine's scale
struct DmRegul {
    float ph, pt, pr, qh, qt, qr, lscale;
};

template <typename Vec>
__device__ __forceinline__ float dm_sq(const Vec &a) {   // this lane's part of |a|^2
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) s += a.x[i] * a.x[i];
    return s;
}

template <int G, int VEC, int NCH, bool REG>
__global__ __launch_bounds__(256) void k_step_distmult(StepParams P, LossParams L, DmRegul Q,
                                                       const int64_t *__restrict__ bh,
                                                       const int64_t *__restrict__ bt,
                                                       const int64_t *__restrict__ br, DmSink sink,
                                                       float *__restrict__ lpart) {
    using Vec = V<G, VEC, 1>;
    constexpr int PW = G * VEC;                 // floats of a piece
    constexpr int RW = VEC == 4 ? PW : 0;       // floats of a group's transpose row (row_atomic)
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
    const int64_t hp = bh[b], tp = bt[b], rp = br[b];
    float ps = 0.f;     // the positive's score (pass 1)
    float dldp = 0.f;   // dL / d(ps) (pass 2)
    // REG: this lane's part of the squared norms of the positive's rows and of sum rho / 2 |row|^2 over the
    // negatives' own rows; the slots that share the positive's (h, r) and (r, t)
    float nh2 = 0.f, nt2 = 0.f, nr2 = 0.f, rl = 0.f;
    int n0 = 0, n1 = 0;

    for (int pass = 0; pass < 2; ++pass) {
        for (int o = 0; o < D; o += PW) {
            // ---- the positive's piece: h, r, t, u = h o r, w = r o t
            Vec H, R, T, u, w;
            vload(H, P.ent + hp * (int64_t)D + o, D - o, lane);
            vload(T, P.ent + tp * (int64_t)D + o, D - o, lane);
            vload(R, P.rel + rp * (int64_t)D + o, D - o, lane);
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) {
                u.x[i] = H.x[i] * R.x[i];
                w.x[i] = R.x[i] * T.x[i];
            }
            if (pass == 0) {
                ps += vdot(u, T);   // (vdot sums over the group)
                if (REG) {
                    nh2 += dm_sq(H);
                    nt2 += dm_sq(T);
                    nr2 += dm_sq(R);
                }
            }
            // on-chip sums of this piece: aA = sum c_k t_k over the negatives that keep (h, r), aB = sum c_k h_k over
            // those that keep (r, t). Each chunk sums into accumulators of its own first (as k_step_adv: shorter
            // float32 chains)
            Vec aA, aB;
            vzero(aA); vzero(aB);
            for (int c0 = 0; c0 < neg; c0 += NCH) {
                int64_t hk[NCH], tk[NCH];
                int kind[NCH];   // 0: keeps (h, r): row t_k; 1: keeps (r, t): row h_k; -1: nothing (here)
                unsigned other = 0;   // bit i: slot i is any other negative: the three-row path below
                Vec E[NCH], cA, cB;
                vzero(cA); vzero(cB);
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    kind[i] = -1;
                    if (c0 + i >= neg) continue;
                    if (!REG && pass == 1 && sc[c0 + i] == 0.f) continue;   // no gradient through this negative
                    const int64_t x = (int64_t)(c0 + i + 1) * bs + b;
                    hk[i] = bh[x]; tk[i] = bt[x];
                    const int64_t rk = br[x];
                    kind[i] = rk != rp ? -1 : (hk[i] == hp ? 0 : (tk[i] == tp ? 1 : -1));
                    if (kind[i] < 0) other |= 1u << i;
                    else vload(E[i], P.ent + (kind[i] == 0 ? tk[i] : hk[i]) * (int64_t)D + o, D - o, lane);
                }
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    if (kind[i] < 0) continue;
                    if (pass == 0) {
                        const float d = kind[i] == 0 ? vdot(u, E[i]) : vdot(E[i], w);
                        if (lane == 0) sc[c0 + i] = o == 0 ? d : sc[c0 + i] + d;
                        if (REG) {
                            rl += 0.5f * (kind[i] == 0 ? Q.qt : Q.qh) * dm_sq(E[i]);
                            if (o == 0) {
                                if (kind[i] == 0) ++n0; else ++n1;
                            }
                        }
                        continue;
                    }
                    const float ck = sc[c0 + i];   // dL / ds_k
                    Vec g;
                    if (kind[i] == 0) {
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) {
                            cA.x[j] += ck * E[i].x[j];
                            g.x[j] = ck * u.x[j];
                            if (REG) g.x[j] += Q.qt * E[i].x[j];
                        }
                        sink.ent(tk[i], g, tb, D, o, lane);
                    } else {
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) {
                            cB.x[j] += ck * E[i].x[j];
                            g.x[j] = ck * w.x[j];
                            if (REG) g.x[j] += Q.qh * E[i].x[j];
                        }
                        sink.ent(hk[i], g, tb, D, o, lane);
                    }
                }
                // any other slot (another relation, or both entities replaced): its own three rows; one copy of the
                // code, a slot at a time (the samplers draw such slots only as relation corruptions)
#pragma unroll 1
                for (int i = 0; i < NCH; ++i) {
                    if (!((other >> i) & 1u)) continue;
                    const int64_t x = (int64_t)(c0 + i + 1) * bs + b;
                    const int64_t hx = bh[x], tx = bt[x], rx = br[x];
                    Vec X, Y, Z;
                    vload(X, P.ent + hx * (int64_t)D + o, D - o, lane);
                    vload(Y, P.rel + rx * (int64_t)D + o, D - o, lane);
                    vload(Z, P.ent + tx * (int64_t)D + o, D - o, lane);
                    if (pass == 0) {
                        float d = 0.f;
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) d += (X.x[j] * Y.x[j]) * Z.x[j];
                        d = gsum<G>(d);
                        if (lane == 0) sc[c0 + i] = o == 0 ? d : sc[c0 + i] + d;
                        if (REG) rl += 0.5f * (Q.qh * dm_sq(X) + Q.qr * dm_sq(Y) + Q.qt * dm_sq(Z));
                        continue;
                    }
                    const float ck = sc[c0 + i];
                    Vec gx, gy, gz;
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        gx.x[j] = ck * (Y.x[j] * Z.x[j]);
                        gy.x[j] = ck * (X.x[j] * Z.x[j]);
                        gz.x[j] = ck * (X.x[j] * Y.x[j]);
                        if (REG) {
                            gx.x[j] += Q.qh * X.x[j];
                            gy.x[j] += Q.qr * Y.x[j];
                            gz.x[j] += Q.qt * Z.x[j];
                        }
                    }
                    sink.ent(hx, gx, tb, D, o, lane);
                    sink.rel(rx, gy, tb, D, o, lane);
                    sink.ent(tx, gz, tb, D, o, lane);
                }
                if (pass == 1) {
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        aA.x[j] += cA.x[j];
                        aB.x[j] += cB.x[j];
                    }
                }
            }
            if (pass == 0) continue;
            // ---- the positive's own gradient (it joins A as c_p t) and the on-chip sums of this piece
            Vec gh, gt, gr;
#pragma unroll
            for (int j = 0; j < Vec::N; ++j) {
                const float a = aA.x[j] + dldp * T.x[j];
                gh.x[j] = R.x[j] * a;
                gt.x[j] = R.x[j] * aB.x[j] + dldp * u.x[j];
                gr.x[j] = H.x[j] * a + T.x[j] * aB.x[j];
                if (REG) {
                    gh.x[j] += (Q.ph + Q.qh * (float)n0) * H.x[j];
                    gt.x[j] += (Q.pt + Q.qt * (float)n1) * T.x[j];
                    gr.x[j] += (Q.pr + Q.qr * (float)(n0 + n1)) * R.x[j];
                }
            }
            if (vnonzero(gr)) sink.rel(rp, gr, tb, D, o, lane);
            if (vnonzero(gh)) sink.ent(hp, gh, tb, D, o, lane);
            if (vnonzero(gt)) sink.ent(tp, gt, tb, D, o, lane);
        }
        if (pass == 1) break;
        // ---- between the passes: weights, loss partial and dL/ds_k, lane-parallel over the group's scores
        __builtin_amdgcn_wave_barrier();   // LDS order inside a wave is program order
        float lp = loss_block<G>(L, P.margin, bs, neg, sc, lane, ps, 1.0f, &dldp);
        if (REG) {
            const float own = rl + 0.5f * ((Q.ph + Q.qh * (float)n0) * nh2 + (Q.pt + Q.qt * (float)n1) * nt2 +
                                           (Q.pr + Q.qr * (float)(n0 + n1)) * nr2);
            lp += gsum<G>(own) * Q.lscale;
        }
        if (lane == 0 && lpart) lpart[b] = lp;
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------- scoring ----------------------
// -s over n triples (mode 0 normal, 1 head_batch: h varies and s = h (r t), 2 tail_batch: t varies), piece by piece
template <int G, int VEC>
__global__ __launch_bounds__(256) void k_score_distmult(StepParams P, int mode, const int64_t *__restrict__ h,
                                                        const int64_t *__restrict__ t, const int64_t *__restrict__ r,
                                                        int64_t n, float *__restrict__ out) {
    using Vec = V<G, VEC, 1>;
    constexpr int GPB = 256 / G;
    constexpr int PW = G * VEC;
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (i >= n) return;
    const int D = (int)P.dim;
    const int64_t hi_ = h[mode == 1 || mode == 0 ? i : 0];
    const int64_t ti_ = t[mode == 2 || mode == 0 ? i : 0];
    const int64_t ri_ = r[mode == 0 ? i : 0];
    float s = 0.f;
    for (int o = 0; o < D; o += PW) {
        Vec H, T, R;
        vload(H, P.ent + hi_ * (int64_t)D + o, D - o, lane);
        vload(T, P.ent + ti_ * (int64_t)D + o, D - o, lane);
        vload(R, P.rel + ri_ * (int64_t)D + o, D - o, lane);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < Vec::N; ++k)
            d += mode == 1 ? H.x[k] * (R.x[k] * T.x[k]) : (H.x[k] * R.x[k]) * T.x[k];
        s += gsum<G>(d);
    }
    if (lane == 0) out[i] = -s;
}

// Candidate scores for link prediction (the layout and candidate orders of k_score_queries). Link prediction for
// DistMult is a plain product [nq][dim] x [dim][E]: a lane group keeps the base rows r o anchor of QT queries in
// registers (whole rows) and ONE pass over an entity row serves all of them as -<base_u, e>; the walk is over the
// entities, and each query places entity e at its own column (candidate order: the truth first, then the others)
template <int G, int VEC, int KCH, int QT>
__global__ __launch_bounds__(256) void k_score_queries_distmult(StepParams P, int side,
                                                                const int64_t *__restrict__ qh,
                                                                const int64_t *__restrict__ qt,
                                                                const int64_t *__restrict__ qr, int64_t nq, int64_t E,
                                                                float *__restrict__ out, int global_order) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t q0 = (int64_t)blockIdx.y * QT;
    if (q0 >= nq) return;
    const int D = (int)P.dim;
    Vec base[QT];
    int64_t truth[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        const int64_t qi = q0 + u < nq ? q0 + u : q0;   // (a tile past the last query repeats its first; not stored)
        const int64_t h = qh[qi], t = qt[qi], r = qr[qi];
        truth[u] = side == 0 ? h : t;
        Vec a, R;
        vload(a, P.ent + (side == 0 ? t : h) * (int64_t)D, D, lane);
        vload(R, P.rel + r * (int64_t)D, D, lane);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) base[u].x[k] = R.x[k] * a.x[k];
    }
    for (int64_t e = (int64_t)blockIdx.x * GPB + grp; e < E; e += (int64_t)gridDim.x * GPB) {
        Vec x;
        vload(x, P.ent + e * (int64_t)D, D, lane);
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            const float s = vdot(x, base[u]);
            const int64_t j = global_order ? e : (e == truth[u] ? 0 : (e < truth[u] ? e + 1 : e));
            if (lane == 0 && q0 + u < nq) out[(q0 + u) * E + j] = -s;
        }
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
// a group's K scores and its transpose row sit in LDS: at most 64 KB of it (the launch default) for one group. The
// limit on neg is step_adv_max_neg's at the same dim, as for RotatE (launch_step_rotate)
static constexpr int64_t kDmLdsFloats = 64 * 1024 / 4;
int64_t step_distmult_max_neg(int64_t dim) {
    const Shape s = pick_shape(dim);
    return kDmLdsFloats - (s.VEC == 4 ? (int64_t)s.KCH * s.G * s.VEC : 0);
}
// rows of negatives in flight per chunk: a piece is 1 or 4 floats per lane and the kernel holds nine piece vectors
// besides, so 4 rows fit every shape (VGPR counts: DESIGN.md section 4)
static constexpr int kDmNch = 4;

hipError_t launch_step_distmult(const StepParams &P, const LossParams &L, const RegulParams &Rg, const int64_t *bh,
                                const int64_t *bt, const int64_t *br, const StepWorkspace &W, hipStream_t st) {
    if (P.batch_size <= 0) return hipSuccess;
    if (P.model != 4 || P.neg < 1 || P.neg > step_distmult_max_neg(P.dim) || L.kind != 1 || L.mflag ||
        Rg.mode < 0 || Rg.mode > 2 || !(Rg.regul >= 0.f))
        return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    // lane groups per block: 256 threads' worth, fewer when their score rows would not fit 64 KB of LDS (see
    // launch_step_adv: a group never straddles a wave and the kernel has no block-wide barrier)
    int64_t gpb = 256 / s.G;
    const int64_t rw = s.VEC == 4 ? (int64_t)s.G * s.VEC : 0;
    const int64_t cap = kDmLdsFloats / (P.neg + rw);   // >= 1: neg <= step_distmult_max_neg
    if (gpb > cap) gpb = cap;
    dev::DmSink sink{W.gent, W.grel, W.fent, W.frel};
    dev::DmRegul Q{};
    const bool reg = Rg.regul != 0.f;
    if (reg) {
        // rho per slot (N = B (1 + K) slots) and per positive, formed in double
        const double B = (double)P.batch_size, N = B * (double)(1 + P.neg), D = (double)P.dim;
        const float rn = (float)(2.0 * (double)Rg.regul / (3.0 * N * D));
        const float rb = (float)(2.0 * (double)Rg.regul / (3.0 * B * D));
        Q.ph = Rg.mode == 2 ? rb : rn;   // tail_batch hands h over once per positive
        Q.pt = Rg.mode == 1 ? rb : rn;   // head_batch: t
        Q.pr = Rg.mode == 0 ? rn : rb;
        Q.qh = Rg.mode == 2 ? 0.f : rn;
        Q.qt = Rg.mode == 1 ? 0.f : rn;
        Q.qr = Rg.mode == 0 ? rn : 0.f;
        float scale, cst;
        loss_affine(L, P, &scale, &cst);
        Q.lscale = 1.0f / scale;
    }
    const dim3 grid((unsigned)((P.batch_size + gpb - 1) / gpb)), block((unsigned)(gpb * s.G));
    const size_t lds = sizeof(float) * (size_t)(gpb * (P.neg + rw));
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        if (reg)
            hipLaunchKernelGGL((dev::k_step_distmult<T::G, T::VEC, kDmNch, true>), grid, block, lds, st, P, L, Q, bh, bt,
                               br, sink, W.lpart);
        else
            hipLaunchKernelGGL((dev::k_step_distmult<T::G, T::VEC, kDmNch, false>), grid, block, lds, st, P, L, Q, bh,
                               bt, br, sink, W.lpart);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_distmult(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                                 int64_t n, float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_distmult<T::G, T::VEC>), grid, block, 0, st, P, mode, h, t, r, n, out);
        e = hipGetLastError();
    });
    return e;
}

// queries per lane group of k_score_queries_distmult (measured: DESIGN.md section 4)
static constexpr int kDmQt = 4;

hipError_t launch_score_queries_distmult(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                         const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                         int global_order) {
    if (nq <= 0) return hipSuccess;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    int64_t bx = (E + gpb - 1) / gpb;
    if (bx > 128) bx = 128;
    const dim3 grid((unsigned)bx, (unsigned)((nq + kDmQt - 1) / kDmQt)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_queries_distmult<T::G, T::VEC, T::KCH, kDmQt>), grid, block, 0, st, P, side,
                           qh, qt, qr, nq, E, out, global_order);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

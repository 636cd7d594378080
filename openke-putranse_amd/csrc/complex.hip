// HIP kernels of ComplEx for gfx950: the external-batch training step under SigmoidLoss (= SoftplusLoss) with or
// without the self-adversarial weights and with the batch regulariser (regul_rate) folded in, and the scores behind
// pt_score / pt_score_queries / pt_score_rows.
//
// Semantics (ComplEx.py:7-64): four tables [rows][dim], ent_re / ent_im / rel_re / rel_im (StepParams::ent / ent_t /
// rel / rel_t), nothing normalised;
//   s = sum_j h_re t_re r_re + h_im t_im r_re + h_re t_im r_im - h_im t_re r_im = Re <h o r, conj(t)>
// is handed to the loss as it is (higher is better; no margin enters), predict returns -s. The loss is loss_block.h's
// SigmoidLoss (SoftplusLoss.py:22-26 is the same function up to nn.Softplus's threshold at 20). regul_rate
// (ComplEx.py:42-56, NegativeSampling.py:28-29) adds regul_rate * (mean h_re^2 + mean h_im^2 + mean t_re^2 + mean
// t_im^2 + mean r_re^2 + mean r_im^2) / 6 over every slot's rows (normal mode only: forward ignores data['mode']):
// with N = B (1 + K) slots, as a gradient rho * row with rho = 2 regul_rate / (6 N dim), as a loss rho / 2 * |row|^2.
//
// Mapping of k_step_complex (k_step_distmult's): ONE lane group owns a positive and its K negatives and walks them
// twice, the row in PIECES of G * VEC floats; pass 1 adds a piece's partial score into the group's LDS score,
// loss_block forms the weights, the loss partial and c_k = dL/ds_k, pass 2 emits gradients. Per piece the structure of
// the complex product stays on chip. With u = h r and w = r conj(t):
//   u_re = h_re r_re - h_im r_im,  u_im = h_im r_re + h_re r_im;
//   w_re = r_re t_re + r_im t_im,  w_im = r_re t_im - r_im t_re
//   a negative that keeps (h, r):  s_k = <u_re, t_re> + <u_im, t_im>; dL/dt_k = c_k (u_re, u_im) goes out through
//                                  row_atomic; A = sum_k c_k t_k stays on chip (the positive joins it as c_p t);
//   a negative that keeps (r, t):  s_k = <w_re, h_re> + <w_im, h_im>; dL/dh_k = c_k (w_re, w_im), B = sum_k c_k h_k;
//   finished once per positive:    dL/dh_re = r_re A_re + r_im A_im,  dL/dh_im = r_re A_im - r_im A_re
//                                  dL/dt_re = r_re B_re - r_im B_im + c_p u_re
//                                  dL/dt_im = r_re B_im + r_im B_re + c_p u_im
//                                  dL/dr_re = h_re A_re + h_im A_im + B_re t_re + B_im t_im
//                                  dL/dr_im = h_re A_im - h_im A_re + B_re t_im - B_im t_re
//   any other slot (a relation corruption, both entities replaced): its own six rows, one slot at a time.
// regul_rate (template flag REG; with REG off none of it is read or computed): rho * row is added to a gradient row
// where that row is written anyway - the corrupted entity's two rows per slot, the positive's six rows with rho times
// the number of slots that share them. The squared norms of every slot's rows are summed in pass 1 and join the loss
// partial DIVIDED BY loss_affine's scale. A regularised step does not skip a negative whose weight underflowed to 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"
#include "loss_block.h"

namespace pt {
namespace dev {

struct CxSink {   // (row_atomic: device.h) re rows into gent / grel, im rows into gentt / grelt
    float *gent, *grel, *gentt, *grelt;
    int *fent, *frel, *fentt, *frelt;
    template <typename Vec>
    __device__ __forceinline__ void ent(int64_t e, const Vec &gre, const Vec &gim, float *tb, int D, int o,
                                        int lane) const {
        row_atomic(gre, gent + e * (int64_t)D + o, tb, D - o, lane);
        row_atomic(gim, gentt + e * (int64_t)D + o, tb, D - o, lane);
        if (lane == 0) {
            fent[e] = 1;
            fentt[e] = 1;
        }
    }
    template <typename Vec>
    __device__ __forceinline__ void rel(int64_t r, const Vec &gre, const Vec &gim, float *tb, int D, int o,
                                        int lane) const {
        row_atomic(gre, grel + r * (int64_t)D + o, tb, D - o, lane);
        row_atomic(gim, grelt + r * (int64_t)D + o, tb, D - o, lane);
        if (lane == 0) {
            frel[r] = 1;
            frelt[r] = 1;
        }
    }
};

// rho of the regulariser (every slot's six rows count alike) and lscale = 1 / loss_affine's scale
struct CxRegul {
    float rho, lscale;
};

template <typename Vec>
__device__ __forceinline__ float cx_sq(const Vec &a, const Vec &b) {   // this lane's part of |a|^2 + |b|^2
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) s += a.x[i] * a.x[i] + b.x[i] * b.x[i];
    return s;
}

template <int G, int VEC, int NCH, bool REG>
__global__ __launch_bounds__(256) void k_step_complex(StepParams P, LossParams L, CxRegul Q,
                                                      const int64_t *__restrict__ bh,
                                                      const int64_t *__restrict__ bt,
                                                      const int64_t *__restrict__ br, CxSink sink,
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
    // REG: this lane's part of the squared norms of the positive's rows (re and im together) and of sum |row|^2 over
    // the negatives' own rows; the slots that share the positive's (h, r) and (r, t)
    float nh2 = 0.f, nt2 = 0.f, nr2 = 0.f, rl = 0.f;
    int n0 = 0, n1 = 0;

    for (int pass = 0; pass < 2; ++pass) {
        for (int o = 0; o < D; o += PW) {
            // ---- the positive's piece: h, r, t (re, im), u = h r, w = r conj(t)
            Vec Hr, Hi, Rr, Ri, Tr, Ti, ur, ui, wr, wi;
            vload(Hr, P.ent + hp * (int64_t)D + o, D - o, lane);
            vload(Hi, P.ent_t + hp * (int64_t)D + o, D - o, lane);
            vload(Tr, P.ent + tp * (int64_t)D + o, D - o, lane);
            vload(Ti, P.ent_t + tp * (int64_t)D + o, D - o, lane);
            vload(Rr, P.rel + rp * (int64_t)D + o, D - o, lane);
            vload(Ri, P.rel_t + rp * (int64_t)D + o, D - o, lane);
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) {
                ur.x[i] = Hr.x[i] * Rr.x[i] - Hi.x[i] * Ri.x[i];
                ui.x[i] = Hi.x[i] * Rr.x[i] + Hr.x[i] * Ri.x[i];
                wr.x[i] = Rr.x[i] * Tr.x[i] + Ri.x[i] * Ti.x[i];
                wi.x[i] = Rr.x[i] * Ti.x[i] - Ri.x[i] * Tr.x[i];
            }
            if (pass == 0) {
                float d = 0.f;
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) d += ur.x[i] * Tr.x[i] + ui.x[i] * Ti.x[i];
                ps += gsum<G>(d);
                if (REG) {
                    nh2 += cx_sq(Hr, Hi);
                    nt2 += cx_sq(Tr, Ti);
                    nr2 += cx_sq(Rr, Ri);
                }
            }
            // on-chip sums of this piece: A = sum c_k t_k over the negatives that keep (h, r), B = sum c_k h_k over
            // those that keep (r, t). Each chunk sums into accumulators of its own first (shorter float32 chains)
            Vec aAr, aAi, aBr, aBi;
            vzero(aAr); vzero(aAi); vzero(aBr); vzero(aBi);
            for (int c0 = 0; c0 < neg; c0 += NCH) {
                int64_t ek[NCH];      // the corrupted entity of a slot that keeps (h, r) or (r, t)
                int kind[NCH];        // 0: keeps (h, r): rows t_k; 1: keeps (r, t): rows h_k; -1: nothing (here)
                unsigned other = 0;   // bit i: slot i is any other negative: the six-row path below
                Vec Er[NCH], Ei[NCH], cAr, cAi, cBr, cBi;
                vzero(cAr); vzero(cAi); vzero(cBr); vzero(cBi);
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    kind[i] = -1;
                    if (c0 + i >= neg) continue;
                    if (!REG && pass == 1 && sc[c0 + i] == 0.f) continue;   // no gradient through this negative
                    const int64_t x = (int64_t)(c0 + i + 1) * bs + b;
                    const int64_t hk = bh[x], tk = bt[x], rk = br[x];
                    kind[i] = rk != rp ? -1 : (hk == hp ? 0 : (tk == tp ? 1 : -1));
                    if (kind[i] < 0) {
                        other |= 1u << i;
                    } else {
                        ek[i] = kind[i] == 0 ? tk : hk;
                        vload(Er[i], P.ent + ek[i] * (int64_t)D + o, D - o, lane);
                        vload(Ei[i], P.ent_t + ek[i] * (int64_t)D + o, D - o, lane);
                    }
                }
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    if (kind[i] < 0) continue;
                    if (pass == 0) {
                        float d = 0.f;
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j)
                            d += kind[i] == 0 ? ur.x[j] * Er[i].x[j] + ui.x[j] * Ei[i].x[j]
                                              : wr.x[j] * Er[i].x[j] + wi.x[j] * Ei[i].x[j];
                        d = gsum<G>(d);
                        if (lane == 0) sc[c0 + i] = o == 0 ? d : sc[c0 + i] + d;
                        if (REG) {
                            rl += cx_sq(Er[i], Ei[i]);
                            if (o == 0) {
                                if (kind[i] == 0) ++n0; else ++n1;
                            }
                        }
                        continue;
                    }
                    const float ck = sc[c0 + i];   // dL / ds_k
                    Vec gr, gi;
                    if (kind[i] == 0) {
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) {
                            cAr.x[j] += ck * Er[i].x[j];
                            cAi.x[j] += ck * Ei[i].x[j];
                            gr.x[j] = ck * ur.x[j];
                            gi.x[j] = ck * ui.x[j];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) {
                            cBr.x[j] += ck * Er[i].x[j];
                            cBi.x[j] += ck * Ei[i].x[j];
                            gr.x[j] = ck * wr.x[j];
                            gi.x[j] = ck * wi.x[j];
                        }
                    }
                    if (REG) {
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j) {
                            gr.x[j] += Q.rho * Er[i].x[j];
                            gi.x[j] += Q.rho * Ei[i].x[j];
                        }
                    }
                    sink.ent(ek[i], gr, gi, tb, D, o, lane);
                }
                // any other slot (another relation, or both entities replaced): its own six rows; one copy of the
                // code, a slot at a time (the samplers draw such slots only as relation corruptions)
#pragma unroll 1
                for (int i = 0; i < NCH; ++i) {
                    if (!((other >> i) & 1u)) continue;
                    const int64_t x = (int64_t)(c0 + i + 1) * bs + b;
                    const int64_t hx = bh[x], tx = bt[x], rx = br[x];
                    Vec Xr, Xi, Yr, Yi, Zr, Zi;
                    vload(Xr, P.ent + hx * (int64_t)D + o, D - o, lane);
                    vload(Xi, P.ent_t + hx * (int64_t)D + o, D - o, lane);
                    vload(Yr, P.rel + rx * (int64_t)D + o, D - o, lane);
                    vload(Yi, P.rel_t + rx * (int64_t)D + o, D - o, lane);
                    vload(Zr, P.ent + tx * (int64_t)D + o, D - o, lane);
                    vload(Zi, P.ent_t + tx * (int64_t)D + o, D - o, lane);
                    if (pass == 0) {
                        float d = 0.f;
#pragma unroll
                        for (int j = 0; j < Vec::N; ++j)
                            d += (Xr.x[j] * Yr.x[j] - Xi.x[j] * Yi.x[j]) * Zr.x[j] +
                                 (Xi.x[j] * Yr.x[j] + Xr.x[j] * Yi.x[j]) * Zi.x[j];
                        d = gsum<G>(d);
                        if (lane == 0) sc[c0 + i] = o == 0 ? d : sc[c0 + i] + d;
                        if (REG) rl += cx_sq(Xr, Xi) + cx_sq(Yr, Yi) + cx_sq(Zr, Zi);
                        continue;
                    }
                    const float ck = sc[c0 + i];
                    Vec gr, gi;
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        gr.x[j] = ck * (Yr.x[j] * Zr.x[j] + Yi.x[j] * Zi.x[j]);
                        gi.x[j] = ck * (Yr.x[j] * Zi.x[j] - Yi.x[j] * Zr.x[j]);
                        if (REG) {
                            gr.x[j] += Q.rho * Xr.x[j];
                            gi.x[j] += Q.rho * Xi.x[j];
                        }
                    }
                    sink.ent(hx, gr, gi, tb, D, o, lane);
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        gr.x[j] = ck * (Xr.x[j] * Zr.x[j] + Xi.x[j] * Zi.x[j]);
                        gi.x[j] = ck * (Xr.x[j] * Zi.x[j] - Xi.x[j] * Zr.x[j]);
                        if (REG) {
                            gr.x[j] += Q.rho * Yr.x[j];
                            gi.x[j] += Q.rho * Yi.x[j];
                        }
                    }
                    sink.rel(rx, gr, gi, tb, D, o, lane);
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        gr.x[j] = ck * (Xr.x[j] * Yr.x[j] - Xi.x[j] * Yi.x[j]);
                        gi.x[j] = ck * (Xi.x[j] * Yr.x[j] + Xr.x[j] * Yi.x[j]);
                        if (REG) {
                            gr.x[j] += Q.rho * Zr.x[j];
                            gi.x[j] += Q.rho * Zi.x[j];
                        }
                    }
                    sink.ent(tx, gr, gi, tb, D, o, lane);
                }
                if (pass == 1) {
#pragma unroll
                    for (int j = 0; j < Vec::N; ++j) {
                        aAr.x[j] += cAr.x[j];
                        aAi.x[j] += cAi.x[j];
                        aBr.x[j] += cBr.x[j];
                        aBi.x[j] += cBi.x[j];
                    }
                }
            }
            if (pass == 0) continue;
            // ---- the positive's own gradient (it joins A as c_p t) and the on-chip sums of this piece
            const float qh = REG ? Q.rho * (float)(1 + n0) : 0.f, qt = REG ? Q.rho * (float)(1 + n1) : 0.f,
                        qr = REG ? Q.rho * (float)(1 + n0 + n1) : 0.f;
            Vec gr, gi;
#pragma unroll
            for (int j = 0; j < Vec::N; ++j) {
                const float ar = aAr.x[j] + dldp * Tr.x[j], ai = aAi.x[j] + dldp * Ti.x[j];
                gr.x[j] = Hr.x[j] * ar + Hi.x[j] * ai + aBr.x[j] * Tr.x[j] + aBi.x[j] * Ti.x[j];
                gi.x[j] = Hr.x[j] * ai - Hi.x[j] * ar + aBr.x[j] * Ti.x[j] - aBi.x[j] * Tr.x[j];
                if (REG) {
                    gr.x[j] += qr * Rr.x[j];
                    gi.x[j] += qr * Ri.x[j];
                }
            }
            if (vnonzero(gr) || vnonzero(gi)) sink.rel(rp, gr, gi, tb, D, o, lane);
#pragma unroll
            for (int j = 0; j < Vec::N; ++j) {
                const float ar = aAr.x[j] + dldp * Tr.x[j], ai = aAi.x[j] + dldp * Ti.x[j];
                gr.x[j] = Rr.x[j] * ar + Ri.x[j] * ai;
                gi.x[j] = Rr.x[j] * ai - Ri.x[j] * ar;
                if (REG) {
                    gr.x[j] += qh * Hr.x[j];
                    gi.x[j] += qh * Hi.x[j];
                }
            }
            if (vnonzero(gr) || vnonzero(gi)) sink.ent(hp, gr, gi, tb, D, o, lane);
#pragma unroll
            for (int j = 0; j < Vec::N; ++j) {
                gr.x[j] = Rr.x[j] * aBr.x[j] - Ri.x[j] * aBi.x[j] + dldp * ur.x[j];
                gi.x[j] = Rr.x[j] * aBi.x[j] + Ri.x[j] * aBr.x[j] + dldp * ui.x[j];
                if (REG) {
                    gr.x[j] += qt * Tr.x[j];
                    gi.x[j] += qt * Ti.x[j];
                }
            }
            if (vnonzero(gr) || vnonzero(gi)) sink.ent(tp, gr, gi, tb, D, o, lane);
        }
        if (pass == 1) break;
        // ---- between the passes: weights, loss partial and dL/ds_k, lane-parallel over the group's scores
        __builtin_amdgcn_wave_barrier();   // LDS order inside a wave is program order
        float lp = loss_block<G>(L, P.margin, bs, neg, sc, lane, ps, 1.0f, &dldp);
        if (REG) {
            const float own = rl + (float)(1 + n0) * nh2 + (float)(1 + n1) * nt2 + (float)(1 + n0 + n1) * nr2;
            lp += gsum<G>(own) * (0.5f * Q.rho * Q.lscale);
        }
        if (lane == 0 && lpart) lpart[b] = lp;
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------- scoring ----------------------
// -s over n triples (mode 0 normal, 1 head_batch: h varies, t and r are read at index 0; 2 tail_batch: t varies), piece
// by piece
template <int G, int VEC>
__global__ __launch_bounds__(256) void k_score_complex(StepParams P, int mode, const int64_t *__restrict__ h,
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
        Vec Hr, Hi, Tr, Ti, Rr, Ri;
        vload(Hr, P.ent + hi_ * (int64_t)D + o, D - o, lane);
        vload(Hi, P.ent_t + hi_ * (int64_t)D + o, D - o, lane);
        vload(Tr, P.ent + ti_ * (int64_t)D + o, D - o, lane);
        vload(Ti, P.ent_t + ti_ * (int64_t)D + o, D - o, lane);
        vload(Rr, P.rel + ri_ * (int64_t)D + o, D - o, lane);
        vload(Ri, P.rel_t + ri_ * (int64_t)D + o, D - o, lane);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < Vec::N; ++k)
            d += (Hr.x[k] * Rr.x[k] - Hi.x[k] * Ri.x[k]) * Tr.x[k] + (Hi.x[k] * Rr.x[k] + Hr.x[k] * Ri.x[k]) * Ti.x[k];
        s += gsum<G>(d);
    }
    if (lane == 0) out[i] = -s;
}

// Candidate scores for link prediction (the layout and candidate orders of k_score_queries_distmult). A lane group
// keeps the base rows of QT queries in registers (whole rows, re and im: w = r conj(t) when the head varies, u = h r
// when the tail does) and ONE pass over an entity's two rows serves all of them as -(<base_re, e_re> + <base_im, e_im>)
template <int G, int VEC, int KCH, int QT>
__global__ __launch_bounds__(256) void k_score_queries_complex(StepParams P, int side,
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
    Vec bre[QT], bim[QT];
    int64_t truth[QT];
#pragma unroll
    for (int u = 0; u < QT; ++u) {
        const int64_t qi = q0 + u < nq ? q0 + u : q0;   // (a tile past the last query repeats its first; not stored)
        const int64_t h = qh[qi], t = qt[qi], r = qr[qi];
        truth[u] = side == 0 ? h : t;
        const int64_t a = side == 0 ? t : h;
        Vec ar, ai, Rr, Ri;
        vload(ar, P.ent + a * (int64_t)D, D, lane);
        vload(ai, P.ent_t + a * (int64_t)D, D, lane);
        vload(Rr, P.rel + r * (int64_t)D, D, lane);
        vload(Ri, P.rel_t + r * (int64_t)D, D, lane);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) {
            if (side == 0) {   // w = r conj(t)
                bre[u].x[k] = Rr.x[k] * ar.x[k] + Ri.x[k] * ai.x[k];
                bim[u].x[k] = Rr.x[k] * ai.x[k] - Ri.x[k] * ar.x[k];
            } else {           // u = h r
                bre[u].x[k] = ar.x[k] * Rr.x[k] - ai.x[k] * Ri.x[k];
                bim[u].x[k] = ai.x[k] * Rr.x[k] + ar.x[k] * Ri.x[k];
            }
        }
    }
    for (int64_t e = (int64_t)blockIdx.x * GPB + grp; e < E; e += (int64_t)gridDim.x * GPB) {
        Vec xr, xi;
        vload(xr, P.ent + e * (int64_t)D, D, lane);
        vload(xi, P.ent_t + e * (int64_t)D, D, lane);
#pragma unroll
        for (int u = 0; u < QT; ++u) {
            float d = 0.f;
#pragma unroll
            for (int k = 0; k < Vec::N; ++k) d += xr.x[k] * bre[u].x[k] + xi.x[k] * bim[u].x[k];
            const float s = gsum<G>(d);
            const int64_t j = global_order ? e : (e == truth[u] ? 0 : (e < truth[u] ? e + 1 : e));
            if (lane == 0 && q0 + u < nq) out[(q0 + u) * E + j] = -s;
        }
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
// a group's K scores and its transpose row sit in LDS: at most 64 KB of it (the launch default) for one group. The
// limit on neg is step_distmult_max_neg's at the same dim
static constexpr int64_t kCxLdsFloats = 64 * 1024 / 4;
int64_t step_complex_max_neg(int64_t dim) {
    const Shape s = pick_shape(dim);
    return kCxLdsFloats - (s.VEC == 4 ? (int64_t)s.G * s.VEC : 0);
}
// rows of negatives (re and im each) in flight per chunk: 2 with float4 pieces (232-243 VGPRs; 4 rows need 255-266
// and, with REG, a few AGPR copies), 4 with one-float pieces (171-177). No scratch either way; measured at the example's
// shape: DESIGN.md section 4
static constexpr int cx_nch(int vec) { return vec == 4 ? 2 : 4; }

hipError_t launch_step_complex(const StepParams &P, const LossParams &L, const RegulParams &Rg, const int64_t *bh,
                               const int64_t *bt, const int64_t *br, const StepWorkspace &W, hipStream_t st) {
    if (P.batch_size <= 0) return hipSuccess;
    if (P.model != 5 || P.neg < 1 || P.neg > step_complex_max_neg(P.dim) || L.kind != 1 || L.mflag || Rg.mode != 0 ||
        !(Rg.regul >= 0.f) || !P.ent_t || !P.rel_t || !W.gentt || !W.grelt || !W.fentt || !W.frelt)
        return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    // lane groups per block: 256 threads' worth, fewer when their score rows would not fit 64 KB of LDS (see
    // launch_step_adv: a group never straddles a wave and the kernel has no block-wide barrier)
    int64_t gpb = 256 / s.G;
    const int64_t rw = s.VEC == 4 ? (int64_t)s.G * s.VEC : 0;
    const int64_t cap = kCxLdsFloats / (P.neg + rw);   // >= 1: neg <= step_complex_max_neg
    if (gpb > cap) gpb = cap;
    dev::CxSink sink{W.gent, W.grel, W.gentt, W.grelt, W.fent, W.frel, W.fentt, W.frelt};
    dev::CxRegul Q{};
    const bool reg = Rg.regul != 0.f;
    if (reg) {
        // rho per slot (N = B (1 + K) slots), formed in double
        const double N = (double)P.batch_size * (double)(1 + P.neg), D = (double)P.dim;
        Q.rho = (float)(2.0 * (double)Rg.regul / (6.0 * N * D));
        float scale, cst;
        loss_affine(L, P, &scale, &cst);
        Q.lscale = 1.0f / scale;
    }
    const dim3 grid((unsigned)((P.batch_size + gpb - 1) / gpb)), block((unsigned)(gpb * s.G));
    const size_t lds = sizeof(float) * (size_t)(gpb * (P.neg + rw));
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        constexpr int NCH = cx_nch(T::VEC);
        if (reg)
            hipLaunchKernelGGL((dev::k_step_complex<T::G, T::VEC, NCH, true>), grid, block, lds, st, P, L, Q, bh, bt, br,
                               sink, W.lpart);
        else
            hipLaunchKernelGGL((dev::k_step_complex<T::G, T::VEC, NCH, false>), grid, block, lds, st, P, L, Q, bh, bt, br,
                               sink, W.lpart);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_complex(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                                int64_t n, float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!P.ent_t || !P.rel_t) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_complex<T::G, T::VEC>), grid, block, 0, st, P, mode, h, t, r, n, out);
        e = hipGetLastError();
    });
    return e;
}

// queries per lane group of k_score_queries_complex: two base rows per query, so 4 where a lane holds up to 8 floats of
// a row and 2 beyond (float4 rows at KCH 3 and 4; register counts and timings: DESIGN.md section 4)
static constexpr int cx_qt(int vec, int kch) { return vec * kch <= 8 ? 4 : 2; }
int complex_queries_per_group(int64_t dim) {
    const Shape s = pick_shape(dim);
    return cx_qt(s.VEC, s.KCH);
}

hipError_t launch_score_queries_complex(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                        const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                        int global_order) {
    if (nq <= 0) return hipSuccess;
    if (!P.ent_t || !P.rel_t) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    int64_t bx = (E + gpb - 1) / gpb;
    if (bx > 128) bx = 128;
    const int64_t qt_ = complex_queries_per_group(P.dim);
    const dim3 grid((unsigned)bx, (unsigned)((nq + qt_ - 1) / qt_)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        constexpr int QT = cx_qt(T::VEC, T::KCH);
        hipLaunchKernelGGL((dev::k_score_queries_complex<T::G, T::VEC, T::KCH, QT>), grid, block, 0, st, P, side, qh, qt,
                           qr, nq, E, out, global_order);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

// HIP kernels of RotatE for gfx950: the external-batch training step under SigmoidLoss / MarginLoss with or without
// the self-adversarial weights, and the distances behind pt_score / pt_score_queries / pt_score_rows.
//
// Semantics (RotatE.py:45-91): an entity row is 2 * dim floats, re[0:dim] | im[dim:2 dim]; a relation row is dim
// phases; phi = r / q with q = rel_embedding_range / pi (StepParams::phase_div), c = cos(phi), s = sin(phi);
//   v = h o (c + i s) - t   (head_batch: conj(c + i s) o t - h),   d = sum_j sqrt(v_re[j]^2 + v_im[j]^2);
// the score handed to the loss is gamma - d (the model always carries its margin); losses and weights as in
// step_adv.hip (SigmoidLoss.py:19-26, MarginLoss.py:24-31, weights detached, maximum tie -> half). Backward with
// g = dL/dv (complex; 0 where the modulus is 0, as torch's norm backward) and u = h o (c + i s):
//   dL/dh = g o conj(c + i s),   dL/dt = -g,   dL/dr = (g_im u_re - g_re u_im) / q.
// No row is normalised: every gradient leaves the kernel finished, the optimizer passes apply no Jacobian.
//
// Mapping of k_step_rotate (k_step_adv's): ONE lane group owns a positive and its K negatives and walks them twice.
// Pass 1 puts d_k into LDS; the group then forms the weights, the loss partial and dL/dd_k lane-parallel over those
// K floats; pass 2 re-forms v_k and emits gradients. Everything but d is element-wise in the dims (the modulus is
// per complex element), so BOTH passes run over the row in PIECES of G * VEC floats (one 16-B or 4-B chunk per lane
// and half row): per piece the positive's (c, s, u, t) and five accumulators are 4 (VEC = 4) or 1 float per lane
// each, whatever the dim - at dim 1,024 whole rows would need 11 x 16 floats per lane before any row in flight.
// Pass 1 adds a piece's partial distance into the group's LDS score. Per piece the sampler's structure stays on
// chip: negatives that keep the positive's (h, r) share u - their g_k are summed and rotated back once; negatives
// that keep (r, t) accumulate -sum g_k and the phase gradient; only the corrupted entity's half rows go through
// row_atomic plus their flags; a negative with another relation takes the three-row path. Gradient rows and flags
// of the entity table are half rows: [2 * ent_total][dim] (rotate_half_rows, kernels.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

template <int G>
__device__ __forceinline__ float rot_gmax(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// overflow-safe log(sigmoid(x)) and sigmoid(x)
__device__ __forceinline__ float rot_logsig(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float rot_sigm(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

// c + i s of a piece of phases (full-precision sinf / cosf; a padding lane holds phase 0: c = 1, s = 0)
template <typename Vec>
__device__ __forceinline__ void rot_unit(const Vec &R, float q, Vec &c, Vec &s) {
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        sincosf(R.x[i] / q, &s.x[i], &c.x[i]);
    }
}
// u = e o (c + i s)
template <typename Vec>
__device__ __forceinline__ void rot_fwd(const Vec &er, const Vec &ei, const Vec &c, const Vec &s, Vec &ur, Vec &ui) {
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        ur.x[i] = er.x[i] * c.x[i] - ei.x[i] * s.x[i];
        ui.x[i] = er.x[i] * s.x[i] + ei.x[i] * c.x[i];
    }
}
// w = conj(c + i s) o e
template <typename Vec>
__device__ __forceinline__ void rot_conj(const Vec &er, const Vec &ei, const Vec &c, const Vec &s, Vec &wr, Vec &wi) {
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        wr.x[i] = c.x[i] * er.x[i] + s.x[i] * ei.x[i];
        wi.x[i] = c.x[i] * ei.x[i] - s.x[i] * er.x[i];
    }
}
// this lane's part of sum_j |v_j|
template <typename Vec>
__device__ __forceinline__ float rot_modsum(const Vec &vr, const Vec &vi) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) d += sqrtf(vr.x[i] * vr.x[i] + vi.x[i] * vi.x[i]);
    return d;
}
// g = cd * v / |v| per complex element, 0 where |v| = 0
template <typename Vec>
__device__ __forceinline__ void rot_modbwd(const Vec &vr, const Vec &vi, float cd, Vec &gr, Vec &gi) {
#pragma unroll
    for (int i = 0; i < Vec::N; ++i) {
        const float m = sqrtf(vr.x[i] * vr.x[i] + vi.x[i] * vi.x[i]);
        const float k = m == 0.f ? 0.f : cd / m;
        gr.x[i] = vr.x[i] * k;
        gi.x[i] = vi.x[i] * k;
    }
}

// the piece [o, o + G * VEC) of both halves of entity row e (Dp = dim - o floats of it exist)
template <typename Vec>
__device__ __forceinline__ void rot_load_ent(Vec &er, Vec &ei, const float *ent, int64_t e, int D, int o, int lane) {
    const float *row = ent + e * (2 * (int64_t)D) + o;
    vload(er, row, D - o, lane);
    vload(ei, row + D, D - o, lane);
}

struct RotateSink {   // (row_atomic: device.h)
    float *gent, *grel;
    int *fent, *frel;
    template <typename Vec>
    __device__ __forceinline__ void ent(int64_t e, const Vec &gr, const Vec &gi, float *tb, int D, int o,
                                        int lane) const {
        float *row = gent + e * (2 * (int64_t)D) + o;
        row_atomic(gr, row, tb, D - o, lane);
        row_atomic(gi, row + D, tb, D - o, lane);
        if (lane == 0) {
            fent[2 * e] = 1;
            fent[2 * e + 1] = 1;
        }
    }
    template <typename Vec>
    __device__ __forceinline__ void rel(int64_t r, const Vec &g, float *tb, int D, int o, int lane) const {
        row_atomic(g, grel + r * D + o, tb, D - o, lane);
        if (lane == 0) frel[r] = 1;
    }
};

template <int G, int VEC, int NCH>
__global__ __launch_bounds__(256) void k_step_rotate(StepParams P, LossParams L, const int64_t *__restrict__ bh,
                                                     const int64_t *__restrict__ bt, const int64_t *__restrict__ br,
                                                     RotateSink sink, float *__restrict__ lpart) {
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
    const float q = P.phase_div;
    const int64_t hp = bh[b], tp = bt[b], rp = br[b];
    float dp = 0.f;     // the positive's distance (pass 1), then dL/dd of it (pass 2)
    float dldp = 0.f;

    for (int pass = 0; pass < 2; ++pass) {
        for (int o = 0; o < D; o += PW) {
            // ---- the positive's piece: c, s, u = h o (c + i s), t
            Vec c, s, ur, ui, tr, ti;
            {
                Vec hr, hi, R;
                rot_load_ent(hr, hi, P.ent, hp, D, o, lane);
                rot_load_ent(tr, ti, P.ent, tp, D, o, lane);
                vload(R, P.rel + rp * D + o, D - o, lane);
                rot_unit(R, q, c, s);
                rot_fwd(hr, hi, c, s, ur, ui);
            }
            Vec pr, pi;   // the positive's v
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) {
                pr.x[i] = ur.x[i] - tr.x[i];
                pi.x[i] = ui.x[i] - ti.x[i];
            }
            if (pass == 0) dp += gsum<G>(rot_modsum(pr, pi));
            // on-chip sums of this piece: aG = sum of g_k over the negatives that keep (h, r), plus the positive's;
            // aT = -sum of g_k over those that keep (r, t), minus the positive's; aR = their phase gradients (x q).
            // Each chunk sums into accumulators of its own first (as k_step_adv: shorter float32 chains)
            Vec aGr, aGi, aTr, aTi, aR;
            vzero(aGr); vzero(aGi); vzero(aTr); vzero(aTi); vzero(aR);
            for (int c0 = 0; c0 < neg; c0 += NCH) {
                int64_t hk[NCH], tk[NCH], rk[NCH];
                int kind[NCH];   // 0: keeps (h, r): row t_k; 1: keeps (r, t): row h_k; -1: nothing (here)
                unsigned other = 0;   // bit u: slot u is any other negative: the three-row path below
                Vec Er[NCH], Ei[NCH], cGr, cGi, cTr, cTi, cR;
                vzero(cGr); vzero(cGi); vzero(cTr); vzero(cTi); vzero(cR);
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    kind[u] = -1;
                    if (c0 + u >= neg) continue;
                    if (pass == 1 && sc[c0 + u] == 0.f) continue;   // no gradient through this negative
                    const int64_t x = (int64_t)(c0 + u + 1) * bs + b;
                    hk[u] = bh[x]; tk[u] = bt[x]; rk[u] = br[x];
                    kind[u] = rk[u] != rp ? -1 : (hk[u] == hp ? 0 : (tk[u] == tp ? 1 : -1));
                    if (kind[u] < 0) other |= 1u << u;
                    else rot_load_ent(Er[u], Ei[u], P.ent, kind[u] == 0 ? tk[u] : hk[u], D, o, lane);
                }
#pragma unroll
                for (int u = 0; u < NCH; ++u) {
                    if (kind[u] < 0) continue;
                    Vec vr, vi, kr, ki;   // v_k; u_k of a kind-1 slot
                    if (kind[u] == 0) {
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) {
                            vr.x[i] = ur.x[i] - Er[u].x[i];
                            vi.x[i] = ui.x[i] - Ei[u].x[i];
                        }
                    } else {
                        rot_fwd(Er[u], Ei[u], c, s, kr, ki);
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) {
                            vr.x[i] = kr.x[i] - tr.x[i];
                            vi.x[i] = ki.x[i] - ti.x[i];
                        }
                    }
                    if (pass == 0) {
                        const float d = gsum<G>(rot_modsum(vr, vi));
                        if (lane == 0) sc[c0 + u] = o == 0 ? d : sc[c0 + u] + d;
                        continue;
                    }
                    Vec gr, gi;   // dL/dv_k
                    rot_modbwd(vr, vi, sc[c0 + u], gr, gi);
                    if (kind[u] == 0) {
                        Vec nr, ni;
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) {
                            cGr.x[i] += gr.x[i];
                            cGi.x[i] += gi.x[i];
                            nr.x[i] = -gr.x[i];
                            ni.x[i] = -gi.x[i];
                        }
                        sink.ent(tk[u], nr, ni, tb, D, o, lane);
                    } else {
                        Vec dr, di;
                        rot_conj(gr, gi, c, s, dr, di);   // dL/dh_k = g o conj(c + i s)
#pragma unroll
                        for (int i = 0; i < Vec::N; ++i) {
                            cTr.x[i] -= gr.x[i];
                            cTi.x[i] -= gi.x[i];
                            cR.x[i] += gi.x[i] * kr.x[i] - gr.x[i] * ki.x[i];
                        }
                        sink.ent(hk[u], dr, di, tb, D, o, lane);
                    }
                }
                // any other slot (another relation, or both entities replaced): its own three rows and rotation;
                // one copy of the code, a slot at a time (the samplers draw such slots only as relation corruptions)
#pragma unroll 1
                for (int u = 0; u < NCH; ++u) {
                    if (!((other >> u) & 1u)) continue;
                    const int64_t x = (int64_t)(c0 + u + 1) * bs + b;
                    const int64_t hx = bh[x], tx = bt[x], rx = br[x];
                    Vec xr, xi, yr, yi, R, ck, sk, ar, ai, vr, vi;
                    rot_load_ent(xr, xi, P.ent, hx, D, o, lane);
                    rot_load_ent(yr, yi, P.ent, tx, D, o, lane);
                    vload(R, P.rel + rx * D + o, D - o, lane);
                    rot_unit(R, q, ck, sk);
                    rot_fwd(xr, xi, ck, sk, ar, ai);
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) {
                        vr.x[i] = ar.x[i] - yr.x[i];
                        vi.x[i] = ai.x[i] - yi.x[i];
                    }
                    if (pass == 0) {
                        const float d = gsum<G>(rot_modsum(vr, vi));
                        if (lane == 0) sc[c0 + u] = o == 0 ? d : sc[c0 + u] + d;
                        continue;
                    }
                    Vec gr, gi, dr, di, nr, ni, gp;
                    rot_modbwd(vr, vi, sc[c0 + u], gr, gi);
                    rot_conj(gr, gi, ck, sk, dr, di);
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) {
                        nr.x[i] = -gr.x[i];
                        ni.x[i] = -gi.x[i];
                        gp.x[i] = (gi.x[i] * ar.x[i] - gr.x[i] * ai.x[i]) / q;
                    }
                    sink.ent(hx, dr, di, tb, D, o, lane);
                    sink.ent(tx, nr, ni, tb, D, o, lane);
                    sink.rel(rx, gp, tb, D, o, lane);
                }
                if (pass == 1) {
#pragma unroll
                    for (int i = 0; i < Vec::N; ++i) {
                        aGr.x[i] += cGr.x[i];
                        aGi.x[i] += cGi.x[i];
                        aTr.x[i] += cTr.x[i];
                        aTi.x[i] += cTi.x[i];
                        aR.x[i] += cR.x[i];
                    }
                }
            }
            if (pass == 0) continue;
            // ---- the positive's own gradient and the on-chip sums of this piece
            if (dldp != 0.f) {
                Vec gr, gi;
                rot_modbwd(pr, pi, -dldp, gr, gi);   // d(score) / dd = -1
#pragma unroll
                for (int i = 0; i < Vec::N; ++i) {
                    aGr.x[i] += gr.x[i];
                    aGi.x[i] += gi.x[i];
                    aTr.x[i] -= gr.x[i];
                    aTi.x[i] -= gi.x[i];
                }
            }
            Vec dr, di, gp;
            rot_conj(aGr, aGi, c, s, dr, di);   // dL/dh = (sum g) o conj(c + i s)
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) gp.x[i] = ((aGi.x[i] * ur.x[i] - aGr.x[i] * ui.x[i]) + aR.x[i]) / q;
            if (vnonzero(gp)) sink.rel(rp, gp, tb, D, o, lane);
            if (vnonzero(dr) || vnonzero(di)) sink.ent(hp, dr, di, tb, D, o, lane);
            if (vnonzero(aTr) || vnonzero(aTi)) sink.ent(tp, aTr, aTi, tb, D, o, lane);
        }
        if (pass == 1) break;
        // ---- between the passes: weights, loss partial and dL/dd_k, lane-parallel over the group's scores
        __builtin_amdgcn_wave_barrier();   // LDS order inside a wave is program order
        const float invB = 1.0f / (float)bs;
        const float ps = L.gamma - dp;
        float zt = 0.f, ext = 0.f, winv = 1.0f / (float)neg;
        if (L.adv) {
            zt = L.kind == 1 ? L.temp : -L.temp;
            float mx = -INFINITY;
            for (int k = lane; k < neg; k += G) {
                const float n = L.gamma - sc[k];
                mx = fmaxf(mx, zt > 0.f ? n : -n);
            }
            mx = rot_gmax<G>(mx);
            ext = zt > 0.f ? mx : -mx;   // the score of the largest weight: every exponent below is <= 0
            float se = 0.f;
            for (int k = lane; k < neg; k += G) se += expf(zt * ((L.gamma - sc[k]) - ext));
            winv = 1.0f / gsum<G>(se);
        }
        float lp = 0.f, cs = 0.f;
        for (int k = lane; k < neg; k += G) {
            const float n = L.gamma - sc[k];
            const float w = L.adv ? expf(zt * (n - ext)) * winv : winv;
            float cn;   // dL / dn_k
            if (L.kind == 1) {
                lp += w * rot_logsig(-n);
                cn = w * rot_sigm(n) * (0.5f * invB);
            } else {
                const float a = ps - n, m = P.margin;
                lp += w * (a > -m ? a : -m);
                const float hc = a > -m ? 1.0f : (a == -m ? 0.5f : 0.f);
                cs += w * hc;
                cn = -(w * hc) * invB;
            }
            sc[k] = -cn;   // dL / dd_k
        }
        lp = gsum<G>(lp);
        if (L.kind == 1) {
            lp += rot_logsig(ps);
            dldp = -rot_sigm(-ps) * (0.5f * invB);
        } else {
            dldp = gsum<G>(cs) * invB;
        }
        if (lane == 0 && lpart) lpart[b] = lp;
        __builtin_amdgcn_wave_barrier();
    }
}

// ---------------------------------------------------------------- scoring ----------------------
// the distance d over n triples (mode 0 normal, 1 head_batch: h varies, 2 tail_batch: t varies), piece by piece
template <int G, int VEC>
__global__ __launch_bounds__(256) void k_score_rotate(StepParams P, int mode, const int64_t *__restrict__ h,
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
    float d = 0.f;
    for (int o = 0; o < D; o += PW) {
        Vec hr, hi, tr, ti, R, c, s, wr, wi, vr, vi;
        rot_load_ent(hr, hi, P.ent, hi_, D, o, lane);
        rot_load_ent(tr, ti, P.ent, ti_, D, o, lane);
        vload(R, P.rel + ri_ * D + o, D - o, lane);
        rot_unit(R, P.phase_div, c, s);
        if (mode == 1) {
            rot_conj(tr, ti, c, s, wr, wi);
#pragma unroll
            for (int k = 0; k < Vec::N; ++k) {
                vr.x[k] = wr.x[k] - hr.x[k];
                vi.x[k] = wi.x[k] - hi.x[k];
            }
        } else {
            rot_fwd(hr, hi, c, s, wr, wi);
#pragma unroll
            for (int k = 0; k < Vec::N; ++k) {
                vr.x[k] = wr.x[k] - tr.x[k];
                vi.x[k] = wi.x[k] - ti.x[k];
            }
        }
        d += gsum<G>(rot_modsum(vr, vi));
    }
    if (lane == 0) out[i] = d;
}

// Candidate distances for link prediction (the layout and candidate orders of k_score_queries): per query the base
// row - h o r for tail prediction, conj(r) o t for head prediction - is formed once and kept in registers (two whole
// half rows); the entity table then streams past it as |base - e|
template <int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_score_queries_rotate(StepParams P, int side, const int64_t *__restrict__ qh,
                                                              const int64_t *__restrict__ qt,
                                                              const int64_t *__restrict__ qr, int64_t nq, int64_t E,
                                                              float *__restrict__ out, int global_order) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t qi = blockIdx.y;
    if (qi >= nq) return;
    const int D = (int)P.dim;
    const int64_t D2 = 2 * (int64_t)D;
    const int64_t h = qh[qi], t = qt[qi], r = qr[qi];
    const int64_t truth = side == 0 ? h : t;
    const int64_t anchor = side == 0 ? t : h;
    Vec br_, bi_;
    {
        Vec ar, ai, R, c, s;
        vload(ar, P.ent + anchor * D2, D, lane);
        vload(ai, P.ent + anchor * D2 + D, D, lane);
        vload(R, P.rel + r * D, D, lane);
        rot_unit(R, P.phase_div, c, s);
        if (side == 0) rot_conj(ar, ai, c, s, br_, bi_); else rot_fwd(ar, ai, c, s, br_, bi_);
    }
    float *row = out + qi * E;
    for (int64_t j = (int64_t)blockIdx.x * GPB + grp; j < E; j += (int64_t)gridDim.x * GPB) {
        const int64_t e = global_order ? j : (j == 0 ? truth : (j - 1 < truth ? j - 1 : j));
        Vec xr, xi, vr, vi;
        vload(xr, P.ent + e * D2, D, lane);
        vload(xi, P.ent + e * D2 + D, D, lane);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) {
            vr.x[k] = br_.x[k] - xr.x[k];
            vi.x[k] = bi_.x[k] - xi.x[k];
        }
        const float d = gsum<G>(rot_modsum(vr, vi));
        if (lane == 0) row[j] = d;
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
// a group's K scores and its transpose row sit in LDS: at most 64 KB of it (the launch default) for one group. The
// limit on neg is step_adv_max_neg's at the same dim (a whole row's transpose space set aside), so a configuration
// that trains TransE under a weighted loss trains RotatE too; the kernel itself needs one piece of it
static constexpr int64_t kRotLdsFloats = 64 * 1024 / 4;
int64_t step_rotate_max_neg(int64_t dim) {
    const Shape s = pick_shape(dim);
    return kRotLdsFloats - (s.VEC == 4 ? (int64_t)s.KCH * s.G * s.VEC : 0);
}
// rows of negatives in flight per chunk (NCH): 4 with one-float pieces (156 VGPRs: three waves per SIMD), 2 with
// float4 pieces (237 VGPRs: two waves per SIMD; 4 in flight take 263, one wave). Read from the code object's
// metadata; no shape uses scratch
constexpr int rot_nch(int vec) { return vec == 4 ? 2 : 4; }

hipError_t launch_step_rotate(const StepParams &P, const LossParams &L, const int64_t *bh, const int64_t *bt,
                              const int64_t *br, const StepWorkspace &W, hipStream_t st) {
    if (P.batch_size <= 0) return hipSuccess;
    if (P.model != 3 || P.neg < 1 || P.neg > step_rotate_max_neg(P.dim) || !(P.phase_div > 0.f) || !L.mflag)
        return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    // lane groups per block: 256 threads' worth, fewer when their score rows would not fit 64 KB of LDS (see
    // launch_step_adv: a group never straddles a wave and the kernel has no block-wide barrier)
    int64_t gpb = 256 / s.G;
    const int64_t rw = s.VEC == 4 ? (int64_t)s.G * s.VEC : 0;
    const int64_t cap = kRotLdsFloats / (P.neg + rw);   // >= 1: neg <= step_rotate_max_neg
    if (gpb > cap) gpb = cap;
    dev::RotateSink sink{W.gent, W.grel, W.fent, W.frel};
    const dim3 grid((unsigned)((P.batch_size + gpb - 1) / gpb)), block((unsigned)(gpb * s.G));
    const size_t lds = sizeof(float) * (size_t)(gpb * (P.neg + rw));
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_step_rotate<T::G, T::VEC, rot_nch(T::VEC)>), grid, block, lds, st, P, L, bh, bt, br, sink,
                           W.lpart);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_rotate(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                               int64_t n, float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!(P.phase_div > 0.f)) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_rotate<T::G, T::VEC>), grid, block, 0, st, P, mode, h, t, r, n, out);
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_score_queries_rotate(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                       const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                       int global_order) {
    if (nq <= 0) return hipSuccess;
    if (!(P.phase_div > 0.f)) return hipErrorInvalidValue;
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    int64_t bx = (E + gpb - 1) / gpb;
    if (bx > 128) bx = 128;
    const dim3 grid((unsigned)bx, (unsigned)nq), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        hipLaunchKernelGGL((dev::k_score_queries_rotate<T::G, T::VEC, T::KCH>), grid, block, 0, st, P, side, qh, qt,
                           qr, nq, E, out, global_order);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

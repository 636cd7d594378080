// HIP kernels of TransE / TransH scoring for gfx950 (MI355X), and the dim rule of the single-model path. (The batch
// samplers are sample.hip, universe link prediction is lp.hip.)
//
// Layout and mapping
//  * Rows are held by lane groups (struct Shape, kernels.h).
//  * This is gather work (no dense contraction): the roofline is HBM / Infinity-Cache bandwidth, not MFMA.
//
// Semantics (cited in DESIGN.md): forward = TransE.py:46-74 / TransH.py:52-93.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

// ---------------------------------------------------------------- scoring ----------------------
// model.predict over n triples (mode 0 normal, 1 head_batch: h varies, 2 tail_batch: t varies)
template <int MODEL, int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_score(StepParams P, int mode, const int64_t *__restrict__ h,
                                               const int64_t *__restrict__ t, const int64_t *__restrict__ r,
                                               int64_t n, float *__restrict__ out) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (i >= n) return;
    const int D = (int)P.dim;
    const int64_t hi = h[mode == 1 || mode == 0 ? i : 0];
    const int64_t ti = t[mode == 2 || mode == 0 ? i : 0];
    const int64_t ri = r[mode == 0 ? i : 0];
    Vec H, T, R, hh, th, rh, v;
    vload(H, P.ent + hi * D, D, lane);
    vload(T, P.ent + ti * D, D, lane);
    vload(R, P.rel + ri * D, D, lane);
    if constexpr (MODEL == 1) {
        Vec W, nW;
        vload(W, P.normv + ri * D, D, lane);
        vnormalize(W, nW);
        const float hd = vdot(H, nW), td = vdot(T, nW);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) {
            H.x[k] = H.x[k] - hd * nW.x[k];
            T.x[k] = T.x[k] - td * nW.x[k];
        }
    }
    if (P.norm_flag) {
        vnormalize(H, hh);
        vnormalize(R, rh);
        vnormalize(T, th);
    } else {
        hh = H; rh = R; th = T;
    }
#pragma unroll
    for (int k = 0; k < Vec::N; ++k)
        v.x[k] = mode == 1 ? hh.x[k] + (rh.x[k] - th.x[k]) : (hh.x[k] + rh.x[k]) - th.x[k];
    const float s = vpnorm(v, P.p_norm);
    if (lane == 0) out[i] = s;
}

// Candidate scoring for link prediction: row q holds the scores of query q's candidate list in the
// order getHeadBatch/getTailBatch emit it ([truth, 0..E-1 without truth], Test.h:37-107), with the
// association of model.predict for that mode (head_batch: h + (r - t); tail_batch: (h + r) - t).
template <int MODEL, int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_score_queries(StepParams P, int side, const int64_t *__restrict__ qh,
                                                       const int64_t *__restrict__ qt, const int64_t *__restrict__ qr,
                                                       int64_t nq, int64_t E, float *__restrict__ out, int global_order) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int grp = threadIdx.x / G;
    const int64_t q = blockIdx.y;
    if (q >= nq) return;
    const int D = (int)P.dim;
    const int64_t h = qh[q], t = qt[q], r = qr[q];
    const int64_t truth = side == 0 ? h : t;
    const int64_t anchor = side == 0 ? t : h;
    Vec A, R, ah, rh, nW, base;
    vload(A, P.ent + anchor * D, D, lane);
    vload(R, P.rel + r * D, D, lane);
    if constexpr (MODEL == 1) {
        Vec W;
        vload(W, P.normv + r * D, D, lane);
        vnormalize(W, nW);
        const float ad = vdot(A, nW);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) A.x[k] = A.x[k] - ad * nW.x[k];
    }
    if (P.norm_flag) {
        vnormalize(A, ah);
        vnormalize(R, rh);
    } else {
        ah = A; rh = R;
    }
#pragma unroll
    for (int k = 0; k < Vec::N; ++k) base.x[k] = side == 0 ? rh.x[k] - ah.x[k] : ah.x[k] + rh.x[k];
    float *row = out + q * E;
    for (int64_t j = (int64_t)blockIdx.x * GPB + grp; j < E; j += (int64_t)gridDim.x * GPB) {
        // candidate order of getHeadBatch/getTailBatch ([truth, 0..E-1 without truth], Test.h:37-107),
        // or column = entity id (global_order, the layout pt_rank_rows ranks)
        const int64_t e = global_order ? j : (j == 0 ? truth : (j - 1 < truth ? j - 1 : j));
        Vec X, xh, v;
        vload(X, P.ent + e * D, D, lane);
        if constexpr (MODEL == 1) {
            const float xd = vdot(X, nW);
#pragma unroll
            for (int k = 0; k < Vec::N; ++k) X.x[k] = X.x[k] - xd * nW.x[k];
        }
        if (P.norm_flag) vnormalize(X, xh); else xh = X;
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) v.x[k] = side == 0 ? xh.x[k] + base.x[k] : base.x[k] - xh.x[k];
        const float s = vpnorm(v, P.p_norm);
        if (lane == 0) row[j] = s;
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
constexpr bool shape_listed(const Shape &s) { return for_shape(s, [](auto) {}); }
// dims 1..512 have their instances under both layouts; dims 516..1,024 in multiples of 4 under the float4 layout only
constexpr bool narrow_dispatches(int64_t dim) {
    return dim >= 1 && dim <= 512 && shape_listed(pick_shape(dim)) && shape_listed(pick_shape(dim, false));
}
constexpr bool wide_dispatches(int64_t dim) {
    return dim > 512 && dim <= 1024 && dim % 4 == 0 && shape_listed(pick_shape(dim));
}
constexpr bool dim_dispatches(int64_t dim, int model) {
    return narrow_dispatches(dim) || (model != 2 && model >= 0 && model <= 5 && wide_dispatches(dim));
}
constexpr bool dim_rule_holds() {
    for (int64_t dim = 1; dim <= 512; ++dim)
        for (int model = 0; model < 6; ++model)
            if (!dim_dispatches(dim, model)) return false;
    for (int64_t dim = 513; dim <= 1100; ++dim)
        for (int model = 0; model < 6; ++model)
            if (dim_dispatches(dim, model) != (model != 2 && dim <= 1024 && dim % 4 == 0)) return false;
    return !dim_dispatches(0, 0) && !dim_dispatches(513, 0) && !dim_dispatches(514, 0) && !dim_dispatches(1028, 0) &&
           !dim_dispatches(516, 2) && dim_dispatches(1024, 3) && !dim_dispatches(1028, 3) &&
           dim_dispatches(1024, 4) && !dim_dispatches(1028, 4) && dim_dispatches(1024, 5) &&
           !dim_dispatches(1028, 5);
}
static_assert(dim_rule_holds(),
              "PT_SHAPES must cover dims 1..512 under both layouts and dims 516..1024 (multiples of 4) as float4 rows "
              "for TransE / TransH / RotatE / DistMult / ComplEx; 513, 514, 1028 and TransD above 512 must not dispatch");

bool model_dim_supported(int64_t dim, int model) { return model >= 0 && model <= 5 && dim_dispatches(dim, model); }
bool narrow_dim_supported(int64_t dim) { return narrow_dispatches(dim); }

hipError_t launch_score(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r, int64_t n,
                        float *out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (P.model == 2) return launch_score_transd(P, mode, h, t, r, n, out, st);
    if (P.model == 3) return launch_score_rotate(P, mode, h, t, r, n, out, st);
    if (P.model == 4) return launch_score_distmult(P, mode, h, t, r, n, out, st);
    if (P.model == 5) return launch_score_complex(P, mode, h, t, r, n, out, st);
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        for_value<0, 1>(P.model != 0, [&](auto m) {
            using T = decltype(sh);
            hipLaunchKernelGGL((dev::k_score<m.value, T::G, T::VEC, T::KCH>), grid, block, 0, st, P, mode, h, t, r, n,
                               out);
            e = hipGetLastError();
        });
    });
    return e;
}

hipError_t launch_score_queries(const StepParams &P, int side, const int64_t *qh, const int64_t *qt, const int64_t *qr,
                                int64_t nq, int64_t E, float *out, hipStream_t st, int global_order) {
    if (nq <= 0) return hipSuccess;
    if (P.model == 2) return launch_score_queries_transd(P, side, qh, qt, qr, nq, E, out, st, global_order);
    if (P.model == 3) return launch_score_queries_rotate(P, side, qh, qt, qr, nq, E, out, st, global_order);
    if (P.model == 4) return launch_score_queries_distmult(P, side, qh, qt, qr, nq, E, out, st, global_order);
    if (P.model == 5) return launch_score_queries_complex(P, side, qh, qt, qr, nq, E, out, st, global_order);
    const Shape s = pick_shape(P.dim);
    const int64_t gpb = 256 / s.G;
    int64_t bx = (E + gpb - 1) / gpb;
    if (bx > 128) bx = 128;
    const dim3 grid((unsigned)bx, (unsigned)nq), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        for_value<0, 1>(P.model != 0, [&](auto m) {
            using T = decltype(sh);
            hipLaunchKernelGGL((dev::k_score_queries<m.value, T::G, T::VEC, T::KCH>), grid, block, 0, st, P, side, qh,
                               qt, qr, nq, E, out, global_order);
            e = hipGetLastError();
        });
    });
    return e;
}

}  // namespace pt

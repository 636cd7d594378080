// HIP kernel of the dense Adam apply pass for gfx950: the counterpart of k_apply (apply.hip) for torch.optim.Adam
// as Trainer.py:77-82 builds it (betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad).
//
// Adam is dense: every row of every table moves on every step (a row with a zero gradient still decays m and v and
// moves while its m is nonzero), so one lane group (device.h row layout) owns one row of one table:
//   flagged row:   load its gradient row, multiply by the normalise Jacobian of the pre-step row where the table's
//                  gradient is in normalised space, re-zero the gradient row and the flag;
//   unflagged row: g = 0 without reading the gradient row;
//   every row:     m' = m + (1 - b1)(g - m);  v' = b2 v + (1 - b2) g^2;
//                  w' = w - step_size * m' / (sqrt(v') / bc2_sqrt + eps)
// with step_size = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) computed on the host in double, and IEEE sqrt and
// division (the denominator is the ill-conditioned part). Block 0 reduces the step's loss partials in a fixed order.
// Floor: w, m, v read and written = 6 row-array passes over all tables (+ the touched gradient rows).
//
// L3 regulariser (template flag L3; DistMult.py:67-68, NegativeSampling.py:30-31: l3 * (||ent||_3^3 + ||rel||_3^3)):
// its gradient 3 l3 x |x| is dense, like this pass, so it joins g on the pre-step row, flagged or not, with no
// further pass over HBM. The loss needs sum |x|^3 over the whole tables: every block writes the sum over its rows to
// l3part[block] (groups in a fixed order through LDS) and k_l3_loss, one block, adds l3 * sum(l3part) to the step's
// loss in a fixed order (one same-address float atomic per block would serialise at the memory side: kernels.h on
// lpart). With the flag off the kernel is the code it was before the flag existed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

struct AdamTable {
    float *w, *m, *v, *grad;
    int *flag;
    int64_t rows;
    int jacobian;
};
struct AdamApply {
    AdamTable t[3];
    int ntab;
    int64_t dim;
    float beta2, omb1, omb2, eps, step_size, bc2_sqrt;   // omb = 1 - beta, formed on the host in double
    // loss (block 0): loss (+)= scale * sum(lpart[0 .. bs)) + cst
    float *loss;
    const float *lpart;
    int64_t bs;
    float scale, cst;
    int loss_assign;
    // L3 instantiation only (appended: the fields above keep their places in the argument block)
    float l3c;       // 3 * l3_regul_rate
    float *l3part;   // [blocks]: sum |x|^3 over a block's pre-step rows
};

__device__ __forceinline__ void adam_block0(const AdamApply &A) {
    const int lane = (int)threadIdx.x;
    float s = 0.f;
    for (int64_t i0 = lane; i0 < A.bs; i0 += 64 * 8) {   // 8 independent loads in flight per lane
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u * 64 < A.bs ? A.lpart[i0 + u * 64] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    s = gsum<64>(s);
    if (lane == 0) {
        const float l = s * A.scale + A.cst;
        if (A.loss_assign) *A.loss = l; else *A.loss += l;
    }
}

template <int G, int VEC, int KCH, bool L3 = false>
__global__ __launch_bounds__(256) void k_apply_adam(AdamApply A) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (blockIdx.x == 0 && threadIdx.x < 64 && A.loss && A.lpart) adam_block0(A);
    int ti = 0;
    while (ti < A.ntab && row >= A.t[ti].rows) {
        row -= A.t[ti].rows;
        ++ti;
    }
    // (L3: a block-wide barrier follows, so the groups past the last row stay, with nothing to add)
    if (!L3 && ti >= A.ntab) return;
    float cube = 0.f;   // L3: this lane's part of sum |x|^3 of the pre-step row
    if (!L3 || ti < A.ntab) {
        const AdamTable &T = A.t[ti];
        const int D = (int)A.dim;
        const int64_t off = row * D;
        Vec x, m, v, g;
        vload(x, T.w + off, D, lane);
        vload(m, T.m + off, D, lane);
        vload(v, T.v + off, D, lane);
        const int flagged = T.flag[row];
        if (flagged) {
            Vec gr;
            vload(gr, T.grad + off, D, lane);
            if (T.jacobian) {
                const float n = sqrtf(vdot(x, x));
                vnormalize_bwd(x, n, gr, g);
            } else {
                g = gr;
            }
            Vec z;
            vzero(z);
            vstore(z, T.grad + off, D, lane);
            if (lane == 0) T.flag[row] = 0;
        } else {
            vzero(g);
        }
        if constexpr (L3) {
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) {
                const float sq = x.x[i] * fabsf(x.x[i]);   // x |x|: the gradient's shape, 0 at 0
                g.x[i] += A.l3c * sq;
                cube += fabsf(sq * x.x[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) {
            m.x[i] = m.x[i] + A.omb1 * (g.x[i] - m.x[i]);
            v.x[i] = A.beta2 * v.x[i] + A.omb2 * g.x[i] * g.x[i];
            const float den = sqrtf(v.x[i]) / A.bc2_sqrt + A.eps;
            x.x[i] = x.x[i] - A.step_size * (m.x[i] / den);
        }
        vstore(m, T.m + off, D, lane);
        vstore(v, T.v + off, D, lane);
        vstore(x, T.w + off, D, lane);
    }
    if constexpr (L3) {
        __shared__ float s_cube[GPB];
        cube = gsum<G>(cube);
        if (lane == 0) s_cube[threadIdx.x / G] = cube;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int i = 0; i < GPB; ++i) s += s_cube[i];
            A.l3part[blockIdx.x] = s;
        }
    }
}

// loss += l3 * sum(part[0 .. n)): one block, every thread a strided share in a fixed order, then an LDS tree
__global__ __launch_bounds__(256) void k_l3_loss(const float *__restrict__ part, int64_t n, float l3,
                                                 float *__restrict__ loss) {
    __shared__ float s_sum[256];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += part[i];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss += l3 * s_sum[0];
}

}  // namespace dev

int64_t apply_adam_blocks(const StepParams &P) {
    const int64_t rows = P.ent_total + P.rel_total * (P.model == 1 ? 2 : 1);
    const int64_t gpb = 256 / pick_shape(P.dim).G;
    return (rows + gpb - 1) / gpb;
}

hipError_t launch_apply_adam(const StepParams &P, const StepWorkspace &W, const AdamParams &Ad, int64_t bs,
                             float loss_scale, float loss_cst, float *loss, hipStream_t st, float l3, float *l3part) {
    const Shape s = pick_shape(P.dim);
    if (l3 != 0.f && !l3part) return hipErrorInvalidValue;
    dev::AdamApply A{};
    A.ntab = 0;
    const int ent_j = P.model == 0 && P.norm_flag;   // (gradient conventions per table: device.h group_step)
    A.t[A.ntab++] = dev::AdamTable{P.ent, Ad.m[0], Ad.v[0], W.gent, W.fent, P.ent_total, ent_j};
    A.t[A.ntab++] = dev::AdamTable{P.rel, Ad.m[1], Ad.v[1], W.grel, W.frel, P.rel_total, P.norm_flag};
    if (P.model == 1) A.t[A.ntab++] = dev::AdamTable{P.normv, Ad.m[2], Ad.v[2], W.gnorm, W.fnorm, P.rel_total, 1};
    for (int i = 0; i < A.ntab; ++i)
        if (!A.t[i].m || !A.t[i].v) return hipErrorInvalidValue;
    A.dim = P.dim;
    A.beta2 = (float)Ad.beta2;
    A.omb1 = (float)(1.0 - Ad.beta1);
    A.omb2 = (float)(1.0 - Ad.beta2);
    A.eps = (float)Ad.eps;
    A.step_size = Ad.step_size; A.bc2_sqrt = Ad.bc2_sqrt;
    A.loss = loss;
    A.lpart = W.lpart;
    A.bs = bs;
    A.scale = loss_scale;
    A.cst = loss_cst;
    A.loss_assign = P.loss_assign;
    A.l3c = 3.0f * l3;
    A.l3part = l3part;
    int64_t rows = 0;
    for (int i = 0; i < A.ntab; ++i) rows += A.t[i].rows;
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((rows + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        if (l3 != 0.f)
            hipLaunchKernelGGL((dev::k_apply_adam<T::G, T::VEC, T::KCH, true>), grid, block, 0, st, A);
        else
            hipLaunchKernelGGL((dev::k_apply_adam<T::G, T::VEC, T::KCH>), grid, block, 0, st, A);
        e = hipGetLastError();
    });
    if (e == hipSuccess && l3 != 0.f && loss) {   // (grid.x == apply_adam_blocks(P) partials)
        hipLaunchKernelGGL(dev::k_l3_loss, dim3(1), dim3(256), 0, st, l3part, (int64_t)grid.x, l3, loss);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace pt

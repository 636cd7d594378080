// HIP kernels of the optimizer apply pass (sparse SGD / Adagrad rows) for gfx950.
//
// Layout and mapping
//  * Rows are held by lane groups (struct Shape, kernels.h); one group applies one table row.
//  * This is gather/axpy work (no dense contraction): the roofline is HBM / Infinity-Cache bandwidth
//    and the memory-side float-atomic rate, not MFMA.
//
// Semantics (all cited in DESIGN.md): sampler = Base.cpp:185-310 + Corrupt.h:9-105 + Random.h:18-29;
// forward = TransE.py:46-74 / TransH.py:52-93; loss = MarginLoss.py:24-28 via NegativeSampling.py:13-31;
// backward = torch autograd of those ops (normalize Jacobian, sign / v/||v|| norm derivatives, maximum
// tie -> half); update = torch.optim.SGD / Adagrad (eps 1e-10) as built in Trainer.py:62-88, applied
// only to rows with a nonzero gradient (identical to the dense update).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "graph.h"
#include "kernels.h"
#include "rng.h"

namespace pt {
namespace dev {
using pt::CsrWork;

// Sparse apply: for every touched row finish the gradient (normalize Jacobian of the pre-step row
// when that table's gradient is in normalized space) and run SGD / Adagrad; then clear the row.
struct ApplyTable {
    float *w, *acc, *grad;
    int *flag;
    int64_t rows;
    int jacobian;
    const int *start;       // CSR of extra contribution rows (NULL: none): rows start[r] .. start[r+1]-1
    const int *pstart;      // a second bucket of contribution rows, the positives' stored rows (CsrWork::pstart;
                            // NULL: none): rows pstart[r] .. pstart[r+1]-1, summed after the first bucket's
};
struct ApplyParams {
    ApplyTable t[3];
    int ntab;
    int64_t dim;
    int opt;
    float lr;
    // sampler advance + loss (done by block 0)
    uint64_t *states;
    int64_t threads, bs, dpp;
    float *loss;
    const float *lpart;   // [bs] per-positive loss partials of the step
    float margin, inv_count;
    int loss_assign;
    const float *contrib;   // [n][dim] the contribution rows both buckets index (NULL: none)
};

// block 0, first wave: advance the sampler streams and reduce the step's loss partials in a fixed
// order: loss += inv_count * sum(lpart) + margin (MarginLoss.py:24-28)
__device__ __forceinline__ void apply_block0(const ApplyParams &A) {
    const int lane = (int)threadIdx.x;
    if (A.states) advance_states(A.states, A.threads, A.bs, A.dpp, lane);
    if (A.loss && A.lpart) {
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
            const float l = s * A.inv_count + A.margin;
            if (A.loss_assign) *A.loss = l; else *A.loss += l;
        }
    }
}

template <int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_apply(ApplyParams A) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    int64_t row = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (blockIdx.x == 0 && threadIdx.x < 64) apply_block0(A);
    int ti = 0;
    while (ti < A.ntab && row >= A.t[ti].rows) {
        row -= A.t[ti].rows;
        ++ti;
    }
    if (ti >= A.ntab) return;
    const ApplyTable &T = A.t[ti];
    const int flagged = T.flag[row];
    int c0 = 0, c1 = 0;
    if (T.start) {
        c0 = T.start[row];
        c1 = T.start[row + 1];
    }
    if (!flagged && c0 == c1) return;
    const int D = (int)A.dim;
    Vec x, gsum_, g;
    vload(x, T.w + row * D, D, lane);
    if (flagged) vload(gsum_, T.grad + row * D, D, lane); else vzero(gsum_);
    // contributions of this step's corrupted-entity slots (counting-sort order)
    int j = c0;
    for (; j + 4 <= c1; j += 4) {
        Vec c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) vload(c[u], A.contrib + (int64_t)(j + u) * D, D, lane);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) gsum_.x[i] += c[u].x[i];
    }
    for (; j < c1; ++j) {
        Vec c;
        vload(c, A.contrib + (int64_t)j * D, D, lane);
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) gsum_.x[i] += c.x[i];
    }
    if (T.jacobian) {
        const float n = sqrtf(vdot(x, x));
        vnormalize_bwd(x, n, gsum_, g);
    } else {
        g = gsum_;
    }
    if (A.opt == 0) {
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) x.x[i] = x.x[i] + (-A.lr) * g.x[i];
    } else {
        Vec a;
        vload(a, T.acc + row * D, D, lane);
#pragma unroll
        for (int i = 0; i < Vec::N; ++i) {
            a.x[i] = a.x[i] + g.x[i] * g.x[i];
            x.x[i] = x.x[i] + (-A.lr) * g.x[i] / (sqrtf(a.x[i]) + 1e-10f);
        }
        vstore(a, T.acc + row * D, D, lane);
    }
    vstore(x, T.w + row * D, D, lane);
    if (flagged) {
        Vec z;
        vzero(z);
        vstore(z, T.grad + row * D, D, lane);
        if (lane == 0) T.flag[row] = 0;
    }
}

// Apply pass with float4 rows and raw-buffer access (D % 4 == 0, offsets within 31 bits): one lane
// group per table row. The row (and its Adagrad state) load is issued before the flag / bucket range
// loads return; a bucket's contribution rows stream NC at a time with out-of-range offsets past its
// end (the hardware returns zeros, so the adds need no branches), summed in bucket order after the
// row's own gradient row. A row has up to two buckets, read as one stream: the negatives' counting-sort rows
// (entity table) and the positives' stored rows (entity and relation tables, at most the cap long); its
// gradient row is loaded, re-zeroed and un-flagged only when flagged (the uses beyond the cap).
template <int G, int VEC, int KCH, int NC>
__global__ __launch_bounds__(256) void k_apply_buf(ApplyParams A) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int64_t gi = uni<G>((int32_t)(blockIdx.x * GPB + threadIdx.x / G));   // scalar at G = 64
    if (blockIdx.x == 0 && threadIdx.x < 64) apply_block0(A);
    const int D = (int)A.dim;
    const uint32_t rowb = (uint32_t)D * 4u;
    // the group's row: its table and the row inside it
    int64_t row = gi;
    int ti = 0;
    while (ti < A.ntab && row >= A.t[ti].rows) {
        row -= A.t[ti].rows;
        ++ti;
    }
    const bool live = ti < A.ntab;
    int flag = 0, c0 = 0, c1 = 0, p0 = 0, p1 = 0;
    Vec x, g, a;
    // (the one-trip loops keep the instruction stream of the former rows-per-group loops: DESIGN.md §4)
    // ---- every load of the row in flight together
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        if (!live) continue;
        const ApplyTable &T = A.t[ti];
        const uint32_t tb = (uint32_t)T.rows * rowb;
        bload(x, make_rsrc(T.w, tb), (uint32_t)row * rowb, D, lane);
        if (A.opt != 0) bload(a, make_rsrc(T.acc, tb), (uint32_t)row * rowb, D, lane);
        flag = T.flag[row];
        if (T.start) {
            c0 = T.start[row];
            c1 = T.start[row + 1];
        }
        if (T.pstart) {
            p0 = T.pstart[row];
            p1 = T.pstart[row + 1];
        }
    }
    int len = 0, n0 = 0;
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        if (!live) continue;
        const ApplyTable &T = A.t[ti];
        bload(g, make_rsrc(T.grad, (uint32_t)T.rows * rowb), flag ? (uint32_t)row * rowb : kOob, D, lane);
        n0 = c1 - c0;
        len = n0 + (p1 - p0);
    }
    // ---- contribution rows: the row's buckets streamed NC at a time, out-of-range past their end (zeros),
    // summed in bucket order, the negatives' bucket first
    const auto c_rs = make_rsrc(A.contrib, 0x7fffffffu);
    for (int j = 0; j < len; j += NC) {
        Vec c[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int i = j + q;
            const int r = i < n0 ? c0 + i : p0 + (i - n0);
            bload(c[q], c_rs, i < len ? (uint32_t)r * rowb : kOob, D, lane);
        }
#pragma unroll
        for (int q = 0; q < NC; ++q)
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) g.x[i] += c[q].x[i];
    }
    // ---- the update
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        if (!live || (!flag && len == 0)) continue;   // untouched row: unchanged
        const ApplyTable &T = A.t[ti];
        const uint32_t tb = (uint32_t)T.rows * rowb;
        Vec gg;
        if (T.jacobian) {
            const float n = sqrtf(vdot(x, x));
            vnormalize_bwd(x, n, g, gg);
        } else {
            gg = g;
        }
        if (A.opt == 0) {
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) x.x[i] = x.x[i] + (-A.lr) * gg.x[i];
        } else {
#pragma unroll
            for (int i = 0; i < Vec::N; ++i) {
                a.x[i] = a.x[i] + gg.x[i] * gg.x[i];
                x.x[i] = x.x[i] + (-A.lr) * gg.x[i] / (sqrtf(a.x[i]) + 1e-10f);
            }
            bstore(a, make_rsrc(T.acc, tb), (uint32_t)row * rowb, D, lane);
        }
        bstore(x, make_rsrc(T.w, tb), (uint32_t)row * rowb, D, lane);
        if (flag) {
            Vec z;
            vzero(z);
            bstore(z, make_rsrc(T.grad, tb), (uint32_t)row * rowb, D, lane);
            if (lane == 0) T.flag[row] = 0;
        }
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
hipError_t launch_apply(const StepParams &P, const StepWorkspace &W, uint64_t *states, int64_t threads, int64_t bs,
                        int64_t dpp, float *loss, hipStream_t st, const CsrWork *csr) {
    const Shape s = pick_shape(P.dim);
    dev::ApplyParams A{};
    A.ntab = 0;
    const int ent_j = P.model == 0 && P.norm_flag;
    // on a counting-sort batch the relation rows come first in the grid: their buckets of stored positive rows
    // are the longest (up to the relation cap), so they must not be the kernel's tail
    const dev::ApplyTable ent{P.ent, P.ent_acc, W.gent, W.fent, P.ent_total, ent_j, csr ? csr->start : nullptr,
                              csr ? csr->pstart : nullptr};
    const dev::ApplyTable rel{P.rel, P.rel_acc, W.grel, W.frel, P.rel_total, P.norm_flag, nullptr,
                              csr && csr->pstart ? csr->pstart + P.ent_total : nullptr};
    A.t[A.ntab++] = csr ? rel : ent;
    A.t[A.ntab++] = csr ? ent : rel;
    if (P.model == 1)
        A.t[A.ntab++] = dev::ApplyTable{P.normv, P.norm_acc, W.gnorm, W.fnorm, P.rel_total, 1, nullptr, nullptr};
    A.contrib = csr ? csr->contrib : nullptr;
    A.dim = P.dim;
    A.opt = P.opt;
    A.lr = P.lr;
    A.states = states;
    A.threads = threads;
    A.bs = bs;
    A.dpp = dpp;
    A.loss = loss;
    A.lpart = W.lpart;
    A.margin = P.margin;
    A.inv_count = P.inv_count;
    A.loss_assign = P.loss_assign;
    int64_t rows = 0;
    for (int i = 0; i < A.ntab; ++i) rows += A.t[i].rows;
    // float4 rows through raw buffers (k_apply_buf) where the offsets fit 31 bits - the contribution rows count
    // only when there are any - else k_apply
    const bool buf = P.dim % 4 == 0 && offsets_fit31(P, csr ? csr_con_rows(P.batch_size, P.neg) : 0);
    const int64_t gpb = 256 / s.G;
    const dim3 grid((unsigned)((rows + gpb - 1) / gpb)), block(256);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        using T = decltype(sh);
        if constexpr (T::VEC == 4) {
            // contribution rows in flight per lane group: 8 for one-chunk float4 rows (C2: the bucket of a row
            // - Poisson, mean 3.6 at C2 - mostly in one round trip; measured 12.0 vs 12.6 us), else 4
            constexpr int NC = T::G == 64 && T::KCH == 1 ? 8 : 4;
            if (buf) {
                hipLaunchKernelGGL((dev::k_apply_buf<T::G, 4, T::KCH, NC>), grid, block, 0, st, A);
                e = hipGetLastError();
                return;
            }
        }
        hipLaunchKernelGGL((dev::k_apply<T::G, T::VEC, T::KCH>), grid, block, 0, st, A);
        e = hipGetLastError();
    });
    return e;
}

}  // namespace pt

// HIP kernels of universe link prediction (global energy estimation) for gfx950 (MI355X).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "kernels.h"

namespace pt {
namespace dev {

// ---------------------------------------------------------------- universe link prediction ------
// Global energy estimation (Parallel_Universe_Config.py:446-554): for every (key, universe) pair score
// every local entity of the universe as the missing side and MIN it into the key's global row
// (scores are norms >= 0, so float order == int order and atomicMin on the bits is exact).
// side 0 = head prediction (anchor is the tail: e + (r - anchor)), side 1 = tail prediction
// (anchor is the head: (anchor + r) - e).
//
// k_lp_bases: one lane group per pair: the pair's normalized (projected for TransH) anchor combined
//   with its relation -> base[pair][D] (+ the relation's normal for TransH), and the null_vector tuple
//   score of the key in this universe (calc_tuple_score, :378-388: raw anchor, no projection).
// k_lp_scan_t: one workgroup per (tile of 64 entities, universe): each entity row is loaded (and, for TransE,
//   normalized) ONCE and scored against every pair of its universe - the universe's rows are read once
//   per tile instead of once per pair.
// One launch pair covers every universe whose dim takes the same lane-group shape (each universe's own dim
// at run time); the pairs' base / normal rows are `ds` floats apart (the largest dim of the launch).
template <int MODEL, int G, int VEC, int KCH>
__global__ __launch_bounds__(256) void k_lp_bases(const LpUniverseDev *__restrict__ us, const LpPair *__restrict__ pairs,
                                                  int64_t n_pairs, int p_norm, int norm_flag, int64_t ds,
                                                  float *__restrict__ base, float *__restrict__ normal,
                                                  float *__restrict__ tuple_min) {
    using Vec = V<G, VEC, KCH>;
    constexpr int GPB = 256 / G;
    const int lane = threadIdx.x % G;
    const int64_t pi = (int64_t)blockIdx.x * GPB + threadIdx.x / G;
    if (pi >= n_pairs) return;
    const LpPair pr = pairs[pi];
    const LpUniverseDev U = us[pr.universe];
    const int D = (int)U.dim;
    Vec A, R, ah, rh, nW, b;
    vload(A, U.ent + (int64_t)pr.anchor * D, D, lane);
    vload(R, U.rel + (int64_t)pr.rel * D, D, lane);
    if (norm_flag) vnormalize(R, rh); else rh = R;
    if (tuple_min) {
        Vec an, v;
        if (norm_flag) vnormalize(A, an); else an = A;
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) v.x[k] = pr.side == 0 ? rh.x[k] - an.x[k] : an.x[k] + rh.x[k];
        const float sc = vpnorm(v, p_norm);
        if (lane == 0) atomicMin(reinterpret_cast<int *>(tuple_min + pr.key), __float_as_int(sc));
    }
    if constexpr (MODEL == 1) {
        Vec W;
        vload(W, U.normv + (int64_t)pr.rel * D, D, lane);
        vnormalize(W, nW);
        const float ad = vdot(A, nW);
#pragma unroll
        for (int k = 0; k < Vec::N; ++k) A.x[k] = A.x[k] - ad * nW.x[k];
        vstore(nW, normal + pi * ds, D, lane);
    }
    if (norm_flag) vnormalize(A, ah); else ah = A;
#pragma unroll
    for (int k = 0; k < Vec::N; ++k) b.x[k] = pr.side == 0 ? rh.x[k] - ah.x[k] : ah.x[k] + rh.x[k];
    vstore(b, base + pi * ds, D, lane);
}

// k_lp_scan_t: the scan, transposed against the lane-group kernels - one LANE per entity. A workgroup (NW waves)
// stages a tile of 64 consecutive local entity rows in LDS once (row stride D + 1 floats: lane e reading float d of
// its row hits bank (e + d) mod 64, conflict-free), and each wave walks every NW-th of the universe's pairs: for a pair, every
// lane sums its own entity's |x + b| (or squares) sequentially over d with the pair's base row uniform across
// the wave - no cross-lane reduction per score - and MINs its score into the key row with one atomic
// instruction for 64 entities, skipped when the row already holds a score no larger (the rows only decrease,
// so a stale read can only make an atomic unnecessary, never wrong). TransE rows are normalized once per
// tile (inverse norm per lane); TransH rows are projected on the pair's normal and normalized per pair.
// sum over d < D of f(d) in 8 interleaved partial sums, combined pairwise: 8 independent add chains per lane
// and a rounding error of order (D / 8 + 3) ulp, near the tree reductions of the lane-group kernels
template <typename F>
__device__ __forceinline__ float sum8(int D, F f) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int d = 0;
    for (; d + 8 <= D; d += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += f(d + k);
    }
    for (int k = 0; d + k < D; ++k) a[k] += f(d + k);
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// acc + |v| as one VOP3 add with the abs source modifier. (Left to itself the compiler packs the adds of two
// partial sums into v_pk_add_f32, which has no abs modifier, and spends a v_and_b32 per term on |v|: 2 VALU
// instructions per term instead of 1.5 with v_pk_fma_f32 + this.)
__device__ __forceinline__ float add_abs(float acc, float v) {
    float r;
    asm("v_add_f32_e64 %0, %1, |%2|" : "=v"(r) : "v"(acc), "v"(v));
    return r;
}

// NP sums of the sum8 form (the same partial sums and combination order for each) over one pass of d: the
// caller's function f(q, d) for sum q reads shared operands (the LDS row) once for all of them. MODE 1: the terms
// are |f(q, d)| (a + |v|, one add); MODE 2: the terms are f(q, d)^2, accumulated by an explicit fma(v, v, a).
// (The TransE scan states every rounding explicitly - an fma where the step is an fma, nothing left to the
// compiler's contraction, which had fused some of a loop's products and not others: the two-pair pass and the
// one-pair remainder of k_lp_scan_t then rounded the same pair's score differently; tests/test_gpu_lp_scan.py.)
template <int NP, int MODE = 0, typename F>
__device__ __forceinline__ void sum8xn(int D, F f, float (&r)[NP]) {
    float a[NP][8];
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int k = 0; k < 8; ++k) a[q][k] = 0.f;
    int d = 0;
    auto step = [&](float acc, float v) {
        return MODE == 1 ? add_abs(acc, v) : MODE == 2 ? __builtin_fmaf(v, v, acc) : acc + v;
    };
    auto group = [&](int d0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < NP; ++q) a[q][k] = step(a[q][k], f(q, d0 + k));
    };
    // (two 8-dim groups per iteration: the next group's operand loads issue before the current group's waits;
    // unrolled by hand - the compiler does not unroll a loop holding the asm add of add_abs)
    for (; d + 16 <= D; d += 16) {
        group(d);
        group(d + 8);
    }
    if (d + 8 <= D) {
        group(d);
        d += 8;
    }
    for (int k = 0; d + k < D; ++k)
#pragma unroll
        for (int q = 0; q < NP; ++q) a[q][k] = step(a[q][k], f(q, d + k));
#pragma unroll
    for (int q = 0; q < NP; ++q)
        r[q] = ((a[q][0] + a[q][1]) + (a[q][2] + a[q][3])) + ((a[q][4] + a[q][5]) + (a[q][6] + a[q][7]));
}

#ifndef PT_LP_PAIRS
#define PT_LP_PAIRS 2   // (measured r05, C4 k_lp_scan_t total: 1 pair 137.9 ms, 2 pairs 99.4, 4 pairs 105.3, 8 pairs 128.5)
#endif

template <int MODEL, int NW>
__global__ __launch_bounds__(64 * NW) void k_lp_scan_t(const LpUniverseDev *__restrict__ us, const LpPair *__restrict__ pairs,
                                                   const int64_t *__restrict__ uoff, const int32_t *__restrict__ uids,
                                                   int p_norm, int norm_flag, int64_t global_E, int64_t ds,
                                                   const float *__restrict__ base, const float *__restrict__ normal,
                                                   float *__restrict__ rows) {
    extern __shared__ float s_x[];   // [64][D + 1]
    // (the wave index made provably uniform: the pair walk, its LpPair records and base rows then live in scalar
    // registers and load through the scalar cache, instead of every lane loading the same base-row words)
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int32_t u = uids[blockIdx.y];
    const LpUniverseDev U = us[u];
    const int D = (int)U.dim, S = D + 1;
    const int64_t p0 = uoff[2 * u], p1 = uoff[2 * u + 1];
    for (int64_t e0 = (int64_t)blockIdx.x * 64; e0 < U.ent_total; e0 += (int64_t)gridDim.x * 64) {
        const int ne = U.ent_total - e0 < 64 ? (int)(U.ent_total - e0) : 64;
        __syncthreads();   // (the previous tile's readers are done)
        const float *src = U.ent + e0 * D;
        for (int i = (int)threadIdx.x; i < ne * D; i += 64 * NW) {
            const int r = i / D;
            s_x[r * S + (i - r * D)] = src[i];
        }
        __syncthreads();
        const bool live = lane < ne;
        float *xr = s_x + (live ? lane : 0) * S;
        const int64_t col = live ? U.remap[e0 + lane] : 0;
        float inv = 1.f;
        if (MODEL == 0 && norm_flag) {   // F.normalize's scale of this lane's row
            float n2[1];
            sum8xn<1, 2>(D, [&](int, int d) { return xr[d]; }, n2);
            const float n = sqrtf(n2[0]);
            inv = 1.0f / (n > kEps ? n : kEps);
        }
        int64_t pi = p0 + wave;
        if constexpr (MODEL == 0) {
            // TransE: the tile's rows normalized in place once (x * inv: the same rounded products the per-pair form
            // computed), then the wave's pairs PT_LP_PAIRS at a time - pi, pi + NW, ... share every LDS read of the row.
            // Each score keeps its expression and its sum8 order, so the scores are bit-identical to one pair at a time.
            // (the NW waves share the tile: every wave has read it for its norm, then wave 0 normalizes it while the
            // others wait)
            __syncthreads();
            if (wave == 0 && live && norm_flag) {
                for (int d = 0; d < D; ++d) xr[d] = xr[d] * inv;
            }
            __syncthreads();
            constexpr int NPP = PT_LP_PAIRS;   // pairs per pass: pi, pi + NW, ..., pi + NW (NPP - 1)
            for (; pi + NW * (NPP - 1) < p1; pi += NW * NPP) {
                LpPair pr[NPP];
                const float *bq[NPP];
                float sg[NPP], acc[NPP];
                int *cell[NPP];
                int old[NPP];
#pragma unroll
                for (int q = 0; q < NPP; ++q) {
                    pr[q] = pairs[pi + NW * q];
                    bq[q] = base + (pi + NW * q) * ds;
                    sg[q] = pr[q].side == 0 ? 1.f : -1.f;
                    // the key-row cells this pass may lower, read before the sums (their latency hidden behind them)
                    cell[q] = reinterpret_cast<int *>(rows + (int64_t)pr[q].key * global_E + col);
                    old[q] = live ? __builtin_nontemporal_load(cell[q]) : 0;
                }
                if (p_norm == 1)
                    sum8xn<NPP, 1>(D, [&](int q, int d) { return __builtin_fmaf(sg[q], xr[d], bq[q][d]); }, acc);
                else
                    sum8xn<NPP, 2>(D, [&](int q, int d) { return __builtin_fmaf(sg[q], xr[d], bq[q][d]); }, acc);
                if (live) {
#pragma unroll
                    for (int q = 0; q < NPP; ++q) {
                        const float sc = p_norm == 1 ? acc[q] : sqrtf(acc[q]);
                        const int bits = __float_as_int(sc);
                        if (bits < old[q]) atomicMin(cell[q], bits);
                    }
                }
            }
            inv = 1.f;   // (the row is normalized in LDS now)
        }
        for (; pi < p1; pi += NW) {
            const LpPair pr = pairs[pi];
            const float *b = base + pi * ds;
            const float sg = pr.side == 0 ? 1.f : -1.f;   // side 0: x-hat + b; side 1: b - x-hat
            float acc;
            if constexpr (MODEL == 0) {   // (the row is normalized in LDS: inv = 1)
                float a1[1];
                if (p_norm == 1)
                    sum8xn<1, 1>(D, [&](int, int d) { return __builtin_fmaf(sg, xr[d] * inv, b[d]); }, a1);
                else
                    sum8xn<1, 2>(D, [&](int, int d) { return __builtin_fmaf(sg, xr[d] * inv, b[d]); }, a1);
                acc = a1[0];
            } else {
                const float *nw = normal + pi * ds;
                const float xd = sum8(D, [&](int d) { return xr[d] * nw[d]; });
                float sc = 1.f;
                if (norm_flag) {
                    const float n = sqrtf(sum8(D, [&](int d) {
                        const float t = xr[d] - xd * nw[d];
                        return t * t;
                    }));
                    sc = 1.0f / (n > kEps ? n : kEps);
                }
                acc = p_norm == 1 ? sum8(D, [&](int d) { return fabsf(sg * ((xr[d] - xd * nw[d]) * sc) + b[d]); })
                                  : sum8(D, [&](int d) {
                                        const float v = sg * ((xr[d] - xd * nw[d]) * sc) + b[d];
                                        return v * v;
                                    });
            }
            const float score = p_norm == 1 ? acc : sqrtf(acc);
            if (live) {
                int *cell = reinterpret_cast<int *>(rows + (int64_t)pr.key * global_E + col);
                const int bits = __float_as_int(score);
                if (bits < *cell) atomicMin(cell, bits);
            }
        }
    }
}

}  // namespace dev

// ==================================================================== host launcher ============
// k_lp_scan_t's waves per workgroup sharing one tile (measured r05, C4's nine launches: 4 waves 85.3 ms, 8 waves
// 77.1 ms, 16 waves 91.3 ms, profiles/r05_c4_lp_waves.json)
static constexpr int kLpWaves = 8;

hipError_t launch_lp_min(const LpUniverseDev *us, const LpPair *pairs, int64_t n_pairs, const int64_t *uoff,
                         const int32_t *uids, int64_t n_active, int64_t dim, int64_t max_ent, int model, int p_norm,
                         int norm_flag, int64_t global_E, int64_t ds, float *base, float *normal, float *rows,
                         float *tuple_min, hipStream_t st) {
    if (n_pairs <= 0) return hipSuccess;
    const Shape s = pick_shape(dim);
    // the scan's tile of 64 rows in LDS (row stride dim + 1): at most 64 * 513 floats = 128 KB at a dispatched dim
    const size_t lds_t = sizeof(float) * 64 * (size_t)(dim + 1);
    const int64_t gpb = 256 / s.G;
    const dim3 gb((unsigned)((n_pairs + gpb - 1) / gpb)), block(256), bt(64 * kLpWaves);
    hipError_t e = hipErrorInvalidValue;
    for_shape(s, [&](auto sh) {
        for_value<0, 1>(model != 0, [&](auto m) {
            using T = decltype(sh);
            // (the shapes of dims above 512, which pt_lp_min_scores refuses, have no instance here)
            if constexpr (T::VEC * T::KCH <= 8) {
                const auto scan = dev::k_lp_scan_t<m.value, kLpWaves>;
                if (lds_t > (64 << 10)) {
                    e = hipFuncSetAttribute(reinterpret_cast<const void *>(scan),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_t);
                    if (e != hipSuccess) return;
                }
                for (int64_t y0 = 0; y0 < n_active; y0 += 65535) {   // (grid.y holds 65,535 universes)
                    if (y0 == 0)
                        hipLaunchKernelGGL((dev::k_lp_bases<m.value, T::G, T::VEC, T::KCH>), gb, block, 0, st, us,
                                           pairs, n_pairs, p_norm, norm_flag, ds, base, normal, tuple_min);
                    const dim3 gt((unsigned)((max_ent + 63) / 64),
                                  (unsigned)(n_active - y0 < 65535 ? n_active - y0 : 65535));
                    hipLaunchKernelGGL(scan, gt, bt, lds_t, st, us, pairs, uoff, uids + y0, p_norm, norm_flag, global_E,
                                       ds, base, normal, rows);
                }
                e = hipGetLastError();
            }
        });
    });
    return e;
}

}  // namespace pt

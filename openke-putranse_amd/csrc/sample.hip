// HIP kernels of the batch samplers for gfx950 (MI355X): sampling() into arrays, and the counting-sort sampling
// passes of the large-negative training path (fused in LDS, split over parts, or two passes).
//
// Semantics (cited in DESIGN.md): sampler = Base.cpp:185-310 + Corrupt.h:9-105 + Random.h:18-29.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"
#include "graph.h"
#include "kernels.h"
#include "rng.h"

namespace pt {
namespace dev {
using pt::CsrWork;

// sampling() into arrays (one thread per positive, Base.cpp:185-264); the stream advance is a separate
// kernel. mode 0: a coin per negative picks the replaced side (draw_negative); mode -1 (sampling_head)
// replaces the head via corrupt_tail, mode 1 (sampling_tail) the tail via corrupt_head - no coin, and
// corrupt_*'s default filter_flag = true (Base.cpp:233-245). Then neg_rel relation corruptions
// (corrupt_rel, p = false, filter_flag = true: Corrupt.h:108-135, :179-189) drawn among the relations
// not yet linking (h, t) - the same run search as the entity corruptions, over the cmp_rel list.
__global__ void k_sample(DeviceGraph g, const uint64_t *__restrict__ states, int64_t threads, int64_t bs, int64_t neg,
                         int64_t neg_rel, int mode, int bern, int filter, int64_t *__restrict__ oh,
                         int64_t *__restrict__ ot, int64_t *__restrict__ orr, float *__restrict__ oy) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= bs) return;
    const int64_t per_neg = mode == 0 ? 2 : 1;
    const PosDraw pd = draw_positive(g, states, threads, bs, b, 1 + per_neg * neg + neg_rel);
    const int64_t hp = pd.h, rp = pd.r, tp = pd.t;
    oh[b] = hp; ot[b] = tp; orr[b] = rp;
    if (oy) oy[b] = 1.f;
    for (int64_t k = 0; k < neg; ++k) {
        int64_t hh = hp, tt = tp;
        if (mode == 0) {
            int tail_side;
            const int64_t e = draw_negative(g, pd, k, bern, filter, &tail_side);
            if (tail_side) tt = e; else hh = e;
        } else {
            uint64_t s = lcg_jump(pd.s1, (uint64_t)k);
            if (mode < 0) hh = corrupt_in_run(g.tail_h, pd.tr_lo, pd.tr_hi, g.ent_total, s);
            else tt = corrupt_in_run(g.head_t, pd.hr_lo, pd.hr_hi, g.ent_total, s);
        }
        const int64_t o = (k + 1) * bs + b;
        oh[o] = hh;
        ot[o] = tt;
        orr[o] = rp;
        if (oy) oy[o] = -1.f;
    }
    if (neg_rel > 0) {
        const int2 run = g.ht_run[pd.idx];
        for (int64_t k = 0; k < neg_rel; ++k) {
            uint64_t s = lcg_jump(pd.s1, (uint64_t)(per_neg * neg + k));
            const int64_t o = (neg + k + 1) * bs + b;
            oh[o] = hp;
            ot[o] = tp;
            orr[o] = corrupt_in_run(g.rel_r, run.x, run.y, g.rel_total, s);
            if (oy) oy[o] = -1.f;
        }
    }
}

// busy-waits `us` microseconds (100 MHz constant wall clock): keeps a stream occupied while the host
// enqueues a measured sequence behind it
__global__ void k_spin(int64_t us) {
    const uint64_t t0 = wall_clock64();
    while (wall_clock64() - t0 < (uint64_t)us * 100) __builtin_amdgcn_s_sleep(8);
}

__global__ void k_advance(uint64_t *states, int64_t threads, int64_t bs, int64_t dpp) {
    advance_states(states, threads, bs, dpp, (int)threadIdx.x);
}

// Counting-sort (CSR) sampling pass of the large-negative path: one thread per (positive, negative)
// slot draws exactly what getBatch draws for it (stream jump to the slot) and reserves the slot's
// place in its corrupted entity's bucket. Thread k == neg of a positive records the positive.
__global__ __launch_bounds__(256) void k_sample_csr(DeviceGraph g, const uint64_t *__restrict__ states,
                                                    int64_t threads, int64_t bs, int64_t neg, int bern, int filter,
                                                    int64_t calls, CsrWork w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_call = bs * (neg + 1);
    if (idx >= calls * per_call) return;
    const int64_t call = idx / per_call, rem = idx - call * per_call;
    const int64_t b = rem / (neg + 1), k = rem - b * (neg + 1);
    const PosDraw pd = draw_positive(g, states, threads, bs, b, 1 + 2 * neg, call);
    if (k == neg) {
        w.pos[call * bs + b] = make_int4((int)pd.h, (int)pd.r, (int)pd.t, 0);
        return;
    }
    int side;
    const int64_t e = draw_negative(g, pd, k, bern, filter, &side);
    const int64_t o = call * bs * neg + b * neg + k;
    w.neg[o] = (int32_t)((e << 1) | side);
    w.off[o] = atomicAdd(&w.cnt[call * w.cnt_stride + e], 1);
}

// The split sampler's cross-workgroup exchange (k_sample_part): relaxed read-modify-writes at AGENT scope,
// spelled out. Agent-scope atomics are performed at the device's coherence point (not in an XCD's L2), so
// every part's count adds and ticket are seen by the last part whatever XCDs the parts run on; nothing else
// the parts share inside the launch is read before a kernel boundary.
__device__ __forceinline__ int32_t agent_add(int32_t *p, int32_t v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t agent_exch(int32_t *p, int32_t v) {
    return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One negative slot's draw from its positive's LDS record (k_sample_sort, k_sample_part): the coin and the
// corruption draw of draw_negative with the same stream offsets and arithmetic; when the drawn index
// falls inside the known-entity run, the boundary search over it (corrupt_in_run) is left to the caller
// (q open; otherwise q is closed and e is the entity).
struct SlotDraw {
    RunSearch q;
    int64_t e;
    int side;
    bool search;
};

// jump maps of the LCG by 2k draws for k < kJumpTab, staged in LDS once per workgroup: a slot's stream
// start is then one 64-bit multiply-add away from its positive's state instead of a square-and-multiply
// loop (the loop remains for k >= kJumpTab)
constexpr int kJumpTab = 256;
__device__ __forceinline__ int32_t jump_tab_len(int64_t neg) { return neg < kJumpTab ? (int32_t)neg : kJumpTab; }
template <int NT>
__device__ __forceinline__ void jump_tab_fill(Affine *jt, int64_t neg, int tid) {
    for (int32_t k = tid; k < jump_tab_len(neg); k += NT) jt[k] = lcg_power((uint64_t)(2 * k));
}

__device__ __forceinline__ SlotDraw slot_prepare(const int32_t *q, int32_t k, int64_t E, int filter,
                                                 const DeviceGraph &g, const Affine *jt) {
    SlotDraw d;
    const uint64_t s1 = *reinterpret_cast<const uint64_t *>(q + 10);
    uint64_t s;
    if (k < kJumpTab) { const Affine m = jt[k]; s = m.a * s1 + m.c; }
    else s = lcg_jump(s1, (uint64_t)(2 * k));
    d.side = (float)(lcg_next(s) % 1000ULL) < __int_as_float(q[0]) ? 1 : 0;
    d.search = false;
    d.q.l = 0;
    d.q.r = 1;   // closed
    if (filter) {
        const int32_t *vals = d.side ? g.head_t : g.tail_h;
        const int32_t lo = d.side ? q[1] : q[3], hi = d.side ? q[2] : q[4];
        const int32_t vlo = d.side ? q[5] : q[7], vhi = d.side ? q[6] : q[8];
        const int64_t tmp = rand_max(s, E - (hi - lo + 1));
        if (tmp < vlo) d.e = tmp;
        else if (tmp > vhi - hi + lo - 1) d.e = tmp + hi - lo + 1;
        else { d.search = true; d.q = run_search(vals, lo, hi, vlo, vhi, (int32_t)tmp); d.e = 0; }
    } else {
        const int64_t tmp = rand_max(s, E - 1);
        const int64_t skip = d.side ? q[5] : q[6];
        d.e = tmp < skip ? tmp : tmp + 1;
    }
    return d;
}

// two slots' boundary searches stepped in lock step (both gathers in flight together)
__device__ __forceinline__ void slot_search2(SlotDraw &d0, SlotDraw &d1) {
    for (;;) {
        const bool a0 = rs_open(d0.q), a1 = rs_open(d1.q);
        if (!(a0 || a1)) break;
        const int32_t m0 = a0 ? rs_probe(d0.q) : 0, m1 = a1 ? rs_probe(d1.q) : 0;
        const int32_t v0 = a0 ? d0.q.vals[m0] : 0, v1 = a1 ? d1.q.vals[m1] : 0;   // only open searches load
        if (a0) rs_update(d0.q, m0, v0);
        if (a1) rs_update(d1.q, m1, v1);
    }
    if (d0.search) d0.e = rs_entity(d0.q);
    if (d1.search) d1.e = rs_entity(d1.q);
}

// SL slots' boundary searches in lock step
template <int SL>
__device__ __forceinline__ void slot_searchN(SlotDraw (&d)[SL]) {
    for (;;) {
        bool a[SL], any = false;
#pragma unroll
        for (int i = 0; i < SL; ++i) { a[i] = rs_open(d[i].q); any |= a[i]; }
        if (!any) break;
        int32_t m[SL], v[SL];
#pragma unroll
        for (int i = 0; i < SL; ++i) m[i] = a[i] ? rs_probe(d[i].q) : 0;
#pragma unroll
        for (int i = 0; i < SL; ++i) v[i] = a[i] ? d[i].q.vals[m[i]] : 0;   // only open searches load
#pragma unroll
        for (int i = 0; i < SL; ++i)
            if (a[i]) rs_update(d[i].q, m[i], v[i]);
    }
#pragma unroll
    for (int i = 0; i < SL; ++i)
        if (d[i].search) d[i].e = rs_entity(d[i].q);
}

// Sampling + counting sort of one sampled call per workgroup, entirely in LDS (when the bucket counts
// and the call's positives fit): the positives are drawn once (not once per slot), every slot's
// negative reserves its rank with an LDS atomic, the counts are scanned in LDS and every slot's
// destination resolved - the same pos / neg / start / destination arrays as k_sample_csr +
// k_scan_counts, without the 52,000 returning global atomics per call and the second pass.
// The sampler streams are read only; the caller advances them afterwards (k_advance).
__global__ __launch_bounds__(1024) void k_sample_sort(DeviceGraph g, const uint64_t *__restrict__ states,
                                                      int64_t threads, int64_t bs, int64_t neg, int bern, int filter,
                                                      int64_t n, CsrWork w) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    __shared__ int32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t call = blockIdx.x;
    Affine *jt = reinterpret_cast<Affine *>(lds);                        // [jump_tab_len(neg)] jump maps
    int32_t *cnt = lds + 4 * jump_tab_len(neg);                          // [n] counts, then starts
    // per positive [12] int32: prob bits, hr_lo hr_hi tr_lo tr_hi, then (filter) the run bounds'
    // values head_t[hr_lo] head_t[hr_hi] tail_h[tr_lo] tail_h[tr_hi] or (no filter) h t, pad, stream state
    // after the index draw (8 B): every slot's draw needs global memory only inside a run's boundary search
    int32_t *pi = cnt + ((n + 3) & ~int64_t(3));
    for (int64_t i = tid; i < n; i += 1024) cnt[i] = 0;
    jump_tab_fill<1024>(jt, neg, tid);
    const int64_t dpp = 1 + 2 * neg;
    for (int64_t b = tid; b < bs; b += 1024) {
        const PosDraw pd = draw_positive(g, states, threads, bs, b, dpp, call);
        int32_t *q = pi + 12 * b;
        q[0] = __float_as_int(bern ? g.bern_prob[pd.r] : 500.f);
        q[1] = pd.hr_lo; q[2] = pd.hr_hi; q[3] = pd.tr_lo; q[4] = pd.tr_hi;
        if (filter) {
            q[5] = g.head_t[pd.hr_lo]; q[6] = g.head_t[pd.hr_hi];
            q[7] = g.tail_h[pd.tr_lo]; q[8] = g.tail_h[pd.tr_hi];
        } else {
            q[5] = (int32_t)pd.h; q[6] = (int32_t)pd.t; q[7] = 0; q[8] = 0;
        }
        *reinterpret_cast<uint64_t *>(q + 10) = pd.s1;
        w.pos[call * bs + b] = make_int4((int)pd.h, (int)pd.r, (int)pd.t, 0);
    }
    __syncthreads();
    const int64_t slots = bs * neg;
    const int64_t E = g.ent_total;
    int32_t *nrec = w.neg + call * slots;
    int32_t *noff = w.off + call * slots;
    // slots o and o + 1024 per iteration (o = b * neg + k, walked with incremental (b, k) instead of a 64-bit
    // division per slot); their runs' boundary searches advance in lock step so both gathers are in
    // flight together. A missing second slot (past the end) draws and writes nothing.
    const int32_t neg32 = (int32_t)neg, db = 1024 / neg32, dk = 1024 - db * neg32;
    int32_t b = tid / neg32, k = tid - b * neg32;
    for (int64_t o = tid; o < slots; o += 2048) {
        int32_t b2 = b + db, k2 = k + dk;
        if (k2 >= neg32) { k2 -= neg32; ++b2; }
        const bool two = o + 1024 < slots;
        SlotDraw d0 = slot_prepare(pi + 12 * b, k, E, filter, g, jt);
        SlotDraw d1 = slot_prepare(pi + 12 * (two ? b2 : b), two ? k2 : k, E, filter, g, jt);
        if (!two) { d1.q.l = 0; d1.q.r = 1; d1.search = false; }   // no second slot: its search stays closed
        slot_search2(d0, d1);
        const int64_t e0 = d0.e;
        nrec[o] = (int32_t)((e0 << 1) | d0.side);
        noff[o] = atomicAdd(&cnt[e0], 1);
        if (two) {
            const int64_t e1 = d1.e;
            nrec[o + 1024] = (int32_t)((e1 << 1) | d1.side);
            noff[o + 1024] = atomicAdd(&cnt[e1], 1);
        }
        b = b2 + db; k = k2 + dk;
        if (k >= neg32) { k -= neg32; ++b; }
    }
    __syncthreads();
    // exclusive scan of cnt[0, n): contiguous chunks per thread, wave shuffles, LDS wave totals
    const int64_t per = (n + 1023) / 1024;
    const int64_t lo = tid * per, hi = lo + per < n ? lo + per : n;
    int32_t tsum = 0;
    for (int64_t i = lo; i < hi; ++i) tsum += cnt[i];
    int32_t incl = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    int32_t run = incl - tsum;
    for (int q = 0; q < wid; ++q) run += wtot[q];
    int32_t *start = w.start + call * w.start_stride;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t c = cnt[i];
        cnt[i] = run;
        start[i] = run;
        run += c;
    }
    if (tid == 1023) start[n] = run;   // the last thread's chunk ends at n (or is empty): run = total
    __syncthreads();
    for (int64_t o = tid; o < slots; o += 1024) noff[o] = cnt[nrec[o] >> 1] + noff[o];
}

// LDS bucket rank of entity e: 16-bit packed counts (two buckets per word; a part never holds 65536
// slots, so a half never carries into the other) or plain 32-bit counts
template <bool PACK>
__device__ __forceinline__ int32_t lds_rank(int32_t *cnt, int64_t e) {
    if constexpr (PACK) {
        const int sh = (int)(e & 1) << 4;
        return (atomicAdd(&cnt[e >> 1], 1 << sh) >> sh) & 0xffff;
    } else {
        return atomicAdd(&cnt[e], 1);
    }
}
template <bool PACK>
__device__ __forceinline__ int32_t lds_bucket(const int32_t *cnt, int64_t e) {
    if constexpr (PACK) return (cnt[e >> 1] >> ((int)(e & 1) << 4)) & 0xffff;
    else return cnt[e];
}

// Split sampling + counting sort: `parts` workgroups per sampled call (grid calls x parts), so a chunk
// of few steps still fills the chip (k_sample_sort runs one workgroup per call). Part p owns positives
// [p*bs/parts, (p+1)*bs/parts) of its call and all their slots. It draws them exactly as k_sample_sort
// does (positives once, per-positive constants in LDS, two slots per thread with lock-step run
// searches) and ranks every slot in an LDS count of its corrupted entity (16-bit packed counts when a
// call has < 65536 slots; the call's global counts are then packed the same way). It then reserves
// each touched bucket's range in the call's global counts with ONE returning atomic per touched count
// word and turns its slots' LDS ranks into ranks inside the call-wide buckets. The part whose ticket add comes last exchanges the global counts with zeros (atomics on
// both sides: every part's adds are seen, and the counts are clear for the next chunk) and scans them
// into start[]; the last call's last part then advances the sampler streams. off[] keeps the ranks
// (CsrWork::rank_only): the step kernel adds start[entity] when it loads a slot's record.
template <int NT, bool PACK, int SL>
__global__ __launch_bounds__(NT) void k_sample_part(DeviceGraph g, uint64_t *__restrict__ states,
                                                    int64_t threads, int64_t bs, int64_t neg, int bern, int filter,
                                                    int64_t parts, CsrWork w) {
    extern __shared__ __attribute__((aligned(16))) int32_t lds[];
    __shared__ int32_t wtot[NT / 64];
    __shared__ int32_t is_last;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t call = blockIdx.x / parts, part = blockIdx.x - call * parts;
    const int64_t b0 = part * bs / parts, b1 = (part + 1) * bs / parts;
    const int64_t E = g.ent_total;
    const int64_t cwords = PACK ? (E + 1) >> 1 : E;
    Affine *jt = reinterpret_cast<Affine *>(lds);        // [jump_tab_len(neg)] jump maps
    int32_t *cnt = lds + 4 * jump_tab_len(neg);
    int32_t *pi = cnt + ((cwords + 3) & ~int64_t(3));    // [b1 - b0][12] positive records (k_sample_sort)
    for (int64_t i = tid; i < cwords; i += NT) cnt[i] = 0;
    jump_tab_fill<NT>(jt, neg, tid);
    const int64_t dpp = 1 + 2 * neg;
    for (int64_t b = b0 + tid; b < b1; b += NT) {
        const PosDraw pd = draw_positive(g, states, threads, bs, b, dpp, call);
        int32_t *q = pi + 12 * (b - b0);
        q[0] = __float_as_int(bern ? g.bern_prob[pd.r] : 500.f);
        q[1] = pd.hr_lo; q[2] = pd.hr_hi; q[3] = pd.tr_lo; q[4] = pd.tr_hi;
        if (filter) {
            q[5] = g.head_t[pd.hr_lo]; q[6] = g.head_t[pd.hr_hi];
            q[7] = g.tail_h[pd.tr_lo]; q[8] = g.tail_h[pd.tr_hi];
        } else {
            q[5] = (int32_t)pd.h; q[6] = (int32_t)pd.t; q[7] = 0; q[8] = 0;
        }
        *reinterpret_cast<uint64_t *>(q + 10) = pd.s1;
        w.pos[call * bs + b] = make_int4((int)pd.h, (int)pd.r, (int)pd.t, 0);
    }
    __syncthreads();
    const int64_t slots = bs * neg;
    int32_t *nrec = w.neg + call * slots;
    int32_t *noff = w.off + call * slots;
    const int64_t o0 = b0 * neg, o1 = b1 * neg;
    // thread tid takes slots o0 + tid + NT*m (m = 0, 1, ...): pairs (o, o + NT) per iteration, (b, k)
    // relative to b0 walked incrementally
    const int32_t neg32 = (int32_t)neg, db = NT / neg32, dk = NT - db * neg32;
    int32_t b = tid / neg32, k = tid - b * neg32;
    // a part of at most SL * NT slots (the usual case) keeps its slots' entities and LDS ranks in registers
    // until the bucket bases are known: one store per slot, no reload
    const bool one = o1 - o0 <= (int64_t)SL * NT;
    int32_t keep_e[SL], keep_r[SL];
#pragma unroll
    for (int i = 0; i < SL; ++i) keep_e[i] = keep_r[i] = 0;
    for (int64_t o = o0 + tid; o < o1; o += SL * NT) {
        // SL slots o + i*NT per iteration, their run searches in lock step; a slot past the end draws nothing
        SlotDraw d[SL];
        int32_t bi = b, ki = k;
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            const bool live = o + i * NT < o1;
            d[i] = slot_prepare(pi + 12 * (live ? bi : b), live ? ki : k, E, filter, g, jt);
            if (!live) { d[i].q.l = 0; d[i].q.r = 1; d[i].search = false; }
            bi += db; ki += dk;
            if (ki >= neg32) { ki -= neg32; ++bi; }
        }
        slot_searchN<SL>(d);
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            if (o + i * NT < o1) {
                nrec[o + i * NT] = (int32_t)((d[i].e << 1) | d[i].side);
                const int32_t r = lds_rank<PACK>(cnt, d[i].e);
                if (one) {
                    keep_e[i] = (int32_t)d[i].e;
                    keep_r[i] = r;
                } else {
                    noff[o + i * NT] = r;
                }
            }
        }
        b = bi; k = ki;
    }
    __syncthreads();
    // reserve this part's range in every touched call-wide bucket with one returning atomic per count
    // word (packed: the call's global counts are packed the same way, each half < 65536, so one add
    // reserves both buckets); the LDS word becomes the bases. Batches of 8 words per thread keep the
    // atomics in flight together (a returned value is only waited for at its LDS write).
    int32_t *gcnt = w.cnt + call * w.cnt_stride;
    for (int64_t i0 = tid; i0 < cwords; i0 += 8 * NT) {
        int32_t v[8], r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int64_t i = i0 + u * NT;
            v[u] = i < cwords ? cnt[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = v[u] ? agent_add(&gcnt[i0 + u * NT], v[u]) : 0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (v[u]) cnt[i0 + u * NT] = r[u];
    }
    __syncthreads();
    // rank inside the call-wide bucket: from registers, or re-read (same thread, same addresses)
    if (one) {
#pragma unroll
        for (int i = 0; i < SL; ++i)
            if (o0 + tid + i * NT < o1) noff[o0 + tid + i * NT] = keep_r[i] + lds_bucket<PACK>(cnt, keep_e[i]);
    } else {
        for (int64_t o = o0 + tid; o < o1; o += NT) noff[o] += lds_bucket<PACK>(cnt, nrec[o] >> 1);
    }
    // every wave's count atomics have returned (their values were used): count this part done. No fence:
    // everything the parts exchange inside this launch is an agent-scope atomic RMW (count words, tickets,
    // the last part's exchanges), performed at the device's coherence point. A part's count adds have
    // returned before the barrier, so they are performed before its ticket add is issued; the last part's
    // exchanges depend on its ticket's returned value, so they are performed after every other part's
    // ticket and therefore after every count add. The plain stores (slot ranks, starts) are read only by
    // later launches. (Measured on the driver's 20-step chunk: thread 0 fencing around the tickets 2.7 ->
    // 3.4-4.1 us per step, every thread fencing 9.5-11.4 us: each fence writes back the XCD's L2.)
    __syncthreads();
    if (tid == 0) is_last = agent_add(&w.tick[call], 1) == (int32_t)(parts - 1);
    __syncthreads();
    if (!is_last) return;
    if (tid == 0) w.tick[call] = 0;   // plain store: read again only by a later launch (kernel boundary)
    // last part: the call's bucket sizes, exchanged with zeros (atomics on both sides: every part's adds
    // are seen, and the counts are clear for the next chunk) into LDS, 8 exchanges in flight per thread
    for (int64_t i0 = tid; i0 < cwords; i0 += 8 * NT) {
        int32_t r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = i0 + u * NT < cwords ? agent_exch(&gcnt[i0 + u * NT], 0) : 0;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u * NT < cwords) cnt[i0 + u * NT] = r[u];
    }
    __syncthreads();
    // exclusive scan over the entities into start[]: contiguous words per thread, wave shuffles, LDS
    // wave totals (k_sample_sort's scan on the packed or plain words)
    int32_t *start = w.start + call * w.start_stride;
    const int64_t per = (cwords + NT - 1) / NT;
    const int64_t lo = tid * per, hi = lo + per < cwords ? lo + per : cwords;
    int32_t tsum = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = cnt[i];
        tsum += PACK ? (v & 0xffff) + (int32_t)((uint32_t)v >> 16) : v;
    }
    int32_t incl = tsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    int32_t run = incl - tsum;
    for (int q = 0; q < wid; ++q) run += wtot[q];
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = cnt[i];
        if constexpr (PACK) {
            start[2 * i] = run;
            run += v & 0xffff;
            if (2 * i + 1 < E) start[2 * i + 1] = run;
            run += (int32_t)((uint32_t)v >> 16);
        } else {
            start[i] = run;
            run += v;
        }
    }
    if (tid == NT - 1) start[E] = run;   // the last thread's chunk ends at the end (or is empty): run = total
    // the last call's last part advances the sampler streams past every call's draws: every part of every
    // call read them (positive draws) before its count atomics and tickets
    __syncthreads();
    if (tid == 0) is_last = agent_add(&w.tick[gridDim.x / parts], 1) == (int32_t)(gridDim.x / parts - 1);
    __syncthreads();
    if (!is_last) return;
    if (tid == 0) w.tick[gridDim.x / parts] = 0;   // plain store: read again only by a later launch
    // plain stores of the advanced states: read only by later launches (every part of this launch read them
    // before its ticket add, which returned before this last part's)
    if (tid < 64) advance_states(states, threads, bs, dpp * (int64_t)(gridDim.x / parts), tid);
}

// exclusive scan of the bucket sizes (one workgroup of 1024 threads, tiles of 16384 counts: 16
// contiguous counts per thread, wave shuffles for the thread totals, LDS for the 16 wave totals),
// zeroing the counts for the next step; also advances the sampler streams by this call's draws
// (the sampling pass was their only reader)
__global__ __launch_bounds__(1024) void k_scan_counts(int32_t *__restrict__ cnt_all, int32_t *__restrict__ start_all,
                                                      int64_t n, uint64_t *states, int64_t threads, int64_t bs,
                                                      int64_t dpp, CsrWork w, int64_t slots) {
    __shared__ int32_t wtot[16];
    __shared__ int32_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // one workgroup per sampled call; workgroup 0 advances the streams by all the calls' draws
    int32_t *cnt = cnt_all + (int64_t)blockIdx.x * ((n + 3) & ~int64_t(3));        // rows padded to 16 B
    int32_t *start = start_all + (int64_t)blockIdx.x * ((n + 4) & ~int64_t(3));
    if (blockIdx.x == 0 && tid < 64 && states) advance_states(states, threads, bs, dpp * (int64_t)gridDim.x, tid);
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 16384) {
        const int64_t lo = base + (int64_t)tid * 16;
        int32_t v[16];
        if (lo + 16 <= n) {
            const int4 *p4 = reinterpret_cast<const int4 *>(cnt + lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int4 x = p4[q];
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) v[q] = lo + q < n ? cnt[lo + q] : 0;
        }
        int32_t tsum = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) tsum += v[q];
        int32_t incl = tsum;   // inclusive wave scan of the thread totals
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wtot[wid] = incl;
        __syncthreads();
        int32_t wpre = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int32_t t = wtot[w];
            wpre += w < wid ? t : 0;
            total += t;
        }
        int32_t run = carry_s + wpre + incl - tsum;
        if (lo + 16 <= n) {
            int32_t o[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                o[q] = run;
                run += v[q];
            }
            int4 *s4 = reinterpret_cast<int4 *>(start + lo);
            int4 *c4 = reinterpret_cast<int4 *>(cnt + lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s4[q] = make_int4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
                c4[q] = make_int4(0, 0, 0, 0);
            }
        } else {
            for (int q = 0; q < 16 && lo + q < n; ++q) {
                start[lo + q] = run;
                run += v[q];
                cnt[lo + q] = 0;
            }
        }
        __syncthreads();
        if (tid == 0) carry_s += total;
        __syncthreads();
    }
    if (tid == 0) start[n] = carry_s;
    __syncthreads();
    // resolve every slot's destination row in the contribution buffer: start[e] + rank (the step kernel
    // then needs no dependent lookup). off[] is overwritten in place by the destination.
    const int32_t *neg = w.neg + (int64_t)blockIdx.x * slots;
    int32_t *off = w.off + (int64_t)blockIdx.x * slots;
    for (int64_t i = tid; i < slots; i += 1024) off[i] = start[neg[i] >> 1] + off[i];
}

// Stored rows for the positives' gradients (one workgroup of 1024 threads per sampled step, all in LDS; reads
// w.pos only, after any of the three samplers). Every positive uses three table rows: entity rows h and t and
// relation row r (row n_ent + r of the combined index). A use's rank in its row is reserved with an LDS atomic;
// the first `cap` uses of a row (ent_cap / rel_cap by table) get a contribution row of their own, the step
// kernel stores the gradient there and the apply pass sums the row's bucket; later uses keep the float atomics
// (pdst -1), so no bucket grows past its cap whatever the graph. The clipped counts are scanned like
// k_scan_counts' (tiles of 16,384: 16 contiguous counts per thread) into pstart[], offset by `base` = the
// negatives' bs * neg rows of the same contribution array.
__global__ __launch_bounds__(1024) void k_pos_slots(CsrWork w, int64_t bs, int32_t base, int32_t n_ent,
                                                    int32_t n_rows, int32_t ent_cap, int32_t rel_cap) {
    extern __shared__ int32_t s_use[];   // [n_rows] uses of a row, then the start of its clipped bucket
    __shared__ int32_t wtot[16];
    __shared__ int32_t carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int4 *pos = w.pos + (int64_t)blockIdx.x * bs;
    int4 *pdst = w.pdst + (int64_t)blockIdx.x * bs;
    int32_t *pstart = w.pstart + (int64_t)blockIdx.x * w.pstart_stride;
    for (int32_t i = tid; i < n_rows; i += 1024) s_use[i] = 0;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    // ---- every use's rank in its row (parked in pdst: the thread that wrote a record reads it back below)
    for (int64_t b = tid; b < bs; b += 1024) {
        const int4 q = pos[b];
        const int32_t kh = atomicAdd(&s_use[q.x], 1);
        const int32_t kr = atomicAdd(&s_use[n_ent + q.y], 1);
        const int32_t kt = atomicAdd(&s_use[q.z], 1);
        pdst[b] = make_int4(kh, kr, kt, 0);
    }
    __syncthreads();
    // ---- exclusive scan of min(uses, cap), in place
    for (int32_t tile = 0; tile < n_rows; tile += 16384) {
        const int32_t lo = tile + tid * 16;
        int32_t v[16];
        int32_t tsum = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int32_t i = lo + q;
            const int32_t cap = i < n_ent ? ent_cap : rel_cap;
            const int32_t c = i < n_rows ? s_use[i] : 0;
            v[q] = c < cap ? c : cap;
            tsum += v[q];
        }
        int32_t incl = tsum;   // inclusive wave scan of the thread totals
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63) wtot[wid] = incl;
        __syncthreads();
        int32_t wpre = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int32_t t = wtot[k];
            wpre += k < wid ? t : 0;
            total += t;
        }
        int32_t run = carry_s + wpre + incl - tsum;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int32_t i = lo + q;
            if (i < n_rows) {
                s_use[i] = run;
                pstart[i] = base + run;
            }
            run += v[q];
        }
        __syncthreads();
        if (tid == 0) carry_s += total;
        __syncthreads();
    }
    if (tid == 0) pstart[n_rows] = base + carry_s;
    // ---- ranks -> contribution rows
    for (int64_t b = tid; b < bs; b += 1024) {
        const int4 q = pos[b];
        const int4 k = pdst[b];
        pdst[b] = make_int4(k.x < ent_cap ? base + s_use[q.x] + k.x : -1,
                            k.y < rel_cap ? base + s_use[n_ent + q.y] + k.y : -1,
                            k.z < ent_cap ? base + s_use[q.z] + k.z : -1, 0);
    }
}

}  // namespace dev

// ==================================================================== host launchers ===========
hipError_t launch_sample(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                         int64_t neg_rel, int mode, int bern, int filter, int64_t *h, int64_t *t, int64_t *r, float *y,
                         hipStream_t st) {
    if (bs <= 0) return hipSuccess;
    const int bl = 256;
    hipLaunchKernelGGL(dev::k_sample, dim3((unsigned)((bs + bl - 1) / bl)), dim3(bl), 0, st, g, states, threads, bs,
                       neg, neg_rel, mode, bern, filter, h, t, r, y);
    return hipGetLastError();
}

hipError_t launch_spin(int64_t us, hipStream_t st) {
    hipLaunchKernelGGL(dev::k_spin, dim3(1), dim3(64), 0, st, us);
    return hipGetLastError();
}

hipError_t launch_advance(uint64_t *states, int64_t threads, int64_t bs, int64_t dpp, hipStream_t st) {
    hipLaunchKernelGGL(dev::k_advance, dim3(1), dim3(64), 0, st, states, threads, bs, dpp);
    return hipGetLastError();
}

hipError_t launch_sample_csr(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                             int bern, int filter, int64_t calls, const CsrWork &w, hipStream_t st) {
    const int64_t n = calls * bs * (neg + 1);
    hipLaunchKernelGGL(dev::k_sample_csr, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, states, threads, bs,
                       neg, bern, filter, calls, w);
    return hipGetLastError();
}

static size_t jump_tab_bytes(int64_t neg) { return 16 * (size_t)(neg < 256 ? neg : 256); }   // kJumpTab
static size_t sample_sort_lds(int64_t bs, int64_t neg, int64_t n) {
    // jump maps + counts + per-positive records
    return jump_tab_bytes(neg) + 4 * (size_t)((n + 3) & ~int64_t(3)) + 48 * (size_t)bs;
}
static const size_t kSampleSortLds = 160 * 1024 - 256;   // leaves room for the static wave totals

bool sample_sort_prepare(int64_t bs, int64_t neg, int64_t n, int64_t start_stride) {
    if (sample_sort_lds(bs, neg, n) > kSampleSortLds || n + 1 > start_stride || n >= (int64_t(1) << 30)) return false;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(dev::k_sample_sort),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSampleSortLds) == hipSuccess;
}

hipError_t launch_sample_sort(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                              int bern, int filter, int64_t calls, int64_t n, const CsrWork &w, hipStream_t st) {
    const size_t lds = sample_sort_lds(bs, neg, n);
    if (lds > kSampleSortLds || n + 1 > w.start_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_sample_sort, dim3((unsigned)calls), dim3(1024), lds, st, g, states, threads, bs, neg,
                       bern, filter, n, w);
    return hipGetLastError();
}

// split sampler: threads per workgroup, LDS plan
static constexpr int kPartNT = 512;
static bool part_pack(int64_t bs, int64_t neg) { return bs * neg < 65536; }
static size_t sample_part_lds(int64_t bs, int64_t neg, int64_t n, int64_t parts) {
    const int64_t cw = part_pack(bs, neg) ? (n + 1) >> 1 : n;
    const int64_t np = (bs + parts - 1) / parts + 1;   // positives of the largest part
    return jump_tab_bytes(neg) + 4 * (size_t)((cw + 3) & ~int64_t(3)) + 48 * (size_t)np;
}

// lock-step slots per thread: 4 when a part holds >= 3 slots per thread, else 2
static int part_sl(int64_t bs, int64_t neg, int64_t parts) {
    const int64_t per = (bs + parts - 1) / parts * neg;
    return per >= 3 * kPartNT ? 4 : 2;
}

template <bool PACK>
static hipError_t part_attr() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dev::k_sample_part<kPartNT, PACK, 2>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSampleSortLds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(dev::k_sample_part<kPartNT, PACK, 4>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSampleSortLds);
}

bool sample_part_fits(int64_t bs, int64_t neg, int64_t n, int64_t parts) {
    return parts >= 1 && parts <= bs && neg >= 1 && sample_part_lds(bs, neg, n, parts) <= kSampleSortLds &&
           n < (int64_t(1) << 30) && bs * neg < (int64_t(1) << 30);
}

bool sample_part_prepare(int64_t bs, int64_t neg, int64_t n, int64_t parts) {
    if (!sample_part_fits(bs, neg, n, parts)) return false;
    return (part_pack(bs, neg) ? part_attr<true>() : part_attr<false>()) == hipSuccess;
}

hipError_t launch_sample_part(const DeviceGraph &g, uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                              int bern, int filter, int64_t calls, int64_t parts, int64_t n, const CsrWork &w,
                              hipStream_t st) {
    if (!sample_part_fits(bs, neg, n, parts) || n + 1 > w.start_stride || n > w.cnt_stride || !w.tick)
        return hipErrorInvalidValue;
    const size_t lds = sample_part_lds(bs, neg, n, parts);
    const dim3 grid((unsigned)(calls * parts));
    const bool pk = part_pack(bs, neg);
    const int sl = part_sl(bs, neg, parts);
#define PT_PART(PK_, SL_)                                                                                          \
    if (pk == PK_ && sl == SL_) {                                                                                  \
        hipLaunchKernelGGL((dev::k_sample_part<kPartNT, PK_, SL_>), grid, dim3(kPartNT), lds, st, g, states, threads, \
                           bs, neg, bern, filter, parts, w);                                                       \
        return hipGetLastError();                                                                                  \
    }
    PT_PART(true, 2) PT_PART(true, 4) PT_PART(false, 2) PT_PART(false, 4)
#undef PT_PART
    return hipErrorInvalidValue;
}

// k_pos_slots keeps one count per entity and relation row in LDS
static size_t pos_slots_lds(int64_t ent_total, int64_t rel_total) { return 4 * (size_t)(ent_total + rel_total); }

bool pos_slots_prepare(int64_t bs, int64_t neg, int64_t ent_total, int64_t rel_total) {
    if (pos_slots_lds(ent_total, rel_total) > kSampleSortLds || csr_con_rows(bs, neg) >= (int64_t(1) << 30)) return false;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(dev::k_pos_slots),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSampleSortLds) == hipSuccess;
}

hipError_t launch_pos_slots(const CsrWork &w, int64_t bs, int64_t neg, int64_t ent_total, int64_t rel_total,
                            int ent_cap, int rel_cap, int64_t calls, hipStream_t st) {
    const size_t lds = pos_slots_lds(ent_total, rel_total);
    if (lds > kSampleSortLds || ent_total + rel_total + 1 > w.pstart_stride || !w.pdst || !w.pstart)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dev::k_pos_slots, dim3((unsigned)calls), dim3(1024), lds, st, w, bs, (int32_t)(bs * neg),
                       (int32_t)ent_total, (int32_t)(ent_total + rel_total), (int32_t)ent_cap, (int32_t)rel_cap);
    return hipGetLastError();
}

hipError_t launch_scan_counts(const CsrWork &w, int64_t n, int64_t calls, uint64_t *states, int64_t threads,
                              int64_t bs, int64_t dpp, hipStream_t st) {
    hipLaunchKernelGGL(dev::k_scan_counts, dim3((unsigned)calls), dim3(1024), 0, st, w.cnt, w.start, n, states, threads,
                       bs, dpp, w, bs * ((dpp - 1) / 2));
    return hipGetLastError();
}

}  // namespace pt

// The single-model trainer runtime of libputranse_hip.so (include/putranse.h: pt_trainer_*): its gradient and
// counting-sort workspaces, the choice of sampling path per chunk, the launch sequence of a run (captured into
// one hipGraph per epoch shape by pt_trainer_run), the measurement hook and the reference-order mode.
#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "common.h"
#include "graph.h"
#include "kernels.h"
#include "ordered.h"
#include "trainer.h"

struct GraphKey {
    const void *sampler, *graph, *losses, *states;
    int64_t bs, neg, bern, filter, steps;
    bool operator<(const GraphKey &o) const {
        return std::tie(sampler, graph, losses, states, bs, neg, bern, filter, steps) <
               std::tie(o.sampler, o.graph, o.losses, o.states, o.bs, o.neg, o.bern, o.filter, o.steps);
    }
};

// uses of a table row by one step's positives that get a stored contribution row (the rest keep the float atomics):
// measured on the fb15k237-shaped graph at batch 2000
static const int32_t kDefaultEntCap = 8, kDefaultRelCap = 32;

struct pt_trainer {
    pt::StepParams P{};
    pt::StepWorkspace W{};
    void *ws_block = nullptr;
    size_t ws_bytes = 0;   // gradient rows + touched flags (all zero between steps)
    // counting-sort gradient path for large neg (allocated on first use, grown as needed)
    void *csr_block = nullptr;
    size_t csr_cap = 0;
    pt::CsrWork csr{};
    int64_t csr_bs = 0, csr_neg = 0, csr_chunk = 0;   // layout the workspace was carved for
    bool csr_fused = false;                             // k_sample_sort plan fits LDS
    bool csr_part = false;                              // k_sample_part prepared (its LDS limit raised)
    int last_path = -1;                                 // sampling path of the last enqueued chunk (PT_PATH_*)
    int64_t lpart_cap = 0;                             // W.lpart capacity (positives)
    int device = -1;
    hipStream_t cap = nullptr;
    std::map<GraphKey, hipGraphExec_t> graphs;
    int path_override = -1;                             // pt_trainer_set_sampling: PT_PATH_* or -1 (automatic)
    int64_t parts_override = 0;                         // split-sampler workgroups per call (0: automatic)
    // stored positive rows (pt_trainer_set_positive_caps): the caps asked for (-1: the library's choice) and whether
    // the carved (bs, neg) takes the stored path at all (k_step_csr + k_apply_buf, k_pos_slots' plan fits LDS)
    int32_t ent_cap_set = -1, rel_cap_set = -1;
    bool pos_stored = false;
    int32_t ent_cap() const { return !pos_stored ? 0 : ent_cap_set < 0 ? kDefaultEntCap : ent_cap_set; }
    int32_t rel_cap() const { return !pos_stored ? 0 : rel_cap_set < 0 ? kDefaultRelCap : rel_cap_set; }
    // reference-order (deterministic) mode: ordered.hip's step on k_sample batches (pt_trainer_set_deterministic)
    bool ordered = false;
    void *ord_block = nullptr;
    size_t ord_cap = 0;
    int64_t *ord_h = nullptr, *ord_t = nullptr, *ord_r = nullptr;
    float *ord_y = nullptr, *ord_score = nullptr, *ord_ds = nullptr;
    float *ord_g = nullptr;   // [4][seq][dim] per-slot gradient rows
    // weighted losses and dense Adam (external batches only): pt_trainer_set_loss / pt_trainer_set_adam
    pt::LossParams loss{};
    pt::AdamParams adam{};
    bool adam_set = false;
    int64_t adam_step = 0;   // steps done
    // DistMult's regularisers (pt_trainer_set_regul) and the Adam pass's per-block sum |x|^3 partials
    pt::RegulParams regul{};
    float *l3part = nullptr;
    // anything the in-kernel-sampled, captured and reference-order paths do not compute
    bool extended() const {
        return !loss.plain() || P.opt == PT_ADAM || P.model == PT_TRANSD || P.model == PT_ROTATE ||
               P.model == PT_DISTMULT || P.model == PT_COMPLEX;
    }
    void drop_graphs() {
        for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
    ~pt_trainer() {
        drop_graphs();
        if (cap) (void)hipStreamDestroy(cap);
        if (ws_block) (void)hipFree(ws_block);
        if (csr_block) (void)hipFree(csr_block);
        if (W.lpart) (void)hipFree(W.lpart);
        if (ord_block) (void)hipFree(ord_block);
        if (l3part) (void)hipFree(l3part);
    }
};

namespace {

// negatives at or above this count take the counting-sort path
bool use_csr(int64_t neg) { return neg >= 4; }

// arguments of in-kernel-sampled steps
int check_step_args(const pt::StepParams &P, pt_sampler *s, int64_t bs, int64_t neg) {
    PT_CHECK(bs > 0 && neg > 0, PT_EINVAL, "batch_size and neg_ent must be positive");
    PT_CHECK(s && s->g && s->d_states, PT_ESTATE, "in-kernel sampling needs a sampler bound to a graph");
    PT_CHECK(s->g->ent_total <= P.ent_total && s->g->rel_total <= P.rel_total, PT_EINVAL,
             "graph ids exceed the model tables");
    PT_CHECK(s->g->ent_total > 1, PT_EINVAL, "graph needs at least two entities");
    pt::StepParams Q = P;
    Q.batch_size = bs;
    PT_CHECK(pt::narrow_dim_supported(P.dim) || pt::step_fits(Q, neg, use_csr(neg)), PT_ENOTSUP,
             "in-kernel sampling at dims above 512 trains TransE with neg_ent >= 4 and tables plus contribution rows "
             "under 2^31 bytes (pt_trainer_fused_supported): train external batches instead");
    PT_CHECK(pt::step_fits(Q, neg, use_csr(neg)), PT_ENOTSUP, "neg_ent too large for the LDS draw buffer");
    return PT_OK;
}

// whether pt_trainer_run takes (bs, neg): the checks it makes on the trainer itself, in its order
bool fused_supported(const pt_trainer *t, int64_t bs, int64_t neg) {
    if (t->extended() || bs <= 0 || neg <= 0) return false;
    if (t->ordered) return true;
    pt::StepParams Q = t->P;
    Q.batch_size = bs;
    return pt::step_fits(Q, neg, use_csr(neg));
}

}  // namespace

extern "C" int pt_trainer_create(const pt_model_desc *m, pt_trainer **out) {
    PT_CHECK(out, PT_EINVAL, "pt_trainer_create: null argument");
    auto t = std::make_unique<pt_trainer>();
    int rc = pt::desc_to_params(m, t->P);
    if (rc) return rc;
    PT_HIP(hipGetDevice(&t->device));
    // (RotatE: gradient rows and flags of the entity table are half rows, 2 * ent_total of them)
    const int64_t E = (m->model == PT_ROTATE ? 2 : 1) * t->P.ent_total, R = t->P.rel_total, D = t->P.dim;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t ge = al(4 * E * D), gr = al(4 * R * D), gn = m->model == PT_TRANSH ? al(4 * R * D) : 0;
    const size_t fe = al(4 * E), fr = al(4 * R), fn = m->model == PT_TRANSH ? al(4 * R) : 0;
    // TransD: gradient rows and flags of ent_transfer / rel_transfer, shaped like ent / rel (ComplEx: of its im tables)
    const bool td = m->model == PT_TRANSD || m->model == PT_COMPLEX;
    const size_t total = ge + gr + gn + fe + fr + fn + (td ? ge + gr + fe + fr : 0);
    PT_HIP(hipMalloc(&t->ws_block, total));
    PT_HIP(hipMemset(t->ws_block, 0, total));
    t->ws_bytes = total;
    char *b = (char *)t->ws_block;
    t->W.gent = (float *)b; b += ge;
    t->W.grel = (float *)b; b += gr;
    t->W.gnorm = gn ? (float *)b : nullptr; b += gn;
    t->W.fent = (int *)b; b += fe;
    t->W.frel = (int *)b; b += fr;
    t->W.fnorm = fn ? (int *)b : nullptr; b += fn;
    if (td) {
        t->W.gentt = (float *)b; b += ge;
        t->W.grelt = (float *)b; b += gr;
        t->W.fentt = (int *)b; b += fe;
        t->W.frelt = (int *)b;
    }
    PT_HIP(hipStreamCreateWithFlags(&t->cap, hipStreamNonBlocking));
    *out = t.release();
    return PT_OK;
}
extern "C" int pt_trainer_free(pt_trainer *t) {
    delete t;
    return PT_OK;
}
extern "C" int pt_trainer_update_desc(pt_trainer *t, const pt_model_desc *m) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    pt::StepParams P{};
    int rc = pt::desc_to_params(m, P);
    if (rc) return rc;
    PT_CHECK(P.model == t->P.model && P.ent_total <= t->P.ent_total && P.rel_total <= t->P.rel_total &&
                 P.dim == t->P.dim,
             PT_EINVAL, "descriptor shape differs from the trainer's workspace");
    t->P = P;
    t->drop_graphs();
    return PT_OK;
}

static const int64_t kCsrChunk = 256;   // steps pre-sampled per sampling/scan launch pair
// the fused sampling kernel runs one workgroup per call (~200 us each at C2, latency-bound draws), so it
// only beats the split form once a chunk fills enough CUs on its own
static const int64_t kSampleSortMinCalls = 96;
// the split sampler (k_sample_part) runs ceil(kPartTarget / calls) workgroups per call
static const int64_t kPartTarget = 512;

// Sampling path for a chunk of `calls` steps: pt_trainer_set_sampling forces one (`forced`, where its plan fits); by
// default the fused kernel for chunks of >= kSampleSortMinCalls steps, the split sampler below that.
static int64_t part_count(const pt_trainer *t, int64_t calls, int64_t bs) {
    int64_t p = t->parts_override > 0 ? t->parts_override : (kPartTarget + calls - 1) / calls;
    if (p < 2) p = 2;
    return p > bs ? bs : p;
}
static int choose_path(const pt_trainer *t, int64_t calls, int64_t bs, int64_t neg, int forced) {
    const bool part_ok = t->csr_part && pt::sample_part_fits(bs, neg, t->P.ent_total, part_count(t, calls, bs));
    if (forced == PT_PATH_FUSED && t->csr_fused) return PT_PATH_FUSED;
    if (forced == PT_PATH_PART && part_ok) return PT_PATH_PART;
    if (forced == PT_PATH_TWO_PASS) return PT_PATH_TWO_PASS;
    if (t->csr_fused && calls >= kSampleSortMinCalls) return PT_PATH_FUSED;
    if (part_ok) return PT_PATH_PART;
    return PT_PATH_TWO_PASS;
}

// Workspace of the counting-sort path, carved once per (bs, neg): room for a chunk of pre-sampled
// steps (<= kCsrChunk, fewer when a step's arrays are large) plus one step's gradient rows. A new
// (bs, neg) re-carves it (and drops captured graphs, whose kernels hold the old pointers).
static int ensure_csr(pt_trainer *t, int64_t bs, int64_t neg) {
    if (t->csr_block && t->csr_bs == bs && t->csr_neg == neg) return PT_OK;
    // ---- sizes: per call the positives, slot records, slot destinations, bucket counts and starts; the
    // chunk's tickets; one step's contribution rows
    const int64_t E = t->P.ent_total, R = t->P.rel_total, D = t->P.dim;
    const int64_t cs = (E + 3) & ~int64_t(3), ss = (E + 4) & ~int64_t(3), ps = (E + R + 4) & ~int64_t(3);
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t per_call = 32 * bs + 8 * bs * neg + 4 * cs + 4 * ss + 4 * ps + 4 + 1024;
    const int64_t chunk = std::min<int64_t>(kCsrChunk, (int64_t)std::max<size_t>(1, ((size_t)512 << 20) / per_call));
    const size_t a_pos = al(16 * bs * chunk), a_neg = al(4 * bs * neg * chunk), a_off = a_neg,
                 a_cnt = al(4 * cs * chunk), a_start = al(4 * ss * chunk), a_tick = al(4 * chunk + 4),
                 a_con = al(4 * pt::csr_con_rows(bs, neg) * D), a_pdst = a_pos, a_pstart = al(4 * ps * chunk);
    const size_t need = a_pos + a_neg + a_off + a_cnt + a_start + a_tick + a_con + a_pdst + a_pstart;
    // ---- (re)allocation
    PT_HIP(hipDeviceSynchronize());   // queued work may still use the old carving
    t->drop_graphs();
    if (need > t->csr_cap) {
        if (t->csr_block) (void)hipFree(t->csr_block);
        t->csr_block = nullptr;
        t->csr_cap = 0;
        PT_HIP(hipMalloc(&t->csr_block, need));
        t->csr_cap = need;
    }
    PT_HIP(hipMemset(t->csr_block, 0, need));   // bucket counts start at zero; the scan re-zeroes them
    // ---- carving
    char *b = (char *)t->csr_block;
    t->csr.pos = (int4 *)b; b += a_pos;
    t->csr.neg = (int32_t *)b; b += a_neg;
    t->csr.off = (int32_t *)b; b += a_off;
    t->csr.cnt = (int32_t *)b; b += a_cnt;
    t->csr.start = (int32_t *)b; b += a_start;
    t->csr.tick = (int32_t *)b; b += a_tick;
    t->csr.contrib = (float *)b; b += a_con;
    t->csr.pdst = (int4 *)b; b += a_pdst;
    t->csr.pstart = (int32_t *)b;
    t->csr.cnt_stride = cs;
    t->csr.start_stride = ss;
    t->csr.pstart_stride = ps;
    // no positive row stored until k_pos_slots says so: every destination -1, every bucket empty
    PT_HIP(hipMemset(t->csr.pdst, 0xff, a_pdst));
    PT_HIP(hipMemsetD32((hipDeviceptr_t)t->csr.pstart, (int)(bs * neg), (size_t)(ps * chunk)));
    t->csr_bs = bs;
    t->csr_neg = neg;
    t->csr_chunk = chunk;
    // ---- LDS plans: sampling + counting sort in LDS (one workgroup per call, or split over parts) when the
    // plans fit (sets the kernels' LDS attributes here, outside any stream capture)
    t->csr_fused = pt::sample_sort_prepare(bs, neg, E, ss);
    t->csr_part = pt::sample_part_prepare(bs, neg, E, std::min<int64_t>(bs, kPartTarget));
    // the stored path is on only where both k_step_csr and k_apply_buf run (decided here, once per carving)
    pt::StepParams Q = t->P;
    Q.batch_size = bs;
    Q.neg = neg;
    t->pos_stored = pt::csr_fast_path(Q) && pt::pos_slots_prepare(bs, neg, E, R);
    return PT_OK;
}

// Launch recorder for the measurement hook: an event pair around every launch, by kernel kind
// (0 sampling, 1 bucket scan, 2 forward/backward, 3 optimizer apply).
struct Timing {
    // events created up front (hipEventCreate between launches would stall the enqueue and let the
    // GPU idle inside a measured interval)
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> ev;
    int reserve(size_t n) {
        pool.resize(n);
        for (auto &e : pool) PT_HIP(hipEventCreate(&e));
        return PT_OK;
    }
    int begin(int kind, hipStream_t st, hipEvent_t *a) {
        if (used >= pool.size()) return pt::fail(PT_EHIP, "timing event pool exhausted");
        *a = pool[used++];
        PT_HIP(hipEventRecord(*a, st));
        ev.emplace_back(kind, *a, nullptr);
        return PT_OK;
    }
    int end(hipStream_t st) {
        if (used >= pool.size()) return pt::fail(PT_EHIP, "timing event pool exhausted");
        hipEvent_t b = pool[used++];
        PT_HIP(hipEventRecord(b, st));
        std::get<2>(ev.back()) = b;
        return PT_OK;
    }
    ~Timing() {
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

#define PT_TIMED(kind, call)                                  \
    do {                                                      \
        hipEvent_t a_;                                        \
        if (tm && tm->begin(kind, st, &a_)) return PT_EHIP;   \
        PT_HIP(call);                                         \
        if (tm && tm->end(st)) return PT_EHIP;                \
    } while (0)

// Sample `calls` consecutive steps into the counting-sort workspace (pos / neg / destination / start,
// calls <= csr_chunk): sampling + counting sort in LDS, one workgroup per call (then the stream advance)
// or split over parts per call (then the destination resolve + stream advance), or the two-pass form
// (global-atomic counts, separate scan) when no LDS plan fits. `forced` = PT_PATH_* or -1 (automatic).
static int enqueue_sample_chunk(pt_trainer *t, pt_sampler *s, pt::CsrWork &w, int64_t bs, int64_t neg,
                                int64_t bern, int64_t filter, int64_t calls, int forced, hipStream_t st, Timing *tm) {
    const pt::DeviceGraph dg = s->g->dev;
    const int64_t dpp = 1 + 2 * neg;
    const int path = choose_path(t, calls, bs, neg, forced);
    t->last_path = path;
    w.rank_only = path == PT_PATH_PART;   // the split sampler leaves bucket ranks (the step resolves them)
    if (path == PT_PATH_FUSED) {
        PT_TIMED(0, pt::launch_sample_sort(dg, s->d_states, s->threads, bs, neg, (int)bern, (int)filter, calls,
                                           t->P.ent_total, w, st));
        PT_TIMED(1, pt::launch_advance(s->d_states, s->threads, bs, dpp * calls, st));
    } else if (path == PT_PATH_PART) {
        const int64_t parts = part_count(t, calls, bs);
        PT_TIMED(0, pt::launch_sample_part(dg, s->d_states, s->threads, bs, neg, (int)bern, (int)filter, calls,
                                           parts, t->P.ent_total, w, st));
    } else {
        PT_TIMED(0, pt::launch_sample_csr(dg, s->d_states, s->threads, bs, neg, (int)bern, (int)filter, calls, w, st));
        PT_TIMED(1, pt::launch_scan_counts(w, t->P.ent_total, calls, s->d_states, s->threads, bs, dpp, st));
    }
    // the positives' stored rows (caps 0 / 0: pdst and pstart stay as ensure_csr left them, all atomic)
    if (t->ent_cap() > 0 || t->rel_cap() > 0)
        PT_TIMED(0, pt::launch_pos_slots(w, bs, neg, t->P.ent_total, t->P.rel_total, t->ent_cap(), t->rel_cap(), calls,
                                         st));
    return PT_OK;
}

// the trainer's step parameters for batches of bs positives x neg negatives
static pt::StepParams batch_params(const pt_trainer *t, int64_t bs, int64_t neg) {
    pt::StepParams P = t->P;
    P.batch_size = bs;
    P.neg = neg;
    P.inv_count = 1.0f / (float)(bs * neg);
    return P;
}

// Enqueue `steps` in-kernel-sampled steps; step i adds its loss to d_losses[i]. Large neg takes the
// counting-sort path: one sampling + one scan launch per chunk of up to kCsrChunk steps (the batch
// stream does not depend on the tables, so it is drawn ahead), then k_step + k_apply per step.
static int enqueue_run(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern, int64_t filter,
                       int64_t steps, float *d_losses, hipStream_t st, Timing *tm = nullptr, bool assign = false) {
    pt::StepParams P = batch_params(t, bs, neg);
    P.loss_assign = assign ? 1 : 0;   // d_losses[i] = step i's loss (no zeroing pass needed)
    const int64_t dpp = 1 + 2 * neg;
    const pt::DeviceGraph dg = s->g->dev;
    if (use_csr(neg)) {
        PT_CHECK(t->csr_block, PT_ESTATE, "counting-sort workspace not allocated");
        const int64_t chunk = t->csr_chunk;
        for (int64_t c0 = 0; c0 < steps; c0 += chunk) {
            const int64_t calls = std::min(chunk, steps - c0);
            // (sets t->csr.rank_only, read by the steps and by pt_trainer_run_timed's re-timing)
            int rc = enqueue_sample_chunk(t, s, t->csr, bs, neg, bern, filter, calls, t->path_override, st, tm);
            if (rc) return rc;
            for (int64_t j = 0; j < calls; ++j) {
                const pt::CsrWork v = pt::csr_view(t->csr, j, bs, neg);
                float *loss = d_losses ? d_losses + c0 + j : nullptr;
                PT_TIMED(2, pt::launch_step(P, dg, s->d_states, s->threads, (int)bern, (int)filter, nullptr, nullptr,
                                            nullptr, t->W, loss, st, &v));
                PT_TIMED(3, pt::launch_apply(P, t->W, nullptr, 0, bs, dpp, loss, st, &v));
            }
        }
    } else {
        t->last_path = PT_PATH_SAMPLED;
        for (int64_t i = 0; i < steps; ++i) {
            float *loss = d_losses ? d_losses + i : nullptr;
            PT_TIMED(2, pt::launch_step(P, dg, s->d_states, s->threads, (int)bern, (int)filter, nullptr, nullptr,
                                        nullptr, t->W, loss, st));
            PT_TIMED(3, pt::launch_apply(P, t->W, s->d_states, s->threads, bs, dpp, loss, st));
        }
    }
    return PT_OK;
}

// One step on an external batch: plain MarginLoss without a model margin -> k_step, any other loss -> k_step_adv;
// SGD / Adagrad -> k_apply, Adam -> k_apply_adam (its step count advances here)
// (ev: optional three events recorded before the step kernel, between the two kernels and after the apply kernel)
static int enqueue_external(pt_trainer *t, int64_t bs, int64_t neg, const int64_t *bh, const int64_t *bt,
                            const int64_t *br, float *d_loss, hipStream_t st, hipEvent_t *ev = nullptr) {
    pt::StepParams P = batch_params(t, bs, neg);
    const bool adam = P.opt == PT_ADAM;
    PT_CHECK(!adam || t->adam_set, PT_ESTATE, "PT_ADAM needs pt_trainer_set_adam before the first step");
    float scale = P.inv_count, cst = P.margin;   // loss = scale * sum(lpart) + cst
    if (ev) PT_HIP(hipEventRecord(ev[0], st));
    const bool complex = P.model == PT_COMPLEX;
    const bool transd = P.model == PT_TRANSD || complex;   // (two optimizer passes: transd_transfer_pass)
    const float l3 = P.model == PT_DISTMULT ? t->regul.l3 : 0.f;
    if (complex) {
        PT_CHECK(t->loss.kind == PT_LOSS_SIGMOID && !t->loss.mflag, PT_ENOTSUP,
                 "PT_COMPLEX trains under PT_LOSS_SIGMOID on the raw score (pt_trainer_set_loss before the first "
                 "step): PT_LOSS_MARGIN and a model margin are not implemented for it");
        PT_CHECK(neg <= pt::step_complex_max_neg(P.dim), PT_ENOTSUP,
                 "neg_ent " + std::to_string(neg) + " too large for the PT_COMPLEX step's LDS score buffer (max " +
                     std::to_string(pt::step_complex_max_neg(P.dim)) + ")");
        pt::loss_affine(t->loss, P, &scale, &cst);
        PT_HIP(pt::launch_step_complex(P, t->loss, t->regul, bh, bt, br, t->W, st));
    } else if (P.model == PT_DISTMULT) {
        PT_CHECK(t->loss.kind == PT_LOSS_SIGMOID && !t->loss.mflag, PT_ENOTSUP,
                 "PT_DISTMULT trains under PT_LOSS_SIGMOID on the raw score (pt_trainer_set_loss before the first "
                 "step): PT_LOSS_MARGIN and a model margin are not implemented for it");
        PT_CHECK(l3 == 0.f || adam, PT_ENOTSUP,
                 "PT_DISTMULT: l3_regul_rate is dense and rides the PT_ADAM pass only (not PT_SGD / PT_ADAGRAD)");
        PT_CHECK(neg <= pt::step_distmult_max_neg(P.dim), PT_ENOTSUP,
                 "neg_ent " + std::to_string(neg) + " too large for the PT_DISTMULT step's LDS score buffer (max " +
                     std::to_string(pt::step_distmult_max_neg(P.dim)) + ")");
        if (l3 != 0.f && !t->l3part)   // (sized by the tables: allocated once)
            PT_HIP(hipMalloc(&t->l3part, sizeof(float) * (size_t)pt::apply_adam_blocks(P)));
        pt::loss_affine(t->loss, P, &scale, &cst);
        PT_HIP(pt::launch_step_distmult(P, t->loss, t->regul, bh, bt, br, t->W, st));
    } else if (P.model == PT_ROTATE) {
        PT_CHECK(t->loss.mflag, PT_ENOTSUP,
                 "PT_ROTATE scores gamma - d: pt_trainer_set_loss with score_margin_flag = 1 and the model's margin "
                 "must come before the first step");
        PT_CHECK(neg <= pt::step_rotate_max_neg(P.dim), PT_ENOTSUP,
                 "neg_ent " + std::to_string(neg) + " too large for the PT_ROTATE step's LDS score buffer (max " +
                     std::to_string(pt::step_rotate_max_neg(P.dim)) + ")");
        pt::loss_affine(t->loss, P, &scale, &cst);
        PT_HIP(pt::launch_step_rotate(P, t->loss, bh, bt, br, t->W, st));
        P = pt::rotate_half_rows(P);   // the optimizer passes see the entity table as half rows
    } else if (P.model == PT_TRANSD) {
        PT_CHECK(t->loss.plain(), PT_ENOTSUP,
                 "SigmoidLoss, adversarial weights and a model margin train TransE only (TransD is not implemented)");
        PT_HIP(pt::launch_step_transd(P, bh, bt, br, t->W, st));
    } else if (t->loss.plain()) {
        PT_HIP(pt::launch_step(P, pt::DeviceGraph{}, nullptr, 0, 0, 0, bh, bt, br, t->W, d_loss, st));
    } else {
        PT_CHECK(P.model == PT_TRANSE, PT_ENOTSUP,
                 "SigmoidLoss, adversarial weights and a model margin train TransE only (TransH is not implemented)");
        PT_CHECK(neg <= pt::step_adv_max_neg(P.dim), PT_ENOTSUP,
                 "neg_ent " + std::to_string(neg) + " too large for the weighted step's LDS score buffer (max " +
                     std::to_string(pt::step_adv_max_neg(P.dim)) + ")");
        pt::loss_affine(t->loss, P, &scale, &cst);
        PT_HIP(pt::launch_step_adv(P, t->loss, bh, bt, br, t->W, st));
    }
    if (ev) PT_HIP(hipEventRecord(ev[1], st));
    if (adam) {
        pt::AdamParams A = t->adam;
        const double step = (double)(t->adam_step + 1);
        A.step_size = (float)((double)P.lr / (1.0 - std::pow(A.beta1, step)));
        A.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(A.beta2, step));
        PT_HIP(pt::launch_apply_adam(P, t->W, A, bs, scale, cst, d_loss, st, l3, t->l3part));
        if (transd) {   // the two transfer tables: a second pass with no loss (transd_transfer_pass)
            pt::StepParams P2;
            pt::StepWorkspace W2;
            pt::transd_transfer_pass(P, t->W, &P2, &W2);
            pt::AdamParams A2 = A;
            A2.m[0] = A.m[3]; A2.m[1] = A.m[4];
            A2.v[0] = A.v[3]; A2.v[1] = A.v[4];
            PT_HIP(pt::launch_apply_adam(P2, W2, A2, bs, 0.f, 0.f, nullptr, st));
        }
        ++t->adam_step;
    } else {
        P.inv_count = scale;   // (the apply pass reads these two for the loss only)
        P.margin = cst;
        PT_HIP(pt::launch_apply(P, t->W, nullptr, 0, bs, 1 + 2 * neg, d_loss, st));
        if (transd) {
            pt::StepParams P2;
            pt::StepWorkspace W2;
            pt::transd_transfer_pass(P, t->W, &P2, &W2);
            PT_HIP(pt::launch_apply(P2, W2, nullptr, 0, bs, 1 + 2 * neg, nullptr, st));
        }
    }
    if (ev) PT_HIP(hipEventRecord(ev[2], st));
    return PT_OK;
}

static const char *kExtendedMsg =
    "a non-default loss (pt_trainer_set_loss), PT_ADAM, PT_TRANSD, PT_ROTATE, PT_DISTMULT and PT_COMPLEX train external "
    "batches only: in-kernel sampling, captured runs and the reference-order mode are not implemented for them";

// per-positive loss partials for batches of up to `bs` positives (grown on demand, never during a
// capture: callers prepare before enqueueing)
static int ensure_lpart(pt_trainer *t, int64_t bs) {
    if (bs <= t->lpart_cap) return PT_OK;
    PT_HIP(hipDeviceSynchronize());   // queued work may still use the old buffer
    t->drop_graphs();
    if (t->W.lpart) (void)hipFree(t->W.lpart);
    t->W.lpart = nullptr;
    t->lpart_cap = 0;
    PT_HIP(hipMalloc(&t->W.lpart, sizeof(float) * (size_t)bs));
    t->lpart_cap = bs;
    return PT_OK;
}

static int prepare_sampled(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg) {
    int rc = check_step_args(t->P, s, bs, neg);
    if (rc) return rc;
    rc = ensure_lpart(t, bs);
    if (rc) return rc;
    rc = s->g->upload();
    if (rc) return rc;
    if (use_csr(neg)) return ensure_csr(t, bs, neg);
    return PT_OK;
}

// ---- reference-order mode (ordered.hip): workspace for batches of up to `seq` slots
static int ensure_ordered(pt_trainer *t, int64_t seq) {
    const int64_t D = t->P.dim;
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t need = 3 * al(8 * seq) + 3 * al(4 * seq) + al(16 * (size_t)seq * D);
    if (need <= t->ord_cap) return PT_OK;
    PT_HIP(hipDeviceSynchronize());   // queued ordered steps may still use the old block
    if (t->ord_block) (void)hipFree(t->ord_block);
    t->ord_block = nullptr;
    t->ord_cap = 0;
    PT_HIP(hipMalloc(&t->ord_block, need));
    t->ord_cap = need;
    char *b = (char *)t->ord_block;
    t->ord_h = (int64_t *)b; b += al(8 * seq);
    t->ord_t = (int64_t *)b; b += al(8 * seq);
    t->ord_r = (int64_t *)b; b += al(8 * seq);
    t->ord_y = (float *)b; b += al(4 * seq);
    t->ord_score = (float *)b; b += al(4 * seq);
    t->ord_ds = (float *)b; b += al(4 * seq);
    t->ord_g = (float *)b;
    return PT_OK;
}

static int enqueue_ordered(pt_trainer *t, int64_t bs, int64_t neg, const int64_t *bh, const int64_t *bt,
                           const int64_t *br, float *loss, int assign, hipStream_t st) {
    const pt::StepParams &P = t->P;
    pt::OrderedStep S{};
    S.model = P.model; S.p_norm = P.p_norm; S.norm_flag = P.norm_flag; S.opt = P.opt;
    S.lr = P.lr; S.margin = P.margin;
    S.ent_total = P.ent_total; S.rel_total = P.rel_total; S.dim = P.dim;
    S.ent = P.ent; S.rel = P.rel; S.normv = P.normv;
    S.ent_acc = P.ent_acc; S.rel_acc = P.rel_acc; S.norm_acc = P.norm_acc;
    S.h = bh; S.t = bt; S.r = br;
    S.bs = bs; S.neg = neg; S.seq = bs * (1 + neg);
    S.score = t->ord_score; S.ds = t->ord_ds;
    S.gh = t->ord_g; S.gt = S.gh + S.seq * P.dim; S.gr = S.gt + S.seq * P.dim; S.gw = S.gr + S.seq * P.dim;
    PT_HIP(pt::launch_ordered_step(S, loss, assign, st));
    return PT_OK;
}

// `steps` sampled steps in reference order: k_sample's batch (bit-identical to sampling()), then the step
static int enqueue_ordered_run(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern, int64_t filter,
                               int64_t steps, float *d_losses, int assign, hipStream_t st) {
    PT_CHECK(s && s->g && s->d_states, PT_ESTATE, "in-kernel sampling needs a sampler bound to a graph");
    PT_CHECK(s->g->ent_total > 1, PT_EINVAL, "graph needs at least two entities");
    PT_CHECK(s->g->ent_total <= t->P.ent_total && s->g->rel_total <= t->P.rel_total, PT_EINVAL,
             "graph ids exceed the model tables");
    int rc = s->g->upload();
    if (rc) return rc;
    rc = ensure_ordered(t, bs * (1 + neg));
    if (rc) return rc;
    t->last_path = -1;
    for (int64_t i = 0; i < steps; ++i) {
        PT_HIP(pt::launch_sample(s->g->dev, s->d_states, s->threads, bs, neg, 0, 0, (int)bern, (int)filter, t->ord_h,
                                 t->ord_t, t->ord_r, t->ord_y, st));
        PT_HIP(pt::launch_advance(s->d_states, s->threads, bs, 1 + 2 * neg, st));
        rc = enqueue_ordered(t, bs, neg, t->ord_h, t->ord_t, t->ord_r, d_losses ? d_losses + i : nullptr, assign, st);
        if (rc) return rc;
    }
    return PT_OK;
}

extern "C" int pt_trainer_set_sampling(pt_trainer *t, int32_t path, int64_t parts) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(path >= -1 && path <= PT_PATH_PART, PT_EINVAL, "sampling path must be -1 or PT_PATH_FUSED/PART/TWO_PASS");
    PT_CHECK(parts >= 0, PT_EINVAL, "parts must be >= 0");
    t->path_override = path;
    t->parts_override = parts;
    t->drop_graphs();   // captured epochs hold the previous choice
    return PT_OK;
}

extern "C" int pt_trainer_set_positive_caps(pt_trainer *t, int32_t ent_cap, int32_t rel_cap) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(ent_cap >= -1 && rel_cap >= -1, PT_EINVAL, "positive caps must be >= 0, or -1 for the library's choice");
    PT_HIP(hipDeviceSynchronize());   // queued work may still read the previous slots
    t->ent_cap_set = ent_cap;
    t->rel_cap_set = rel_cap;
    t->drop_graphs();   // captured epochs hold the previous caps
    t->csr_bs = 0;      // re-carve: pdst / pstart return to "nothing stored"
    return PT_OK;
}
extern "C" int pt_trainer_positive_caps(const pt_trainer *t, int32_t *ent_cap, int32_t *rel_cap) {
    PT_CHECK(t && ent_cap && rel_cap, PT_EINVAL, "pt_trainer_positive_caps: null argument");
    *ent_cap = t->ent_cap_set < 0 ? kDefaultEntCap : t->ent_cap_set;
    *rel_cap = t->rel_cap_set < 0 ? kDefaultRelCap : t->rel_cap_set;
    return PT_OK;
}

extern "C" int pt_trainer_set_deterministic(pt_trainer *t, int32_t on) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(!on || pt::ordered_dim_supported(t->P.dim), PT_ENOTSUP, "reference-order mode: dim too large");
    PT_CHECK(!on || t->P.model != PT_TRANSD, PT_ENOTSUP, "reference-order mode is not implemented for TransD");
    PT_CHECK(!on || t->P.model != PT_ROTATE, PT_ENOTSUP, "reference-order mode is not implemented for PT_ROTATE");
    PT_CHECK(!on || t->P.model != PT_DISTMULT, PT_ENOTSUP, "reference-order mode is not implemented for PT_DISTMULT");
    PT_CHECK(!on || t->P.model != PT_COMPLEX, PT_ENOTSUP, "reference-order mode is not implemented for PT_COMPLEX");
    t->ordered = on != 0;
    return PT_OK;
}
extern "C" int pt_trainer_get_deterministic(const pt_trainer *t) { return t && t->ordered ? 1 : 0; }

extern "C" int pt_trainer_set_loss(pt_trainer *t, const pt_loss_desc *l) {
    PT_CHECK(t && l, PT_EINVAL, "pt_trainer_set_loss: null argument");
    PT_CHECK(l->kind == PT_LOSS_MARGIN || l->kind == PT_LOSS_SIGMOID, PT_EINVAL,
             "loss kind must be PT_LOSS_MARGIN or PT_LOSS_SIGMOID");
    pt::LossParams L{};
    L.kind = l->kind;
    L.adv = l->adv ? 1 : 0;
    L.temp = l->adv ? l->temperature : 0.f;
    L.mflag = l->score_margin_flag ? 1 : 0;
    L.gamma = l->score_margin_flag ? l->score_margin : 0.f;
    PT_CHECK(t->P.model != PT_DISTMULT || (L.kind == PT_LOSS_SIGMOID && !L.mflag), PT_ENOTSUP,
             "PT_DISTMULT trains under PT_LOSS_SIGMOID on the raw score: PT_LOSS_MARGIN and score_margin_flag != 0 are "
             "not implemented for it");
    PT_CHECK(t->P.model != PT_COMPLEX || (L.kind == PT_LOSS_SIGMOID && !L.mflag), PT_ENOTSUP,
             "PT_COMPLEX trains under PT_LOSS_SIGMOID on the raw score: PT_LOSS_MARGIN and score_margin_flag != 0 (a "
             "model margin) are not implemented for it");
    PT_CHECK(L.plain() || t->P.model == PT_TRANSE || t->P.model == PT_ROTATE || t->P.model == PT_DISTMULT ||
                 t->P.model == PT_COMPLEX,
             PT_ENOTSUP,
             "SigmoidLoss, adversarial weights and a model margin train TransE only (TransH is not implemented)");
    t->loss = L;
    return PT_OK;
}

extern "C" int pt_trainer_set_regul(pt_trainer *t, const pt_regul_desc *r) {
    PT_CHECK(t && r, PT_EINVAL, "pt_trainer_set_regul: null argument");
    PT_CHECK(std::isfinite(r->regul_rate) && r->regul_rate >= 0.f && std::isfinite(r->l3_regul_rate) &&
                 r->l3_regul_rate >= 0.f,
             PT_EINVAL, "pt_trainer_set_regul: regul_rate and l3_regul_rate must be finite and >= 0");
    PT_CHECK(r->batch_mode >= 0 && r->batch_mode <= 2, PT_EINVAL,
             "pt_trainer_set_regul: batch_mode must be 0 (normal), 1 (head_batch) or 2 (tail_batch)");
    PT_CHECK(t->P.model != PT_COMPLEX || r->batch_mode == 0, PT_ENOTSUP,
             "PT_COMPLEX takes batch_mode 0 (normal) only: ComplEx.forward ignores the batch mode");
    PT_CHECK(t->P.model != PT_COMPLEX || r->l3_regul_rate == 0.f, PT_ENOTSUP,
             "PT_COMPLEX has no l3 regulariser (ComplEx defines none): l3_regul_rate must be 0");
    PT_CHECK(t->P.model == PT_DISTMULT || t->P.model == PT_COMPLEX ||
                 (r->regul_rate == 0.f && r->l3_regul_rate == 0.f),
             PT_ENOTSUP, "regul_rate trains PT_DISTMULT and PT_COMPLEX only, l3_regul_rate PT_DISTMULT only");
    t->regul.regul = r->regul_rate;
    t->regul.l3 = r->l3_regul_rate;
    t->regul.mode = r->batch_mode;
    return PT_OK;
}

extern "C" int pt_trainer_set_adam(pt_trainer *t, const pt_adam_state *a) {
    PT_CHECK(t && a, PT_EINVAL, "pt_trainer_set_adam: null argument");
    PT_CHECK(a->ent_m && a->ent_v && a->rel_m && a->rel_v && (t->P.model != PT_TRANSH || (a->norm_m && a->norm_v)) &&
                 ((t->P.model != PT_TRANSD && t->P.model != PT_COMPLEX) ||
                  (a->ent_transfer_m && a->ent_transfer_v && a->rel_transfer_m && a->rel_transfer_v)),
             PT_EINVAL, "Adam needs exp_avg and exp_avg_sq buffers for every table");
    PT_CHECK(a->beta1 >= 0. && a->beta1 < 1. && a->beta2 >= 0. && a->beta2 < 1. && a->eps >= 0. && a->step >= 0,
             PT_EINVAL, "Adam: betas must be in [0, 1), eps and step non-negative");
    t->adam.m[0] = a->ent_m; t->adam.m[1] = a->rel_m; t->adam.m[2] = a->norm_m;
    t->adam.v[0] = a->ent_v; t->adam.v[1] = a->rel_v; t->adam.v[2] = a->norm_v;
    // (the appended fields are read for TransD and, as the im tables' moments, for ComplEx only)
    const bool td = t->P.model == PT_TRANSD || t->P.model == PT_COMPLEX;
    t->adam.m[3] = td ? a->ent_transfer_m : nullptr; t->adam.m[4] = td ? a->rel_transfer_m : nullptr;
    t->adam.v[3] = td ? a->ent_transfer_v : nullptr; t->adam.v[4] = td ? a->rel_transfer_v : nullptr;
    t->adam.beta1 = a->beta1; t->adam.beta2 = a->beta2; t->adam.eps = a->eps;
    t->adam_step = a->step;
    t->adam_set = true;
    return PT_OK;
}
extern "C" int64_t pt_trainer_adam_step(const pt_trainer *t) { return t ? t->adam_step : -1; }

extern "C" int pt_trainer_step(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern, int64_t filter,
                               const int64_t *d_bh, const int64_t *d_bt, const int64_t *d_br, float *d_loss,
                               void *stream) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    if (d_bh) {
        PT_CHECK(d_bt && d_br, PT_EINVAL, "external batch needs h, t and r arrays");
        PT_CHECK(bs > 0 && neg > 0, PT_EINVAL, "batch_size and neg_ent must be positive");
        if (t->ordered) {
            PT_CHECK(!t->extended(), PT_ENOTSUP, kExtendedMsg);
            int rc = ensure_ordered(t, bs * (1 + neg));
            if (rc) return rc;
            return enqueue_ordered(t, bs, neg, d_bh, d_bt, d_br, d_loss, 0, (hipStream_t)stream);
        }
        int rc = ensure_lpart(t, bs);
        if (rc) return rc;
        return enqueue_external(t, bs, neg, d_bh, d_bt, d_br, d_loss, (hipStream_t)stream);
    }
    PT_CHECK(bs > 0 && neg > 0, PT_EINVAL, "batch_size and neg_ent must be positive");
    PT_CHECK(!t->extended(), PT_ENOTSUP, kExtendedMsg);
    if (t->ordered) return enqueue_ordered_run(t, s, bs, neg, bern, filter, 1, d_loss, 0, (hipStream_t)stream);
    int rc = prepare_sampled(t, s, bs, neg);
    if (rc) return rc;
    return enqueue_run(t, s, bs, neg, bern, filter, 1, d_loss, (hipStream_t)stream);
}

// Measurement hook of the external-batch step: `steps` steps on one batch, events around both launches of each
extern "C" int pt_trainer_steps_timed(pt_trainer *t, int64_t bs, int64_t neg, const int64_t *d_bh,
                                      const int64_t *d_bt, const int64_t *d_br, int64_t steps, float *d_loss,
                                      float *ms2, void *stream) {
    PT_CHECK(t && d_bh && d_bt && d_br && ms2 && steps > 0, PT_EINVAL, "pt_trainer_steps_timed: bad argument");
    PT_CHECK(bs > 0 && neg > 0, PT_EINVAL, "batch_size and neg_ent must be positive");
    PT_CHECK(!t->ordered, PT_ENOTSUP, "pt_trainer_steps_timed times the fast path (reference-order mode is on)");
    int rc = ensure_lpart(t, bs);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    Timing tm;   // (its pool only: the events are created up front and destroyed with it)
    rc = tm.reserve((size_t)(3 * steps));
    if (rc) return rc;
    PT_HIP(pt::launch_spin(20000, st));   // hold the stream while the host enqueues every launch
    for (int64_t i = 0; i < steps; ++i) {
        rc = enqueue_external(t, bs, neg, d_bh, d_bt, d_br, d_loss, st, &tm.pool[(size_t)(3 * i)]);
        if (rc) {   // the events of the launches already queued are destroyed with `tm`: let them finish first
            (void)hipStreamSynchronize(st);
            return rc;
        }
    }
    PT_HIP(hipStreamSynchronize(st));
    double tot[2] = {0, 0};
    for (int64_t i = 0; i < steps; ++i)
        for (int k = 0; k < 2; ++k) {
            float ms = 0;
            PT_HIP(hipEventElapsedTime(&ms, tm.pool[(size_t)(3 * i + k)], tm.pool[(size_t)(3 * i + k + 1)]));
            tot[k] += ms;
        }
    ms2[0] = (float)(tot[0] / (double)steps);
    ms2[1] = (float)(tot[1] / (double)steps);
    return PT_OK;
}

// `steps` in-kernel-sampled steps launched one by one with an event pair around every launch on
// `stream` (measurement hook for bench.py's roofline). ms4[k] = total duration of kernel kind k
// (0 sampling, 1 bucket scan, 2 forward/backward, 3 optimizer) divided by `steps`. Synchronizes.
extern "C" int pt_trainer_run_timed(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern,
                                    int64_t filter, int64_t steps, float *d_losses, float *ms4, void *stream) {
    PT_CHECK(t && ms4 && steps > 0, PT_EINVAL, "pt_trainer_run_timed: bad argument");
    PT_CHECK(!t->ordered, PT_ENOTSUP, "pt_trainer_run_timed times the fast path (reference-order mode is on)");
    PT_CHECK(!t->extended(), PT_ENOTSUP, kExtendedMsg);
    int rc = prepare_sampled(t, s, bs, neg);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    Timing tm;
    rc = tm.reserve((size_t)(8 * steps + 64));
    if (rc) return rc;
    // hold the stream in a short spin kernel while the host enqueues every measured launch, so each
    // kernel starts as soon as its predecessor ends (no host-side gaps inside an event pair)
    PT_HIP(pt::launch_spin(20000, st));
    rc = enqueue_run(t, s, bs, neg, bern, filter, steps, d_losses, st, &tm, true);
    if (rc) return rc;
    PT_HIP(hipStreamSynchronize(st));
    double tot[4] = {0, 0, 0, 0};
    for (auto &e : tm.ev) {
        float ms = 0;
        PT_HIP(hipEventElapsedTime(&ms, std::get<1>(e), std::get<2>(e)));
        tot[std::get<0>(e)] += ms;
    }
    for (int k = 0; k < 4; ++k) ms4[k] = (float)(tot[k] / (double)steps);
    if (!use_csr(neg)) return PT_OK;
    // Counting-sort path: the per-step kernels are re-timed back to back (as a captured epoch runs
    // them), one event pair per loop instead of one per launch, on the last pre-sampled batch:
    //   loop 1: `steps` x (forward/backward, apply)  -> T_sa;   loop 2: `steps` x forward/backward -> T_s
    // ms4[2] = T_s / steps, ms4[3] = (T_sa - T_s) / steps. The tables, Adagrad state, gradient rows and
    // flags are restored afterwards, so training state is exactly as the measured run left it.
    pt::StepParams P = batch_params(t, bs, neg);
    const int64_t E = P.ent_total, R = P.rel_total, D = P.dim, dpp = 1 + 2 * neg;
    std::vector<std::pair<float *, size_t>> keep = {{P.ent, 4 * E * D}, {P.rel, 4 * R * D}};
    if (P.normv) keep.push_back({P.normv, 4 * R * D});
    if (P.opt != 0) {
        keep.push_back({P.ent_acc, 4 * E * D});
        keep.push_back({P.rel_acc, 4 * R * D});
        if (P.norm_acc) keep.push_back({P.norm_acc, 4 * R * D});
    }
    size_t nb = 0;
    for (auto &k : keep) nb += k.second;
    char *bak = nullptr;
    PT_HIP(hipMalloc(&bak, nb));
    size_t off = 0;
    for (auto &k : keep) {
        PT_HIP(hipMemcpyAsync(bak + off, k.first, k.second, hipMemcpyDeviceToDevice, st));
        off += k.second;
    }
    const pt::DeviceGraph dg = s->g->dev;
    const pt::CsrWork v = pt::csr_view(t->csr, 0, bs, neg);
    hipEvent_t ev[4] = {tm.pool[0], tm.pool[1], tm.pool[2], tm.pool[3]};
    int erc = PT_OK;
    if (pt::launch_spin(20000, st) != hipSuccess || hipEventRecord(ev[0], st) != hipSuccess) erc = PT_EHIP;
    for (int64_t i = 0; i < steps && !erc; ++i) {
        if (pt::launch_step(P, dg, s->d_states, s->threads, (int)bern, (int)filter, nullptr, nullptr, nullptr, t->W,
                            nullptr, st, &v) != hipSuccess ||
            pt::launch_apply(P, t->W, nullptr, 0, bs, dpp, nullptr, st, &v) != hipSuccess)
            erc = PT_EHIP;
    }
    if (!erc && (hipEventRecord(ev[1], st) != hipSuccess || pt::launch_spin(20000, st) != hipSuccess ||
                 hipEventRecord(ev[2], st) != hipSuccess))
        erc = PT_EHIP;
    for (int64_t i = 0; i < steps && !erc; ++i) {
        if (pt::launch_step(P, dg, s->d_states, s->threads, (int)bern, (int)filter, nullptr, nullptr, nullptr, t->W,
                            nullptr, st, &v) != hipSuccess)
            erc = PT_EHIP;
    }
    if (!erc && hipEventRecord(ev[3], st) != hipSuccess) erc = PT_EHIP;
    // restore
    off = 0;
    for (auto &k : keep) {
        if (hipMemcpyAsync(k.first, bak + off, k.second, hipMemcpyDeviceToDevice, st) != hipSuccess) erc = PT_EHIP;
        off += k.second;
    }
    if (hipMemsetAsync(t->ws_block, 0, t->ws_bytes, st) != hipSuccess) erc = PT_EHIP;
    const hipError_t se = hipStreamSynchronize(st);
    (void)hipFree(bak);
    if (erc) return pt::fail(erc, "pt_trainer_run_timed: isolation timing launch failed");
    PT_HIP(se);
    float t_sa = 0, t_s = 0;
    PT_HIP(hipEventElapsedTime(&t_sa, ev[0], ev[1]));
    PT_HIP(hipEventElapsedTime(&t_s, ev[2], ev[3]));
    ms4[2] = t_s / (float)steps;
    ms4[3] = (t_sa - t_s) / (float)steps;
    return PT_OK;
}

// Shims of the removed fused step + apply, slot-scale mode and two-launch split sampling (opt-in modes measured
// slower), kept for callers that switch them off or ask whether they ran: off (0; for the split also
// -1, its former automatic) is accepted, on is PT_ENOTSUP, and the getters report 0
extern "C" int pt_trainer_set_step_apply(pt_trainer *t, int32_t on) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(!on, PT_ENOTSUP,
             "pt_trainer_set_step_apply: the fused step + apply was removed (measured slower, DESIGN.md §4)");
    return PT_OK;
}
extern "C" int pt_trainer_step_apply(const pt_trainer *) { return 0; }

extern "C" int pt_trainer_set_slot_scale(pt_trainer *t, int32_t on) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(!on, PT_ENOTSUP,
             "pt_trainer_set_slot_scale: the slot-scale mode was removed (measured slower, DESIGN.md §4)");
    return PT_OK;
}
extern "C" int pt_trainer_slot_scale(const pt_trainer *) { return 0; }

extern "C" int pt_trainer_set_sample_split(pt_trainer *t, int64_t head) {
    PT_CHECK(t, PT_EINVAL, "null trainer");
    PT_CHECK(head >= -1, PT_EINVAL, "head must be >= -1");
    PT_CHECK(head <= 0, PT_ENOTSUP,
             "pt_trainer_set_sample_split: the two-launch split sampling was removed (measured slower, DESIGN.md §4)");
    return PT_OK;
}

extern "C" int pt_trainer_last_path(const pt_trainer *t) { return t ? t->last_path : -1; }

extern "C" int pt_trainer_sample_csr(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern,
                                     int64_t filter, int64_t calls, int32_t path, int32_t *h_pos, int32_t *h_neg,
                                     int32_t *h_dst, int32_t *h_start, void *stream) {
    PT_CHECK(t && s && h_pos && h_neg && h_dst && h_start, PT_EINVAL, "pt_trainer_sample_csr: null argument");
    PT_CHECK(calls > 0, PT_EINVAL, "pt_trainer_sample_csr: calls must be positive");
    PT_CHECK(path >= -1 && path <= PT_PATH_PART, PT_EINVAL, "pt_trainer_sample_csr: path must be -1 or PT_PATH_*");
    int rc = prepare_sampled(t, s, bs, neg);
    if (rc) return rc;
    if (!t->csr_block) {   // small neg runs the in-step sampler; carve the counting-sort workspace anyway
        rc = ensure_csr(t, bs, neg);
        if (rc) return rc;
    }
    PT_CHECK(calls <= t->csr_chunk, PT_EINVAL, "pt_trainer_sample_csr: calls exceeds the workspace chunk");
    if (path == PT_PATH_FUSED) PT_CHECK(t->csr_fused, PT_ENOTSUP, "fused sampling plan does not fit LDS");
    if (path == PT_PATH_PART)
        PT_CHECK(t->csr_part && pt::sample_part_fits(bs, neg, t->P.ent_total, part_count(t, calls, bs)), PT_ENOTSUP,
                 "split sampling plan does not fit LDS");
    hipStream_t st = (hipStream_t)stream;
    rc = enqueue_sample_chunk(t, s, t->csr, bs, neg, bern, filter, calls, path, st, nullptr);
    if (rc) return rc;
    const pt::CsrWork &w = t->csr;
    const int64_t E = t->P.ent_total, slots = bs * neg;
    std::vector<int4> pos((size_t)(calls * bs));
    PT_HIP(hipMemcpyAsync(pos.data(), w.pos, sizeof(int4) * pos.size(), hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(h_neg, w.neg, 4 * (size_t)(calls * slots), hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpyAsync(h_dst, w.off, 4 * (size_t)(calls * slots), hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpy2DAsync(h_start, 4 * (size_t)(E + 1), w.start, 4 * (size_t)w.start_stride, 4 * (size_t)(E + 1),
                            (size_t)calls, hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st));
    if (w.rank_only)   // split sampler: ranks inside the buckets -> destination rows
        for (int64_t c = 0; c < calls; ++c)
            for (int64_t o = 0; o < slots; ++o)
                h_dst[c * slots + o] += h_start[c * (E + 1) + (h_neg[c * slots + o] >> 1)];
    for (size_t i = 0; i < pos.size(); ++i) {
        h_pos[3 * i] = pos[i].x;
        h_pos[3 * i + 1] = pos[i].y;
        h_pos[3 * i + 2] = pos[i].z;
    }
    return PT_OK;
}

extern "C" int pt_trainer_positive_slots(pt_trainer *t, int64_t calls, int32_t *h_pdst, int32_t *h_pstart,
                                         int32_t *stored, void *stream) {
    PT_CHECK(t && h_pdst && h_pstart && stored, PT_EINVAL, "pt_trainer_positive_slots: null argument");
    PT_CHECK(t->csr_block && calls > 0 && calls <= t->csr_chunk, PT_ESTATE,
             "pt_trainer_positive_slots: no sampled chunk of that many calls (pt_trainer_sample_csr first)");
    hipStream_t st = (hipStream_t)stream;
    const pt::CsrWork &w = t->csr;
    const int64_t bs = t->csr_bs, n = t->P.ent_total + t->P.rel_total + 1;
    std::vector<int4> d((size_t)(calls * bs));
    PT_HIP(hipMemcpyAsync(d.data(), w.pdst, sizeof(int4) * d.size(), hipMemcpyDeviceToHost, st));
    PT_HIP(hipMemcpy2DAsync(h_pstart, 4 * (size_t)n, w.pstart, 4 * (size_t)w.pstart_stride, 4 * (size_t)n, (size_t)calls,
                            hipMemcpyDeviceToHost, st));
    PT_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < d.size(); ++i) {
        h_pdst[3 * i] = d[i].x;
        h_pdst[3 * i + 1] = d[i].y;
        h_pdst[3 * i + 2] = d[i].z;
    }
    *stored = t->pos_stored ? 1 : 0;
    return PT_OK;
}

extern "C" int pt_trainer_fused_supported(const pt_trainer *t, int64_t bs, int64_t neg) {
    return t && fused_supported(t, bs, neg) ? 1 : 0;
}

extern "C" int pt_trainer_run(pt_trainer *t, pt_sampler *s, int64_t bs, int64_t neg, int64_t bern, int64_t filter,
                              int64_t steps, float *d_losses, void *stream) {
    PT_CHECK(t && d_losses, PT_EINVAL, "pt_trainer_run: null argument");
    PT_CHECK(steps > 0, PT_EINVAL, "steps must be positive");
    PT_CHECK(!t->extended(), PT_ENOTSUP, kExtendedMsg);
    if (t->ordered) {
        PT_CHECK(bs > 0 && neg > 0, PT_EINVAL, "batch_size and neg_ent must be positive");
        return enqueue_ordered_run(t, s, bs, neg, bern, filter, steps, d_losses, 1, (hipStream_t)stream);
    }
    int rc = prepare_sampled(t, s, bs, neg);
    if (rc) return rc;
    GraphKey key{s, s->g->dev.rec, d_losses, s->d_states, bs, neg, bern, filter, steps};
    auto it = t->graphs.find(key);
    if (it == t->graphs.end()) {
        hipGraph_t graph;
        PT_HIP(hipStreamBeginCapture(t->cap, hipStreamCaptureModeThreadLocal));
        int erc = PT_OK;
        erc = enqueue_run(t, s, bs, neg, bern, filter, steps, d_losses, t->cap, nullptr, true);
        hipError_t ce = hipStreamEndCapture(t->cap, &graph);
        if (erc) return erc;
        PT_HIP(ce);
        hipGraphExec_t exec;
        hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        PT_HIP(ie);
        it = t->graphs.emplace(key, exec).first;
    }
    PT_HIP(hipGraphLaunch(it->second, (hipStream_t)stream));
    return PT_OK;
}

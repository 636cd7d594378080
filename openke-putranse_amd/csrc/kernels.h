// Host-side launch interface of the HIP kernels (kernels.hip and the other .hip files).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "graph.h"

namespace pt {

struct StepParams {
    int model, p_norm, norm_flag, opt;
    float lr, margin;
    int64_t ent_total, rel_total, dim;
    float *ent, *rel, *normv;
    float *ent_acc, *rel_acc, *norm_acc;
    int64_t batch_size, neg;
    float inv_count;   // 1 / (batch_size * neg)
    int loss_assign = 0;   // the apply pass stores the step's loss (=) instead of adding it (+=)
    // TransD (model 2): ent_transfer / rel_transfer and their Adagrad state; ComplEx (model 5): ent_im / rel_im and
    // theirs (appended: the fields above keep their places in the argument blocks of the TransE / TransH kernels)
    float *ent_t = nullptr, *rel_t = nullptr;
    float *ent_t_acc = nullptr, *rel_t_acc = nullptr;
    // RotatE (model 3): an entity row holds 2 * dim floats (re | im), a relation row dim phases; phase = r / phase_div
    float phase_div = 0.f;
};

struct StepWorkspace {
    float *gent = nullptr, *grel = nullptr, *gnorm = nullptr;   // gradient rows (zero between steps)
    int *fent = nullptr, *frel = nullptr, *fnorm = nullptr;      // touched-row flags
    // per-positive loss partials [batch]: sum over the positive's negatives of max(p - n, -m); the apply
    // pass reduces them in a fixed order into the step's loss (one same-address float atomic per
    // positive serialises at the memory side: it cost ~13 us per C2 step)
    float *lpart = nullptr;
    // TransD: gradient rows and touched flags of ent_transfer / rel_transfer
    float *gentt = nullptr, *grelt = nullptr;
    int *fentt = nullptr, *frelt = nullptr;
};

// Workspace of the counting-sort (CSR) gradient path for large neg (see k_sample_csr). The sampling
// and scan passes fill `calls` consecutive steps at once (pos/neg/off/cnt/start are [calls][...]);
// a per-step view (csr_view) offsets the pointers to one step.
struct CsrWork {
    int4 *pos = nullptr;        // [calls][bs] (h, r, t, -)
    int32_t *neg = nullptr;     // [calls][bs*neg] entity << 1 | tail_side
    int32_t *off = nullptr;     // [calls][bs*neg] destination row of the slot in the counting-sort order
                                // (rank_only: its rank inside the entity's bucket; the step adds start[e])
    int32_t *cnt = nullptr;     // [calls][cnt_stride] bucket sizes (zero between uses)
    int32_t *start = nullptr;   // [calls][start_stride] exclusive prefix of cnt (E+1 used)
    float *contrib = nullptr;   // [bs*neg][dim] gradient rows of the corrupted entities (one step)
    int32_t *tick = nullptr;    // [calls + 1] parts of a call done, then calls done (k_sample_part; zero between uses)
    int rank_only = 0;          // off[] holds bucket ranks (k_sample_part) instead of destinations
    int64_t cnt_stride = 0, start_stride = 0;
    // stored positive rows (k_pos_slots): the first `cap` uses of a table row by a step's positives get a row of
    // `contrib` after the bs*neg rows of the negatives; later uses keep the float atomics
    int4 *pdst = nullptr;       // [calls][bs] contrib rows of the positive's (h, r, t) gradients, -1 = atomic path
    int32_t *pstart = nullptr;  // [calls][pstart_stride] starts of the rows' clipped buckets: entity e at [e],
                                // relation r at [ent_total + r]; ent_total + rel_total + 1 used
    int64_t pstart_stride = 0;
};

inline CsrWork csr_view(const CsrWork &w, int64_t call, int64_t bs, int64_t neg) {
    CsrWork v = w;
    v.pos = w.pos + call * bs;
    v.neg = w.neg + call * bs * neg;
    v.off = w.off + call * bs * neg;
    v.cnt = w.cnt + call * w.cnt_stride;
    v.start = w.start + call * w.start_stride;
    v.pdst = w.pdst + call * bs;
    v.pstart = w.pstart + call * w.pstart_stride;
    return v;
}

struct LpUniverseDev {
    const float *ent, *rel, *normv;
    const int64_t *remap;   // local -> global entity
    int64_t ent_total, dim;
};

struct LpPair {
    int32_t key, universe, anchor, rel, side;   // local anchor entity / relation ids
};

// Lane-group shape of a row of D floats. Tables are row-major fp32 [rows][dim]. A "lane group" of G lanes (G | 64,
// a power of two) owns one row-sized vector: lane l holds chunks c = k*G + l (k < KCH) of VEC consecutive floats,
// so a row is read with fully coalesced 16-B (VEC=4) or 4-B (VEC=1) accesses and every reduction is a shuffle
// butterfly inside the group.
struct Shape {
    int G, VEC, KCH;
};

// The shape of a dim-D row: float4 chunks when vec4 and D % 4 == 0, else single floats. For D % 4 == 0 this is
// G = the smallest power of two in [2, 64] that is >= D / 4 (64 beyond), KCH = ceil(D / 4 / G): the rule of the
// float4-only kernels (k_step_csr, k_apply_buf), which therefore take pick_shape(D) as it is.
constexpr Shape pick_shape(int64_t D, bool vec4 = true) {
    const int VEC = vec4 && D % 4 == 0 ? 4 : 1;
    const int64_t chunks = D / VEC;
    int G = 1;
    while (G < chunks && G < 64) G <<= 1;
    if (G < 2) G = 2;
    int KCH = (int)((chunks + G - 1) / G);
    if (VEC == 1) {   // VEC=1 instantiations exist for power-of-two chunk counts
        int k = 1;
        while (k < KCH) k <<= 1;
        KCH = k;
    }
    return Shape{G, VEC, KCH};
}

// instantiated (G, VEC, KCH) row shapes: float4 rows up to dim 1,024 (KCH 3 and 4: dims 516..1,024, TransE and TransH
// RotatE, DistMult and ComplEx single models only; model_dim_supported is the rule), one-float rows up to dim 512
#define PT_SHAPES(X)                                                                                  \
    X(2, 4, 1) X(4, 4, 1) X(8, 4, 1) X(16, 4, 1) X(32, 4, 1) X(64, 4, 1) X(64, 4, 2) X(64, 4, 3)     \
    X(64, 4, 4)                                                                                       \
    X(2, 1, 1) X(4, 1, 1) X(8, 1, 1) X(16, 1, 1) X(32, 1, 1) X(64, 1, 1) X(64, 1, 2) X(64, 1, 4)    \
    X(64, 1, 8)

// Run-time values to template arguments, for the launchers: for_shape calls f(ShapeTag<G, VEC, KCH>{}) for the
// PT_SHAPES entry equal to s, for_value<Vs...> calls f(std::integral_constant<int, V>{}) for the V equal to v
// (model 0/1, p_norm 1/2, booleans, ...); both return whether one matched. f is a generic lambda that names the
// kernel instance from its argument's type; a kernel with float4 rows only filters with if constexpr (T::VEC == 4).
template <int G_, int VEC_, int KCH_>
struct ShapeTag {
    static constexpr int G = G_, VEC = VEC_, KCH = KCH_;
};
template <typename F>
constexpr bool for_shape(const Shape &s, F &&f) {
#define PT_FOR_SHAPE(G_, V_, K_)                    \
    if (s.G == G_ && s.VEC == V_ && s.KCH == K_) { \
        f(ShapeTag<G_, V_, K_>{});                  \
        return true;                                \
    }
    PT_SHAPES(PT_FOR_SHAPE)
#undef PT_FOR_SHAPE
    return false;
}
template <int... Vs, typename F>
constexpr bool for_value(int v, F &&f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- kernels.hip: the dim rule and the score kernels
// The one dim rule of the single-model path (pt_model_dim_supported answers it for models 0-2): dims 1..512 for every model (both row layouts
// exist), dims 516..1,024 in multiples of 4 (float4 rows only) for TransE (0), TransH (1), RotatE (3), DistMult (4)
// and ComplEx (5); nothing else. RotatE's dim is its relation row's: an entity row is two such rows, re | im; ComplEx's
// is the row length of one of its four tables
bool model_dim_supported(int64_t dim, int model);
// dims at which both row layouts exist (1..512): what the one-float kernels (k_step_sampled, k_lp_scan_t's tile) take
bool narrow_dim_supported(int64_t dim);
hipError_t launch_score(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r, int64_t n,
                        float *out, hipStream_t st);
hipError_t launch_score_queries(const StepParams &P, int side, const int64_t *qh, const int64_t *qt, const int64_t *qr,
                                int64_t nq, int64_t E, float *out, hipStream_t st, int global_order = 0);
// ---- lp.hip: universe link prediction
// pairs sorted by universe; universe u's pairs are pairs[uoff[2u] .. uoff[2u+1]); uids = the n_active universes with
// pairs, all of dims that take dim's lane-group shape (pick_shape); base / normal: scratch [n_pairs][ds >= every dim]
hipError_t launch_lp_min(const LpUniverseDev *us, const LpPair *pairs, int64_t n_pairs, const int64_t *uoff,
                         const int32_t *uids, int64_t n_active, int64_t dim, int64_t max_ent, int model, int p_norm,
                         int norm_flag, int64_t global_E, int64_t ds, float *base, float *normal, float *rows,
                         float *tuple_min, hipStream_t st);
// ---- sample.hip: the batch samplers
hipError_t launch_sample(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                         int64_t neg_rel, int mode, int bern, int filter, int64_t *h, int64_t *t, int64_t *r, float *y,
                         hipStream_t st);
hipError_t launch_spin(int64_t us, hipStream_t st);
hipError_t launch_advance(uint64_t *states, int64_t threads, int64_t bs, int64_t dpp, hipStream_t st);
hipError_t launch_sample_csr(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                             int bern, int filter, int64_t calls, const CsrWork &w, hipStream_t st);
// one workgroup per call: sampling + LDS counting sort + scan; the streams are NOT advanced (launch_advance)
hipError_t launch_sample_sort(const DeviceGraph &g, const uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                              int bern, int filter, int64_t calls, int64_t n, const CsrWork &w, hipStream_t st);
// `parts` workgroups per call: sampling + LDS counting sort of each part, call-wide buckets reserved with one atomic
// per touched count word, the last part of a call scans, the last call advances the streams; off[] holds bucket
// ranks (the caller sets CsrWork::rank_only for the step kernels)
hipError_t launch_sample_part(const DeviceGraph &g, uint64_t *states, int64_t threads, int64_t bs, int64_t neg,
                              int bern, int filter, int64_t calls, int64_t parts, int64_t n, const CsrWork &w,
                              hipStream_t st);
// whether a kernel's LDS plan fits (sample_part_fits: with `parts` parts per call); the *_prepare forms also raise the
// kernel's LDS limit (call outside any stream capture). Where neither fits: launch_sample_csr + launch_scan_counts
bool sample_sort_prepare(int64_t bs, int64_t neg, int64_t n, int64_t start_stride);
bool sample_part_fits(int64_t bs, int64_t neg, int64_t n, int64_t parts);
bool sample_part_prepare(int64_t bs, int64_t neg, int64_t n, int64_t parts);
hipError_t launch_scan_counts(const CsrWork &w, int64_t n, int64_t calls, uint64_t *states, int64_t threads,
                              int64_t bs, int64_t dpp, hipStream_t st);
// the positives' stored gradient rows of `calls` steps (k_pos_slots, one workgroup per step): counts every row's uses
// by the step's positives in LDS, clips them at ent_cap / rel_cap and writes pdst / pstart; reads w.pos only.
// pos_slots_prepare: whether its LDS plan fits (raises the kernel's LDS limit: call outside any stream capture)
bool pos_slots_prepare(int64_t bs, int64_t neg, int64_t ent_total, int64_t rel_total);
hipError_t launch_pos_slots(const CsrWork &w, int64_t bs, int64_t neg, int64_t ent_total, int64_t rel_total,
                            int ent_cap, int rel_cap, int64_t calls, hipStream_t st);
// the raw-buffer kernels (k_step_csr, k_apply_buf) address the ent / rel tables and con_rows contribution rows with
// byte offsets that must fit 31 bits
inline bool offsets_fit31(const StepParams &P, int64_t con_rows) {
    return (P.ent_total + P.rel_total + con_rows) * P.dim * 4 < (int64_t(1) << 31);
}
// contribution rows of a counting-sort step: one per negative slot and three per positive (CsrWork::pdst)
inline int64_t csr_con_rows(int64_t bs, int64_t neg) { return bs * (neg + 3); }
// whether launch_step takes k_step_csr on a counting-sort batch (then launch_apply takes k_apply_buf)
bool csr_fast_path(const StepParams &P);
bool step_fits(const StepParams &P, int64_t neg, bool csr);
hipError_t launch_step(const StepParams &P, const DeviceGraph &g, const uint64_t *states, int64_t threads, int bern,
                       int filter, const int64_t *bh, const int64_t *bt, const int64_t *br, const StepWorkspace &W,
                       float *loss, hipStream_t st, const CsrWork *csr = nullptr);
hipError_t launch_apply(const StepParams &P, const StepWorkspace &W, uint64_t *states, int64_t threads, int64_t bs,
                        int64_t dpp, float *loss, hipStream_t st, const CsrWork *csr = nullptr);
// Loss of the weighted external-batch step (step_adv.hip; pt_loss_desc): kind 0 MarginLoss (margin = StepParams::
// margin), 1 SigmoidLoss; adv = self-adversarial weights softmax(+-temp * n) over a positive's negatives (else 1/K);
// mflag = the model's own margin: the score handed to the loss is gamma - d instead of d
struct LossParams {
    int kind = 0, adv = 0;
    float temp = 0.f;
    int mflag = 0;
    float gamma = 0.f;
    bool plain() const { return kind == 0 && !adv && !mflag; }
};
// lpart[b] of k_step_adv sums to the step's loss as scale * sum + cst
inline void loss_affine(const LossParams &L, const StepParams &P, float *scale, float *cst) {
    *scale = L.kind == 1 ? -0.5f / (float)P.batch_size : 1.0f / (float)P.batch_size;
    *cst = L.kind == 1 ? 0.f : P.margin;
}
// dense Adam (adam.hip; pt_adam_state): m / v per table, the step's bias corrections computed on the host in double
struct AdamParams {
    // tables 0-2: ent, rel, norm_vector; 3-4: TransD's ent_transfer, rel_transfer (ComplEx's ent_im, rel_im)
    float *m[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;   // (1 - beta in double: 1.0f - 0.999f is 1.3e-5 off 0.001)
    float step_size = 0.f;   // lr / (1 - beta1^t)
    float bc2_sqrt = 1.f;    // sqrt(1 - beta2^t)
};
// largest neg k_step_adv takes at this dim (a lane group's scores and its transpose row sit in LDS)
int64_t step_adv_max_neg(int64_t dim);
hipError_t launch_step_adv(const StepParams &P, const LossParams &L, const int64_t *bh, const int64_t *bt,
                           const int64_t *br, const StepWorkspace &W, hipStream_t st);
// every row of every table: gradient row (flagged rows only) -> normalize Jacobian -> Adam; block 0 reduces the
// loss partials: loss (+)= loss_scale * sum(lpart) + loss_cst
// l3 != 0 (DistMult's l3_regul_rate): 3 l3 x |x| joins every row's gradient and a second, one-block launch adds
// l3 * sum |x|^3 over the pre-step tables to the loss from the per-block partials l3part[apply_adam_blocks(P)]
hipError_t launch_apply_adam(const StepParams &P, const StepWorkspace &W, const AdamParams &A, int64_t bs,
                             float loss_scale, float loss_cst, float *loss, hipStream_t st, float l3 = 0.f,
                             float *l3part = nullptr);
int64_t apply_adam_blocks(const StepParams &P);
// TransD (transd.hip): the external-batch step under plain MarginLoss (entity and transfer gradients finished in the
// kernel, the relation's left in normalised space), and the scores; launch_score / launch_score_queries route model 2
// to the latter two. The optimizer pass runs twice for TransD: (ent, rel), then transd_transfer_pass's view
hipError_t launch_step_transd(const StepParams &P, const int64_t *bh, const int64_t *bt, const int64_t *br,
                              const StepWorkspace &W, hipStream_t st);
hipError_t launch_score_transd(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                               int64_t n, float *out, hipStream_t st);
hipError_t launch_score_queries_transd(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                       const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                       int global_order);
// the (ent_transfer, rel_transfer) pair of a TransD step - or the (ent_im, rel_im) pair of a ComplEx step, which rides
// the same fields - seen as the (ent, rel) pair of a second optimizer pass: no Jacobian (the step kernel finished both
// gradients), no loss partials (the first pass reduced them)
inline void transd_transfer_pass(const StepParams &P, const StepWorkspace &W, StepParams *P2, StepWorkspace *W2) {
    *P2 = P;
    P2->ent = P.ent_t; P2->rel = P.rel_t;
    P2->ent_acc = P.ent_t_acc; P2->rel_acc = P.rel_t_acc;
    P2->norm_flag = 0;
    *W2 = W;
    W2->gent = W.gentt; W2->grel = W.grelt;
    W2->fent = W.fentt; W2->frel = W.frelt;
    W2->lpart = nullptr;
}

// RotatE (rotate.hip): the external-batch step under every loss LossParams expresses (the score handed to the loss is
// gamma - d, always), and the distances d behind pt_score*; launch_score / launch_score_queries route model 3 to the
// latter two. The gradient rows, flags and optimizer state of the entity table are [2 * ent_total][dim] half rows:
// the optimizer pass runs once, on rotate_half_rows' view
int64_t step_rotate_max_neg(int64_t dim);
hipError_t launch_step_rotate(const StepParams &P, const LossParams &L, const int64_t *bh, const int64_t *bt,
                              const int64_t *br, const StepWorkspace &W, hipStream_t st);
hipError_t launch_score_rotate(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                               int64_t n, float *out, hipStream_t st);
hipError_t launch_score_queries_rotate(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                       const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                       int global_order);
// a RotatE model's tables as the optimizer passes see them: the entity table as 2 * ent_total rows of dim floats
// (every float of it is a parameter of its own: no Jacobian), the phases as they are
inline StepParams rotate_half_rows(const StepParams &P) {
    StepParams Q = P;
    Q.ent_total = 2 * P.ent_total;
    Q.norm_flag = 0;
    return Q;
}

// DistMult (distmult.hip, model 4): tables laid out like TransE's, nothing normalised (the optimizer passes apply no
// Jacobian). The external-batch step under SigmoidLoss with or without the adversarial weights (the score s = <h, r,
// t> goes to the loss as it is: no model margin), with DistMult.regularization folded in; the scores -s behind
// pt_score*; launch_score / launch_score_queries route model 4 to the latter two.
// regul: regul_rate; l3: l3_regul_rate (the Adam pass's, launch_apply_adam); mode: how the data loader handed the
// batch over (0 normal, 1 head_batch, 2 tail_batch), which decides what the regulariser's means run over
struct RegulParams {
    float regul = 0.f, l3 = 0.f;
    int mode = 0;
};
int64_t step_distmult_max_neg(int64_t dim);
hipError_t launch_step_distmult(const StepParams &P, const LossParams &L, const RegulParams &Rg, const int64_t *bh,
                                const int64_t *bt, const int64_t *br, const StepWorkspace &W, hipStream_t st);
hipError_t launch_score_distmult(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                                 int64_t n, float *out, hipStream_t st);
hipError_t launch_score_queries_distmult(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                         const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                         int global_order);

// ComplEx (complex.hip, model 5): four tables [rows][dim]; ent / rel carry the re halves, ent_t / rel_t the im halves
// (their Adagrad sums in ent_t_acc / rel_t_acc, their gradient rows and flags in gentt / grelt / fentt / frelt), nothing
// normalised. The external-batch step under SigmoidLoss with or without the adversarial weights (the score goes to the
// loss as it is: no model margin), with ComplEx.regularization folded in (RegulParams::regul; mode 0 only, no l3); the
// scores -s behind pt_score*; launch_score / launch_score_queries route model 5 to the latter two. The optimizer pass
// runs twice: (ent_re, rel_re), then transd_transfer_pass's view of (ent_im, rel_im)
int64_t step_complex_max_neg(int64_t dim);
hipError_t launch_step_complex(const StepParams &P, const LossParams &L, const RegulParams &Rg, const int64_t *bh,
                               const int64_t *bt, const int64_t *br, const StepWorkspace &W, hipStream_t st);
hipError_t launch_score_complex(const StepParams &P, int mode, const int64_t *h, const int64_t *t, const int64_t *r,
                                int64_t n, float *out, hipStream_t st);
// queries a lane group of k_score_queries_complex serves per pass over the entity rows at this dim
int complex_queries_per_group(int64_t dim);
hipError_t launch_score_queries_complex(const StepParams &P, int side, const int64_t *qh, const int64_t *qt,
                                        const int64_t *qr, int64_t nq, int64_t E, float *out, hipStream_t st,
                                        int global_order);

hipError_t launch_torch_init(const pt_torch_init_job *d_jobs, int64_t n, hipStream_t st);
hipError_t launch_rank_rows(const float *rows, int64_t E, const int64_t *row_of, const int64_t *truth,
                            const float *repl, const int64_t *part_off, const int64_t *part, int64_t nq, int64_t *raw,
                            int64_t *filt, hipStream_t st);
hipError_t launch_rank_types(const float *rows, int64_t E, const int64_t *row_of, const int64_t *truth,
                             const float *repl, const int64_t *rel, const int64_t *type_lef, const int64_t *type_rig,
                             const int64_t *types, const int64_t *part_off, const int64_t *part, int64_t nq,
                             int64_t *raw, int64_t *filt, hipStream_t st);

}  // namespace pt

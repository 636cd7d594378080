// C-ABI of libputranse_hip.so (include/putranse.h): the reentrant pt_* entry points for graphs, samplers, scoring,
// universes and link prediction, all executing batch construction / scoring on the GPU.
// (The trainer runtime, pt_trainer_*, is trainer.cpp; the universe-set runtime, pt_universe_set_* and
// pt_universes_train, is universe_set.cpp; the reference's Base.so symbols are legacy.cpp.)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <thread>
#include <vector>

#include "common.h"
#include "graph.h"
#include "kernels.h"
#include "rng.h"
#include "trainer.h"
#include "universe.h"

// ======================================================================== errors =================
namespace pt {
namespace {
thread_local std::string g_err;
}
void set_error(int code, const std::string &msg) { g_err = "[putranse error " + std::to_string(code) + "] " + msg; }
int fail(int code, const std::string &msg) {
    set_error(code, msg);
    return code;
}
}  // namespace pt

extern "C" const char *pt_last_error(void) { return pt::g_err.c_str(); }
extern "C" int pt_version(void) { return 1; }

// ======================================================================== model descriptor =======
int pt::desc_to_params(const pt_model_desc *m, pt::StepParams &P) {
    PT_CHECK(m, PT_EINVAL, "null model descriptor");
    PT_CHECK(m->model == PT_TRANSE || m->model == PT_TRANSH || m->model == PT_TRANSD || m->model == PT_ROTATE ||
                 m->model == PT_DISTMULT || m->model == PT_COMPLEX,
             PT_EINVAL, "model must be PT_TRANSE, PT_TRANSH, PT_TRANSD, PT_ROTATE, PT_DISTMULT or PT_COMPLEX");
    PT_CHECK(m->model == PT_DISTMULT || m->model == PT_COMPLEX || m->p_norm == 1 || m->p_norm == 2, PT_ENOTSUP,
             "p_norm must be 1 or 2");
    PT_CHECK(m->opt == PT_SGD || m->opt == PT_ADAGRAD || m->opt == PT_ADAM, PT_EINVAL,
             "opt must be PT_SGD, PT_ADAGRAD or PT_ADAM");
    PT_CHECK(m->model != PT_TRANSD || pt::model_dim_supported(m->dim, m->model), PT_ENOTSUP,
             "embedding dim " + std::to_string(m->dim) + " not supported: TransD takes dims 1..512");
    PT_CHECK(pt::model_dim_supported(m->dim, m->model), PT_ENOTSUP,
             "embedding dim " + std::to_string(m->dim) +
                 " not supported: TransE, TransH, RotatE, DistMult and ComplEx take dims 1..512 and multiples of 4 from 516 "
                 "to 1024");
    PT_CHECK(m->model != PT_ROTATE || (std::isfinite(m->phase_div) && m->phase_div > 0.f), PT_EINVAL,
             "PT_ROTATE needs a finite phase divisor > 0 (pt_model_desc.phase_div = rel_embedding_range / pi)");
    PT_CHECK(m->ent && m->rel && m->ent_total > 0 && m->rel_total > 0, PT_EINVAL, "missing tables");
    PT_CHECK(m->model != PT_TRANSH || m->normv, PT_EINVAL, "TransH needs norm_vector");
    PT_CHECK(m->model != PT_TRANSD || (m->ent_transfer && m->rel_transfer), PT_EINVAL,
             "TransD needs ent_transfer and rel_transfer");
    PT_CHECK(m->model != PT_COMPLEX || (m->ent_transfer && m->rel_transfer), PT_EINVAL,
             "PT_COMPLEX needs its im tables in ent_transfer and rel_transfer (ent and rel carry the re tables)");
    PT_CHECK(m->opt != PT_ADAGRAD || (m->ent_acc && m->rel_acc && (m->model != PT_TRANSH || m->norm_acc) &&
                                      ((m->model != PT_TRANSD && m->model != PT_COMPLEX) ||
                                       (m->ent_transfer_acc && m->rel_transfer_acc))),
             PT_EINVAL, "Adagrad needs state_sum buffers");
    P.model = m->model;
    P.p_norm = m->p_norm;
    P.norm_flag = m->norm_flag ? 1 : 0;
    P.opt = m->opt;
    P.lr = m->lr;
    P.margin = m->margin;
    P.ent_total = m->ent_total;
    P.rel_total = m->rel_total;
    P.dim = m->dim;
    P.ent = m->ent; P.rel = m->rel; P.normv = m->normv;
    P.ent_acc = m->ent_acc; P.rel_acc = m->rel_acc; P.norm_acc = m->norm_acc;
    if (m->model == PT_ROTATE) P.phase_div = m->phase_div;
    // (p_norm, norm_flag and normv are not read: nothing of either model is normalised)
    if (m->model == PT_DISTMULT || m->model == PT_COMPLEX) {
        P.p_norm = 1;
        P.norm_flag = 0;
        P.normv = nullptr;
    }
    if (m->model == PT_TRANSD || m->model == PT_COMPLEX) {   // (PT_COMPLEX: the im tables and their Adagrad sums)
        P.ent_t = m->ent_transfer; P.rel_t = m->rel_transfer;
        P.ent_t_acc = m->ent_transfer_acc; P.rel_t_acc = m->rel_transfer_acc;
    }
    return PT_OK;
}

// (answers for the three translational models, as it always has: PT_ROTATE's dims are PT_TRANSE's, putranse.h)
extern "C" int pt_model_dim_supported(int64_t dim, int32_t model) {
    return model >= PT_TRANSE && model <= PT_TRANSD && pt::model_dim_supported(dim, model) ? 1 : 0;
}

// ======================================================================== graphs =================
// Opt-in count-header record format for every *2id.txt reader (pt_graph_load, importTrainFiles,
// importTestFiles); the default keeps the reference's line-count contract (Reader.h:176-196).
extern "C" int pt_set_count_header(int on) {
    pt::set_count_header(on != 0);
    return PT_OK;
}
extern "C" int pt_get_count_header(void) { return pt::count_header() ? 1 : 0; }

extern "C" int pt_graph_load(const char *in_path, pt_graph **out) {
    PT_CHECK(in_path && out, PT_EINVAL, "pt_graph_load: null argument");
    auto *g = new pt_graph();
    int rc = pt::load_graph(in_path, g->g);
    if (rc) {
        delete g;
        return rc;
    }
    *out = g;
    return PT_OK;
}
extern "C" int pt_graph_free(pt_graph *g) {
    delete g;
    return PT_OK;
}
extern "C" int64_t pt_graph_ent_total(const pt_graph *g) { return g ? g->g.ent_total : -1; }
extern "C" int64_t pt_graph_rel_total(const pt_graph *g) { return g ? g->g.rel_total : -1; }
extern "C" int64_t pt_graph_train_total(const pt_graph *g) { return g ? g->g.train_total : -1; }
extern "C" int pt_graph_triples(const pt_graph *g, int64_t *h, int64_t *t, int64_t *r) {
    PT_CHECK(g && h && t && r, PT_EINVAL, "pt_graph_triples: null argument");
    for (int64_t i = 0; i < g->g.train_total; ++i) {
        h[i] = g->g.list[i].h;
        t[i] = g->g.list[i].t;
        r[i] = g->g.list[i].r;
    }
    return PT_OK;
}

// ======================================================================== sampler ================
int pt::sampler_init(pt_sampler *s, pt::Graph *g, int64_t threads, const uint64_t *seeds) {
    PT_CHECK(threads > 0 && threads <= 64, PT_ENOTSUP, "threads must be in [1, 64]");
    PT_HIP(hipGetDevice(&s->device));
    s->g = g;
    s->threads = threads;
    if (g) {
        int rc = g->upload();
        if (rc) return rc;
    }
    PT_HIP(hipMalloc(&s->d_states, sizeof(uint64_t) * 64));
    PT_HIP(hipMemset(s->d_states, 0, sizeof(uint64_t) * 64));
    if (seeds) PT_HIP(hipMemcpy(s->d_states, seeds, sizeof(uint64_t) * (size_t)threads, hipMemcpyHostToDevice));
    return PT_OK;
}

extern "C" int pt_sampler_create(pt_graph *g, int64_t threads, const uint64_t *seeds, pt_sampler **out) {
    PT_CHECK(g && out && seeds, PT_EINVAL, "pt_sampler_create: null argument");
    auto *s = new pt_sampler();
    int rc = pt::sampler_init(s, &g->g, threads, seeds);
    if (rc) {
        delete s;
        return rc;
    }
    *out = s;
    return PT_OK;
}
extern "C" int pt_sampler_free(pt_sampler *s) {
    delete s;
    return PT_OK;
}
extern "C" int pt_sampler_set_seeds(pt_sampler *s, const uint64_t *seeds) {
    PT_CHECK(s && seeds, PT_EINVAL, "pt_sampler_set_seeds: null argument");
    PT_HIP(hipMemcpy(s->d_states, seeds, sizeof(uint64_t) * (size_t)s->threads, hipMemcpyHostToDevice));
    return PT_OK;
}
extern "C" int pt_sampler_get_seeds(pt_sampler *s, uint64_t *seeds) {
    PT_CHECK(s && seeds, PT_EINVAL, "pt_sampler_get_seeds: null argument");
    PT_HIP(hipMemcpy(seeds, s->d_states, sizeof(uint64_t) * (size_t)s->threads, hipMemcpyDeviceToHost));
    return PT_OK;
}
extern "C" int pt_sampler_sample_ex(pt_sampler *s, int64_t bs, int64_t neg, int64_t neg_rel, int64_t mode,
                                    int64_t bern, int64_t filter, int64_t *d_h, int64_t *d_t, int64_t *d_r, float *d_y,
                                    void *stream) {
    PT_CHECK(s && s->g && d_h && d_t && d_r, PT_EINVAL, "pt_sampler_sample: null argument");
    PT_CHECK(bs >= 0 && neg >= 0 && neg_rel >= 0, PT_EINVAL, "negative batch size or negative rate");
    PT_CHECK(mode >= -1 && mode <= 1, PT_EINVAL, "sampling mode must be 0, -1 (head_batch) or 1 (tail_batch)");
    PT_CHECK(s->g->ent_total > 1, PT_EINVAL, "graph needs at least two entities");
    int rc = s->g->upload();
    if (rc) return rc;
    PT_CHECK(neg_rel == 0 || !s->g->ht_full, PT_EINVAL,
             "corrupt_rel: an (h,t) pair is linked by every relation (the reference divides by zero, Corrupt.h:135)");
    hipStream_t st = (hipStream_t)stream;
    PT_HIP(pt::launch_sample(s->g->dev, s->d_states, s->threads, bs, neg, neg_rel, (int)mode, (int)bern, (int)filter,
                             d_h, d_t, d_r, d_y, st));
    PT_HIP(pt::launch_advance(s->d_states, s->threads, bs, 1 + (mode == 0 ? 2 : 1) * neg + neg_rel, st));
    return PT_OK;
}

extern "C" int pt_sampler_sample(pt_sampler *s, int64_t bs, int64_t neg, int64_t bern, int64_t filter, int64_t *d_h,
                                 int64_t *d_t, int64_t *d_r, float *d_y, void *stream) {
    return pt_sampler_sample_ex(s, bs, neg, 0, 0, bern, filter, d_h, d_t, d_r, d_y, stream);
}

// ======================================================================== scoring and metrics ====
extern "C" int pt_score(const pt_model_desc *m, int32_t mode, const int64_t *d_h, const int64_t *d_t,
                        const int64_t *d_r, int64_t n, float *d_out, void *stream) {
    pt::StepParams P{};
    pt_model_desc mm = *m;
    if (!mm.ent_acc) { mm.opt = PT_SGD; }
    int rc = pt::desc_to_params(&mm, P);
    if (rc) return rc;
    PT_CHECK(mode >= 0 && mode <= 2, PT_EINVAL, "mode must be 0 (normal), 1 (head_batch) or 2 (tail_batch)");
    PT_CHECK(d_h && d_t && d_r && d_out, PT_EINVAL, "pt_score: null argument");
    PT_HIP(pt::launch_score(P, mode, d_h, d_t, d_r, n, d_out, (hipStream_t)stream));
    return PT_OK;
}

extern "C" int pt_score_queries(const pt_model_desc *m, int32_t side, const int64_t *d_qh, const int64_t *d_qt,
                                const int64_t *d_qr, int64_t nq, float *d_out, void *stream) {
    pt::StepParams P{};
    pt_model_desc mm = *m;
    if (!mm.ent_acc) mm.opt = PT_SGD;
    int rc = pt::desc_to_params(&mm, P);
    if (rc) return rc;
    PT_CHECK(side == 0 || side == 1, PT_EINVAL, "side must be 0 (head prediction) or 1 (tail prediction)");
    PT_CHECK(nq <= 65535, PT_EINVAL, "at most 65535 queries per call");
    PT_CHECK((d_qh && d_qt && d_qr && d_out) || nq == 0, PT_EINVAL, "pt_score_queries: null argument");
    PT_HIP(pt::launch_score_queries(P, side, d_qh, d_qt, d_qr, nq, P.ent_total, d_out, (hipStream_t)stream));
    return PT_OK;
}

extern "C" int pt_score_rows(const pt_model_desc *m, int32_t side, const int64_t *d_qh, const int64_t *d_qt,
                             const int64_t *d_qr, int64_t nq, float *d_out, void *stream) {
    pt::StepParams P{};
    pt_model_desc mm = *m;
    if (!mm.ent_acc) mm.opt = PT_SGD;
    int rc = pt::desc_to_params(&mm, P);
    if (rc) return rc;
    PT_CHECK(side == 0 || side == 1, PT_EINVAL, "side must be 0 (head prediction) or 1 (tail prediction)");
    PT_CHECK(nq <= 65535, PT_EINVAL, "at most 65535 queries per call");
    PT_CHECK((d_qh && d_qt && d_qr && d_out) || nq == 0, PT_EINVAL, "pt_score_rows: null argument");
    PT_HIP(pt::launch_score_queries(P, side, d_qh, d_qt, d_qr, nq, P.ent_total, d_out, (hipStream_t)stream, 1));
    return PT_OK;
}

// Test.h:213-223 + :398-454 accumulation for n ranked queries (float accumulators, same order)
extern "C" int pt_lp_metrics(const int64_t *rank_head, const int64_t *frank_head, const int64_t *rank_tail,
                             const int64_t *frank_tail, int64_t n, float *metrics) {
    PT_CHECK(metrics && (n == 0 || (rank_head && frank_head && rank_tail && frank_tail)), PT_EINVAL,
             "pt_lp_metrics: null argument");
    float lf10 = 0, lf3 = 0, lf1 = 0, lfr = 0, lfi = 0, rf10 = 0, rf3 = 0, rf1 = 0, rfr = 0, rfi = 0;
    float l10 = 0, l3 = 0, l1 = 0, lr = 0, li = 0, r10 = 0, r3 = 0, r1 = 0, rr = 0, ri = 0;
    for (int64_t q = 0; q < n; ++q) {
        const int64_t a = rank_head[q], fa = frank_head[q], b = rank_tail[q], fb = frank_tail[q];
        if (fa < 10) lf10 += 1; if (a < 10) l10 += 1; if (fa < 3) lf3 += 1; if (a < 3) l3 += 1;
        if (fa < 1) lf1 += 1; if (a < 1) l1 += 1;
        lfr += (float)(fa + 1); lr += (float)(1 + a);
        lfi = (float)((double)lfi + 1.0 / (double)(fa + 1)); li = (float)((double)li + 1.0 / (double)(a + 1));
        if (fb < 10) rf10 += 1; if (b < 10) r10 += 1; if (fb < 3) rf3 += 1; if (b < 3) r3 += 1;
        if (fb < 1) rf1 += 1; if (b < 1) r1 += 1;
        rfr += (float)(1 + fb); rr += (float)(1 + b);
        rfi = (float)((double)rfi + 1.0 / (double)(1 + fb)); ri = (float)((double)ri + 1.0 / (double)(1 + b));
    }
    const float N = (float)n;
    lfr /= N; rfr /= N; lfi /= N; rfi /= N; lf10 /= N; lf3 /= N; lf1 /= N; rf10 /= N; rf3 /= N; rf1 /= N;
    lr /= N; rr /= N; li /= N; ri /= N; l10 /= N; l3 /= N; l1 /= N; r10 /= N; r3 /= N; r1 /= N;
    metrics[0] = (lfi + rfi) / 2; metrics[1] = (lfr + rfr) / 2; metrics[2] = (lf10 + rf10) / 2;
    metrics[3] = (lf3 + rf3) / 2; metrics[4] = (lf1 + rf1) / 2;
    metrics[5] = (li + ri) / 2; metrics[6] = (lr + rr) / 2; metrics[7] = (l10 + r10) / 2;
    metrics[8] = (l3 + r3) / 2; metrics[9] = (l1 + r1) / 2;
    return PT_OK;
}

// ======================================================================== universes ==============
extern "C" int pt_universe_build(const pt_graph *g, int64_t seed, int64_t threads, int64_t tc, float balance,
                                 pt_universe **out) {
    PT_CHECK(g && out, PT_EINVAL, "pt_universe_build: null argument");
    PT_CHECK(threads > 0 && threads <= 64 && tc > 0, PT_EINVAL, "bad threads / triple constraint");
    auto *u = new pt_universe();
    pt::GlibcRand rng((uint32_t)seed);   // srand(seed) (Random.h:37-42)
    u->u.seeds.resize((size_t)threads);
    for (auto &x : u->u.seeds) x = (uint64_t)(int64_t)rng.next();   // randReset (Random.h:10-15)
    pt::build_universe(g->g, rng, tc, balance, u->u);
    *out = u;
    return PT_OK;
}

extern "C" int pt_universe_build_many(const pt_graph *g, int64_t n, const int64_t *seeds, int64_t threads,
                                      const int64_t *tcs, const float *balances, int64_t n_workers, pt_universe **out) {
    PT_CHECK(g && seeds && tcs && balances && out, PT_EINVAL, "pt_universe_build_many: null argument");
    if (n_workers <= 0) n_workers = std::max(1u, std::thread::hardware_concurrency());
    n_workers = std::min<int64_t>(n_workers, std::max<int64_t>(n, 1));
    std::atomic<int64_t> next{0};
    std::atomic<int> err{0};
    auto work = [&]() {
        for (int64_t i; (i = next.fetch_add(1)) < n;) {
            pt_universe *u = nullptr;
            int rc = pt_universe_build(g, seeds[i], threads, tcs[i], balances[i], &u);
            if (rc) err = rc;
            out[i] = u;
        }
    };
    std::vector<std::thread> pool;
    for (int64_t w = 1; w < n_workers; ++w) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    return err.load();
}
extern "C" int pt_universe_free(pt_universe *u) {
    delete u;
    return PT_OK;
}
extern "C" int64_t pt_universe_ent_total(const pt_universe *u) { return u ? u->u.g.ent_total : -1; }
extern "C" int64_t pt_universe_rel_total(const pt_universe *u) { return u ? u->u.g.rel_total : -1; }
extern "C" int64_t pt_universe_train_total(const pt_universe *u) { return u ? u->u.g.train_total : -1; }
extern "C" int pt_universe_remaps(const pt_universe *u, int64_t *ent_remap, int64_t *rel_remap) {
    PT_CHECK(u, PT_EINVAL, "null universe");
    if (ent_remap) std::copy(u->u.ent_remap.begin(), u->u.ent_remap.end(), ent_remap);
    if (rel_remap) std::copy(u->u.rel_remap.begin(), u->u.rel_remap.end(), rel_remap);
    return PT_OK;
}
extern "C" pt_graph *pt_universe_graph(pt_universe *u) {
    // pt_graph is a thin wrapper over pt::Graph; the universe owns it
    return u ? reinterpret_cast<pt_graph *>(&u->u.g) : nullptr;
}
extern "C" int pt_universe_seeds(const pt_universe *u, uint64_t *seeds) {
    PT_CHECK(u && seeds, PT_EINVAL, "null argument");
    std::copy(u->u.seeds.begin(), u->u.seeds.end(), seeds);
    return PT_OK;
}

// initial universe tables, torch-CPU-generator-identical (torch_init.hip)
extern "C" int pt_torch_init_tables(const pt_torch_init_job *jobs, int64_t n, void *stream) {
    PT_CHECK(n >= 0 && (jobs || n == 0), PT_EINVAL, "pt_torch_init_tables: null jobs");
    if (n == 0) return PT_OK;
    for (int64_t i = 0; i < n; ++i) {
        const pt_torch_init_job &J = jobs[i];
        PT_CHECK(J.ntab >= 0 && J.ntab <= 4 && J.skip >= 0, PT_EINVAL, "pt_torch_init_tables: bad job");
        for (int k = 0; k < J.ntab; ++k)
            PT_CHECK(J.numel[k] >= 0 && (J.out[k] || J.numel[k] == 0), PT_EINVAL, "pt_torch_init_tables: null table");
    }
    hipStream_t st = (hipStream_t)stream;
    pt_torch_init_job *d = nullptr;
    PT_HIP(hipMallocAsync((void **)&d, sizeof(pt_torch_init_job) * (size_t)n, st));
    hipError_t e = hipMemcpyAsync(d, jobs, sizeof(pt_torch_init_job) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = pt::launch_torch_init(d, n, st);
    const hipError_t f = hipFreeAsync(d, st);
    const hipError_t w = hipStreamSynchronize(st);   // the caller's job array may go away on return
    if (e == hipSuccess) e = f != hipSuccess ? f : w;
    if (e != hipSuccess) return pt::fail(PT_EHIP, std::string("pt_torch_init_tables: ") + hipGetErrorString(e));
    return PT_OK;
}

// ======================================================================== link prediction =======
// keys of one batch of pt_lp_min_scores: as many score rows (global_ent_total floats each) as fit the batch
// budget of 192 MB, at least one
static int64_t lp_keys_per_batch(int64_t global_ent_total) {
    const int64_t batch_mb = 192;
    return std::max<int64_t>(1, (batch_mb << 20) / (4 * std::max<int64_t>(global_ent_total, 1)));
}
extern "C" int64_t pt_lp_keys_per_batch(int64_t global_ent_total) { return lp_keys_per_batch(global_ent_total); }

extern "C" int pt_lp_min_scores(const pt_lp_universe *us, int64_t n_universes, int32_t model, int32_t p_norm,
                                int32_t norm_flag, const pt_lp_pair *pairs, int64_t n_pairs,
                                int64_t global_ent_total, float *d_key_rows, float *d_key_tuple, void *stream) {
    PT_CHECK(model != PT_TRANSD, PT_ENOTSUP, "pt_lp_min_scores: PuTransD universes are not built yet (PT_TRANSD)");
    PT_CHECK(model != PT_ROTATE, PT_ENOTSUP, "pt_lp_min_scores: PT_ROTATE trains and ranks one model, not universes");
    PT_CHECK(model != PT_DISTMULT, PT_ENOTSUP,
             "pt_lp_min_scores: PT_DISTMULT trains and ranks one model, not universes");
    PT_CHECK(model != PT_COMPLEX, PT_ENOTSUP, "pt_lp_min_scores: PT_COMPLEX trains and ranks one model, not universes");
    PT_CHECK((us && pairs && d_key_rows) || n_pairs == 0, PT_EINVAL, "pt_lp_min_scores: null argument");
    if (n_pairs == 0) return PT_OK;
    hipStream_t st = (hipStream_t)stream;
    // per universe once: its dim is at most 512 (the scan's LDS tile of 64 x (dim + 1) floats, and its one-float
    // rows), and the job key of its row shape (below)
    auto shape_key = [](int64_t dim) {
        const pt::Shape s = pt::pick_shape(dim);
        return (int64_t)s.G * 10000 + (int64_t)s.VEC * 100 + s.KCH;
    };
    std::vector<int64_t> u_shape((size_t)n_universes, -1);
    for (int64_t u = 0; u < n_universes; ++u)
        if (pt::narrow_dim_supported(us[u].dim)) u_shape[(size_t)u] = shape_key(us[u].dim);
    for (int64_t i = 0; i < n_pairs; ++i) {
        const pt_lp_pair &p = pairs[i];
        PT_CHECK(p.universe >= 0 && p.universe < n_universes, PT_EINVAL, "pair universe out of range");
        const pt_lp_universe &U = us[p.universe];
        PT_CHECK(p.anchor >= 0 && p.anchor < U.ent_total && p.rel >= 0 && p.rel < U.rel_total, PT_EINVAL,
                 "pair local ids out of range");
        PT_CHECK(p.side == 0 || p.side == 1, PT_EINVAL, "pair side must be 0 or 1");
        PT_CHECK(p.key >= 0, PT_EINVAL, "pair key must be non-negative");
        PT_CHECK(u_shape[(size_t)p.universe] >= 0, PT_ENOTSUP, "dim not supported");
    }
    // Jobs = (lane-group row shape of the universes' dims, key batch): one launch pair per job covers every
    // dim of that shape (C3's ~80 dims take ~10 shapes: one launch pair per dim left most of the GPU idle). A
    // key batch's score rows (keys x global_ent_total floats) are sized to stay resident in the Infinity
    // Cache while its pairs' atomicMins land (lp_keys_per_batch's 192 MB); inside a job the pairs are
    // sorted by universe so each universe's entity rows are read once per job.
    int64_t n_keys = 0;
    for (int64_t i = 0; i < n_pairs; ++i) n_keys = std::max<int64_t>(n_keys, (int64_t)pairs[i].key + 1);
    const int64_t keys_per_batch = lp_keys_per_batch(global_ent_total);
    const int64_t n_batches = (n_keys + keys_per_batch - 1) / keys_per_batch;
    // jobs ordered by (shape key, batch); the pairs of a (job, universe) keep their input order: a counting sort
    // over (job, universe) in place of per-job per-universe vectors (2 M pairs for C4)
    std::vector<int64_t> shapes(u_shape);
    std::sort(shapes.begin(), shapes.end());
    shapes.erase(std::unique(shapes.begin(), shapes.end()), shapes.end());
    std::vector<int32_t> u_si((size_t)n_universes);
    for (int64_t u = 0; u < n_universes; ++u)
        u_si[(size_t)u] = (int32_t)(std::lower_bound(shapes.begin(), shapes.end(), u_shape[(size_t)u]) - shapes.begin());
    const int64_t n_jobs = (int64_t)shapes.size() * n_batches;
    auto job_of = [&](const pt_lp_pair &p) { return (int64_t)u_si[(size_t)p.universe] * n_batches + p.key / keys_per_batch; };
    std::vector<int64_t> cnt((size_t)(n_jobs * n_universes + 1), 0);
    for (int64_t i = 0; i < n_pairs; ++i) ++cnt[(size_t)(job_of(pairs[i]) * n_universes + pairs[i].universe + 1)];
    for (size_t c = 1; c < cnt.size(); ++c) cnt[c] += cnt[c - 1];
    std::vector<pt::LpPair> hp((size_t)n_pairs);
    {
        std::vector<int64_t> fill(cnt.begin(), cnt.end() - 1);
        for (int64_t i = 0; i < n_pairs; ++i) {
            const pt_lp_pair &p = pairs[i];
            hp[(size_t)fill[(size_t)(job_of(p) * n_universes + p.universe)]++] =
                pt::LpPair{p.key, p.universe, p.anchor, p.rel, p.side};
        }
    }
    std::vector<pt::LpUniverseDev> hu((size_t)n_universes);
    for (int64_t i = 0; i < n_universes; ++i)
        hu[i] = pt::LpUniverseDev{us[i].ent, us[i].rel, us[i].normv, us[i].d_ent_remap, us[i].ent_total, us[i].dim};
    // host staging, kept alive until the stream has consumed it (synchronize at the end). Per job: its
    // pairs contiguous and sorted by universe; uoff[job][2u], uoff[job][2u+1] = universe u's range
    // relative to the job's first pair
    std::vector<int64_t> uoff;
    std::vector<int32_t> uids;
    struct DimJob {
        int64_t dim, p_begin, p_end, u_begin, u_end, max_ent, uoff_begin;
    };
    std::vector<DimJob> dj;
    for (int64_t j = 0; j < n_jobs; ++j) {
        const int64_t b0 = cnt[(size_t)(j * n_universes)], b1 = cnt[(size_t)((j + 1) * n_universes)];
        if (b1 == b0) continue;
        DimJob d{0, b0, b1, (int64_t)uids.size(), 0, 0, (int64_t)uoff.size()};   // dim: the largest
        uoff.resize(uoff.size() + 2 * (size_t)n_universes, 0);
        for (int64_t u = 0; u < n_universes; ++u) {
            const int64_t lo = cnt[(size_t)(j * n_universes + u)], hi = cnt[(size_t)(j * n_universes + u + 1)];
            if (hi == lo) continue;
            uoff[d.uoff_begin + 2 * u] = lo - b0;
            uoff[d.uoff_begin + 2 * u + 1] = hi - b0;
            uids.push_back((int32_t)u);
            d.max_ent = std::max(d.max_ent, us[u].ent_total);
            d.dim = std::max(d.dim, us[u].dim);
        }
        d.u_end = (int64_t)uids.size();
        dj.push_back(d);
    }
    int64_t max_dim = 0;
    for (auto &d : dj) max_dim = std::max(max_dim, d.dim);
    max_dim = (max_dim + 3) & ~int64_t(3);   // every job's scratch region 16-byte aligned (float4 rows)
    const size_t scratch = (size_t)n_pairs * (size_t)max_dim * (model == 1 ? 2 : 1);
    char *blk = nullptr;
    const size_t bytes = sizeof(pt::LpUniverseDev) * hu.size() + sizeof(pt::LpPair) * hp.size() +
                         sizeof(int64_t) * uoff.size() + sizeof(int32_t) * (uids.size() + 1) + sizeof(float) * scratch +
                         5 * 256;
    PT_HIP(hipMallocAsync((void **)&blk, bytes, st));
    auto carve = [&](size_t n) {
        char *p = blk;
        blk += (n + 255) & ~size_t(255);
        return p;
    };
    char *base0 = blk;
    auto *du = (pt::LpUniverseDev *)carve(sizeof(pt::LpUniverseDev) * hu.size());
    auto *dp = (pt::LpPair *)carve(sizeof(pt::LpPair) * hp.size());
    auto *duoff = (int64_t *)carve(sizeof(int64_t) * uoff.size());
    auto *duids = (int32_t *)carve(sizeof(int32_t) * (uids.size() + 1));
    auto *dbase = (float *)carve(sizeof(float) * scratch);
    PT_HIP(hipMemcpyAsync(du, hu.data(), sizeof(pt::LpUniverseDev) * hu.size(), hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(dp, hp.data(), sizeof(pt::LpPair) * hp.size(), hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(duoff, uoff.data(), sizeof(int64_t) * uoff.size(), hipMemcpyHostToDevice, st));
    PT_HIP(hipMemcpyAsync(duids, uids.data(), sizeof(int32_t) * uids.size(), hipMemcpyHostToDevice, st));
    int rc = PT_OK;
    for (auto &d : dj) {
        const int64_t np = d.p_end - d.p_begin;
        float *b = dbase + d.p_begin * max_dim * (model == 1 ? 2 : 1);   // the group's own scratch region
        float *nrm = model == 1 ? b + np * d.dim : nullptr;
        const hipError_t e = pt::launch_lp_min(du, dp + d.p_begin, np, duoff + d.uoff_begin, duids + d.u_begin,
                                               d.u_end - d.u_begin,
                                               d.dim, d.max_ent, model, p_norm, norm_flag, global_ent_total,
                                               d.dim, b, nrm, d_key_rows, d_key_tuple, st);
        if (e != hipSuccess) {
            rc = pt::fail(PT_EHIP, std::string("launch_lp_min: ") + hipGetErrorString(e));
            break;
        }
    }
    (void)hipFreeAsync(base0, st);
    PT_HIP(hipStreamSynchronize(st));   // host vectors above must outlive the async copies
    return rc;
}

extern "C" int pt_rank_rows(const float *d_rows, int64_t ent_total, const int64_t *d_row_of, const int64_t *d_truth,
                            const float *d_repl, const int64_t *d_part_off, const int64_t *d_part, int64_t n,
                            int64_t *d_raw, int64_t *d_filt, void *stream) {
    if (n == 0) return PT_OK;
    PT_CHECK(d_rows && d_row_of && d_truth && d_part_off && d_raw && d_filt && ent_total > 0, PT_EINVAL,
             "pt_rank_rows: null argument");
    PT_HIP(pt::launch_rank_rows(d_rows, ent_total, d_row_of, d_truth, d_repl, d_part_off, d_part, n, d_raw, d_filt,
                                (hipStream_t)stream));
    return PT_OK;
}

extern "C" int pt_rank_types(const float *d_rows, int64_t ent_total, const int64_t *d_row_of, const int64_t *d_truth,
                             const float *d_repl, const int64_t *d_rel, const int64_t *d_type_lef,
                             const int64_t *d_type_rig, const int64_t *d_types, const int64_t *d_part_off,
                             const int64_t *d_part, int64_t n, int64_t *d_raw, int64_t *d_filt, void *stream) {
    if (n == 0) return PT_OK;
    PT_CHECK(d_rows && d_row_of && d_truth && d_rel && d_type_lef && d_type_rig && d_types && d_part_off && d_raw &&
                 d_filt && ent_total > 0,
             PT_EINVAL, "pt_rank_types: null argument");
    PT_HIP(pt::launch_rank_types(d_rows, ent_total, d_row_of, d_truth, d_repl, d_rel, d_type_lef, d_type_rig, d_types,
                                 d_part_off, d_part, n, d_raw, d_filt, (hipStream_t)stream));
    return PT_OK;
}

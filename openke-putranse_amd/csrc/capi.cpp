// C-ABI of libputranse_hip.so (include/putranse.h): reentrant pt_* entry points and the reference's
// Base.so symbols for the hot path, all executing batch construction / training / scoring on the GPU.
// (The trainer runtime, pt_trainer_*, is trainer.cpp; the universe-set runtime, pt_universe_set_* and
// pt_universes_train, is universe_set.cpp.)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "tuning.h"
#include "common.h"
#include "graph.h"
#include "kernels.h"
#include "ordered.h"
#include "rng.h"
#include "trainer.h"
#include "universe.h"
#include "universes.h"

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
    PT_CHECK(m->model == PT_TRANSE || m->model == PT_TRANSH || m->model == PT_TRANSD, PT_EINVAL,
             "model must be PT_TRANSE, PT_TRANSH or PT_TRANSD");
    PT_CHECK(m->p_norm == 1 || m->p_norm == 2, PT_ENOTSUP, "p_norm must be 1 or 2");
    PT_CHECK(m->opt == PT_SGD || m->opt == PT_ADAGRAD || m->opt == PT_ADAM, PT_EINVAL,
             "opt must be PT_SGD, PT_ADAGRAD or PT_ADAM");
    PT_CHECK(m->model != PT_TRANSD || pt::model_dim_supported(m->dim, m->model), PT_ENOTSUP,
             "embedding dim " + std::to_string(m->dim) + " not supported: TransD takes dims 1..512");
    PT_CHECK(pt::model_dim_supported(m->dim, m->model), PT_ENOTSUP,
             "embedding dim " + std::to_string(m->dim) +
                 " not supported: TransE and TransH take dims 1..512 and multiples of 4 from 516 to 1024");
    PT_CHECK(m->ent && m->rel && m->ent_total > 0 && m->rel_total > 0, PT_EINVAL, "missing tables");
    PT_CHECK(m->model != PT_TRANSH || m->normv, PT_EINVAL, "TransH needs norm_vector");
    PT_CHECK(m->model != PT_TRANSD || (m->ent_transfer && m->rel_transfer), PT_EINVAL,
             "TransD needs ent_transfer and rel_transfer");
    PT_CHECK(m->opt != PT_ADAGRAD || (m->ent_acc && m->rel_acc && (m->model != PT_TRANSH || m->norm_acc) &&
                                      (m->model != PT_TRANSD || (m->ent_transfer_acc && m->rel_transfer_acc))),
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
    if (m->model == PT_TRANSD) {
        P.ent_t = m->ent_transfer; P.rel_t = m->rel_transfer;
        P.ent_t_acc = m->ent_transfer_acc; P.rel_t_acc = m->rel_transfer_acc;
    }
    if (const char *v = pt_tuning_env("PT_STEP_DBG")) P.dbg = atoi(v);
    return PT_OK;
}

extern "C" int pt_model_dim_supported(int64_t dim, int32_t model) {
    return pt::model_dim_supported(dim, model) ? 1 : 0;
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
// budget (PT_LP_BATCH_MB in the tuning build, default 192), at least one
static int64_t lp_keys_per_batch(int64_t global_ent_total) {
    int64_t batch_mb = 192;
    if (const char *v = pt_tuning_env("PT_LP_BATCH_MB")) batch_mb = std::max<int64_t>(1, atoll(v));
    return std::max<int64_t>(1, (batch_mb << 20) / (4 * std::max<int64_t>(global_ent_total, 1)));
}
extern "C" int64_t pt_lp_keys_per_batch(int64_t global_ent_total) { return lp_keys_per_batch(global_ent_total); }

extern "C" int pt_lp_min_scores(const pt_lp_universe *us, int64_t n_universes, int32_t model, int32_t p_norm,
                                int32_t norm_flag, const pt_lp_pair *pairs, int64_t n_pairs,
                                int64_t global_ent_total, float *d_key_rows, float *d_key_tuple, void *stream) {
    PT_CHECK(model != PT_TRANSD, PT_ENOTSUP, "pt_lp_min_scores: PuTransD universes are not built yet (PT_TRANSD)");
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
    // Cache while its pairs' atomicMins land (PT_LP_BATCH_MB, default 192); inside a job the pairs are
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

// ======================================================================== Base.so surface ========
// One process-global context with the reference's semantics (Setting.h / Random.h / Reader.h /
// UniverseSetting.h / Test.h / Valid.h globals). Sampling, training and scoring run on the GPU.
namespace {

struct TestAcc {   // the reference's float accumulators (Test.h:14-21)
    float l_filter_tot = 0, l3_filter_tot = 0, l1_filter_tot = 0, l_filter_rank = 0, l_filter_reci = 0;
    float r_filter_tot = 0, r3_filter_tot = 0, r1_filter_tot = 0, r_filter_rank = 0, r_filter_reci = 0;
    float l_tot = 0, l3_tot = 0, l1_tot = 0, l_rank = 0, l_reci = 0;
    float r_tot = 0, r3_tot = 0, r1_tot = 0, r_rank = 0, r_reci = 0;
};

struct Legacy {
    std::mutex mu;
    std::string in_path = "../data/FB15K/";
    int64_t threads = 1, bern = 0, seed = 0;
    pt::GlibcRand rng{1};
    std::vector<uint64_t> states;
    std::unique_ptr<pt::Graph> train;        // importTrainFiles
    std::string train_path;
    bool train_header = false;               // record format train was read with
    int import_rc = PT_OK;                   // status of the last importTrainFiles / importTestFiles
    std::unique_ptr<pt::Universe> uni;       // getParallelUniverse
    bool swapped = false;
    pt_sampler sampler;                      // device states; g follows the active graph
    bool sampler_ready = false;
    // device batch buffers for the host-pointer sampling()
    int64_t *dbuf = nullptr;
    size_t dbuf_cap = 0;
    // test / valid data
    bool load_all = false;
    int64_t ent_total = 0, rel_total = 0, test_total = 0, valid_total = 0, triple_total = 0, train_lines = 0;
    std::vector<pt::Triple> test, valid;
    pt_known *known = nullptr;
    int64_t last_head = 0, last_tail = 0, last_vhead = 0, last_vtail = 0;
    TestAcc acc, acc_tc;                     // unconstrained / type-constrained accumulators
    float mrr = 0, mr = 0, hit10 = 0, hit3 = 0, hit1 = 0;
    float mrr_tc = 0, mr_tc = 0, hit10_tc = 0, hit3_tc = 0, hit1_tc = 0;
    float l_valid = 0, r_valid = 0, valid_hit10 = 0;
    // importTypeFiles (Reader.h:344-396): per relation [lef, rig) into the sorted head / tail type lists
    bool types_loaded = false;
    std::vector<int64_t> type_lef[2], type_rig[2], type_list[2];

    pt::Graph *active() { return swapped && uni ? &uni->g : train.get(); }
    int64_t E() { pt::Graph *g = active(); return g ? g->ent_total : ent_total; }
};

Legacy &L() {
    static Legacy *l = new Legacy();   // never destroyed: device frees at exit are unsafe
    return *l;
}

void legacy_err(int rc) {
    if (rc) fprintf(stderr, "%s\n", pt_last_error());
}

int legacy_sync_sampler(Legacy &l) {
    if (!l.sampler_ready) {
        int rc = pt::sampler_init(&l.sampler, nullptr, 64, nullptr);
        if (rc) return rc;
        l.sampler.threads = std::max<int64_t>(1, l.threads);
        l.sampler_ready = true;
    }
    l.sampler.g = l.active();
    return PT_OK;
}

int legacy_push_states(Legacy &l) {
    int rc = legacy_sync_sampler(l);
    if (rc) return rc;
    std::vector<uint64_t> s(64, 0);
    std::copy(l.states.begin(), l.states.end(), s.begin());
    PT_HIP(hipMemcpy(l.sampler.d_states, s.data(), sizeof(uint64_t) * 64, hipMemcpyHostToDevice));
    l.sampler.threads = std::max<int64_t>(1, (int64_t)l.states.size());
    return PT_OK;
}

}  // namespace

extern "C" pt_sampler *pt_legacy_sampler(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    if (legacy_sync_sampler(l)) return nullptr;
    return &l.sampler;
}

extern "C" void setInPath(char *path) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    l.in_path = path ? path : "";
    printf("Input Files Path : %s\n", l.in_path.c_str());
}
extern "C" void setOutPath(char *path) { (void)path; }
extern "C" void setWorkThreads(int64_t threads) { L().threads = threads; }
extern "C" int64_t getWorkThreads(void) { return L().threads; }
extern "C" void setBern(int64_t con) { L().bern = con; }
extern "C" void setRandomSeed(int64_t seed) {
    Legacy &l = L();
    l.seed = seed == -1 ? (int64_t)time(nullptr) : seed;
    l.rng.seed_with((uint32_t)l.seed);
}
extern "C" int64_t getRandomSeed(void) { return L().seed; }
extern "C" void randReset(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    l.states.assign((size_t)std::max<int64_t>(1, l.threads), 0);
    for (auto &s : l.states) s = (uint64_t)(int64_t)l.rng.next();
    legacy_err(legacy_push_states(l));
}
extern "C" void importTrainFiles(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    printf("The toolkit is importing datasets.\n");
    if (l.train && l.train_path == l.in_path && l.train_header == pt::count_header() && !l.swapped) {
        l.import_rc = PT_OK;
        return;   // identical re-import
    }
    auto g = std::make_unique<pt::Graph>();
    int rc = pt::load_graph(l.in_path, *g);
    l.import_rc = rc;
    if (rc) {
        legacy_err(rc);
        return;
    }
    (void)hipDeviceSynchronize();   // an older graph may still be read by queued kernels
    l.train = std::move(g);
    l.train_path = l.in_path;
    l.train_header = pt::count_header();
    l.ent_total = l.train->ent_total;
    l.rel_total = l.train->rel_total;
    legacy_err(l.train->upload());
    legacy_err(legacy_sync_sampler(l));
    printf("The total of train triples is %ld.\n", (long)l.train->train_total);
}
// The reference's import functions return void and crash on bad input; ours report through this.
extern "C" int pt_legacy_import_status(void) { return L().import_rc; }
extern "C" int64_t getEntityTotal(void) { Legacy &l = L(); return l.active() ? l.active()->ent_total : l.ent_total; }
extern "C" int64_t getRelationTotal(void) { Legacy &l = L(); return l.active() ? l.active()->rel_total : l.rel_total; }
extern "C" int64_t getTrainTotal(void) { Legacy &l = L(); return l.active() ? l.active()->train_total : l.train_lines; }
extern "C" int64_t getTestTotal(void) { return L().test_total; }
extern "C" int64_t getValidTotal(void) { return L().valid_total; }
extern "C" int64_t getTripleTotal(void) { return L().triple_total; }

extern "C" void sampling(int64_t *bh, int64_t *bt, int64_t *br, float *by, int64_t bs, int64_t neg, int64_t neg_rel,
                         int64_t mode, int64_t filter, int64_t p, int64_t val_loss) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    if (val_loss) {   // positives of the validation list (Base.cpp:255-262)
        for (int64_t b = 0; b < bs && b < (int64_t)l.valid.size(); ++b) {
            bh[b] = l.valid[b].h; bt[b] = l.valid[b].t; br[b] = l.valid[b].r; by[b] = 1;
        }
        return;
    }
    if (neg_rel > 0 && p) {   // corrupt_rel's p branch reads a relation-probability table never loaded
        legacy_err(pt::fail(PT_ENOTSUP, "sampling: p = 1 (probability-weighted corrupt_rel) is not supported"));
        return;
    }
    if (!l.active()) {
        legacy_err(pt::fail(PT_ESTATE, "sampling before importTrainFiles"));
        return;
    }
    int rc = legacy_sync_sampler(l);
    if (rc) return legacy_err(rc);
    const int64_t seq = bs * (1 + neg + neg_rel);
    const size_t need = (size_t)seq * 3 * sizeof(int64_t) + (size_t)seq * sizeof(float);
    if (need > l.dbuf_cap) {
        if (l.dbuf) (void)hipFree(l.dbuf);
        l.dbuf = nullptr;
        if (hipMalloc(&l.dbuf, need) != hipSuccess) return legacy_err(pt::fail(PT_ENOMEM, "sampling buffers"));
        l.dbuf_cap = need;
    }
    int64_t *dh = l.dbuf, *dt = dh + seq, *dr = dt + seq;
    float *dy = (float *)(dr + seq);
    rc = pt_sampler_sample_ex(&l.sampler, bs, neg, neg_rel, mode, l.bern, filter, dh, dt, dr, dy, nullptr);
    if (rc) return legacy_err(rc);
    (void)hipMemcpy(bh, dh, sizeof(int64_t) * seq, hipMemcpyDeviceToHost);
    (void)hipMemcpy(bt, dt, sizeof(int64_t) * seq, hipMemcpyDeviceToHost);
    (void)hipMemcpy(br, dr, sizeof(int64_t) * seq, hipMemcpyDeviceToHost);
    (void)hipMemcpy(by, dy, sizeof(float) * seq, hipMemcpyDeviceToHost);
}

// Neighbourhood getters of TrainDataLoader.get_positive_entities / get_negative_entities /
// get_entity_relations (Base.cpp:312-466) over the active graph (the swapped universe after swapHelpers):
// `is_tail` != 0 scans the entity's run of the cmp_tail list (partners = heads), else its run of the
// cmp_head list (partners = tails); positives are the partners under `relation`, negatives those under
// any other relation, in list order.
static const pt::Graph *legacy_graph_or_null(const char *who) {
    const pt::Graph *g = L().active();
    if (!g) pt::fail(PT_ESTATE, std::string(who) + " before importTrainFiles");
    return g;
}
static int64_t legacy_partners(int64_t entity, int64_t relation, int64_t is_tail, bool positive, int64_t *out) {
    const pt::Graph *g = legacy_graph_or_null("entity neighbourhood getter");
    if (!g || entity < 0 || entity >= g->ent_total) return 0;
    const auto &lst = is_tail ? g->tail : g->head;
    const int64_t lo = is_tail ? g->lef_tail[(size_t)entity] : g->lef_head[(size_t)entity];
    const int64_t hi = is_tail ? g->rig_tail[(size_t)entity] : g->rig_head[(size_t)entity];
    int64_t n = 0;
    for (int64_t i = lo; i <= hi; ++i) {
        const pt::Triple &x = lst[(size_t)i];
        if ((x.r == relation) == positive) {
            if (out) out[n] = is_tail ? x.h : x.t;
            ++n;
        }
    }
    return n;
}
extern "C" int64_t getNumOfNegatives(int64_t entity, int64_t relation, int64_t is_tail) {
    return legacy_partners(entity, relation, is_tail, false, nullptr);
}
extern "C" int64_t getNumOfPositives(int64_t entity, int64_t relation, int64_t is_tail) {
    return legacy_partners(entity, relation, is_tail, true, nullptr);
}
extern "C" void getNegativeEntities(int64_t *out, int64_t entity, int64_t relation, int64_t is_tail) {
    legacy_partners(entity, relation, is_tail, false, out);
}
extern "C" void getPositiveEntities(int64_t *out, int64_t entity, int64_t relation, int64_t is_tail) {
    legacy_partners(entity, relation, is_tail, true, out);
}
static int64_t legacy_entity_relations(int64_t entity, int64_t is_tail, int64_t *out) {
    const pt::Graph *g = legacy_graph_or_null("getEntityRelations");
    if (!g || entity < 0 || entity >= g->ent_total) return 0;
    const auto &lst = is_tail ? g->tail : g->head;
    const int64_t lo = is_tail ? g->lef_tail[(size_t)entity] : g->lef_head[(size_t)entity];
    const int64_t hi = is_tail ? g->rig_tail[(size_t)entity] : g->rig_head[(size_t)entity];
    int64_t n = 0, cur = -1;
    for (int64_t i = lo; i <= hi; ++i) {
        if (lst[(size_t)i].r != cur) {
            cur = lst[(size_t)i].r;
            // the reference never advances its output index (Base.cpp:442-466): every distinct relation
            // lands in out[0], so out[0] ends as the last one and the rest of the buffer is untouched
            if (out) out[0] = cur;
            ++n;
        }
    }
    return n;
}
extern "C" int64_t getNumOfEntityRelations(int64_t entity, int64_t is_tail) {
    return legacy_entity_relations(entity, is_tail, nullptr);
}
extern "C" void getEntityRelations(int64_t *out, int64_t entity, int64_t is_tail) {
    legacy_entity_relations(entity, is_tail, out);
}

extern "C" int64_t pt_legacy_bern(void) { return L().bern; }

// the global context's test / valid lists in the reference's ranking order (cmp_rel2, Reader.h:311-312)
extern "C" int64_t pt_legacy_eval_triples(int32_t valid, int64_t *h, int64_t *t, int64_t *r) {
    Legacy &l = L();
    const std::vector<pt::Triple> &v = valid ? l.valid : l.test;
    if (h && t && r)
        for (size_t i = 0; i < v.size(); ++i) { h[i] = v[i].h; t[i] = v[i].t; r[i] = v[i].r; }
    return (int64_t)v.size();
}
extern "C" const pt_known *pt_legacy_known(void) { return L().known; }
extern "C" pt_graph *pt_legacy_graph(void) {
    // the full training graph of importTrainFiles (never the swapped universe): pt_graph wraps pt::Graph
    return reinterpret_cast<pt_graph *>(L().train.get());
}

extern "C" void getParallelUniverse(int64_t tc, float balance) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    if (!l.train) return legacy_err(pt::fail(PT_ESTATE, "getParallelUniverse before importTrainFiles"));
    l.uni = std::make_unique<pt::Universe>();
    pt::build_universe(*l.train, l.rng, tc, balance, *l.uni);
    printf("Universe configured. \n");
}
extern "C" int64_t getEntityTotalUniverse(void) {
    Legacy &l = L();
    if (!l.uni) return 0;
    return l.swapped ? l.train->ent_total : l.uni->g.ent_total;
}
extern "C" int64_t getRelationTotalUniverse(void) {
    Legacy &l = L();
    if (!l.uni) return 0;
    return l.swapped ? l.train->rel_total : l.uni->g.rel_total;
}
extern "C" int64_t getTrainTotalUniverse(void) {
    Legacy &l = L();
    if (!l.uni) return 0;
    return l.swapped ? l.train->train_total : l.uni->g.train_total;
}
extern "C" void getEntityRemapping(int64_t *out) {
    Legacy &l = L();
    if (l.uni) std::copy(l.uni->ent_remap.begin(), l.uni->ent_remap.end(), out);
}
extern "C" void getRelationRemapping(int64_t *out) {
    Legacy &l = L();
    if (l.uni) std::copy(l.uni->rel_remap.begin(), l.uni->rel_remap.end(), out);
}
extern "C" void swapHelpers(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    if (!l.uni) return legacy_err(pt::fail(PT_ESTATE, "swapHelpers without a universe"));
    l.swapped = !l.swapped;
    if (l.swapped) legacy_err(l.uni->g.upload());
    legacy_err(legacy_sync_sampler(l));
}
extern "C" void resetUniverse(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    l.swapped = false;
    (void)hipDeviceSynchronize();   // queued steps may still read the universe graph
    l.uni.reset();
    legacy_err(legacy_sync_sampler(l));
}

// ----------------------------------------------------------------------- test / valid ----------
// A test / valid / train / triple2id list under the current record format (graph.h record_count).
static bool read_list(const std::string &path, std::vector<pt::Triple> &out) {
    bool ok = true;
    std::string err;
    const int64_t n = pt::record_count(path, &ok, &err);
    if (!ok) return false;
    return pt::read_triples(path, n, out) && (!pt::count_header() || (int64_t)out.size() == n);
}

extern "C" void activateLoadOfAllTriples(int64_t) { L().load_all = true; }

extern "C" void importTestFiles(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    bool ok = true;
    l.rel_total = pt::record_count(l.in_path + "relation2id.txt", &ok);
    l.ent_total = pt::record_count(l.in_path + "entity2id.txt", &ok);
    std::vector<pt::Triple> train_all;
    l.import_rc = PT_EIO;
    if (!ok || !read_list(l.in_path + "test2id.txt", l.test) || !read_list(l.in_path + "train2id.txt", train_all) ||
        !read_list(l.in_path + "valid2id.txt", l.valid))
        return legacy_err(pt::fail(PT_EIO, "importTestFiles: missing or malformed test/train/valid file under " +
                                               l.in_path));
    l.test_total = (int64_t)l.test.size();
    l.valid_total = (int64_t)l.valid.size();
    l.train_lines = (int64_t)train_all.size();
    std::vector<pt::Triple> all;
    if (l.load_all) {
        if (!read_list(l.in_path + "triple2id.txt", all))
            return legacy_err(pt::fail(PT_EIO, "importTestFiles: triple2id.txt missing"));
    } else {
        all = l.test;
        all.insert(all.end(), train_all.begin(), train_all.end());
        all.insert(all.end(), l.valid.begin(), l.valid.end());
    }
    l.triple_total = (int64_t)all.size();
    // type lists read for an earlier import belong to that dataset: a type-constrained ranking of this one
    // reads its own type_constrain.txt (importTypeFiles again, or the drop-in Tester's load on first use)
    l.types_loaded = false;
    std::vector<int64_t> h(all.size()), t(all.size()), r(all.size());
    for (size_t i = 0; i < all.size(); ++i) { h[i] = all[i].h; t[i] = all[i].t; r[i] = all[i].r; }
    pt_known *k = nullptr;
    pt_known_create(h.data(), t.data(), r.data(), (int64_t)all.size(), &k);
    if (l.known) pt_known_free(l.known);
    l.known = k;
    l.import_rc = PT_OK;
    std::sort(l.test.begin(), l.test.end(), pt::cmp_rel2);    // Reader.h:311-312
    std::sort(l.valid.begin(), l.valid.end(), pt::cmp_rel2);
    printf("The total of test triples is %ld.\n", (long)l.test_total);
}

namespace pt {
void rank_one(const pt_known &k, int64_t E, int64_t h, int64_t t, int64_t r, int side, const float *con,
              int64_t *raw, int64_t *filt);
bool known_has(const pt_known &k, int64_t h, int64_t t, int64_t r);
}

// ------------------------------------------------------------------ triple classification -------
namespace {
// corrupt_head / corrupt_tail with the known-triple filter (Corrupt.h:9-105, filter_flag true) over the
// training graph's sorted lists on the host: heads = 1 draws a replacement TAIL for (key = h, r) from
// trainHead, heads = 0 a replacement HEAD for (key = t, r) from trainTail. An entity without training
// triples makes the reference read trainHead[-1] (its ll is -1): that is the calloc block's header,
// larger than any entity id, so `tmp < trainHead[ll].t` holds and the draw is returned as is - emulated
// by reading index -1 as "larger than every id" (index n, never reached by a non-empty list, likewise).
int64_t host_corrupt(const pt::Graph &g, bool heads, int64_t key, int64_t r, uint64_t &state) {
    const std::vector<pt::Triple> &L = heads ? g.head : g.tail;
    const std::vector<int64_t> &lef = heads ? g.lef_head : g.lef_tail, &rig = heads ? g.rig_head : g.rig_tail;
    const int64_t n = (int64_t)L.size();
    auto val = [&](int64_t k) -> int64_t {
        if (k < 0 || k >= n) return INT64_MAX / 4;
        return heads ? L[(size_t)k].t : L[(size_t)k].h;
    };
    int64_t lo = lef[(size_t)key] - 1, hi = rig[(size_t)key], mid;
    while (lo + 1 < hi) {
        mid = (lo + hi) >> 1;
        if (L[(size_t)mid].r >= r) hi = mid; else lo = mid;
    }
    const int64_t ll = hi;
    lo = lef[(size_t)key];
    hi = rig[(size_t)key] + 1;
    while (lo + 1 < hi) {
        mid = (lo + hi) >> 1;
        if (L[(size_t)mid].r <= r) lo = mid; else hi = mid;
    }
    const int64_t rr = lo;
    state = state * 25214903917ULL + 11ULL;   // randd (Random.h:18-22)
    const int64_t tmp = (int64_t)(state % (uint64_t)(g.ent_total - (rr - ll + 1)));
    if (tmp < val(ll)) return tmp;
    if (tmp > val(rr) - rr + ll - 1) return tmp + rr - ll + 1;
    lo = ll;
    hi = rr + 1;
    while (lo + 1 < hi) {
        mid = (lo + hi) >> 1;
        if (val(mid) - mid + ll - 1 < tmp) lo = mid; else hi = mid;
    }
    return tmp + lo - ll + 1;
}
}  // namespace

// getTestBatch (Test.h:576-599): the test triples and one negative each - a coin from sampler thread 0
// (randd(0) % 1000 < 500) picks corrupt_head(0, h, r) (new tail) or corrupt_tail(0, t, r) (new head).
// The stream is the process-global sampler's thread 0 (device-resident here: read, advanced, written
// back), so the negatives continue the same random sequence as in the reference.
extern "C" void getTestBatch(int64_t *ph, int64_t *pt_, int64_t *pr, int64_t *nh, int64_t *nt, int64_t *nr) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    pt::Graph *g = l.train.get();
    if (!g || g->ent_total < 2) {
        legacy_err(pt::fail(PT_ESTATE, "getTestBatch: importTrainFiles() first"));
        return;
    }
    uint64_t s0 = l.states.empty() ? 0 : l.states[0];
    if (l.sampler_ready && hipMemcpy(&s0, l.sampler.d_states, sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) {
        legacy_err(pt::fail(PT_EHIP, "getTestBatch: reading the sampler state failed"));
        return;
    }
    for (size_t i = 0; i < l.test.size(); ++i) {
        const pt::Triple &q = l.test[i];
        pt::Triple neg = q;
        s0 = s0 * 25214903917ULL + 11ULL;
        if ((int64_t)(s0 % 1000ULL) < 500) neg.t = host_corrupt(*g, true, q.h, q.r, s0);
        else neg.h = host_corrupt(*g, false, q.t, q.r, s0);
        ph[i] = q.h; pt_[i] = q.t; pr[i] = q.r;
        nh[i] = neg.h; nt[i] = neg.t; nr[i] = neg.r;
    }
    if (!l.states.empty()) l.states[0] = s0;
    if (l.sampler_ready &&
        hipMemcpy(l.sampler.d_states, &s0, sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        legacy_err(pt::fail(PT_EHIP, "getTestBatch: writing the sampler state failed"));
}

extern "C" void initTest(void) {
    Legacy &l = L();
    l.last_head = l.last_tail = 0;
    l.acc = TestAcc{};
    l.acc_tc = TestAcc{};
}

static void fill_batch(const pt::Triple &q, int64_t E, int side, int64_t *ph, int64_t *pt_, int64_t *pr) {
    ph[0] = q.h; pt_[0] = q.t; pr[0] = q.r;
    const int64_t truth = side == 0 ? q.h : q.t;
    for (int64_t i = 1; i < E; ++i) {
        const int64_t c = i - 1 < truth ? i - 1 : i;
        ph[i] = side == 0 ? c : q.h;
        pt_[i] = side == 0 ? q.t : c;
        pr[i] = q.r;
    }
}

extern "C" void getHeadBatch(int64_t *ph, int64_t *pt_, int64_t *pr) {
    Legacy &l = L();
    fill_batch(l.test[(size_t)l.last_head++], l.ent_total, 0, ph, pt_, pr);
}
extern "C" void getTailBatch(int64_t *ph, int64_t *pt_, int64_t *pr) {
    Legacy &l = L();
    fill_batch(l.test[(size_t)l.last_tail++], l.ent_total, 1, ph, pt_, pr);
}

static void accumulate(TestAcc &a, int side, int64_t raw, int64_t filt) {
    float &ft = side == 0 ? a.l_filter_tot : a.r_filter_tot, &f3 = side == 0 ? a.l3_filter_tot : a.r3_filter_tot,
          &f1 = side == 0 ? a.l1_filter_tot : a.r1_filter_tot, &fr = side == 0 ? a.l_filter_rank : a.r_filter_rank,
          &fi = side == 0 ? a.l_filter_reci : a.r_filter_reci;
    float &rt = side == 0 ? a.l_tot : a.r_tot, &r3 = side == 0 ? a.l3_tot : a.r3_tot,
          &r1 = side == 0 ? a.l1_tot : a.r1_tot, &rr = side == 0 ? a.l_rank : a.r_rank,
          &ri = side == 0 ? a.l_reci : a.r_reci;
    if (filt < 10) ft += 1;
    if (raw < 10) rt += 1;
    if (filt < 3) f3 += 1;
    if (raw < 3) r3 += 1;
    if (filt < 1) f1 += 1;
    if (raw < 1) r1 += 1;
    fr += (float)(filt + 1);
    rr += (float)(1 + raw);
    fi = (float)((double)fi + 1.0 / (double)(filt + 1));
    ri = (float)((double)ri + 1.0 / (double)(raw + 1));
}

// importTypeFiles (Reader.h:352-396): `type_constrain.txt` in the input folder - a count, then for each of
// relationTotal relations a line of head types and a line of tail types, `r n e_1 .. e_n`; every list is
// sorted in place. (The reference's Python never calls it; testHead/testTail with type_constrain read
// these arrays.)
extern "C" void importTypeFiles(void) {
    Legacy &l = L();
    std::lock_guard<std::mutex> lk(l.mu);
    const std::string path = l.in_path + "type_constrain.txt";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return legacy_err(pt::fail(PT_EIO, "importTypeFiles: cannot open " + path));
    const int64_t R = l.rel_total;
    for (int s = 0; s < 2; ++s) {
        l.type_lef[s].assign((size_t)R, 0);
        l.type_rig[s].assign((size_t)R, 0);
        l.type_list[s].clear();
    }
    long tmp = 0;
    bool ok = fscanf(f, "%ld", &tmp) == 1;
    for (int64_t i = 0; ok && i < R; ++i) {
        for (int s = 0; s < 2 && ok; ++s) {
            long rel = 0, tot = 0;
            ok = fscanf(f, "%ld %ld", &rel, &tot) == 2 && rel >= 0 && rel < R && tot >= 0;
            if (!ok) break;
            std::vector<int64_t> &v = l.type_list[s];
            l.type_lef[s][(size_t)rel] = (int64_t)v.size();
            for (long j = 0; j < tot && ok; ++j) {
                long e = 0;
                ok = fscanf(f, "%ld", &e) == 1;
                v.push_back(e);
            }
            l.type_rig[s][(size_t)rel] = (int64_t)v.size();
            std::sort(v.begin() + l.type_lef[s][(size_t)rel], v.end());
        }
    }
    fclose(f);
    l.types_loaded = ok;
    if (!ok) legacy_err(pt::fail(PT_EIO, "importTypeFiles: malformed " + path));
}

// Type-constrained counts of one query (Test.h:168-178 / :288-298). The reference walks candidate
// POSITIONS j = 1..E-1 and matches j against the relation's sorted type list as an ENTITY id, so the
// score it compares for type entity j is con[j] (the candidate at position j) and the filter asks
// _find about entity j; nothing is counted when con[0] == inf. Restated as is.
static void rank_constrained(const Legacy &l, const pt::Triple &q, int side, const float *con, int64_t *raw,
                             int64_t *filt) {
    int64_t s = 0, fs = 0;
    const float minimal = con[0];
    if (minimal != INFINITY) {
        const std::vector<int64_t> &v = l.type_list[side];
        const int64_t lo = l.type_lef[side][(size_t)q.r], hi = l.type_rig[side][(size_t)q.r];
        for (int64_t k = lo; k < hi; ++k) {
            const int64_t j = v[(size_t)k];
            if (j < 1 || j >= l.ent_total || (k > lo && v[(size_t)k - 1] == j)) continue;
            if (con[j] < minimal) {
                ++s;
                if (!(side == 0 ? pt::known_has(*l.known, j, q.t, q.r) : pt::known_has(*l.known, q.h, j, q.r))) ++fs;
            }
        }
    }
    *raw = s;
    *filt = fs;
}

static void test_one(float *con, int64_t idx, int64_t type_constrain, int side) {
    Legacy &l = L();
    const pt::Triple &q = l.test[(size_t)idx];
    int64_t raw, filt;
    pt::rank_one(*l.known, l.ent_total, q.h, q.t, q.r, side, con, &raw, &filt);
    accumulate(l.acc, side, raw, filt);
    if (type_constrain) {
        if (!l.types_loaded) {
            legacy_err(pt::fail(PT_ESTATE, "type_constrain needs importTypeFiles() first (the reference reads "
                                           "unallocated type arrays, Test.h:127-130)"));
            return;
        }
        rank_constrained(l, q, side, con, &raw, &filt);
        accumulate(l.acc_tc, side, raw, filt);
    }
}
extern "C" void testHead(float *con, int64_t idx, int64_t type_constrain) { test_one(con, idx, type_constrain, 0); }
extern "C" void testTail(float *con, int64_t idx, int64_t type_constrain) { test_one(con, idx, type_constrain, 1); }

// test_link_prediction's averaging (Test.h:408-454, constrained block :456-502)
static void finish_acc(TestAcc &a, float n, float out[5]) {
    a.l_rank /= n; a.r_rank /= n; a.l_reci /= n; a.r_reci /= n;
    a.l_tot /= n; a.l3_tot /= n; a.l1_tot /= n; a.r_tot /= n; a.r3_tot /= n; a.r1_tot /= n;
    a.l_filter_rank /= n; a.r_filter_rank /= n; a.l_filter_reci /= n; a.r_filter_reci /= n;
    a.l_filter_tot /= n; a.l3_filter_tot /= n; a.l1_filter_tot /= n;
    a.r_filter_tot /= n; a.r3_filter_tot /= n; a.r1_filter_tot /= n;
    out[0] = (a.l_filter_reci + a.r_filter_reci) / 2;
    out[1] = (a.l_filter_rank + a.r_filter_rank) / 2;
    out[2] = (a.l_filter_tot + a.r_filter_tot) / 2;
    out[3] = (a.l3_filter_tot + a.r3_filter_tot) / 2;
    out[4] = (a.l1_filter_tot + a.r1_filter_tot) / 2;
}

extern "C" void test_link_prediction(int64_t type_constrain) {
    Legacy &l = L();
    if (type_constrain) {
        float m[5];
        finish_acc(l.acc_tc, (float)l.test_total, m);
        l.mrr_tc = m[0]; l.mr_tc = m[1]; l.hit10_tc = m[2]; l.hit3_tc = m[3]; l.hit1_tc = m[4];
        printf("type constraint results:\n");
        printf("averaged(filter):\t %f \t %f \t %f \t %f \t %f \n", m[0], m[1], m[2], m[3], m[4]);
    }
    TestAcc &a = l.acc;
    float m[5];
    finish_acc(a, (float)l.test_total, m);
    printf("metric:\t\t\t MRR \t\t MR \t\t hit@10 \t hit@3  \t hit@1 \n");
    printf("averaged(raw):\t\t %f \t %f \t %f \t %f \t %f \n", (a.l_reci + a.r_reci) / 2, (a.l_rank + a.r_rank) / 2,
           (a.l_tot + a.r_tot) / 2, (a.l3_tot + a.r3_tot) / 2, (a.l1_tot + a.r1_tot) / 2);
    l.mrr = m[0]; l.mr = m[1]; l.hit10 = m[2]; l.hit3 = m[3]; l.hit1 = m[4];
    printf("averaged(filter):\t %f \t %f \t %f \t %f \t %f \n", l.mrr, l.mr, l.hit10, l.hit3, l.hit1);
}
extern "C" float getTestLinkMRR(int64_t tc) { return tc ? L().mrr_tc : L().mrr; }
extern "C" float getTestLinkMR(int64_t tc) { return tc ? L().mr_tc : L().mr; }
extern "C" float getTestLinkHit10(int64_t tc) { return tc ? L().hit10_tc : L().hit10; }
extern "C" float getTestLinkHit3(int64_t tc) { return tc ? L().hit3_tc : L().hit3; }
extern "C" float getTestLinkHit1(int64_t tc) { return tc ? L().hit1_tc : L().hit1; }

// the loaded type lists for the GPU ranking: side 0 heads, 1 tails; lef/rig per relation (relTotal
// entries each) and the lists; returns the list length (-1 before importTypeFiles). NULL outputs skip.
extern "C" int64_t pt_legacy_types(int32_t side, int64_t *lef, int64_t *rig, int64_t *list) {
    Legacy &l = L();
    if (!l.types_loaded || (side != 0 && side != 1)) return -1;
    const auto &lv = l.type_lef[side], &rv = l.type_rig[side], &tv = l.type_list[side];
    if (lef) std::copy(lv.begin(), lv.end(), lef);
    if (rig) std::copy(rv.begin(), rv.end(), rig);
    if (list) std::copy(tv.begin(), tv.end(), list);
    return (int64_t)tv.size();
}

extern "C" void validInit(void) {
    Legacy &l = L();
    l.last_vhead = l.last_vtail = 0;
    l.l_valid = l.r_valid = 0;
}
extern "C" void getValidHeadBatch(int64_t *ph, int64_t *pt_, int64_t *pr) {
    Legacy &l = L();
    fill_batch(l.valid[(size_t)l.last_vhead++], l.ent_total, 0, ph, pt_, pr);
}
extern "C" void getValidTailBatch(int64_t *ph, int64_t *pt_, int64_t *pr) {
    Legacy &l = L();
    fill_batch(l.valid[(size_t)l.last_vtail++], l.ent_total, 1, ph, pt_, pr);
}
extern "C" void validHead(float *con, int64_t idx) {
    Legacy &l = L();
    const pt::Triple &q = l.valid[(size_t)idx];
    int64_t raw, filt;
    pt::rank_one(*l.known, l.ent_total, q.h, q.t, q.r, 0, con, &raw, &filt);
    if (filt < 10) l.l_valid += 1;
}
extern "C" void validTail(float *con, int64_t idx) {
    Legacy &l = L();
    const pt::Triple &q = l.valid[(size_t)idx];
    int64_t raw, filt;
    pt::rank_one(*l.known, l.ent_total, q.h, q.t, q.r, 1, con, &raw, &filt);
    if (filt < 10) l.r_valid += 1;
}
extern "C" float getValidHit10(void) {
    Legacy &l = L();
    l.l_valid /= (float)l.valid_total;
    l.r_valid /= (float)l.valid_total;
    l.valid_hit10 = (l.l_valid + l.r_valid) / 2;
    return l.valid_hit10;
}

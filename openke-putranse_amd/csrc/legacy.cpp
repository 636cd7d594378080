// The reference's Base.so symbols of libputranse_hip.so (setInPath ... getValidHit10) and the pt_legacy_* accessors
// of their context. (The reentrant pt_* entry points are capi.cpp.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "graph.h"
#include "rng.h"
#include "trainer.h"
#include "universe.h"

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

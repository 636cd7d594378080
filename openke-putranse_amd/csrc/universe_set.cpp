// The universe-set runtime of libputranse_hip.so (include/putranse.h: pt_universe_set_*, pt_universes_train):
// plans a set of universes (kernel class per universe, one launch per class, CU share per launch, LDS plan),
// lays out its device workspace and trains it with the persistent multi-universe kernel (universes.hip).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "graph.h"
#include "ordered.h"
#include "universes.h"

// Streams of the universe trainer's concurrent class launches: created once per device for the whole process
// and shared by every set. Each is created with a CU mask that covers every CU: the runtime gives such a stream
// a hardware queue of its own instead of sharing one of the process's GPU_MAX_HW_QUEUES (4) queues with the
// caller's streams. With plain streams, a process that already held streams of its own (torch's, the C2 trainer's
// capture stream) got two class launches on one queue, where they ran one after the other (round 4: the C3 set
// 58.7 ms in the default bench process against 35.7 ms standalone).
namespace {
struct ClassStreamPool {
    std::mutex mu;
    std::map<int, std::vector<hipStream_t>> by_dev;   // device -> streams
    // destroyed when the library is unloaded (process exit): the HIP runtime, loaded before this library, is
    // finalized after it, so the queues are released while it still runs
    ~ClassStreamPool() {
        for (auto &kv : by_dev) {
            if (hipSetDevice(kv.first) != hipSuccess) continue;
            for (hipStream_t q : kv.second) (void)hipStreamDestroy(q);
        }
    }
};
ClassStreamPool &class_stream_pool() {
    static ClassStreamPool p;
    return p;
}
// n full-CU-mask streams of `device` (dedicated hardware queues), created on first use
hipError_t class_streams(int device, size_t n, std::vector<hipStream_t> *out) {
    ClassStreamPool &P = class_stream_pool();
    std::lock_guard<std::mutex> lk(P.mu);
    auto &v = P.by_dev[device];
    if (v.size() < n) {
        int cus = 0;
        hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        if (e != hipSuccess) return e;
        std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
        for (int c = 0; c < cus; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
        while (v.size() < n) {
            hipStream_t q = nullptr;
            e = hipExtStreamCreateWithCUMask(&q, (uint32_t)mask.size(), mask.data());
            if (e != hipSuccess) return e;
            v.push_back(q);
        }
    }
    out->assign(v.begin(), v.begin() + (std::ptrdiff_t)n);
    return hipSuccess;
}
}  // namespace

// Compatibility shim. Team universes (several workgroups training one universe) were measured slower at every
// width and removed (rounds 5 and 6); every universe trains on one workgroup, which is width 1.
// The switch stays for callers that set that width explicitly.
extern "C" int pt_set_universe_team_width(int32_t w) {
    PT_CHECK(w == 1, PT_ENOTSUP,
             "pt_set_universe_team_width: team universes were removed (DESIGN.md §4); the only width is 1");
    return PT_OK;
}
extern "C" int32_t pt_get_universe_team_width(void) { return 1; }

// Train many universes with the persistent multi-universe kernel (universes.hip).
struct pt_universe_set {
    int32_t model = 0, p_norm = 1, norm_flag = 1, opt = PT_ADAGRAD;
    int64_t bern = 0, filter = 0, neg = 1;
    int device = -1;
    void *arena = nullptr;
    pt::UniverseDev *d_us = nullptr;      // inside the arena, by row shape, longest-first inside a shape
    int *d_counter = nullptr;             // work-queue counters, one per shape group (inside the arena)
    struct Group {
        int shape;
        int64_t off, n;
        double work;
        int64_t share = 1;   // workgroups (= CUs) of its launch
    };
    std::vector<Group> groups;            // runs of d_us with one shape class (one kernel launch each)
    std::vector<hipEvent_t> events;
    std::vector<hipEvent_t> t_start, t_stop;   // per group launch: timing events of the last train call
    bool timed = false;                        // the last train call recorded them
    pt::UniverseLaunch cfg;
    std::vector<pt::UniverseDev> host;    // same order; loss pointers patched per train call
    std::vector<int64_t> host_loss_off;
    std::vector<int64_t> host_of_job;     // job index -> index in host / d_us
    std::vector<uint64_t> seeds0;         // [host][64]: the jobs' LCG states at creation (pt_universe_set_reset)
    void *graph_arena = nullptr;          // the universes' device graphs (one allocation, one copy)
    uint64_t *prof = nullptr;             // PT_UNI_PROF=1: [n][64] cycle counters + shape (device)
    // reference-order (deterministic) mode (pt_universe_set_deterministic): ordered.hip's universe kernel
    bool ordered = false;
    void *ord_arena = nullptr;            // per universe [4][seq][dim] gradient rows
    int64_t ord_max_seq = 0;
    ~pt_universe_set() {
        for (auto e : events) (void)hipEventDestroy(e);
        for (auto e : t_start) (void)hipEventDestroy(e);
        for (auto e : t_stop) (void)hipEventDestroy(e);
        if (arena) (void)hipFree(arena);
        if (prof) (void)hipFree(prof);
        if (ord_arena) (void)hipFree(ord_arena);
        if (graph_arena) (void)hipFree(graph_arena);
    }
};

// ---------------------------------------------------------------- the steps of pt_universe_set_create
namespace {
using Group = pt_universe_set::Group;

int64_t al(int64_t b) { return (b + 255) & ~int64_t(255); }
const pt::Graph &graph_of(const pt_universe_job &J) { return reinterpret_cast<const pt_graph *>(J.graph)->g; }

// the jobs' argument checks; *neg: the negatives per positive they share (-1: no jobs)
int check_jobs(const pt_universe_job *jobs, int64_t n, int32_t model, int32_t opt, int64_t *neg_out) {
    int64_t neg = -1;
    for (int64_t i = 0; i < n; ++i) {
        const pt_universe_job &J = jobs[i];
        PT_CHECK(J.graph && J.seeds && J.ent && J.rel, PT_EINVAL, "universe job: null graph / seeds / tables");
        PT_CHECK(model == 0 || J.normv, PT_EINVAL, "TransH universe job needs normv");
        PT_CHECK(opt == PT_SGD || (J.ent_acc && J.rel_acc && (model == 0 || J.norm_acc)), PT_EINVAL,
                 "Adagrad universe job needs accumulators");
        PT_CHECK(J.threads > 0 && J.threads <= 64, PT_EINVAL, "universe job: threads must be in [1, 64]");
        PT_CHECK(J.dim > 0 && pt::universe_shape_supported(J.dim, model), PT_EINVAL, "universe job: unsupported dim");
        PT_CHECK(J.batch_size >= 0 && J.epochs >= 0 && J.nbatches >= 0, PT_EINVAL, "universe job: negative sizes");
        PT_CHECK(neg < 0 || J.neg == neg, PT_EINVAL, "universe jobs must share neg");
        PT_CHECK(J.neg >= 1, PT_EINVAL, "universe job: neg must be >= 1");
        neg = J.neg;
        PT_CHECK(graph_of(J).train_total > 0 || J.batch_size == 0, PT_EINVAL, "universe job: empty graph");
        PT_CHECK(J.batch_size * (4 + J.neg) <= 16384, PT_EINVAL, "universe job: batch too large for the LDS work list");
    }
    *neg_out = neg;
    return PT_OK;
}

// layout of the per-universe workspace in one arena (byte offsets)
struct Slot {
    int64_t contrib, grad, flags;
};
struct ArenaPlan {
    std::vector<Slot> slots;   // per job
    int64_t us_off = 0;        // the UniverseDev array
    int64_t counter_off = 0;   // one work-queue counter per row shape
    int64_t total = 0;
};
ArenaPlan plan_arena(const pt_universe_job *jobs, int64_t n, int32_t model) {
    ArenaPlan A;
    A.slots.resize((size_t)n);
    // every universe's LCG states first, 64 words each in set order (one upload, one reset copy)
    int64_t total = al(512 * std::max<int64_t>(n, 1));
    for (int64_t i = 0; i < n; ++i) {
        const pt_universe_job &J = jobs[i];
        const pt::Graph &g = graph_of(J);
        const int64_t rows = g.ent_total + g.rel_total * (model == 1 ? 2 : 1);
        A.slots[i].contrib = total; total += al(4 * J.batch_size * (4 + J.neg) * J.dim);
        A.slots[i].grad = total;   total += al(4 * rows * J.dim);
        A.slots[i].flags = total;  total += al(4 * (g.ent_total + 2 * g.rel_total));
    }
    A.us_off = total;
    total += al((int64_t)sizeof(pt::UniverseDev) * std::max<int64_t>(n, 1));
    A.counter_off = total;
    total += al(sizeof(int) * 64);
    A.total = total;
    return A;
}

// A universe's time (the CU-share model and the queue order): steps x cycles per step, a fixed part plus a
// per-positive part that grows with the padded row (lanes x floats per lane) - fitted to every universe's
// measured cycles per step (r04, PT_UNI_PROF dumps of C3 and C4: 6,587 + bs x (63.3 + 0.681 x row slots);
// residual spread 18 % / 14 %, against 21 % / 20 % for the earlier fixed + rounds-of-positives model)
double universe_work(const pt_universe_job &J, int32_t model) {
    const int rs = pt::universe_shape_row_slots(pt::universe_shape_id(J.dim, model));
    return (double)J.epochs * (double)J.nbatches *
           (6587.0 + (double)std::max<int64_t>(J.batch_size, 1) * (63.3 + 0.681 * rs));
}

// Kernel (class) per universe: its row shape's class kernel, or - for up to three "hot" shapes of class 1
// (TransE), those holding the set's longest universes - a kernel compiled for that shape alone. A class
// kernel is register-allocated for all its shapes at once: the longest C3 universe's shape alone runs its
// chain in 78 instead of 94 Mcycles. At most four launches in all (the hardware queues a process gets).
std::vector<int> choose_classes(const pt_universe_job *jobs, int64_t n, int32_t model) {
    std::vector<int> cls_v((size_t)n);
    std::vector<int> shape_v((size_t)n);
    std::map<int, double> hot_cost;   // class-1 shape -> its longest universe (steps x (4 + rounds))
    for (int64_t i = 0; i < n; ++i) {
        shape_v[i] = pt::universe_shape_id(jobs[i].dim, model);
        cls_v[i] = pt::universe_shape_class(shape_v[i]);
        if (model != PT_TRANSE || cls_v[i] != 1) continue;
        const int64_t gpb = pt::universe_shape_groups(shape_v[i], model);
        const double c = (double)jobs[i].epochs * (double)jobs[i].nbatches *
                         (4.0 + (double)((std::max<int64_t>(jobs[i].batch_size, 1) + gpb - 1) / gpb));
        hot_cost[shape_v[i]] = std::max(hot_cost[shape_v[i]], c);
    }
    std::vector<std::pair<double, int>> cand;
    for (auto &kv : hot_cost) cand.push_back({kv.second, kv.first});
    std::sort(cand.begin(), cand.end(), std::greater<std::pair<double, int>>());
    std::set<int> hot;
    for (auto &c : cand) {
        if (hot.size() >= 3) break;
        std::set<int> h2 = hot;
        h2.insert(c.second);
        std::set<int> launches;
        for (int64_t i = 0; i < n; ++i)
            launches.insert(h2.count(shape_v[i]) ? pt::kUniHotBase + shape_v[i] : cls_v[i]);
        if (launches.size() > 4) break;
        hot = h2;
    }
    for (int64_t i = 0; i < n; ++i)
        if (hot.count(shape_v[i])) cls_v[i] = pt::kUniHotBase + shape_v[i];
    return cls_v;
}

// one persistent launch per class, its universes longest dependent step chain first (the work queue then
// approximates longest-processing-time scheduling over the launch's workgroups). *order: the set order (job
// indices by class, then by work, longest first); returns its runs of one class
std::vector<Group> build_groups(const std::vector<int> &cls_v, const std::vector<double> &works,
                                std::vector<int64_t> *order) {
    const int64_t n = (int64_t)cls_v.size();
    order->resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) (*order)[i] = i;
    std::stable_sort(order->begin(), order->end(), [&](int64_t a, int64_t b) {
        const int sa = cls_v[(size_t)a], sb = cls_v[(size_t)b];
        if (sa != sb) return sa < sb;
        return works[(size_t)a] > works[(size_t)b];
    });
    std::vector<Group> groups;
    for (int64_t k = 0; k < n; ++k) {
        const int sh = cls_v[(size_t)(*order)[k]];
        if (groups.empty() || groups.back().shape != sh) groups.push_back({sh, k, 0, 0.0});
        groups.back().n += 1;
        groups.back().work += works[(size_t)(*order)[k]];
    }
    return groups;
}

// CU shares: a universe's time by the step-cost model (universe_work); give every group one CU,
// then each further CU to the group whose LPT makespan over its current share is longest (the launches run
// concurrently, so the slowest group ends the set)
// (the step-cost model: with it the shares no longer leave C3's float4 hot launch ending 2 ms after
// the longest universe, which the rounds-of-positives model did)
void assign_cu_shares(std::vector<Group> &groups, const std::vector<int64_t> &order, const std::vector<double> &works,
                      int cus) {
    std::vector<std::vector<double>> tg(groups.size());
    for (size_t k = 0; k < groups.size(); ++k) {
        const auto &gr = groups[k];
        for (int64_t q = gr.off; q < gr.off + gr.n; ++q) tg[k].push_back(works[(size_t)order[(size_t)q]]);
        std::sort(tg[k].begin(), tg[k].end(), std::greater<double>());
    }
    auto makespan = [&](size_t k, int64_t s) {
        std::priority_queue<double, std::vector<double>, std::greater<double>> m;
        for (int64_t i = 0; i < s; ++i) m.push(0.0);
        double end = 0;
        for (double t : tg[k]) {
            const double f = m.top() + t;
            m.pop();
            m.push(f);
            end = std::max(end, f);
        }
        return end;
    };
    std::vector<double> ms(groups.size());
    int64_t left = (int64_t)cus;
    for (size_t k = 0; k < groups.size(); ++k) {
        ms[k] = makespan(k, 1);
        left -= groups[k].share;
    }
    for (; left > 0; --left) {
        size_t best = groups.size();
        for (size_t k = 0; k < groups.size(); ++k)
            if (groups[k].share < groups[k].n && (best == groups.size() || ms[k] > ms[best])) best = k;
        if (best == groups.size()) break;
        groups[best].share += 1;
        ms[best] = makespan(best, groups[best].share);
    }
}

// the universes' device graphs: host images built on worker threads (each distinct graph once), placed in
// one allocation (*arena) with one copy
struct GraphImages {
    std::vector<const pt::Graph *> uniq;   // the distinct graphs
    std::vector<int64_t> gidx;             // per job: its graph in uniq
    std::vector<int64_t> goff;             // per distinct graph: byte offset of its image in the arena
};
int upload_graph_images(const pt_universe_job *jobs, int64_t n, void **arena, GraphImages *out) {
    std::vector<const pt::Graph *> &uniq = out->uniq;
    out->gidx.resize((size_t)n);
    {
        std::unordered_map<const pt::Graph *, int64_t> seen;
        for (int64_t i = 0; i < n; ++i) {
            const pt::Graph *gp = &graph_of(jobs[i]);
            auto it = seen.find(gp);
            if (it == seen.end()) {
                it = seen.emplace(gp, (int64_t)uniq.size()).first;
                uniq.push_back(gp);
            }
            out->gidx[i] = it->second;
        }
    }
    std::vector<std::vector<char>> images(uniq.size());
    {
        std::atomic<int64_t> next{0};
        auto work = [&]() {
            for (int64_t k; (k = next.fetch_add(1)) < (int64_t)uniq.size();)
                images[k] = const_cast<pt::Graph *>(uniq[k])->device_image();
        };
        const int64_t nw = std::min<int64_t>(std::max(1u, std::thread::hardware_concurrency()), 16);
        std::vector<std::thread> pool;
        for (int64_t w = 1; w < std::min<int64_t>(nw, (int64_t)uniq.size()); ++w) pool.emplace_back(work);
        work();
        for (auto &th : pool) th.join();
    }
    std::vector<int64_t> &goff = out->goff;
    goff.assign(uniq.size() + 1, 0);
    for (size_t k = 0; k < uniq.size(); ++k) goff[k + 1] = goff[k] + al((int64_t)images[k].size());
    std::vector<char> staging((size_t)std::max<int64_t>(goff.back(), 1));
    for (size_t k = 0; k < uniq.size(); ++k) memcpy(staging.data() + goff[k], images[k].data(), images[k].size());
    PT_HIP(hipMalloc(arena, staging.size()));
    PT_HIP(hipMemcpy(*arena, staging.data(), staging.size(), hipMemcpyHostToDevice));
    return PT_OK;
}

// the set's largest sizes: the launches' LDS is sized for them
struct Maxima {
    int64_t bs = 0, relg = 0, ent = 0, rel = 0, seq = 0, nb = 0;
};

// LDS plan (within the device's per-workgroup limit and half a CU): the work list is required;
// then, each if it still fits, the relation gradient rows (the contended rows of the scatter), the
// entity contribution lists (replace the entity float atomics), the touched flags, and as many
// presampled batches as fit
int plan_lds(pt::UniverseLaunch &C, const Maxima &M, int64_t lds_budget, int32_t model, int64_t neg) {
    C.list_cap = std::max<int64_t>(M.bs * (4 + neg), 1);
    auto a4 = [](int64_t v) { return 4 * ((v + 3) & ~int64_t(3)); };
    const int64_t list_b = a4(C.list_cap);
    const int64_t relg_b = 4 * M.relg * (model == 1 ? 2 : 1);
    int64_t used = list_b;
    PT_CHECK(used <= lds_budget, PT_EINVAL, "universe batch too large for the LDS work list");
    const int64_t per_batch = 12 * M.seq;
    // entity rows as contribution lists (heads for entities and relations, next per slot)
    const int64_t heads_b = a4(M.ent + 2 * M.rel) + a4(M.bs * (4 + neg));
    C.contrib = used + heads_b <= lds_budget;
    used += C.contrib ? heads_b : 0;
    // relation rows: LDS gradient rows (hot rows, few) if they fit, else contribution lists
    C.lds_relgrad = used + relg_b <= lds_budget;
    C.rel_list = C.contrib && !C.lds_relgrad;
    used += C.lds_relgrad ? relg_b : 0;
    // touched flags of the rows that are not lists
    const int64_t nfl = (C.contrib ? 0 : M.ent) + (C.rel_list ? 0 : 2 * M.rel);
    const int64_t flags_b = a4(nfl);
    C.lds_flags = nfl > 0 && used + flags_b <= lds_budget;
    used += C.lds_flags ? flags_b : 0;
    C.pchunk = per_batch > 0 ? std::min<int64_t>(M.nb, (lds_budget - used) / per_batch) : 0;
    if (C.pchunk < 0) C.pchunk = 0;
    used += C.pchunk * per_batch;
    C.lds_bytes = used;
    // agent-scope fences only while some gradient row is a global float atomic (or a flag global)
    C.agent_fence = !(C.contrib && (C.rel_list || (C.lds_relgrad && C.lds_flags)));
    C.threads = 512;
    return PT_OK;
}
}  // namespace

extern "C" int pt_universe_set_create(const pt_universe_job *jobs, int64_t n, int32_t model, int32_t p_norm,
                                      int32_t norm_flag, int32_t opt, int64_t bern, int64_t filter,
                                      pt_universe_set **out) {
    PT_CHECK(out && (jobs || n == 0), PT_EINVAL, "pt_universe_set_create: null argument");
    PT_CHECK(model != PT_TRANSD, PT_ENOTSUP, "PuTransD universes are not built yet (PT_TRANSD trains one model only)");
    PT_CHECK(model != PT_ROTATE, PT_ENOTSUP, "PT_ROTATE trains and ranks one model only: universes are not implemented");
    PT_CHECK(model != PT_DISTMULT, PT_ENOTSUP,
             "PT_DISTMULT trains and ranks one model only: universes are not implemented");
    PT_CHECK(model != PT_COMPLEX, PT_ENOTSUP, "PT_COMPLEX trains and ranks one model only: universes are not implemented");
    PT_CHECK(model == 0 || model == 1, PT_EINVAL, "model must be 0 (TransE) or 1 (TransH)");
    PT_CHECK(p_norm == 1 || p_norm == 2, PT_EINVAL, "p_norm must be 1 or 2");
    PT_CHECK(opt == PT_SGD || opt == PT_ADAGRAD, PT_EINVAL, "opt must be PT_SGD or PT_ADAGRAD");
    auto set = std::make_unique<pt_universe_set>();
    set->model = model; set->p_norm = p_norm; set->norm_flag = norm_flag; set->opt = opt;
    set->bern = bern; set->filter = filter;
    PT_HIP(hipGetDevice(&set->device));
    int64_t neg = -1;
    if (int rc = check_jobs(jobs, n, model, opt, &neg)) return rc;
    set->neg = neg < 0 ? 1 : neg;
    const ArenaPlan arena = plan_arena(jobs, n, model);
    PT_HIP(hipMalloc(&set->arena, (size_t)arena.total));
    char *base = (char *)set->arena;
    PT_HIP(hipMemset(base, 0, (size_t)arena.us_off));
    // LDS budget per universe workgroup: the device's per-workgroup limit, at most half a CU, minus the
    // kernel's static LDS. (The workgroups run one per CU at 256 VGPRs, but the whole CU's LDS measured
    // slower: C5 37.6 -> 352 ms, C4 104 -> 107 ms, C3 unchanged.)
    int max_lds = 64 << 10;
    (void)hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, set->device);
    const int64_t lds_budget = std::min<int64_t>(max_lds, 80 << 10) - 1024 - 2048;   // (2 KB: the static PreTables)
    int cus = 0;
    PT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, set->device));

    // the plan: a kernel class per universe, one launch per class, a CU share per launch
    std::vector<double> works((size_t)n);
    for (int64_t i = 0; i < n; ++i) works[i] = universe_work(jobs[i], model);
    const std::vector<int> cls_v = choose_classes(jobs, n, model);
    std::vector<int64_t> order;
    set->groups = build_groups(cls_v, works, &order);
    PT_CHECK(set->groups.size() <= 64, PT_EINVAL, "too many universe shape classes");
    assign_cu_shares(set->groups, order, works, cus);

    set->d_us = (pt::UniverseDev *)(base + arena.us_off);
    set->d_counter = (int *)(base + arena.counter_off);
    set->host.reserve((size_t)n);
    int64_t loss_off = 0;
    std::vector<int64_t> loss_of((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        loss_of[i] = loss_off;
        loss_off += jobs[i].epochs;
    }
    GraphImages gi;
    if (int rc = upload_graph_images(jobs, n, &set->graph_arena, &gi)) return rc;
    // the universes' descriptors, in set order
    Maxima M;
    set->seeds0.assign((size_t)(64 * std::max<int64_t>(n, 1)), 0);
    for (int64_t i : order) {
        const pt_universe_job &J = jobs[i];
        const pt::Graph &g = *gi.uniq[(size_t)gi.gidx[i]];
        const int64_t k = (int64_t)set->host.size();   // position in the set
        pt::UniverseDev U{};
        U.g = g.bind_image((char *)set->graph_arena + gi.goff[(size_t)gi.gidx[i]]);
        U.states = (uint64_t *)(base + 512 * k);
        std::copy(J.seeds, J.seeds + J.threads, set->seeds0.begin() + 64 * k);
        U.ent = J.ent; U.rel = J.rel; U.normv = J.normv;
        U.ent_acc = J.ent_acc; U.rel_acc = J.rel_acc; U.norm_acc = J.norm_acc;
        float *gr = (float *)(base + arena.slots[i].grad);
        U.gent = gr;
        U.grel = gr + g.ent_total * J.dim;
        U.gnorm = model == 1 ? U.grel + g.rel_total * J.dim : nullptr;
        int32_t *fl = (int32_t *)(base + arena.slots[i].flags);
        U.fent = fl;
        U.frel = fl + g.ent_total;
        U.fnorm = U.frel + g.rel_total;
        U.contrib = (float *)(base + arena.slots[i].contrib);
        U.losses = nullptr;
        U.prof = nullptr;   // pt_universe_set_profiling
        U.threads = J.threads; U.bs = J.batch_size; U.nbatches = J.nbatches; U.epochs = J.epochs; U.dim = J.dim;
        U.lr = J.lr; U.margin = J.margin;
        U.shape = pt::universe_shape_id(J.dim, model);
        if (set->host_of_job.empty()) set->host_of_job.assign((size_t)n, -1);
        set->host_of_job[(size_t)i] = (int64_t)set->host.size();
        set->host.push_back(U);
        set->host_loss_off.push_back(loss_of[i]);
        M.bs = std::max(M.bs, J.batch_size);
        M.relg = std::max(M.relg, g.rel_total * J.dim);
        M.ent = std::max(M.ent, g.ent_total);
        M.rel = std::max(M.rel, g.rel_total);
        M.seq = std::max(M.seq, J.batch_size * (1 + J.neg));
        M.nb = std::max(M.nb, J.nbatches);
    }
    if (n > 0) PT_HIP(hipMemcpy(base, set->seeds0.data(), 8 * set->seeds0.size(), hipMemcpyHostToDevice));
    if (int rc = plan_lds(set->cfg, M, lds_budget, model, set->neg)) return rc;
    *out = set.release();
    return PT_OK;
}

extern "C" int pt_universe_set_deterministic(pt_universe_set *set, int32_t on) {
    PT_CHECK(set, PT_EINVAL, "null universe set");
    // the set enters reference-order mode only once its workspace exists: a failed call leaves the mode as it
    // was (a later train call then runs the fast kernel, never the ordered one without its arena)
    if (!on || set->host.empty() || set->ord_arena) {
        set->ordered = on != 0;
        return PT_OK;
    }
    auto al = [](int64_t b) { return (b + 255) & ~int64_t(255); };
    int64_t total = 0, max_seq = 0;
    std::vector<int64_t> off(set->host.size());
    for (size_t i = 0; i < set->host.size(); ++i) {
        const pt::UniverseDev &U = set->host[i];
        const int64_t seq = U.bs * (1 + set->neg);
        off[i] = total;
        total += al(16 * seq * U.dim);
        max_seq = std::max(max_seq, seq);
    }
    // the launch's LDS (dynamic plan + the kernel's static variables) against the per-workgroup limit
    int blk_lds = 64 << 10;
    (void)hipDeviceGetAttribute(&blk_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, set->device);
    size_t static_lds = 0;
    PT_HIP(pt::ordered_universe_static_lds(&static_lds));
    PT_CHECK(pt::ordered_universe_lds_bytes(max_seq) + (int64_t)static_lds <= (int64_t)blk_lds, PT_ENOTSUP,
             "reference-order mode: universe batch too large for the LDS plan");
    void *arena = nullptr;
    PT_HIP(hipMalloc(&arena, (size_t)std::max<int64_t>(total, 256)));
    set->ord_arena = arena;
    for (size_t i = 0; i < set->host.size(); ++i) set->host[i].ord = (float *)((char *)set->ord_arena + off[i]);
    set->ord_max_seq = max_seq;
    set->ordered = true;
    return PT_OK;
}

extern "C" int pt_universe_set_train(pt_universe_set *set, float *d_losses, void *stream) {
    PT_CHECK(set, PT_EINVAL, "null universe set");
    if (set->host.empty()) return PT_OK;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < set->host.size(); ++i)
        set->host[i].losses = d_losses ? d_losses + set->host_loss_off[i] : nullptr;
    PT_HIP(hipMemcpyAsync(set->d_us, set->host.data(), sizeof(pt::UniverseDev) * set->host.size(),
                          hipMemcpyHostToDevice, st));
    if (set->ordered) {
        int cus = 0;
        PT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, set->device));
        const hipError_t e = pt::launch_universes_ordered(set->d_us, (int64_t)set->host.size(), set->d_counter, cus,
                                                          set->model, set->p_norm, set->norm_flag, set->opt, set->neg,
                                                          (int)set->bern, (int)set->filter, set->ord_max_seq, st);
        if (e != hipSuccess) return pt::fail(PT_EHIP, std::string("launch_universes_ordered: ") + hipGetErrorString(e));
        PT_HIP(hipStreamSynchronize(st));
        return PT_OK;
    }
    // one launch per shape class, concurrently, each over its share of the CUs (set at creation): forked from `st`
    // onto the process's class streams (each on a hardware queue of its own, class_streams) and joined back, so
    // the launches overlap whatever streams the caller's process already holds
    const size_t ng = set->groups.size();
    std::vector<hipStream_t> qs;
    PT_HIP(class_streams(set->device, ng, &qs));
    while (set->events.size() < ng + 1) {
        hipEvent_t ev;
        PT_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        set->events.push_back(ev);
    }
    while (set->t_start.size() < ng) {
        hipEvent_t a, b;
        PT_HIP(hipEventCreate(&a));
        PT_HIP(hipEventCreate(&b));
        set->t_start.push_back(a);
        set->t_stop.push_back(b);
    }
    PT_HIP(hipEventRecord(set->events[0], st));
    for (size_t k = 0; k < ng; ++k) PT_HIP(hipStreamWaitEvent(qs[k], set->events[0], 0));
    for (size_t k = 0; k < ng; ++k) {
        const auto &gr = set->groups[k];
        const int64_t share = gr.share;
        hipStream_t q = qs[k];
        PT_HIP(hipEventRecord(set->t_start[k], q));
        const hipError_t e = pt::launch_universes(set->d_us + gr.off, gr.n, set->d_counter + k, gr.shape, share,
                                                  set->model, set->p_norm, set->norm_flag, set->opt, set->neg,
                                                  (int)set->bern, (int)set->filter, set->cfg, q);
        if (e != hipSuccess) return pt::fail(PT_EHIP, std::string("launch_universes: ") + hipGetErrorString(e));
        PT_HIP(hipEventRecord(set->t_stop[k], q));
    }
    for (size_t k = 0; k < ng; ++k) {
        PT_HIP(hipEventRecord(set->events[k + 1], qs[k]));
        PT_HIP(hipStreamWaitEvent(st, set->events[k + 1], 0));
    }
    // the host array must outlive the async copy: this call returns only after it has been consumed
    PT_HIP(hipStreamSynchronize(st));
    set->timed = true;
    return PT_OK;
}

// the class launches of the last fast-path train call: per launch its start and end (ms after the earliest start,
// HIP events on the launch's stream) and its universe count; the launches overlap when they run concurrently
extern "C" int pt_universe_set_launch_times(pt_universe_set *set, int64_t cap, float *out, int64_t *n_out) {
    PT_CHECK(set && n_out, PT_EINVAL, "pt_universe_set_launch_times: null argument");
    const int64_t ng = set->timed ? (int64_t)set->groups.size() : 0;
    *n_out = ng;
    if (!out || ng == 0) return PT_OK;
    PT_CHECK(cap >= ng, PT_EINVAL, "pt_universe_set_launch_times: cap below the launch count");
    for (int64_t k = 0; k < ng; ++k) {
        float a = 0.f, b = 0.f;
        PT_HIP(hipEventElapsedTime(&a, set->t_start[0], set->t_start[(size_t)k]));
        PT_HIP(hipEventElapsedTime(&b, set->t_start[0], set->t_stop[(size_t)k]));
        out[3 * k] = a;
        out[3 * k + 1] = b;
        out[3 * k + 2] = (float)set->groups[(size_t)k].n;
    }
    float lo = out[0];
    for (int64_t k = 1; k < ng; ++k) lo = std::min(lo, out[3 * k]);
    for (int64_t k = 0; k < ng; ++k) {
        out[3 * k] -= lo;
        out[3 * k + 1] -= lo;
    }
    return PT_OK;
}

// whether universes of this dim train on the fast path (its row shape is compiled into its class kernel)
extern "C" int pt_universe_dim_supported(int64_t dim, int32_t model) {
    return (model == PT_TRANSE || model == PT_TRANSH) && pt::universe_shape_supported(dim, model) ? 1 : 0;
}

// the sampler streams back to the jobs' creation states (a benchmark re-runs the same training from the same
// start: the caller restores the tables and optimizer state)
extern "C" int pt_universe_set_reset(pt_universe_set *set) {
    PT_CHECK(set, PT_EINVAL, "null universe set");
    if (!set->host.empty())   // the states block at the arena's start, in set order
        PT_HIP(hipMemcpy(set->arena, set->seeds0.data(), 8 * set->seeds0.size(), hipMemcpyHostToDevice));
    return PT_OK;
}

extern "C" int pt_universe_set_states(pt_universe_set *set, int64_t job, uint64_t *out) {
    PT_CHECK(set && out, PT_EINVAL, "pt_universe_set_states: null argument");
    PT_CHECK(job >= 0 && job < (int64_t)set->host_of_job.size(), PT_EINVAL, "pt_universe_set_states: bad job index");
    const pt::UniverseDev &U = set->host[(size_t)set->host_of_job[(size_t)job]];
    PT_HIP(hipDeviceSynchronize());
    PT_HIP(hipMemcpy(out, U.states, sizeof(uint64_t) * (size_t)U.threads, hipMemcpyDeviceToHost));
    return PT_OK;
}

// per-universe cycle counters of the fast kernel (clock64 around its phases), off by default
extern "C" int pt_universe_set_profiling(pt_universe_set *set, int32_t on) {
    PT_CHECK(set, PT_EINVAL, "null universe set");
    if (on && !set->prof && !set->host.empty()) {
        PT_HIP(hipMalloc((void **)&set->prof, 512 * set->host.size()));
        PT_HIP(hipMemset(set->prof, 0, 512 * set->host.size()));
    }
    for (size_t i = 0; i < set->host.size(); ++i) set->host[i].prof = on && set->prof ? set->prof + 64 * i : nullptr;
    return PT_OK;
}

// diagnostics: per universe (set order) 64 words: cycles in presampling / phase A / phase B, steps, batch size,
// dim, entities, start / duration (100 MHz wall clock) of the last train call with profiling on; words 60-62
// (the removed team universes' width, barrier cycles and phase-B rows) and words 8-59 (the removed measurement
// build's phase stamps of one step) stay in the layout, reserved and zero; word 63: where the universe ran
extern "C" int pt_universe_set_profile(pt_universe_set *set, uint64_t *out) {
    PT_CHECK(set && out, PT_EINVAL, "null argument");
    PT_CHECK(set->prof, PT_ESTATE, "profiling not enabled (pt_universe_set_profiling)");
    PT_HIP(hipDeviceSynchronize());
    PT_HIP(hipMemcpy(out, set->prof, 512 * set->host.size(), hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_universe_set_free(pt_universe_set *set) {
    if (set) (void)hipDeviceSynchronize();
    delete set;
    return PT_OK;
}

extern "C" int pt_universes_train_ex(const pt_universe_job *jobs, int64_t n, int32_t model, int32_t p_norm,
                                     int32_t norm_flag, int32_t opt, int64_t bern, int64_t filter, int32_t flags,
                                     float *d_losses, void *stream) {
    PT_CHECK((flags & ~PT_DETERMINISTIC) == 0, PT_EINVAL, "pt_universes_train_ex: unknown flags");
    pt_universe_set *set = nullptr;
    int rc = pt_universe_set_create(jobs, n, model, p_norm, norm_flag, opt, bern, filter, &set);
    if (rc) return rc;
    if (flags & PT_DETERMINISTIC) rc = pt_universe_set_deterministic(set, 1);
    if (!rc) rc = pt_universe_set_train(set, d_losses, stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    pt_universe_set_free(set);
    if (!rc && e != hipSuccess) rc = pt::fail(PT_EHIP, std::string("pt_universes_train: ") + hipGetErrorString(e));
    return rc;
}

extern "C" int pt_universes_train(const pt_universe_job *jobs, int64_t n, int32_t model, int32_t p_norm,
                                  int32_t norm_flag, int32_t opt, int64_t bern, int64_t filter, float *d_losses,
                                  void *stream) {
    pt_universe_set *set = nullptr;
    int rc = pt_universe_set_create(jobs, n, model, p_norm, norm_flag, opt, bern, filter, &set);
    if (rc) return rc;
    rc = pt_universe_set_train(set, d_losses, stream);
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    pt_universe_set_free(set);
    if (!rc && e != hipSuccess) rc = pt::fail(PT_EHIP, std::string("pt_universes_train: ") + hipGetErrorString(e));
    return rc;
}

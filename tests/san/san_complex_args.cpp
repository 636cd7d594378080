// Sanitizer program (ASan + UBSan) for the HOST argument checks of PT_COMPLEX in capi.cpp, trainer.cpp and
// universe_set.cpp: the descriptor checks (null im tables, the dim rule, Adagrad sums of the im tables), the dim query
// and every universe entry point's refusal. None of these reaches a kernel launch or dereferences a table pointer. Where
// a device is present pt_trainer_create succeeds and the trainer-level refusals (loss, regulariser, reference-order
// mode, a sampler, captured runs) run too; without one it fails with PT_EHIP and they are skipped.
// Built and run by `make -C openke-putranse_amd san-complex`.
#include <cstdio>
#include <cstring>
#include <string>

#include "putranse.h"

static int failures = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::fprintf(stderr, "CHECK failed %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, pt_last_error()); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

static bool says(const char *word) { return std::strstr(pt_last_error(), word) != nullptr; }

int main() {
    static float tab[4][8 * 8];   // never read by the host checks
    pt_model_desc d;
    std::memset(&d, 0, sizeof d);
    d.model = PT_COMPLEX;
    d.p_norm = 7;   // (not read for PT_COMPLEX)
    d.opt = PT_SGD;
    d.ent_total = 8; d.rel_total = 8; d.dim = 8;
    d.ent = tab[0]; d.rel = tab[1];
    pt_trainer *t = nullptr;
    // the dim query answers 0 for the id; the dim rule is TransE's
    for (int64_t dim : {1, 200, 512, 513, 516, 1024, 1028}) CHECK(pt_model_dim_supported(dim, PT_COMPLEX) == 0);
    // null im tables
    CHECK(pt_trainer_create(&d, &t) == PT_EINVAL && says("PT_COMPLEX") && t == nullptr);
    float out[4];
    int64_t idx[4] = {0, 0, 0, 0};
    CHECK(pt_score(&d, 0, idx, idx, idx, 4, out, nullptr) == PT_EINVAL && says("PT_COMPLEX"));
    CHECK(pt_score_queries(&d, 0, idx, idx, idx, 4, out, nullptr) == PT_EINVAL && says("PT_COMPLEX"));
    CHECK(pt_score_rows(&d, 1, idx, idx, idx, 4, out, nullptr) == PT_EINVAL && says("PT_COMPLEX"));
    d.ent_transfer = tab[2]; d.rel_transfer = tab[3];
    // dims outside the rule
    for (int64_t dim : {0, 513, 514, 1028}) {
        d.dim = dim;
        CHECK(pt_trainer_create(&d, &t) == PT_ENOTSUP && says("ComplEx") && t == nullptr);
    }
    d.dim = 8;
    // Adagrad without the im tables' sums
    d.opt = PT_ADAGRAD;
    d.ent_acc = tab[0]; d.rel_acc = tab[1];
    CHECK(pt_trainer_create(&d, &t) == PT_EINVAL && says("Adagrad") && t == nullptr);
    d.opt = PT_SGD;
    // universes
    CHECK(pt_universe_dim_supported(20, PT_COMPLEX) == 0);
    pt_universe_job job;
    std::memset(&job, 0, sizeof job);
    pt_universe_set *set = nullptr;
    CHECK(pt_universe_set_create(&job, 1, PT_COMPLEX, 1, 1, PT_SGD, 0, 1, &set) == PT_ENOTSUP && says("PT_COMPLEX"));
    CHECK(pt_universes_train(&job, 1, PT_COMPLEX, 1, 1, PT_SGD, 0, 1, nullptr, nullptr) == PT_ENOTSUP &&
          says("PT_COMPLEX"));
    CHECK(pt_universes_train_ex(&job, 1, PT_COMPLEX, 1, 1, PT_SGD, 0, 1, 0, nullptr, nullptr) == PT_ENOTSUP &&
          says("PT_COMPLEX"));
    pt_lp_universe lu;
    pt_lp_pair pair;
    std::memset(&lu, 0, sizeof lu);
    std::memset(&pair, 0, sizeof pair);
    CHECK(pt_lp_min_scores(&lu, 1, PT_COMPLEX, 1, 1, &pair, 1, 8, out, nullptr, nullptr) == PT_ENOTSUP &&
          says("PT_COMPLEX"));
    // a complete descriptor: a trainer where a device is present
    const int rc = pt_trainer_create(&d, &t);
    CHECK((rc == PT_OK) == (t != nullptr));
    if (t) {
        pt_loss_desc l;
        std::memset(&l, 0, sizeof l);
        l.kind = PT_LOSS_MARGIN;
        CHECK(pt_trainer_set_loss(t, &l) == PT_ENOTSUP && says("PT_COMPLEX"));
        l.kind = PT_LOSS_SIGMOID;
        l.score_margin_flag = 1;
        CHECK(pt_trainer_set_loss(t, &l) == PT_ENOTSUP && says("PT_COMPLEX"));
        l.score_margin_flag = 0;
        CHECK(pt_trainer_set_loss(t, &l) == PT_OK);
        pt_regul_desc r = {1.0f, 0.0f, 1};
        CHECK(pt_trainer_set_regul(t, &r) == PT_ENOTSUP && says("PT_COMPLEX"));
        r.batch_mode = 0;
        r.l3_regul_rate = 1e-3f;
        CHECK(pt_trainer_set_regul(t, &r) == PT_ENOTSUP && says("PT_COMPLEX"));
        r.l3_regul_rate = 0.f;
        CHECK(pt_trainer_set_regul(t, &r) == PT_OK);
        CHECK(pt_trainer_set_deterministic(t, 1) == PT_ENOTSUP && says("PT_COMPLEX"));
        CHECK(pt_trainer_step(t, nullptr, 4, 2, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == PT_ENOTSUP &&
              says("PT_COMPLEX"));
        CHECK(pt_trainer_run(t, nullptr, 4, 2, 0, 0, 2, nullptr, nullptr) == PT_ENOTSUP && says("PT_COMPLEX"));
        pt_trainer_free(t);
    } else {
        std::fprintf(stderr, "no device: pt_trainer_create returned %d (%s); trainer-level checks skipped\n", rc,
                     pt_last_error());
    }
    std::fprintf(stderr, "san_complex_args: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}

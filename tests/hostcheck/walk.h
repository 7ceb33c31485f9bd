// TEST INFRASTRUCTURE. What the drivers of this directory share: the mock runtime's hooks (hipmock.cpp), random host data, the
// TRY / EXPECT_INVALID macros of a walk, and run_walks(), the common main: a clean walk, the count of fallible runtime calls it made,
// the walk with its refusals, a long-sequence walk, and -- with `sweep` -- the clean walk once per fallible call with that call
// failing. One driver per program: everything here is local to the translation unit that includes it.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "ppde_hip.h"

extern "C" long hipmock_calls();
extern "C" void hipmock_rearm(long fail_at);
extern "C" long hipmock_launches();
extern "C" long hipmock_allocs();
extern "C" long hipmock_writes();
extern "C" void hipmock_note(const char* text);   // a line of the driver's own in the mock's call trace (HIPMOCK_TRACE)

namespace {
std::mt19937 rng(7);
std::vector<float> rnd(size_t n, float s = 0.1f) {
    std::normal_distribution<float> d(0.f, s);
    std::vector<float> v(n);
    for (auto& x : v) x = d(rng);
    return v;
}
struct Ptrs { std::vector<std::vector<float>> store; std::vector<const float*> p; };
Ptrs many(int count, size_t n) { Ptrs r; for (int i = 0; i < count; ++i) r.store.push_back(rnd(n)); for (auto& v : r.store) r.p.push_back(v.data()); return r; }

// Inside a walk: `int status`, `bool verbose` and a label `done:` in front of the clean-up. WALK_FAIL is how a failed expectation
// leaves; a function without that label redefines it.
#define WALK_FAIL(code) do { status = (code); goto done; } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != PPDE_OK) { if (verbose) fprintf(stderr, "  %s -> %d (%s)\n", #x, rc_, ppde_last_error()); status = rc_; goto done; } } while (0)
// a refusal: PPDE_ERR_INVALID with a message (naming `word`, where one is given), and the runtime sees no launch, allocation, copy
// or fill across the call. The message goes into the call trace.
inline const char* walk_word(const char* word = "") { return word; }
#define EXPECT_INVALID(x, ...) do { const long l_ = hipmock_launches(), a_ = hipmock_allocs(), w_ = hipmock_writes(); int rc_ = (x); \
    hipmock_note(ppde_last_error()); \
    if (rc_ != PPDE_ERR_INVALID || !ppde_last_error()[0] || !strstr(ppde_last_error(), walk_word(__VA_ARGS__))) { \
        fprintf(stderr, "expected PPDE_ERR_INVALID with a message naming '%s' from %s, got %d (%s)\n", walk_word(__VA_ARGS__), #x, rc_, ppde_last_error()); \
        WALK_FAIL(99); } \
    if (hipmock_launches() != l_ || hipmock_allocs() != a_ || hipmock_writes() != w_) { \
        fprintf(stderr, "%s was refused after %ld launches, %ld allocations, %ld copies / fills\n", #x, hipmock_launches() - l_, \
                hipmock_allocs() - a_, hipmock_writes() - w_); WALK_FAIL(98); } } while (0)

// A walk returns the first non-OK status after releasing everything it created. `refusals`: also the calls that must be refused
// (left out of the failure sweep, where an injected failure in front of them would change what they answer).
using Walk = int (*)(int L, int Lp, int win, bool verbose, bool refusals);

// The common main. `line`: the driver's own last line, a format of the two counts. `more`: what the driver checks besides its walks.
int run_walks(int argc, char** argv, const char* line, Walk walk, int (*more)(bool verbose) = nullptr) {
    const bool sweep = argc > 1 && !strcmp(argv[1], "sweep");
    hipmock_rearm(-1);
    int rc = walk(48, 40, 4, true, false);
    if (rc != PPDE_OK) { fprintf(stderr, "clean walk failed: %d (%s)\n", rc, ppde_last_error()); return 1; }
    const long fallible = hipmock_calls();
    rng.seed(7);
    rc = walk(48, 40, 4, true, true);                                                // the same with the refusals in it
    if (rc != PPDE_OK) { fprintf(stderr, "walk with refusals failed: %d (%s)\n", rc, ppde_last_error()); return 1; }
    rc = walk(110, 100, 2, true, true);                                              // two logit groups per thread, chunked CNN, ring Potts kernel
    if (rc != PPDE_OK) { fprintf(stderr, "long-sequence walk failed: %d (%s)\n", rc, ppde_last_error()); return 1; }
    if (more && (rc = more(true)) != PPDE_OK) { fprintf(stderr, "further checks failed: %d (%s)\n", rc, ppde_last_error()); return 1; }
    long failures = 0;
    if (sweep) {
        for (long k = 1; k <= fallible; ++k) {
            rng.seed(7);
            hipmock_rearm(k);
            if (walk(48, 40, 4, false, false) != PPDE_OK) ++failures;                // must fail cleanly: the sanitizer reports anything left behind
        }
        hipmock_rearm(-1);
    }
    printf(line, fallible, failures);
    return 0;
}
}  // namespace

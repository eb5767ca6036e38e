// device_hold_check.cpp -- orc_rust_amd/csrc/device_hold.h (the text liborcgpu.so is built from) as a stand-alone program for the
// sanitizers: who frees a decoded result while device-resident batches view it.
//
// A scenario: a result with N exported arrays and M DLPack tensors.  Every export holds one reference on the same Hold, so which of
// them is released when makes no difference to it -- what counts is how many are out; they are released one by one, and at every
// point of that the owner lets go -- a reader moving on to its next stripe ("done": the result may be recycled), a reader closing, or a plain
// orcgpu_result_free.  Checked after every step: the result is not freed while an export is out; it is not in the spare list
// while an export is out; at the end it has been freed exactly once.  Use after free, double free and leaks are the sanitizers'.
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../orc_rust_amd/csrc/device_hold.h"

using namespace orcgpu_hold;

struct Fake {
  Hold* hold = nullptr;
  int* frees = nullptr;
  std::vector<int> arena = std::vector<int>(16, 7);  // something for the sanitizer to watch
};
static void destroy(void* p) {
  Fake* f = static_cast<Fake*>(p);
  ++*f->frees;
  delete f;
}

static long n_checks = 0;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    ++n_checks;                                                                              \
    if (!(cond)) {                                                                           \
      printf("FAILED %s (line %d): N=%d M=%d owner=%d at=%d\n", #cond, __LINE__, N, M, owner, at); \
      exit(1);                                                                               \
    }                                                                                        \
  } while (0)

enum Owner { READER_DONE_THEN_CLOSE = 0, READER_CLOSE_WHILE_CURRENT = 1, RESULT_FREE = 2, READER_DONE_CLOSE_LAST = 3 };

// the reader closes: what orcgpu_reader_close does with its spare list
static void close_home(Home& home) {
  for (void* p : home_close(home)) hold_owner_done(static_cast<Fake*>(p)->hold, false);
}

// the owner's step comes in front of release number `at` (at == K: behind the last)
static void scenario(int N, int M, int owner, int at) {
  const int K = N + M;
  int frees = 0;
  std::shared_ptr<Home> home = owner == RESULT_FREE ? nullptr : std::make_shared<Home>();
  Fake* f = new Fake();
  f->frees = &frees;
  f->hold = hold_new(f, destroy, home);
  Hold* h = f->hold;
  for (int k = 0; k < K; k++) hold_acquire(h);  // N arrays, then M tensors made from them
  CHECK(hold_exported(h));
  int out = K;
  bool closed = false;
  auto owner_step = [&] {
    if (owner == READER_DONE_THEN_CLOSE || owner == READER_DONE_CLOSE_LAST) {
      hold_owner_done(h, true);  // the reader moves on to the next stripe
      if (out > 0) CHECK(home_take(*home) == nullptr);  // a held result is not handed out for reuse
      CHECK(frees == 0);
      if (owner == READER_DONE_THEN_CLOSE) {
        close_home(*home);
        closed = true;
      }
    } else if (owner == READER_CLOSE_WHILE_CURRENT) {
      hold_owner_done(h, false);  // orcgpu_reader_close frees its current result ...
      close_home(*home);          // ... and its spare ones
      closed = true;
    } else {
      hold_owner_done(h, false);  // orcgpu_result_free
      closed = true;
    }
    CHECK(frees == (out == 0 && closed ? 1 : 0));
  };
  for (int k = 0; k < K; k++) {
    if (k == at) owner_step();
    const bool last = out == 1;
    CHECK(frees == 0);
    hold_release(h);
    out--;
    // never before the last release; at the last one only when the owner has let go for good
    if (!last) CHECK(frees == 0);
    else CHECK(frees == (at <= k && closed ? 1 : 0));
  }
  if (at == K) owner_step();
  if (owner == READER_DONE_CLOSE_LAST) {
    // the result came home (at the reader's step, or at the last release after it): the reader decodes into it again ...
    CHECK(frees == 0);
    void* again = home_take(*home);
    CHECK(again == f);
    CHECK(home_take(*home) == nullptr);
    hold_acquire(h);           // ... exports a batch of the new stripe ...
    hold_owner_done(h, true);  // ... moves on ...
    CHECK(home_take(*home) == nullptr);
    close_home(*home);         // ... and closes
    CHECK(frees == 0);
    hold_release(h);           // the batch outlives the reader
    CHECK(frees == 1);
  }
  CHECK(frees == 1);
}

int main() {
  long scenarios = 0;
  for (int N = 1; N <= 3; N++)
    for (int M = 0; M <= 2; M++)
      for (int owner = 0; owner < 4; owner++)
        for (int at = 0; at <= N + M; at++) {
          scenario(N, M, owner, at);
          scenarios++;
        }
  // ... and from several threads at once: releases race with the reader moving on and closing
  for (int round = 0; round < 200; round++) {
    int frees = 0;
    auto home = std::make_shared<Home>();
    Fake* f = new Fake();
    f->frees = &frees;
    f->hold = hold_new(f, destroy, home);
    Hold* h = f->hold;
    const int K = 8;
    for (int k = 0; k < K; k++) hold_acquire(h);
    std::vector<std::thread> ts;
    for (int k = 0; k < K; k++) ts.emplace_back([h] { hold_release(h); });
    ts.emplace_back([h, &home, round] {
      hold_owner_done(h, round % 2 == 0);
      close_home(*home);
    });
    for (auto& t : ts) t.join();
    close_home(*home);
    if (frees != 1) {
      printf("FAILED threads: round %d freed %d times\n", round, frees);
      return 1;
    }
  }
  printf("ok %ld %ld\n", scenarios, n_checks);
  return 0;
}

// handle_life_test.cpp -- d2slam_amd/csrc/handle_life.h on the host, plain and under the thread sanitizer (tests/test_handle_life_cpu.py): one destroy_requested()
// raced against the pipe_gone() calls of P live pipes.  Exactly one of the P + 1 calls returns true in every round; nothing returns true without a destroy
// request; a repeated request under live pipes is deferred again.  Prints one "ok" line per P, exits non-zero on the first violation.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "handle_life.h"

using d2fe::HandleLife;

#define CHECK(cond, ...)                                                                \
  do {                                                                                  \
    if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } \
  } while (0)

// P pipes go and one destroy is requested (or none), all behind one start flag; returns how many calls said "destroy now" and whether the request was the one
static int race(int P, bool with_destroy, bool* by_request) {
  HandleLife life;
  for (int i = 0; i < P; ++i) life.pipe_added();
  CHECK(life.pipes() == P, "pipes() = %d after %d pipe_added()", life.pipes(), P);
  std::atomic<bool> go{false};
  std::atomic<int> ready{0}, trues{0};
  std::atomic<bool> req{false};
  std::vector<std::thread> th;
  auto wait = [&] { ready.fetch_add(1); while (!go.load(std::memory_order_acquire)) std::this_thread::yield(); };
  for (int i = 0; i < P; ++i) th.emplace_back([&] { wait(); if (life.pipe_gone()) trues.fetch_add(1); });
  if (with_destroy) th.emplace_back([&] { wait(); if (life.destroy_requested()) { trues.fetch_add(1); req.store(true); } });
  while (ready.load() < (int)th.size()) std::this_thread::yield();
  go.store(true, std::memory_order_release);
  for (auto& t : th) t.join();
  CHECK(life.pipes() == 0, "pipes() = %d after every pipe went", life.pipes());
  *by_request = req.load();
  return trues.load();
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
  for (int P : {1, 2, 8}) {
    int by_request = 0, by_pipe = 0;
    for (int r = 0; r < rounds; ++r) {
      bool req = false;
      const int n = race(P, true, &req);
      CHECK(n == 1, "P = %d round %d: %d calls returned true, exactly one must", P, r, n);
      (req ? by_request : by_pipe) += 1;
      const int n0 = race(P, false, &req);
      CHECK(n0 == 0, "P = %d round %d: pipe_gone() returned true %d times with no destroy requested", P, r, n0);
    }
    std::printf("ok %d %d %d %d\n", P, rounds, by_request, by_pipe);
  }
  // in order, one thread: a request under live pipes is deferred, a repeated one again; the last pipe to go -- and only it -- is told to destroy
  HandleLife life;
  CHECK(life.destroy_requested(), "no pipes: destroy now");
  life.pipe_added(); life.pipe_added();
  CHECK(!life.destroy_requested(), "two live pipes: deferred");
  CHECK(!life.destroy_requested(), "a second request under live pipes: deferred again");
  CHECK(life.pipes() == 2, "a request does not change the count");
  CHECK(!life.pipe_gone(), "one pipe left");
  CHECK(!life.destroy_requested(), "one live pipe: still deferred");
  CHECK(life.pipe_gone(), "the last pipe of a doomed handle destroys it");
  CHECK(life.destroy_requested(), "that destroy finds no pipes");
  std::printf("ok sequence\n");
  return 0;
}

// handle_life.h -- "pipes alive / destroy requested" of a handle, under ONE lock.  A pipe's lanes read the parent handle's packed weights, so d2fe_destroy under
// live pipes only marks the handle and the last pipe to go releases it.  Count and mark change under the same mutex: for any interleaving of one
// destroy_requested() with the pipe_gone() calls of the pipes alive exactly one call returns true, the last in lock order, and its caller destroys the handle.
// Plain C++, no HIP: tests/cpp/handle_life_test.cpp drives it from g++ under the thread sanitizer.  Internal.
#pragma once
#include <mutex>

namespace d2fe {

class HandleLife {
  std::mutex mu;
  int alive = 0;
  bool doomed = false;

 public:
  void pipe_added() { std::lock_guard<std::mutex> lk(mu); ++alive; }
  // true: the caller was the last pipe of a doomed handle and must destroy it now
  bool pipe_gone() { std::lock_guard<std::mutex> lk(mu); return --alive == 0 && doomed; }
  // true: no pipes, destroy now; false: marked, the last pipe_gone() will say so
  bool destroy_requested() { std::lock_guard<std::mutex> lk(mu); if (alive > 0) doomed = true; return alive == 0; }
  int pipes() { std::lock_guard<std::mutex> lk(mu); return alive; }
};

}  // namespace d2fe

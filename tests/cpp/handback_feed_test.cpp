// The hand-back feed of a shared round (csrc/handback_feed.hpp) driven by stubs: no device, no library.
//   (a) the stream "runs" while another thread sets the flag words, then is "done": every flagged position is searched exactly once,
//       every other one not at all, positions the label callable rejects are not searched;
//   (b) the stream "runs" a few times and then "fails": every thread returns, the caller sees the failure, nothing is searched twice;
//   (c) no flag words: the feed is closed from the start, the own share is searched and nothing else.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "handback_feed.hpp"

namespace {

constexpr int kThreads = 4;
constexpr size_t kOwn = 400, kDev = 4000, kPositions = kOwn + kDev;

int failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

struct Round {
  std::vector<size_t> own, dev;
  std::vector<uint32_t> flags = std::vector<uint32_t>(kDev, 0u);
  std::vector<std::atomic<int>> searched = std::vector<std::atomic<int>>(kPositions);
  Round() {
    for (size_t k = 0; k < kOwn; k++) own.push_back(k);
    for (size_t j = 0; j < kDev; j++) dev.push_back(kPositions - 1 - j);       // (device order is not position order)
    for (auto &s : searched) s.store(0);
  }
  static bool flagged(size_t j) { return j % 3 == 0; }
  static uint32_t reason(size_t j) { return j % 2 ? 1u : 2u; }                // 1: over the budget
  static bool connected(size_t k) { return k % 5 != 0; }                      // the label cut rejects every fifth position
  template <class Feed> void run_threads(Feed &feed) {
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; t++) th.emplace_back([&] { feed.run([&](size_t k) { searched[k].fetch_add(1); }); });
    for (auto &x : th) x.join();
  }
};

void flags_set_while_running() {
  Round r;
  std::atomic<bool> kernel_ended{false};
  handback::Feed feed(
      r.flags.data(), r.dev, r.own, kPositions,
      [&] { return kernel_ended.load(std::memory_order_acquire) ? handback::Stream::done : handback::Stream::running; },
      [&](size_t k) { return Round::connected(k); });
  std::thread kernel([&] {
    for (size_t j = 0; j < kDev; j++) {
      if (Round::flagged(j)) __atomic_store_n(&r.flags[j], Round::reason(j), __ATOMIC_RELEASE);
      if (j % 500 == 499) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    kernel_ended.store(true, std::memory_order_release);
  });
  r.run_threads(feed);
  kernel.join();
  int64_t n_flagged = 0, n_over = 0;
  for (size_t k = 0; k < kOwn; k++) CHECK(r.searched[k].load() == 1);
  for (size_t j = 0; j < kDev; j++) {
    const size_t k = r.dev[j];
    const bool f = Round::flagged(j);
    n_flagged += f; n_over += f && Round::reason(j) == 1u;
    CHECK(r.searched[k].load() == (f && Round::connected(k) ? 1 : 0));
    CHECK(feed.handled[k] == (f ? 1 : 0));
  }
  CHECK(!feed.failed && feed.stream_done);
  CHECK(feed.handed_back == n_flagged && feed.over_budget == n_over);
}

void stream_fails() {
  Round r;
  for (size_t j = 0; j < kDev; j++) if (Round::flagged(j)) r.flags[j] = Round::reason(j);
  std::atomic<int> asked{0};
  handback::Feed feed(
      r.flags.data(), r.dev, r.own, kPositions, [&] { return asked.fetch_add(1) < 3 ? handback::Stream::running : handback::Stream::failed; },
      [&](size_t k) { return Round::connected(k); });
  r.run_threads(feed);                                          // (a feed that waits for "done" never comes back from here)
  CHECK(feed.failed && !feed.stream_done);
  for (size_t k = 0; k < kOwn; k++) CHECK(r.searched[k].load() == 1);
  for (size_t j = 0; j < kDev; j++) {
    const size_t k = r.dev[j];
    CHECK(r.searched[k].load() <= 1);
    if (!Round::flagged(j) || !Round::connected(k)) CHECK(r.searched[k].load() == 0);
    if (feed.handled[k] && Round::connected(k)) CHECK(r.searched[k].load() == 1);      // what was fed before the failure was drained
  }
}

void no_flag_words() {
  Round r;
  std::atomic<int> asked{0};
  handback::Feed feed(
      nullptr, r.dev, r.own, kPositions, [&] { asked++; return handback::Stream::running; }, [](size_t) { return true; });
  r.run_threads(feed);
  CHECK(asked.load() == 0 && !feed.failed && feed.handed_back == 0);
  for (size_t k = 0; k < kPositions; k++) CHECK(r.searched[k].load() == (k < kOwn ? 1 : 0));
}

}  // namespace

int main() {
  flags_set_while_running();
  stream_fails();
  no_flag_words();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("handback feed ok\n");
  return 0;
}

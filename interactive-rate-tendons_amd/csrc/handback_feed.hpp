// handback_feed.hpp -- the host threads' side of a shared round of tr_roadmap_solve (roadmap_solve_host.inc), free of any HIP header so
// that it can be driven by stubs (tests/cpp/handback_feed_test.cpp).
//
// One team of host threads for the whole shared round: first the host's own share (the searches expected to be longest), then --
// while the kernel is still running -- whatever it hands back, the MOMENT it does: the kernel sets a word per query in pinned
// memory when a search exceeds its budget (or finds no larger table, ...), a thread with nothing else to do polls those
// words and the stream, and feeds the others.  The longest searches of a round -- which bound the launch when a wave has to
// finish them at a tenth of a core's pace -- are thus finished by cores while the waves work through the rest, and the budget
// can be small.
//
// A single producer (whoever holds poll_mu_) appends to the feed and publishes its tail with a release store; the consumers claim
// entries by compare-and-swap on the head.  The feed closes when the stream is no longer running -- finished OR failed: a stream that
// reports an error will never report success, and threads that waited for that would wait for ever.
#pragma once

#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

namespace handback {

enum class Stream { running, done, failed };

// StreamState: Stream()            what the kernel's stream is doing (hipSuccess -> done, hipErrorNotReady -> running, anything else -> failed)
// StillWanted: bool(size_t k)      whether the handed-back position k still needs a search (the label cut); called by the poller only
template <class StreamState, class StillWanted>
class Feed {
 public:
  using Clock = std::chrono::steady_clock;

  // flags[j] != 0: the kernel has handed back the search of position dev_list[j] (1: over its budget); null: nothing can be fed, the
  // feed is closed from the start.  `own`: the host threads' own share.  Positions are below n_positions.
  Feed(const uint32_t *flags, const std::vector<size_t> &dev_list, const std::vector<size_t> &own, size_t n_positions,
       StreamState stream_state, StillWanted still_wanted)
      : handled(n_positions, 0), flags_(flags), dev_(dev_list), own_(own), stream_state_(stream_state), still_wanted_(still_wanted),
        seen_(dev_list.size(), 0), feed_(dev_list.size()), own_left_((int64_t)own.size()), closed_(flags == nullptr) {}

  // One host thread's part: search(k) for positions of the own share, then for fed ones, until the feed is closed and empty.
  template <class Search> void run(Search &&search) {
    const int64_t n_own = (int64_t)own_.size();
    for (;;) {
      const int64_t j = next_own_.load(std::memory_order_relaxed) < n_own ? next_own_.fetch_add(1) : n_own;
      if (j < n_own) {
        search(own_[(size_t)j]);
        if (own_left_.fetch_sub(1) == 1) own_done_at = Clock::now();
        continue;
      }
      int64_t h = head_.load(std::memory_order_relaxed);
      if (h < tail_.load(std::memory_order_acquire)) {
        if (head_.compare_exchange_weak(h, h + 1)) search(feed_[(size_t)h]);
        continue;
      }
      if (closed_.load(std::memory_order_acquire)) {
        if (head_.load() < tail_.load(std::memory_order_acquire)) continue;
        break;
      }
      if (poll_mu_.try_lock()) { poll(); poll_mu_.unlock(); }
      std::this_thread::sleep_for(std::chrono::microseconds(25));
    }
  }

  // for the caller, after every run() has returned
  const Clock::time_point started_at = Clock::now();
  Clock::time_point own_done_at = started_at;                    // the last search of the own share ended
  Clock::time_point stream_done_at = started_at;                 // the poller saw the stream finish (if stream_done)
  bool stream_done = false, failed = false;                      // failed: the stream reported an error
  std::vector<uint8_t> handled;                                  // per position: handed back while the kernel ran
  int64_t handed_back = 0, over_budget = 0;                      // (written by the poller only)

 private:
  void poll() {                                                  // (under poll_mu_)
    const Stream st = stream_state_();                           // asked BEFORE the words are read: one set before the kernel ended is then seen below
    if (st == Stream::done && !stream_done) { stream_done_at = Clock::now(); stream_done = true; }
    int64_t t = tail_.load(std::memory_order_relaxed);
    for (size_t j = 0; j < dev_.size(); j++) {
      const uint32_t why = seen_[j] ? 0u : __atomic_load_n(&flags_[j], __ATOMIC_ACQUIRE);
      if (!why) continue;
      seen_[j] = 1;
      if (why == 1u) over_budget++;
      const size_t k = dev_[j];
      handled[k] = 1;
      handed_back++;
      if (still_wanted_(k)) feed_[(size_t)t++] = k;
    }
    tail_.store(t, std::memory_order_release);
    if (st == Stream::failed) failed = true;
    if (st != Stream::running) closed_.store(true, std::memory_order_release);
  }

  const uint32_t *flags_;
  const std::vector<size_t> &dev_, &own_;
  StreamState stream_state_;
  StillWanted still_wanted_;
  std::vector<uint8_t> seen_;
  std::vector<size_t> feed_;
  std::atomic<int64_t> tail_{0}, head_{0}, next_own_{0}, own_left_;
  std::atomic<bool> closed_;
  std::mutex poll_mu_;
};

}  // namespace handback

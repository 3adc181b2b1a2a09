// roadmap_infra_host.inc -- part of roadmap.hip: what the host side of the unit stands on (clocks, the host threads, the buffer cache).
namespace {

using Clock = std::chrono::steady_clock;
inline double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

inline size_t up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }          // device sub-buffers start at multiples of 256 bytes

// TENDON_HIP_ROADMAP_TIMING=1: the host phases of tr_roadmap_create / tr_roadmap_prepare on stderr (profiles/probe_query_object.py)
struct Laps {
  const bool on;
  Clock::time_point t0 = Clock::now();
  Laps(const RoadmapSwitches &sw, const char *what) : on(sw.timing) { if (on) std::fprintf(stderr, "[%s]", what); }
  void lap(const char *name) {
    if (!on) return;
    const auto t1 = Clock::now();
    std::fprintf(stderr, " %s %.2f ms", name, ms_between(t0, t1));
    t0 = t1;
  }
  ~Laps() { if (on) std::fprintf(stderr, "\n"); }
};

// The library's host threads: started once per process and parked on a condition variable between jobs -- a tr_roadmap_solve runs six
// or seven parallel sections, and starting fifteen threads for each was 0.3 - 0.5 ms a time (2 - 3 ms of a 25 ms batch of queries).
// One job at a time; a caller that finds the team busy (another roadmap's call on another host thread) starts threads of its own as
// before.  Never destroyed: its threads wait inside it when the process ends.
class HostTeam {
  std::mutex mu_, job_mu_;
  std::condition_variable work_, done_;
  std::vector<std::thread> th_;
  const std::function<void(int)> *fn_ = nullptr;
  int T_ = 0, running_ = 0;
  uint64_t epoch_ = 0;
  void worker(int t) {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(int)> *f = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        work_.wait(lk, [&] { return epoch_ != seen; });
        seen = epoch_;
        if (t < T_) f = fn_;
      }
      if (f) {
        inside() = true;
        (*f)(t);
        inside() = false;
        std::lock_guard<std::mutex> lk(mu_);
        if (--running_ == 0) done_.notify_all();
      }
    }
  }
  static bool &inside() { static thread_local bool in = false; return in; }   // this thread is running a section of the team's job
 public:
  static HostTeam &get() { static HostTeam *team = new HostTeam(); return *team; }
  // fn(1) .. fn(T - 1) on the team's threads, fn(0) on the caller's; false (nothing run) when the team is busy
  bool run(int T, const std::function<void(int)> &fn) {
    if (inside()) return false;                 // (a section started from inside a section: threads of its own, as when the team is busy)
    std::unique_lock<std::mutex> job(job_mu_, std::try_to_lock);
    if (!job.owns_lock()) return false;
    struct Mark { Mark() { inside() = true; } ~Mark() { inside() = false; } } mark;
    {
      std::lock_guard<std::mutex> lk(mu_);
      while ((int)th_.size() < T - 1) { const int t = (int)th_.size() + 1; th_.emplace_back([this, t] { worker(t); }); th_.back().detach(); }
      fn_ = &fn; T_ = T; running_ = T - 1; epoch_++;
    }
    work_.notify_all();
    fn(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [&] { return running_ == 0; });
    fn_ = nullptr; T_ = 0;
    return true;
  }
};

// fn(t) for t = 0 .. T-1 on T host threads (the caller's included)
template <class F> void on_threads(int T, F &&fn) {
  if (T <= 1) { fn(0); return; }
  const std::function<void(int)> f = [&fn](int t) { fn(t); };
  if (HostTeam::get().run(T, f)) return;
  std::vector<std::thread> th;
  th.reserve((size_t)T - 1);
  for (int t = 1; t < T; t++) th.emplace_back([&fn, t] { fn(t); });
  fn(0);
  for (auto &x : th) x.join();
}

// Device buffers of the query objects come from a small per-process cache instead of hipMalloc / hipFree: a roadmap build attaches
// and later drops ~0.45 GB of them (block lists, offsets, the landmark arena), six allocations and frees of 0.1 - 1 ms each
// (set_caches 2.8 -> 2.2 ms, prepare 6.1 -> 5.7 ms).  A freed buffer is kept (up to kCacheMaxBytes / kCacheMaxEntries per
// process) and handed to the next request of at least half its size; a failed hipMalloc empties the cache and tries again.
struct DevCache {
  struct Buf { void *p; size_t bytes; int dev; };
  std::mutex mu;
  std::vector<Buf> idle;
  std::unordered_map<void *, Buf> live;
  size_t idle_bytes = 0;
  static constexpr size_t kCacheMaxBytes = (size_t)1 << 30, kCacheMaxEntries = 32;
  hipError_t alloc(int dev, void **out, size_t bytes) {
    bytes = std::max<size_t>(bytes, 256);
    std::lock_guard<std::mutex> lock(mu);
    size_t best = idle.size();
    for (size_t i = 0; i < idle.size(); i++)
      if (idle[i].dev == dev && idle[i].bytes >= bytes && idle[i].bytes <= 2 * bytes + ((size_t)1 << 20) &&
          (best == idle.size() || idle[i].bytes < idle[best].bytes)) best = i;
    if (best < idle.size()) {
      const Buf b = idle[best];
      idle.erase(idle.begin() + (long)best);
      idle_bytes -= b.bytes;
      live[b.p] = b;
      *out = b.p;
      return hipSuccess;
    }
    const size_t cap = (bytes + ((size_t)1 << 16) - 1) & ~(((size_t)1 << 16) - 1);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess && !idle.empty()) {                     // out of memory with buffers parked here: give them back and try again
      for (const Buf &b : idle) (void)hipFree(b.p);
      idle.clear(); idle_bytes = 0;
      e = hipMalloc(&p, cap);
    }
    if (e != hipSuccess) return e;
    live[p] = Buf{p, cap, dev};
    *out = p;
    return hipSuccess;
  }
  // everything parked goes back to the device (an allocation elsewhere in the library ran out of memory: tr_dev_cache_trim)
  void trim() {
    std::lock_guard<std::mutex> lock(mu);
    for (const Buf &b : idle) (void)hipFree(b.p);
    idle.clear(); idle_bytes = 0;
  }
  void release(void *p) {
    if (!p) return;
    // hipFree synchronised with the device; a parked buffer may be handed to its next owner at once, so work that still uses it
    // (a roadmap destroyed with launches in flight) is waited for here
    (void)hipDeviceSynchronize();
    std::lock_guard<std::mutex> lock(mu);
    auto it = live.find(p);
    if (it == live.end()) { (void)hipFree(p); return; }
    const Buf b = it->second;
    live.erase(it);
    if (idle.size() < kCacheMaxEntries && idle_bytes + b.bytes <= kCacheMaxBytes) { idle.push_back(b); idle_bytes += b.bytes; }
    else (void)hipFree(b.p);
  }
};
DevCache &dev_cache() { static DevCache c; return c; }
}  // namespace
void release_idle_search_tables();   // (below: the search tables of the roadmaps that are not in a call right now)
void tr_dev_cache_trim() { release_idle_search_tables(); dev_cache().trim(); }
namespace {

int host_threads(int want) {
  if (want > 0) return want;
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = (unsigned)CPU_COUNT(&set);
  if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {          // a container's CPU quota
    long long quota = 0, period = 0;
    char q[32] = {0};
    if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
      quota = std::atoll(q);
      if (quota > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, quota / period));
    }
    std::fclose(f);
  }
  return (int)std::max(1u, std::min(n, 64u));
}

struct Node {                          // A* state of one vertex in one search: 32 B, one cache line touched per visit
  double g, h;
  int32_t parent, parent_edge;
  uint32_t stamp, closed;
};
struct SeedTarget { int32_t v; double d; int32_t j; };     // astar_seeded: a target vertex, its seed cost, the seed's index in the query's list
struct Scratch {                       // per host thread, reused across queries: generation-stamped A* state
  std::vector<Node> node;
  std::vector<std::pair<double, int32_t>> heap;
  std::vector<SeedTarget> targets;     // (astar_seeded: the targets of the query in hand)
  uint32_t gen = 0;
  bool trace = false;                  // TENDON_HIP_SEARCH_HIST=<file> (set per call by tr_roadmap_solve): astar fills trace_f
  double trace_f[4] = {0, 0, 0, 0};    // h(start), and the key taken off the list at the 2 000th / 3 000th / 4 000th expansion
};

}  // namespace

// A heap array that is NOT zeroed when sized (std::vector would touch all of it on the calling thread: for the 19 MB of arcs of a
// 100 k-vertex roadmap the page faults of that pass cost more than filling them): the pages are first touched by the threads that fill them.
template <class T> struct RawArray {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void resize_uninit(size_t m) { p.reset(new T[m]); n = m; }
  size_t size() const { return n; }
  T *data() { return p.get(); }
  const T *data() const { return p.get(); }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
};
